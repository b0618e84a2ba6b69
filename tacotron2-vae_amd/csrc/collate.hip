// Batch collate from the resident corpus (reference data_utils.py:88-137 TextMelCollate, with the mels already on the device):
// ONE launch gathers B utterances out of the flat stores into the reference's padded batch tensors.  Every output element is
// written exactly once, pads included (the caller hands over torch.empty memory); no atomics, no LDS, plain dword / qword
// accesses that are coalesced along time.
#include "t2v_common.h"
#include "t2v_kernels.h"

// grid = (B, n_mel + 3), block = 256.  Row y of batch row b:
//   y < n_mel      mel channel y:            mel_padded[b][y][t]  = t < T_b ? store[off_b + y T_b + t] : 0
//   y == n_mel     gate:                     gate_padded[b][t]    = t >= T_b - 1
//   y == n_mel + 1 text:                     text_padded[b][s]    = s < L_b ? ids[off_b + s] : 0
//   y == n_mel + 2 the small outputs:        output_lengths[b], the two one-hot rows
// The utterance index is clamped to [0, n_utts) and its counts to [0, T_out] / [0, T_in], so nothing outside a store is read and
// nothing outside an output row is written, whatever idx holds (the host has checked it; a clamped batch is wrong, not a fault).
// A stored utterance keeps its own row stride: frame t of channel y is read at y n_frames[u] + t with t < min(n_frames[u], T_out).
__global__ __launch_bounds__(256) void k_collate_batch(
    const float* __restrict__ mel_store, const int64_t* __restrict__ mel_off, const int32_t* __restrict__ n_frames,
    const int32_t* __restrict__ id_store, const int64_t* __restrict__ id_off, const int32_t* __restrict__ n_ids,
    const int32_t* __restrict__ speaker, const int32_t* __restrict__ emotion, const int32_t* __restrict__ idx, int n_utts,
    int T_in, int T_out, int n_mel, int n_speakers, int n_emotions, int64_t* __restrict__ text_padded,
    float* __restrict__ mel_padded, float* __restrict__ gate_padded, int64_t* __restrict__ output_lengths,
    int64_t* __restrict__ speakers, int64_t* __restrict__ emotions) {
    const int b = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const int u = min(max(idx[b], 0), n_utts - 1);
    if (y <= n_mel) {
        const int stride = max(n_frames[u], 0), Tb = min(stride, T_out);
        if (y < n_mel) {
            const float* src = mel_store + mel_off[u] + (size_t)y * stride;
            float* dst = mel_padded + ((size_t)b * n_mel + y) * T_out;
            for (int t = tid; t < T_out; t += 256) dst[t] = t < Tb ? src[t] : 0.0f;
        } else {
            float* dst = gate_padded + (size_t)b * T_out;
            for (int t = tid; t < T_out; t += 256) dst[t] = t >= Tb - 1 ? 1.0f : 0.0f;
        }
    } else if (y == n_mel + 1) {
        const int Lb = min(max(n_ids[u], 0), T_in);
        const int32_t* src = id_store + id_off[u];
        int64_t* dst = text_padded + (size_t)b * T_in;
        for (int s = tid; s < T_in; s += 256) dst[s] = s < Lb ? (int64_t)src[s] : 0;
    } else {
        if (tid == 0) output_lengths[b] = min(max(n_frames[u], 0), T_out);
        const int spk = speaker[u], emo = emotion[u];
        for (int j = tid; j < n_speakers; j += 256) speakers[(size_t)b * n_speakers + j] = j == spk;
        for (int j = tid; j < n_emotions; j += 256) emotions[(size_t)b * n_emotions + j] = j == emo;
    }
}

extern "C" int t2v_collate_batch(const float* mel_store, const int64_t* mel_off, const int32_t* n_frames,
                                 const int32_t* id_store, const int64_t* id_off, const int32_t* n_ids,
                                 const int32_t* speaker, const int32_t* emotion, const int32_t* idx, int B, int n_utts,
                                 int T_in, int T_out, int n_speakers, int n_emotions, int64_t* text_padded,
                                 float* mel_padded, float* gate_padded, int64_t* output_lengths, int64_t* speakers,
                                 int64_t* emotions, void* stream_) {
    if (!mel_store || !mel_off || !n_frames || !id_store || !id_off || !n_ids || !speaker || !emotion || !idx ||
        !text_padded || !mel_padded || !gate_padded || !output_lengths || !speakers || !emotions)
        return T2V_ERR_ARG;
    if (B < 1 || n_utts < 1 || T_in < 1 || T_out < 1 || n_speakers < 1 || n_emotions < 1) return T2V_ERR_ARG;
    k_collate_batch<<<dim3(B, T2V_NMEL + 3), 256, 0, (hipStream_t)stream_>>>(
        mel_store, mel_off, n_frames, id_store, id_off, n_ids, speaker, emotion, idx, n_utts, T_in, T_out, T2V_NMEL,
        n_speakers, n_emotions, text_padded, mel_padded, gate_padded, output_lengths, speakers, emotions);
    return t2v_check_launch();
}
