// Forced alignment: the best monotonic path through an alignment matrix, and sums of a frame track over its segments.
// (t2v_hip.mas, t2v_hip.segment_means, Synthesizer.durations, evaluate(durations=True), extract_durations.py.)
//
// Measure (row b: A[b, t < n, j < L], nothing else is read; S = max_step; include/t2vae.h states it in full):
//   a(t, j) = max(A[b, t, j], T2V_MAS_FLOOR), a NaN is the floor;  Q(0, 0) = ln a(0, 0);
//   Q(t, j) = ln a(t, j) + max_{s = 0..S} Q(t-1, j-s): logf, then one fp32 add; the smallest s wins a tie;
//   only cells of the band j <= t S, L - 1 - j <= (n - 1 - t) S exist; the path ends in (n - 1, L - 1).
//
// k_mas: one workgroup of 256 threads per row.  Thread i owns the columns i, i + 256, ... (at most MAS_K = 8 of them: T_in <=
// T2V_MAS_MAX_SYMBOLS).  The frames are taken MAS_F = 8 at a time: the loads of the next eight frames' weights are issued
// before the eight dependent steps of the current ones; ln a(t, j) does not depend on the recurrence and stays in registers
// (kept in LDS instead it measured slower: DESIGN 7u).  The two live rows of Q sit in LDS behind
// four cells of -inf, so Q(t-1, j-s) needs no test of j - s; one barrier per frame.  The decision s of every cell of the band
// is one byte of the caller's scratch.  The walk back from (n - 1, L - 1) goes MAS_WF = 64 frames at a time: the workgroup
// copies the window of decisions the path can reach in those frames into LDS and thread 0 follows it there.  The durations
// and starts come from the stored path: a thread that finds the first frame of a segment writes the start of its symbol and
// of the symbols skipped before it, one that finds the last frame writes the end, and a last pass over the symbols takes the
// difference.  Nothing is summed in floating point outside the recurrence, no atomics, no cross-workgroup hand-off: a row
// gives the same bits alone, in any batch, at any stride and with any padding.
// k_segment_means: one thread per symbol adds its segment's counted frames in ascending order.
#include "t2v_common.h"
#include "t2v_kernels.h"

#define MAS_NT 256
#define MAS_K (T2V_MAS_MAX_SYMBOLS / MAS_NT)      // columns per thread at the largest T_in
#define MAS_F 8                                   // frames per block of loads
#define MAS_PAD 4                                 // cells of -inf in front of a row of Q (max_step <= 3)
#define MAS_WF 64                                 // frames per block of the walk back
#define MAS_WW 196                                // bytes per frame of its window of decisions: (MAS_WF - 1) 3 + 1 columns, padded
static_assert(MAS_WF * MAS_WW <= 2 * (MAS_PAD + T2V_MAS_MAX_SYMBOLS) * 4, "the walk's window lives in the rows of Q");

__device__ __forceinline__ float mas_ln(float a) { return logf(a > T2V_MAS_FLOOR ? a : T2V_MAS_FLOOR); }   // NaN: the floor

__global__ __launch_bounds__(MAS_NT) void k_mas(const float* __restrict__ A, long long a_stride_b, long long a_stride_t,
                                                const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_ids, int N,
                                                int T_in, int S, unsigned char* dec, int32_t* path, int path_stride,
                                                int32_t* durations, int32_t* starts, int sym_stride, float* __restrict__ score) {
    __shared__ float Q[2][MAS_PAD + T2V_MAS_MAX_SYMBOLS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(n_frames[b], 0), N), L = min(max(n_ids[b], 0), T_in);    // no length addresses outside the tensor
    int32_t* p = path + (size_t)b * path_stride;
    int32_t* dur = durations + (size_t)b * sym_stride;
    int32_t* sta = starts + (size_t)b * sym_stride;
    const bool feasible = n >= 1 && L >= 1 && (long long)(L - 1) <= (long long)(n - 1) * S;
    const int n_live = feasible ? n : 0;
    for (int t = n_live + tid; t < path_stride; t += MAS_NT) p[t] = -1;
    for (int j = tid; j < sym_stride; j += MAS_NT) {
        dur[j] = 0;
        sta[j] = 0;
    }
    if (!feasible) {
        if (tid == 0) score[b] = __int_as_float(0x7fc00000);
        return;
    }
    if (tid < MAS_PAD) Q[0][tid] = Q[1][tid] = -INFINITY;

    const float* a0 = A + (size_t)b * a_stride_b;
    unsigned char* D = dec + (size_t)b * N * T_in;
    float raw[MAS_F][MAS_K], la[MAS_F][MAS_K];
#pragma unroll
    for (int f = 0; f < MAS_F; ++f)
#pragma unroll
        for (int k = 0; k < MAS_K; ++k) {
            const int j = tid + k * MAS_NT;
            raw[f][k] = (f < n && j < L) ? a0[(size_t)f * a_stride_t + j] : 1.f;
        }
    for (int t0 = 0; t0 < n; t0 += MAS_F) {
#pragma unroll
        for (int f = 0; f < MAS_F; ++f)
#pragma unroll
            for (int k = 0; k < MAS_K; ++k) la[f][k] = mas_ln(raw[f][k]);
#pragma unroll
        for (int f = 0; f < MAS_F; ++f)                                            // the next block's loads, in flight over the steps
#pragma unroll
            for (int k = 0; k < MAS_K; ++k) {
                const int t = t0 + MAS_F + f, j = tid + k * MAS_NT;
                raw[f][k] = (t < n && j < L) ? a0[(size_t)t * a_stride_t + j] : 1.f;
            }
#pragma unroll
        for (int f = 0; f < MAS_F; ++f) {
            const int t = t0 + f;
            if (t < n) {                                                           // uniform over the workgroup
                const float* Qp = Q[(t & 1) ^ 1] + MAS_PAD;
                float* Qc = Q[t & 1] + MAS_PAD;
                const int hi = (int)min((long long)(L - 1), (long long)t * S);
                const int lo = (int)max(0LL, (long long)(L - 1) - (long long)(n - 1 - t) * S);
                unsigned char* Dt = D + (size_t)t * T_in;
#pragma unroll
                for (int k = 0; k < MAS_K; ++k) {
                    const int j = tid + k * MAS_NT;
                    if (j < L) {
                        float q = -INFINITY;
                        if (j >= lo && j <= hi) {
                            float best = 0.f;
                            int arg = 0;
                            if (t > 0) {
                                best = Qp[j];
#pragma unroll
                                for (int s = 1; s <= 3; ++s) {
                                    const float v = Qp[j - s];
                                    if (s <= S && v > best) {                      // strictly larger only: the smallest step wins
                                        best = v;
                                        arg = s;
                                    }
                                }
                            }
                            q = la[f][k] + best;
                            Dt[j] = (unsigned char)arg;
                        }
                        Qc[j] = q;
                    }
                }
            }
            __syncthreads();
        }
    }
    // The walk back, MAS_WF frames at a time (the decisions were stored by this workgroup before the last barrier).  Over a
    // block of frames the path stays within (MAS_WF - 1) S columns below the column it enters with, so the workgroup copies
    // that window of decisions into LDS (the rows of Q are free now) with all its loads in flight, and thread 0 follows the
    // path through LDS: one round trip to memory per block instead of one per frame.
    __shared__ int jcur;
    if (tid == 0) {
        score[b] = Q[(n - 1) & 1][MAS_PAD + L - 1] / (float)n;
        jcur = L - 1;
    }
    __syncthreads();
    unsigned char* W = (unsigned char*)&Q[0][0];                                   // MAS_WF rows of MAS_WW bytes
    const int lane = tid & 63, wave = tid >> 6;
    for (int t1 = n; t1 > 0; t1 -= MAS_WF) {
        const int t0 = max(t1 - MAS_WF, 0), nf = t1 - t0;
        int j = jcur;                                                              // the column of frame t1 - 1
        const int c0 = max(j - (nf - 1) * S, 0), w = j - c0 + 1;                   // w <= (MAS_WF - 1) 3 + 1 < MAS_WW
        for (int f = wave; f < nf; f += MAS_NT / 64)
            for (int c = lane; c < w; c += 64) W[f * MAS_WW + c] = D[(size_t)(t0 + f) * T_in + c0 + c];
        __syncthreads();
        if (tid == 0) {
            for (int t = t1 - 1; t >= t0; --t) {
                p[t] = j;
                const int s = min((int)W[(t - t0) * MAS_WW + (j - c0)], S);        // a cell of the band holds a step <= S
                j = max(j - s, 0);                                                 // inside the block that stays in the window
            }
            jcur = j;
        }
        __syncthreads();
    }
    for (int t = tid; t < n; t += MAS_NT) {
        const int cur = p[t], prev = t > 0 ? p[t - 1] : -1, next = t < n - 1 ? p[t + 1] : -2;
        if (cur != prev)
            for (int k = prev + 1; k <= cur; ++k) sta[k] = t;                      // its own start, and that of the symbols skipped
        if (cur != next) dur[cur] = t + 1;                                         // the segment's end for now
    }
    __syncthreads();
    for (int j = tid; j < L; j += MAS_NT) {
        const int e = dur[j];
        if (e) dur[j] = e - sta[j];
    }
}

__global__ __launch_bounds__(256) void k_segment_means(const float* __restrict__ v, const unsigned char* __restrict__ counted,
                                                       int v_stride, const int32_t* __restrict__ starts,
                                                       const int32_t* __restrict__ durations, int seg_stride, int T_in, int nblk,
                                                       float* __restrict__ sums, int32_t* __restrict__ counts, int out_stride) {
    const int b = blockIdx.x / nblk, j = (blockIdx.x - b * nblk) * 256 + threadIdx.x;
    if (j >= T_in) return;
    const int s = min(max(starts[(size_t)b * seg_stride + j], 0), v_stride);
    const int e = (int)min((long long)s + max(durations[(size_t)b * seg_stride + j], 0), (long long)v_stride);
    const float* vb = v + (size_t)b * v_stride;
    const unsigned char* cb = counted ? counted + (size_t)b * v_stride : nullptr;
    float sum = 0.f;
    int cnt = 0;
    for (int t = s; t < e; ++t)
        if (!cb || cb[t]) {
            sum += vb[t];                                                          // ascending frame order
            ++cnt;
        }
    sums[(size_t)b * out_stride + j] = sum;
    counts[(size_t)b * out_stride + j] = cnt;
}

extern "C" size_t t2v_mas_scratch_bytes(int B, int N, int T_in) {
    if (B < 1 || N < 1 || T_in < 1 || T_in > T2V_MAS_MAX_SYMBOLS) return 0;
    return (size_t)B * N * T_in;
}

extern "C" int t2v_mas(const float* A, long long a_stride_b, long long a_stride_t, const int32_t* n_frames, const int32_t* n_ids,
                       int B, int N, int T_in, int max_step, int32_t* path, int path_stride, int32_t* durations, int32_t* starts,
                       int sym_stride, float* score, void* scratch, void* stream_) {
    if (!A || !n_frames || !n_ids || !path || !durations || !starts || !score || !scratch) return T2V_ERR_ARG;
    if (B < 1 || N < 1 || T_in < 1) return T2V_ERR_ARG;
    if (a_stride_t < T_in || a_stride_b < (long long)(N - 1) * a_stride_t + T_in || path_stride < N || sym_stride < T_in)
        return T2V_ERR_ARG;
    if (T_in > T2V_MAS_MAX_SYMBOLS || max_step < 1 || max_step > 3) return T2V_ERR_DIMS;
    k_mas<<<B, MAS_NT, 0, (hipStream_t)stream_>>>(A, a_stride_b, a_stride_t, n_frames, n_ids, N, T_in, max_step,
                                                  (unsigned char*)scratch, path, path_stride, durations, starts, sym_stride,
                                                  score);
    return t2v_check_launch();
}

extern "C" int t2v_segment_means(const float* v, const void* counted, int v_stride, const int32_t* starts,
                                 const int32_t* durations, int seg_stride, int B, int T_in, float* sums, int32_t* counts,
                                 int out_stride, void* stream_) {
    if (!v || !starts || !durations || !sums || !counts) return T2V_ERR_ARG;
    if (B < 1 || T_in < 1 || v_stride < 1 || seg_stride < T_in || out_stride < T_in) return T2V_ERR_ARG;
    const int nblk = (T_in + 255) / 256;
    if ((long long)B * nblk > 0x7fffffffLL) return T2V_ERR_ARG;
    k_segment_means<<<B * nblk, 256, 0, (hipStream_t)stream_>>>(v, (const unsigned char*)counted, v_stride, starts, durations,
                                                                seg_stride, T_in, nblk, sums, counts, out_stride);
    return t2v_check_launch();
}
