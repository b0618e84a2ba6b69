// Wavs at any sampling rate, in front of the mel front end: a ragged polyphase resampler, an energy trim on the front end's frame
// grid and the crop / 16-bit write-out (Synthesizer(resample=True, trim_db=...), prepare_corpus.py).
//
// Resampler (row b: x[0..n), every sample index outside [0, n) counts as 0 and is never read), ratio up/down in lowest terms:
//   n_out = ceil(n up / down),   y[m] = sum_i t[m down - i up + half] x[i]   over 0 <= i < n and tap index in 0 .. 2 half.
// With a = m down + half, q = a / up and p = a mod up the taps of output m are t[p + j up], j = 0, 1, ..., against x[q - j]:
// phase p has (2 half - p) / up + 1 of them.
//
// k_resample: a lane owns RS_R = 4 outputs of one phase, m, m + S, m + 2 S, m + 3 S with S a multiple of up: they share their
// taps (one load from the table serves four fmas on four independent chains) and read x at q - j, q + D - j, ..., D = S down / up.
// A tile is 4 S consecutive outputs, S <= 1024 the multiple of up that fills workgroups of 256 lanes best (48 -> 16 kHz:
// S = 256, 44.1 -> 16: S = 480 = 256 + 224); lane l of the tile owns the outputs m0 + l + r S, so the lanes of a wave own
// consecutive outputs: their LDS reads advance by down / up samples per lane (3 at 48 kHz: 64 lanes on 64 banks) and their stores
// are contiguous.  The grid is B x tiles x ceil(S / 256) workgroups.  The input window of a workgroup's outputs,
// x[q_min - 2 half / up .. q_max], goes to LDS (zeros outside [0, n); an int16 row is scaled as it is loaded): in one pass when
// it fits RS_XW samples (every pair of common rates: 3 166 samples at 48 -> 16 kHz, 4 763 at 44.1 -> 16), else in passes of
// RS_XW from its high end down, with the reads outside a pass taken as 0.  Every output is one fma chain in ascending j through
// all passes (a product with a staged 0 leaves the sum's bits as they are), four taps' reads issued ahead of their fmas, so
// the order of its sum depends on m alone: a row gives the same bits alone, in any batch and at any stride.  The tap table
// stays in global memory as the caller made it (at most 128 KiB, shared by every workgroup: L2, and L1 when small); the lanes
// of a wave read t[p + j up], one address when up = 1.
//
// Trim: frame t covers [256 t - 512, 256 t + 512), ms[t] its mean square, n / 256 + 1 frames.  k_trim_ms: a workgroup owns 16
// frames; the 19 block sums p_k = sum_{i in [256 k, 256 k + 256)} x_i^2 they share are one wave each (four squares per lane on
// one chain, then a fixed xor butterfly) and ms[t] = (((p_{t-2} + p_{t-1}) + p_t) + p_{t+1}) / 1024: a frame's bits depend on t
// alone.  k_trim_bounds: one workgroup per row, ref = max ms, the outermost frames with ms > ref thr, and the padded bounds.
//
// Crop: k_crop_rows copies y[b][start:end] to column 0 of an output row and zeroes the tail; the int16 form rounds y 32768 to
// nearest-even and clamps, and counts what it clamped and max |y| per row with integer atomics (the order cannot show).
#include "t2v_common.h"
#include "t2v_kernels.h"

#define RS_NT 256
#define RS_XW 8192                                // samples of one LDS pass
#define RS_R 4                                    // outputs per lane, one phase
#define TR_HOP 256
#define TR_F 16                                   // frames per workgroup of k_trim_ms
#define TR_NBLK (TR_F + 3)

template <bool PCM16>
__global__ __launch_bounds__(RS_NT) void k_resample(const void* __restrict__ x_, const int32_t* __restrict__ n_in, int x_stride,
                                                    const float* __restrict__ taps, int up, int down, int half, float scale,
                                                    float* __restrict__ y, int out_stride, int tiles, int S, int vblocks) {
    __shared__ float X[RS_XW];
    const int tid = threadIdx.x;
    const int vb = blockIdx.x % vblocks, bt = blockIdx.x / vblocks;
    const int b = bt / tiles;
    const long long m0 = (long long)(bt - b * tiles) * S * RS_R;       // the tile's first output
    const int n = min(max(n_in[b], 0), x_stride);                      // no length addresses outside the row
    const int n_out = (int)min(((long long)n * up + down - 1) / down, (long long)out_stride);
    float* yb = y + (size_t)b * out_stride;
    const float* xf = (const float*)x_ + (size_t)b * x_stride;
    const int16_t* xs = (const int16_t*)x_ + (size_t)b * x_stride;
    const int two_half = 2 * half;

    // this lane: the outputs m_first + r S, which read x at q + r D - j
    const int l = vb * RS_NT + tid;
    const bool live = l < S;
    const int D = S / up * down;
    const long long m_first = m0 + l;
    // the workgroup: outputs m_min .. m_max, samples q_min - 2 half / up .. q_max
    const long long m_min = m0 + vb * RS_NT, m_max = m0 + min(vb * RS_NT + RS_NT, S) - 1 + (long long)(RS_R - 1) * S;
    if (m_min >= n_out) {                                              // a workgroup of padding
        if (live)
#pragma unroll
            for (int r = 0; r < RS_R; ++r)
                if (m_first + (long long)r * S < out_stride) yb[m_first + (long long)r * S] = 0.f;
        return;
    }
    const long long i_lo = (m_min * down + half) / up - two_half / up, i_hi = (m_max * down + half) / up;
    const long long a = m_first * down + half;
    const long long q = a / up;                                        // x index of tap j of output r: q + r D - j
    const int p = (int)(a - q * up);
    const int kn = live && m_first < n_out ? (two_half - p) / up + 1 : 0;   // taps of this lane's phase
    const float* tp = taps + p;
    float acc[RS_R];
#pragma unroll
    for (int r = 0; r < RS_R; ++r) acc[r] = 0.f;

    if (i_hi - i_lo < RS_XW) {                                         // one pass: every read of every lane lies inside it
        for (int i = tid; i <= (int)(i_hi - i_lo); i += RS_NT) {
            const long long g = i_lo + i;
            float v = 0.f;
            if (g >= 0 && g < n) v = PCM16 ? (float)xs[g] * scale : xf[g];
            X[i] = v;
        }
        __syncthreads();
        const float* xp = X + (int)(q - i_lo);
        int j = 0;
        for (; j + 4 <= kn; j += 4) {
            float t[4], v[4][RS_R];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                t[u] = tp[(j + u) * up];
#pragma unroll
                for (int r = 0; r < RS_R; ++r) v[u][r] = xp[r * D - (j + u)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(t[u], v[u][r], acc[r]);
        }
        for (; j < kn; ++j) {
            const float t = tp[j * up];
#pragma unroll
            for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(t, xp[r * D - j], acc[r]);
        }
    } else {                                                           // passes of RS_XW samples, from the high end down
        for (long long hi = i_hi; hi >= i_lo; hi -= RS_XW) {
            const long long lo = hi - RS_XW + 1;                       // the pass holds x[lo .. hi] at X[0 .. RS_XW)
            if (hi != i_hi) __syncthreads();                           // the last pass is read
            for (int i = tid; i < RS_XW; i += RS_NT) {
                const long long g = lo + i;
                float v = 0.f;
                if (g >= 0 && g < n) v = PCM16 ? (float)xs[g] * scale : xf[g];
                X[i] = v;
            }
            __syncthreads();
            // the taps j that meet the pass for some r: lo <= q + r D - j <= hi
            const int j0 = (int)max(q - hi, 0LL), j1 = (int)min(q + (long long)(RS_R - 1) * D - lo + 1, (long long)kn);
            for (int j = j0; j < j1; ++j) {
                const float t = tp[j * up];
#pragma unroll
                for (int r = 0; r < RS_R; ++r) {
                    const long long idx = q + (long long)r * D - j - lo;
                    acc[r] = fmaf(t, idx >= 0 && idx < RS_XW ? X[idx] : 0.f, acc[r]);
                }
            }
        }
    }
    if (live)
#pragma unroll
        for (int r = 0; r < RS_R; ++r) {
            const long long m = m_first + (long long)r * S;
            if (m < out_stride) yb[m] = m < n_out ? acc[r] : 0.f;
        }
}

// lanes per tile: the multiple of up, at most 1024, that leaves the fewest idle lanes in workgroups of RS_NT (the smallest such)
static int rs_tile_lanes(int up) {
    int best = up;
    long long best_num = 0, best_den = 1;
    for (int S = up; S <= 1024 || S == up; S += up) {
        const long long den = (long long)RS_NT * ((S + RS_NT - 1) / RS_NT);
        if ((long long)S * best_den > best_num * den) {
            best = S;
            best_num = S;
            best_den = den;
        }
    }
    return best;
}

extern "C" int t2v_resample(const void* x, int x_is_pcm16, float scale, const int32_t* n, int x_stride, int B, const float* taps,
                            int up, int down, int half, float* y, int out_stride, void* stream_) {
    if (!x || !n || !y || B < 1 || x_stride < 1 || x_stride > (1 << 30) || out_stride < 1 || up < 1 || down < 1)
        return T2V_ERR_ARG;
    if (up == down) return T2V_OK;                                     // equal rates: nothing to do, nothing launched
    if (!taps || half < 1) return T2V_ERR_ARG;
    if (2LL * half + 1 > T2V_RESAMPLE_MAX_TAPS || up > 2 * half) return T2V_ERR_DIMS;
    const long long need = ((long long)x_stride * up + down - 1) / down;
    if (out_stride < need || out_stride > (1 << 30)) return T2V_ERR_ARG;
    const int S = rs_tile_lanes(up), vblocks = (S + RS_NT - 1) / RS_NT;
    const long long per_tile = (long long)S * RS_R;
    const long long tiles = (out_stride + per_tile - 1) / per_tile;
    if ((long long)B * tiles * vblocks > 0x7fffffffLL) return T2V_ERR_ARG;
    const int grid = (int)(B * tiles * vblocks);
    hipStream_t s = (hipStream_t)stream_;
    if (x_is_pcm16)
        k_resample<true><<<grid, RS_NT, 0, s>>>(x, n, x_stride, taps, up, down, half, scale, y, out_stride, (int)tiles, S, vblocks);
    else
        k_resample<false><<<grid, RS_NT, 0, s>>>(x, n, x_stride, taps, up, down, half, 1.f, y, out_stride, (int)tiles, S, vblocks);
    return t2v_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------- trim
__global__ __launch_bounds__(256) void k_trim_ms(const float* __restrict__ y, const int32_t* __restrict__ n_samples, int y_stride,
                                                 int chunks, float* __restrict__ ms, int ms_stride) {
    __shared__ float P[TR_NBLK];                                       // p_{t0 - 2 + k}
    const int b = blockIdx.x / chunks, t0 = (blockIdx.x - b * chunks) * TR_F, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int n = min(max(n_samples[b], 0), y_stride);
    const int frames = n > 0 ? n / TR_HOP + 1 : 0;
    const float* yb = y + (size_t)b * y_stride;
    for (int k = wave; k < TR_NBLK; k += 4) {
        const long long s0 = (long long)(t0 - 2 + k) * TR_HOP;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long g = s0 + 64 * c + lane;
            const float v = g >= 0 && g < n ? yb[g] : 0.f;
            s = fmaf(v, v, s);
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) P[k] = s;
    }
    __syncthreads();
    if (tid < TR_F) {
        const int t = t0 + tid;
        if (t < ms_stride) ms[(size_t)b * ms_stride + t] = t < frames ? (((P[tid] + P[tid + 1]) + P[tid + 2]) + P[tid + 3]) * (1.f / 1024.f) : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_trim_bounds(const float* __restrict__ ms, int ms_stride, const int32_t* __restrict__ n_samples,
                                                     int y_stride, float thr, int pad_frames, int32_t* __restrict__ bounds) {
    __shared__ float RM[4];
    __shared__ int RF[4], RL[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(n_samples[b], 0), y_stride);
    const int frames = n > 0 ? n / TR_HOP + 1 : 0;
    const float* row = ms + (size_t)b * ms_stride;
    float mx = 0.f;
    for (int t = tid; t < frames; t += 256) mx = fmaxf(mx, row[t]);
    mx = wave_max(mx);
    if (lane == 0) RM[wave] = mx;
    __syncthreads();
    const float ref = fmaxf(fmaxf(RM[0], RM[1]), fmaxf(RM[2], RM[3]));
    const float cut = ref * thr;
    int first = 0x7fffffff, last = -1;
    if (ref > 0.f)
        for (int t = tid; t < frames; t += 256)
            if (row[t] > cut) {
                first = min(first, t);
                last = max(last, t);
            }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        first = min(first, __shfl_xor(first, o, 64));
        last = max(last, __shfl_xor(last, o, 64));
    }
    if (lane == 0) {
        RF[wave] = first;
        RL[wave] = last;
    }
    __syncthreads();
    if (tid == 0) {
        first = min(min(RF[0], RF[1]), min(RF[2], RF[3]));
        last = max(max(RL[0], RL[1]), max(RL[2], RL[3]));
        int start = 0, end = n;
        if (last >= 0) {
            start = (int)min((long long)TR_HOP * max(0, first - pad_frames), (long long)n);
            end = (int)min((long long)n, (long long)TR_HOP * ((long long)last + 1 + pad_frames));
        }
        bounds[2 * b] = start;
        bounds[2 * b + 1] = end;
    }
}

extern "C" int t2v_trim_bounds(const float* y, const int32_t* n, int y_stride, int B, float top_db, int pad_frames, float* ms,
                               int ms_stride, int32_t* bounds, void* stream_) {
    if (!y || !n || !ms || !bounds || B < 1 || y_stride < 1) return T2V_ERR_ARG;
    if (!(top_db > 0.f) || pad_frames < 0 || pad_frames > (1 << 20)) return T2V_ERR_DIMS;
    const int frames = y_stride / TR_HOP + 1;
    const int chunks = (frames + TR_F - 1) / TR_F;
    if (ms_stride < frames || (long long)B * chunks > 0x7fffffffLL) return T2V_ERR_ARG;
    hipStream_t s = (hipStream_t)stream_;
    k_trim_ms<<<B * chunks, 256, 0, s>>>(y, n, y_stride, chunks, ms, ms_stride);
    k_trim_bounds<<<B, 256, 0, s>>>(ms, ms_stride, n, y_stride, (float)pow(10.0, -(double)top_db / 10.0), pad_frames, bounds);
    return t2v_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------- crop
template <bool PCM16>
__global__ __launch_bounds__(256) void k_crop_rows(const float* __restrict__ y, int y_stride, const int32_t* __restrict__ bounds,
                                                   void* __restrict__ out_, int out_stride, int tiles, int32_t* __restrict__ stats) {
    const int b = blockIdx.x / tiles, c = (blockIdx.x - b * tiles) * 256 + threadIdx.x;
    const int start = min(max(bounds[2 * b], 0), y_stride), end = min(max(bounds[2 * b + 1], start), y_stride);
    const bool in = c < end - start;
    const float v = in ? y[(size_t)b * y_stride + start + c] : 0.f;
    if (PCM16) {
        const float r = rintf(v * 32768.f);
        const bool clip = r > 32767.f || r < -32768.f;                 // a NaN is not counted and is written as 0
        if (c < out_stride) ((int16_t*)out_)[(size_t)b * out_stride + c] = (int16_t)(r == r ? fminf(fmaxf(r, -32768.f), 32767.f) : 0.f);
        if (stats) {
            const unsigned long long votes = __ballot(clip);
            float peak = wave_max(fabsf(v));
            if ((threadIdx.x & 63) == 0 && in) {                       // lane 0 is the lowest column: in range if any lane is
                if (votes) atomicAdd(stats + 2 * b, __popcll(votes));
                atomicMax((unsigned*)stats + 2 * b + 1, __float_as_uint(peak));
            }
        }
    } else if (c < out_stride) {
        ((float*)out_)[(size_t)b * out_stride + c] = v;
    }
}

extern "C" int t2v_crop_rows(const float* y, int y_stride, const int32_t* bounds, int B, void* out, int out_is_pcm16, int out_stride,
                             int32_t* stats, void* stream_) {
    if (!y || !bounds || !out || B < 1 || y_stride < 1 || out_stride < 1) return T2V_ERR_ARG;
    // every column a row can hold gets a thread, so the statistics see the whole of [start, end) even when out_stride is short
    const long long tiles = ((long long)max(y_stride, out_stride) + 255) / 256;
    if ((long long)B * tiles > 0x7fffffffLL) return T2V_ERR_ARG;
    hipStream_t s = (hipStream_t)stream_;
    if (stats && !out_is_pcm16) return T2V_ERR_ARG;
    if (stats && hipMemsetAsync(stats, 0, sizeof(int32_t) * 2 * (size_t)B, s) != hipSuccess) return t2v_check_launch();
    if (out_is_pcm16)
        k_crop_rows<true><<<(int)(B * tiles), 256, 0, s>>>(y, y_stride, bounds, out, out_stride, (int)tiles, stats);
    else
        k_crop_rows<false><<<(int)(B * tiles), 256, 0, s>>>(y, y_stride, bounds, out, out_stride, (int)tiles, nullptr);
    return t2v_check_launch();
}
