// Loudness and energy of a ragged batch of waveforms: the K-weighted, gated loudness of ITU-R BS.1770-4 / EBU R 128 and the
// K-weighted level per frame of the front end's grid (t2v_hip.loudness, prepare_corpus.py --lufs, evaluate.py --energy), and
// the in-place row gain that the level normalisation needs.
//
// K-weighting: two cascaded biquads (high shelf, then high pass), in transposed direct form II with the state (s1, s2, t1, t2):
//   y1 = b0 x + s1     s1 <- b1 x - a1 y1 + s2     s2 <- b2 x - a2 y1
//   z  = y1 + t1       t1 <- -2 y1 - d1 z + t2     t2 <- y1 - d2 z
// z is the weighted signal: zero state at sample 0, input 0 past the row's n samples, and z itself counts as 0 outside [0, n).
//
// The recurrence is linear, so a lane can own a chunk (k_loud_filter): one workgroup walks one row in tiles of LD_NT chunks of
// LD_C samples (16 384 samples, staged in LDS with one pad word per chunk so that the lanes' reads, 65 words apart, meet no
// bank twice).  Per tile
//   pass 1  every lane runs its chunk from a zero state and keeps the end state e (4 values);
//   scan    the state at the start of chunk k + 1 is M s_k + e_k with M = A^LD_C, A the zero-input step.  A Hillis-Steele scan
//           over the 64 lanes of a wave (six steps, with M^1, M^2, ..., M^32) gives every lane the state that the chunks of
//           its own wave before it contribute; the state c_w that enters wave w is M^64 c_{w-1} + (total of wave w - 1), from
//           the tile's carry, three steps that every lane does alike; lane l of wave w starts from (exclusive scan) + M^l c_w;
//   pass 2  every lane runs its chunk again from that state and sums z^2 (rounded to fp32) in fp32: z is never stored.
// The powers M^0 .. M^64 are the caller's fp64 table, made from the fp32 coefficients; a lane keeps its M^l in registers for the
// whole row.  Filter state, scan and coefficients are fp64 (below), samples and every sum of squares fp32.
// A chunk's sum is cut where a 100 ms hop boundary falls inside it (at most one does: a hop is >= 800 samples), into the part
// before (A) and behind (B) the boundary; at rates whose hop is a multiple of 64 (16, 32, 48 kHz) B is empty.  A wave none of
// whose chunks holds a boundary or the row's end runs the loop without the masks.
//
// k_loud_reduce, one workgroup per row, builds everything else from the chunk sums: the frame track
// ms[t] = (((p_{t-2} + p_{t-1}) + p_t) + p_{t+1}) / 1024 with p_k the sum of the four chunks of [256 k, 256 k + 256) (the grid
// of f0.hip and of the trim); the hop sums H_j (the pieces of [j hop, (j + 1) hop) in ascending order), the block powers
// (((H_j + H_{j+1}) + H_{j+2}) + H_{j+3}) / (4 hop) of the complete 400 ms blocks, and the two gates in the power domain:
// absolute, power > 10^((-70 + 0.691) / 10); relative, power > 0.1 (mean power of the absolutely gated blocks).
// Every sum has an order that depends on the position in the row alone and there is no float atomic: a row gives the same
// bits alone, in any batch and at any stride.
#include <math.h>

#include "t2v_common.h"
#include "t2v_kernels.h"

#define LD_C T2V_LOUDNESS_CHUNK                   // samples per lane
#define LD_NT 256                                 // lanes = chunks per tile
#define LD_TILE T2V_LOUDNESS_TILE                 // samples per tile
#define LD_U 8                                    // samples whose reads are issued ahead of their fmas
static_assert(LD_TILE == LD_C * LD_NT && LD_C == 64, "a chunk per lane, a pad word per 64 samples");

// The recurrence runs in fp64.  The high pass has a double pole 0.015 (16 kHz) to 0.005 (48 kHz) from z = 1, and in fp32 the
// rounding of its state comes out amplified about 1 / (1 - r)^1.5 times: after a burst near full scale any fp32 form (direct I,
// II or transposed, measured on the CPU) leaves a floor near -85 dBFS, 0.3 dB of error on a frame at -65 LUFS at 48 kHz.
struct ld_state {
    double s1, s2, t1, t2;
};
struct ld_coef {
    double b0, b1, b2, a1, a2, d1, d2;
};

__device__ __forceinline__ double ld_step(ld_state& s, const ld_coef& c, double x) {
    const double y1 = fma(c.b0, x, s.s1);
    s.s1 = fma(-c.a1, y1, fma(c.b1, x, s.s2));
    s.s2 = fma(-c.a2, y1, c.b2 * x);
    const double z = y1 + s.t1;
    s.t1 = fma(-c.d1, z, fma(-2.0, y1, s.t2));
    s.t2 = fma(-c.d2, z, y1);
    return z;
}

// m (row-major 4 x 4) times v, every row one chain in ascending column
__device__ __forceinline__ ld_state ld_matvec(const double* m, const ld_state& v) {
    ld_state r;
    r.s1 = fma(m[3], v.t2, fma(m[2], v.t1, fma(m[1], v.s2, m[0] * v.s1)));
    r.s2 = fma(m[7], v.t2, fma(m[6], v.t1, fma(m[5], v.s2, m[4] * v.s1)));
    r.t1 = fma(m[11], v.t2, fma(m[10], v.t1, fma(m[9], v.s2, m[8] * v.s1)));
    r.t2 = fma(m[15], v.t2, fma(m[14], v.t1, fma(m[13], v.s2, m[12] * v.s1)));
    return r;
}
__device__ __forceinline__ ld_state ld_add(const ld_state& a, const ld_state& b) {
    ld_state r = {a.s1 + b.s1, a.s2 + b.s2, a.t1 + b.t1, a.t2 + b.t2};
    return r;
}

// table: [0..7) the coefficients b0 b1 b2 a1 a2 d1 d2, [8 + 16 p ..) the matrix M^p, p = 0 .. 64, row-major
#define LD_POW(table, p) ((table) + 8 + 16 * (p))

__global__ __launch_bounds__(LD_NT) void k_loud_filter(const float* __restrict__ y, const int32_t* __restrict__ n_samples,
                                                       int y_stride, const double* __restrict__ table, int hop,
                                                       float* __restrict__ parts, int nch_stride) {
    __shared__ float X[LD_TILE + LD_NT];                               // sample i of the tile at i + i / 64
    __shared__ double TW[4][4];                                        // the waves' totals
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(n_samples[b], 0), y_stride);                 // no length addresses outside the row
    const float* yb = y + (size_t)b * y_stride;
    float* pb = parts + (size_t)b * 2 * nch_stride;
    ld_coef c;
    c.b0 = table[0]; c.b1 = table[1]; c.b2 = table[2]; c.a1 = table[3]; c.a2 = table[4]; c.d1 = table[5]; c.d2 = table[6];
    double ml[16];                                                     // M^lane
#pragma unroll
    for (int i = 0; i < 16; ++i) ml[i] = LD_POW(table, lane)[i];
    ld_state carry = {0.0, 0.0, 0.0, 0.0};                             // the state that enters the tile
    const float* xp = X + tid * (LD_C + 1);

    for (int tile0 = 0; tile0 < n; tile0 += LD_TILE) {
        if (tile0) __syncthreads();                                    // the last tile is read
#pragma unroll 1
        for (int i0 = 0; i0 < LD_TILE; i0 += LD_NT * LD_U) {
            float v[LD_U];
#pragma unroll
            for (int u = 0; u < LD_U; ++u) {
                const int g = tile0 + i0 + u * LD_NT + tid;
                v[u] = g < n ? yb[g] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < LD_U; ++u) {
                const int i = i0 + u * LD_NT + tid;
                X[i + (i >> 6)] = v[u];
            }
        }
        __syncthreads();
        const int first = tile0 + tid * LD_C;                          // this lane's chunk: [first, first + 64)
        const int valid = min(n - first, LD_C);                        // <= 0: a chunk of padding
        // pass 1: the end state from a zero state
        ld_state e = {0.0, 0.0, 0.0, 0.0};
        if (valid > 0)
#pragma unroll 1
            for (int i0 = 0; i0 < LD_C; i0 += LD_U) {
                float v[LD_U];
#pragma unroll
                for (int u = 0; u < LD_U; ++u) v[u] = xp[i0 + u];
#pragma unroll
                for (int u = 0; u < LD_U; ++u) ld_step(e, c, v[u]);
            }
        // inclusive scan over the wave: I_l = sum_{j <= l} M^(l - j) e_j (rolled: a step's matrix is read when it is due)
#pragma unroll 1
        for (int s = 0; s < 6; ++s) {
            const int d = 1 << s;
            ld_state o;
            o.s1 = __shfl_up(e.s1, d, 64); o.s2 = __shfl_up(e.s2, d, 64);
            o.t1 = __shfl_up(e.t1, d, 64); o.t2 = __shfl_up(e.t2, d, 64);
            const ld_state m = ld_matvec(LD_POW(table, d), o);
            if (lane >= d) e = ld_add(e, m);
        }
        if (lane == 63) {
            TW[wave][0] = e.s1; TW[wave][1] = e.s2; TW[wave][2] = e.t1; TW[wave][3] = e.t2;
        }
        ld_state ex;                                                   // exclusive: what the wave's earlier chunks leave here
        ex.s1 = __shfl_up(e.s1, 1, 64); ex.s2 = __shfl_up(e.s2, 1, 64);
        ex.t1 = __shfl_up(e.t1, 1, 64); ex.t2 = __shfl_up(e.t2, 1, 64);
        if (lane == 0) ex.s1 = ex.s2 = ex.t1 = ex.t2 = 0.0;
        __syncthreads();
        ld_state cw = carry, mine = carry;                             // the state that enters wave 0, 1, ..., and the tile's end
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w == wave) mine = cw;
            const ld_state t = {TW[w][0], TW[w][1], TW[w][2], TW[w][3]};
            cw = ld_add(ld_matvec(LD_POW(table, 64), cw), t);
        }
        carry = cw;
        // pass 2: the chunk from its true state, z^2 summed before (A) and behind (B) the hop boundary
        if (valid > 0) {
            ld_state s = ld_add(ex, ld_matvec(ml, mine));
            const int boundary = (first / hop + 1) * hop;              // the first hop boundary above `first`
            const int na = min(boundary - first, LD_C);
            float sa = 0.f, sb = 0.f;
            if (__any(valid < LD_C || na < LD_C)) {
#pragma unroll 1
                for (int i0 = 0; i0 < LD_C; i0 += LD_U) {
                    float v[LD_U];
#pragma unroll
                    for (int u = 0; u < LD_U; ++u) v[u] = xp[i0 + u];
#pragma unroll
                    for (int u = 0; u < LD_U; ++u) {
                        const float z = (float)ld_step(s, c, v[u]);
                        const int i = i0 + u;
                        const bool in = i < valid, a = i < na;
                        sa = in && a ? fmaf(z, z, sa) : sa;
                        sb = in && !a ? fmaf(z, z, sb) : sb;
                    }
                }
            } else {
#pragma unroll 1
                for (int i0 = 0; i0 < LD_C; i0 += LD_U) {
                    float v[LD_U];
#pragma unroll
                    for (int u = 0; u < LD_U; ++u) v[u] = xp[i0 + u];
#pragma unroll
                    for (int u = 0; u < LD_U; ++u) {
                        const float z = (float)ld_step(s, c, v[u]);
                        sa = fmaf(z, z, sa);
                    }
                }
            }
            const int k = first / LD_C;                                // < ceil(n / 64) <= nch_stride
            pb[2 * k] = sa;
            pb[2 * k + 1] = sb;
        }
    }
}

// fixed-order sums and maxima over the workgroup: a xor butterfly in every wave, then the four waves in order
__device__ __forceinline__ float ld_wg_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                                   // red is free again
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float ld_wg_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void k_loud_reduce(const float* __restrict__ parts, int nch_stride,
                                                     const int32_t* __restrict__ n_samples, int y_stride, int hop, float abs_gate,
                                                     float* __restrict__ hsum, int nh_stride, float* __restrict__ ms, int ms_stride,
                                                     float* __restrict__ block_pw, int blk_stride, int32_t* __restrict__ rows) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(n_samples[b], 0), y_stride);
    const int nch = (n + LD_C - 1) / LD_C;
    const int frames = n > 0 ? n / 256 + 1 : 0;
    const int nb = n >= 4 * hop ? (n - 4 * hop) / hop + 1 : 0;         // complete blocks
    const int nseg = nb ? nb + 3 : 0;                                  // hops under them: floor(n / hop) <= nh_stride
    const float* pb = parts + (size_t)b * 2 * nch_stride;
    float* hb = hsum + (size_t)b * nh_stride;
    float* bp = block_pw + (size_t)b * blk_stride;

    // the frame track
    for (int t = tid; t < ms_stride; t += 256) {
        float v = 0.f;
        if (t < frames) {
            float p[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k0 = 4 * (t - 2 + q);                        // chunks of [256 (t - 2 + q), + 256)
                float c[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + u;
                    c[u] = k >= 0 && k < nch ? pb[2 * k] + pb[2 * k + 1] : 0.f;
                }
                p[q] = ((c[0] + c[1]) + c[2]) + c[3];
            }
            v = (((p[0] + p[1]) + p[2]) + p[3]) * (1.f / 1024.f);
        }
        ms[(size_t)b * ms_stride + t] = v;
    }
    // the ungated mean square
    float all = 0.f;
    for (int k = tid; k < nch; k += 256) all += pb[2 * k] + pb[2 * k + 1];
    all = ld_wg_sum(all, red);
    // hop sums: the pieces of [j hop, (j + 1) hop) in ascending order
    for (int j = tid; j < nseg; j += 256) {
        const int lo = j * hop, hi = lo + hop;                         // hi <= n
        const int kf = lo / LD_C, kl = (hi - 1) / LD_C;
        float s = 0.f;
        for (int k = kf; k <= kl; ++k) s += (k * LD_C) / hop == j ? pb[2 * k] : pb[2 * k + 1];
        hb[j] = s;
    }
    __syncthreads();                                                   // the hop sums of the other lanes
    // block powers, the absolute gate
    const float inv_blk = 1.f / (4.f * (float)hop);
    float s_abs = 0.f, n_abs = 0.f, mx = 0.f;
    for (int j = tid; j < blk_stride; j += 256) {
        float v = 0.f;
        if (j < nb) {
            v = (((hb[j] + hb[j + 1]) + hb[j + 2]) + hb[j + 3]) * inv_blk;
            mx = fmaxf(mx, v);
            if (v > abs_gate) {
                s_abs += v;
                n_abs += 1.f;                                          // exact: fewer than 2^24 blocks in 2^30 samples
            }
        }
        bp[j] = v;
    }
    s_abs = ld_wg_sum(s_abs, red);
    n_abs = ld_wg_sum(n_abs, red);
    mx = ld_wg_max(mx, red);
    // the relative gate: 10 LU below the mean of the absolutely gated blocks
    const float rel_gate = n_abs > 0.f ? 0.1f * (s_abs / n_abs) : 0.f;
    float s_g = 0.f, n_g = 0.f;
    for (int j = tid; j < nb; j += 256) {
        const float v = bp[j];                                         // this lane's own store
        if (v > abs_gate && v > rel_gate) {
            s_g += v;
            n_g += 1.f;
        }
    }
    s_g = ld_wg_sum(s_g, red);
    n_g = ld_wg_sum(n_g, red);
    if (tid == 0) {
        int32_t* r = rows + 8 * b;
        r[0] = __float_as_int(s_g);
        r[1] = __float_as_int(n > 0 ? all / (float)n : 0.f);
        r[2] = __float_as_int(mx);
        r[3] = (int)n_g;
        r[4] = nb;
        r[5] = r[6] = r[7] = 0;
    }
}

static bool ld_rate_ok(int hop) { return hop >= 800 && hop <= 4800; }  // 100 ms at 8 .. 48 kHz

extern "C" size_t t2v_loudness_scratch_bytes(int B, int y_stride, int hop) {
    if (B < 1 || y_stride < 1 || y_stride > (1 << 30) || !ld_rate_ok(hop)) return 0;
    const size_t nch = ((size_t)y_stride + LD_C - 1) / LD_C, nh = (size_t)y_stride / hop + 1;
    return sizeof(float) * (size_t)B * (2 * nch + nh);
}

extern "C" int t2v_loudness(const float* y, const int32_t* n, int y_stride, int B, const double* table, int hop, float* frame_ms,
                            int ms_stride, float* block_pw, int blk_stride, int32_t* rows, void* scratch, void* stream_) {
    if (!y || !n || !table || !frame_ms || !block_pw || !rows || !scratch || B < 1 || y_stride < 1 || y_stride > (1 << 30))
        return T2V_ERR_ARG;
    if (!ld_rate_ok(hop)) return T2V_ERR_DIMS;
    const int nb_max = y_stride >= 4 * hop ? (y_stride - 4 * hop) / hop + 1 : 0;
    if (ms_stride < y_stride / 256 + 1 || blk_stride < 1 || blk_stride < nb_max) return T2V_ERR_ARG;
    const int nch = (y_stride + LD_C - 1) / LD_C, nh = y_stride / hop + 1;
    float* parts = (float*)scratch;
    float* hsum = parts + (size_t)B * 2 * nch;
    const float abs_gate = (float)pow(10.0, (-70.0 + 0.691) / 10.0);
    hipStream_t s = (hipStream_t)stream_;
    k_loud_filter<<<B, LD_NT, 0, s>>>(y, n, y_stride, table, hop, parts, nch);
    k_loud_reduce<<<B, 256, 0, s>>>(parts, nch, n, y_stride, hop, abs_gate, hsum, nh, frame_ms, ms_stride, block_pw, blk_stride,
                                    rows);
    return t2v_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------- gain
__global__ __launch_bounds__(256) void k_scale_rows(float* __restrict__ y, const int32_t* __restrict__ n_samples, int y_stride,
                                                    const float* __restrict__ gains, int tiles) {
    const int b = blockIdx.x / tiles, c = (blockIdx.x - b * tiles) * 256 + threadIdx.x;
    const int n = min(max(n_samples[b], 0), y_stride);
    if (c < n) y[(size_t)b * y_stride + c] *= gains[b];
}

extern "C" int t2v_scale_rows(float* y, const int32_t* n, int y_stride, int B, const float* gains, void* stream_) {
    if (!y || !n || !gains || B < 1 || y_stride < 1) return T2V_ERR_ARG;
    const long long tiles = ((long long)y_stride + 255) / 256;
    if ((long long)B * tiles > 0x7fffffffLL) return T2V_ERR_ARG;
    k_scale_rows<<<(int)(B * tiles), 256, 0, (hipStream_t)stream_>>>(y, n, y_stride, gains, (int)tiles);
    return t2v_check_launch();
}
