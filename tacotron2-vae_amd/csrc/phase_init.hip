// A phase for a ragged batch of magnitude spectrograms: single-pass spectrogram inversion (Beauregard, Harish and Wyse 2015),
// the start of Griffin-Lim that t2v_hip.spsi_phase, griffin_lim(init='spsi') and vocoder='spsi' take instead of a random draw.
//
// mag: (B, 513, t_stride) as t2v_stft_polar writes it (time contiguous), row b of n[b] frames.  N = 1024 and hop 256, so a
// partial at bin x advances x / 4 turns per frame.  Every turn quantity is a 32-bit fixed-point fraction of a turn, uint32,
// and wraps (tsm.hip's convention).
//   peak        bin k in 1..511 of frame m with M[k] > M[k - 1] and M[k] > M[k + 1] in fp32: the inputs decide, exactly
//   offset      p = (0.5 (a - c)) / ((a - 2 b) + c) in fp64 from a, b, c = M[k - 1], M[k], M[k + 1], each operation rounded
//               on its own; |p| < 1 / 2 at a peak
//   advance     adv(k, m) = ((k & 3) << 30) + rint(p 2^30) at a peak, 0 elsewhere: (k + p) / 4 turns
//   accumulator acc(k, m) = sum of adv(k, m') over m' <= m                                          (k_spsi_scan)
//   assignment  kp = the peak of frame m nearest to k, the lower one on a tie;                      (k_spsi_assign)
//               turns = acc(kp, m) - ((k - kp) << 31) + rint(p(kp, m) 2^31), phase = the turns as radians in [-pi, pi);
//               a frame without a peak is +0 in every bin
// The last line is -pi (k - kp - p): the project's transform refers a frame's phase to the frame's first sample, and there the
// periodic Hann window's transform has phase -pi d (N - 1) / N across its main lobe, d bins from the partial.
//
// k_spsi_scan is k_pv_scan's scan: one wave owns one (b, k) row and walks it in chunks of 64 frames, a Hillis-Steele scan over
// the lanes per chunk and one carry between chunks; it reads rows k - 1, k, k + 1 along time and leaves the accumulators in the
// caller's scratch.  The sum is an integer sum, so it is associative: a row gives the same bits alone, in any batch, at any
// stride and for any chunking, and the error of frame m is at most m + 1 roundings of 2^-30 of a quarter turn.
// k_spsi_assign is k_pv_lock's walk: a workgroup takes 64 frames (the lanes, contiguous in memory) and all 513 bins in eight
// chunks of 65 bins, a wave each: a walk up the chunk finds the peaks and the last peak at or below every bin (a byte in LDS:
// its offset in the chunk), the waves exchange their chunks' first and last peaks, and a walk down finds the next peak at or
// above, picks the nearer, recomputes its offset from the three magnitudes and writes.
//
// Nothing at or past frame n[b] of a row is read, phase_out is +0 from n[b] to t_stride, and there are no atomics.
#include <math.h>

#include "t2v_common.h"
#include "t2v_kernels.h"

#define SP_BINS T2V_TSM_BINS
#define SP_ROWS 4                                  // k_spsi_scan: (b, k) rows, a wave each, per workgroup
#define SP_LW 8                                    // k_spsi_assign: waves, a chunk of bins each
#define SP_LC 65                                   // bins per chunk
static_assert(SP_LW * SP_LC >= SP_BINS && (SP_LW - 1) * SP_LC < SP_BINS, "every wave has a chunk, the chunks cover the bins");
static_assert(SP_LC <= 127, "a peak's offset in its chunk is stored in an int8");

#define SP_TURN 6.283185307179586476925286766559

// fraction of a turn -> radians in [-pi, pi), one fp32 rounding (tsm.hip's pv_radians)
__device__ __forceinline__ float sp_radians(uint32_t t) { return (float)((double)(int32_t)t * (SP_TURN / 4294967296.0)); }

// the parabola's vertex through a, b, c at -1, 0, 1; every operation rounded on its own
__device__ __forceinline__ double sp_offset(float a, float b, float c) {
#pragma clang fp contract(off)
    const double da = (double)a, db = (double)b, dc = (double)c;
    return (0.5 * (da - dc)) / ((da - 2.0 * db) + dc);
}
// rint(p scale) as wrapping turns; |p| < 1 / 2 at a peak, and the conversion saturates whatever else comes
__device__ __forceinline__ uint32_t sp_fixed(double p, double scale) { return (uint32_t)(int32_t)__double2int_rn(p * scale); }

__global__ __launch_bounds__(64 * SP_ROWS) void k_spsi_scan(const float* __restrict__ mag, const int32_t* __restrict__ n_frames, int T,
                                                            int t_stride, uint32_t* __restrict__ acc, int rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * SP_ROWS + (threadIdx.x >> 6);
    if (row >= rows) return;                                           // the whole wave
    const int b = row / SP_BINS, k = row - b * SP_BINS;
    const int n = min(max(n_frames[b], 0), T);                         // no count addresses outside the row
    const bool inner = k >= 1 && k <= SP_BINS - 2;                     // bins 0 and 512 are never peaks: their rows stay 0
    const float* mr = mag + (size_t)row * t_stride;
    uint32_t* ar = acc + (size_t)row * t_stride;
    const uint32_t expect = (uint32_t)(k & 3) << 30;                   // k / 4 turns
    uint32_t carry = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        uint32_t d = 0;
        if (inner && j < n) {
            const float a = mr[j - t_stride], c0 = mr[j], c = mr[j + t_stride];
            if (c0 > a && c0 > c) d = expect + sp_fixed(sp_offset(a, c0, c), 1073741824.0);
        }
        uint32_t s = d;                                                // inclusive scan over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(s, o, 64);
            if (lane >= o) s += v;
        }
        if (j < n) ar[j] = carry + s;
        carry += __shfl(s, 63, 64);
    }
}

__global__ __launch_bounds__(64 * SP_LW) void k_spsi_assign(const float* __restrict__ mag, const int32_t* __restrict__ n_frames, int T,
                                                            int t_stride, const uint32_t* __restrict__ acc,
                                                            float* __restrict__ phase_out, int chunks) {
    __shared__ int8_t LO[SP_LW * SP_LC][64];                           // the chunk's last peak at or below bin k of lane's frame, as
                                                                       // its offset in the chunk; -1: none yet
    __shared__ int16_t TAIL[SP_LW][64], HEAD[SP_LW][64];               // a chunk's last and first peak
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x / chunks, j = (blockIdx.x - b * chunks) * 64 + lane;
    const int n = min(max(n_frames[b], 0), T);
    const bool live = j < n;
    const int k0 = w * SP_LC, k1 = min(k0 + SP_LC, SP_BINS);
    const size_t ob = (size_t)b * SP_BINS * t_stride + (live ? j : 0);
    const float* mb = mag + ob;
    int last = -1, first = -1;
    if (live) {
        float m1 = k0 >= 1 ? mb[(size_t)(k0 - 1) * t_stride] : 0.f, c = mb[(size_t)k0 * t_stride];
        for (int k = k0; k < k1; ++k) {
            const float p1 = k + 1 < SP_BINS ? mb[(size_t)(k + 1) * t_stride] : 0.f;
            if (k >= 1 && k <= SP_BINS - 2 && c > m1 && c > p1) {
                last = k;
                if (first < 0) first = k;
            }
            LO[k][lane] = (int8_t)(last < 0 ? -1 : last - k0);
            m1 = c; c = p1;
        }
    }
    TAIL[w][lane] = (int16_t)last;
    HEAD[w][lane] = (int16_t)first;
    __syncthreads();
    int below = -1, hi = -1;                                           // the nearest peaks in the chunks under and over this one
    for (int v = 0; v < w; ++v)
        if (TAIL[v][lane] >= 0) below = TAIL[v][lane];
    for (int v = SP_LW - 1; v > w; --v)
        if (HEAD[v][lane] >= 0) hi = HEAD[v][lane];
    if (j >= t_stride) return;
    float* pb = phase_out + (size_t)b * SP_BINS * t_stride + j;
    const uint32_t* ab = acc + ob;
    int kq = -1;                                                       // the peak whose turns `base` holds
    uint32_t base = 0;
    for (int k = k1 - 1; k >= k0; --k) {
        float out = 0.f;
        if (live) {
            const int l = LO[k][lane];
            const int lo = l < 0 ? below : k0 + l;
            if (lo == k) hi = k;
            const int kp = lo < 0 ? hi : hi < 0 ? lo : (k - lo <= hi - k ? lo : hi);     // 1..511, or -1: the frame has no peak
            if (kp >= 0) {
                if (kp != kq) {
                    const float* mp = mb + (size_t)kp * t_stride;
                    base = ab[(size_t)kp * t_stride] + sp_fixed(sp_offset(mp[-t_stride], mp[0], mp[t_stride]), 2147483648.0);
                    kq = kp;
                }
                out = sp_radians(base - ((uint32_t)(k - kp) << 31));
            }
        }
        pb[(size_t)k * t_stride] = out;
    }
}

extern "C" size_t t2v_spsi_scratch_bytes(int B, int t_stride) {
    if (B < 1 || t_stride < 1) return 0;
    return sizeof(uint32_t) * (size_t)B * SP_BINS * (size_t)t_stride;
}

extern "C" int t2v_spsi(const float* mag, const int32_t* n_frames, int B, int T, int t_stride, float* phase_out, void* scratch,
                        void* stream_) {
    if (!mag || !n_frames || !phase_out || !scratch) return T2V_ERR_ARG;
    if (B < 1 || T < 1 || t_stride < T || T > T2V_TSM_MAX_FRAMES || t_stride > (1 << 30)) return T2V_ERR_DIMS;
    const int chunks = (t_stride - 1) / 64 + 1;
    if ((long long)B * SP_BINS > 0x7fffffffLL - SP_ROWS || (long long)B * chunks > 0x7fffffffLL) return T2V_ERR_DIMS;
    hipStream_t s = (hipStream_t)stream_;
    const int rows = B * SP_BINS;
    k_spsi_scan<<<(rows + SP_ROWS - 1) / SP_ROWS, 64 * SP_ROWS, 0, s>>>(mag, n_frames, T, t_stride, (uint32_t*)scratch, rows);
    k_spsi_assign<<<B * chunks, 64 * SP_LW, 0, s>>>(mag, n_frames, T, t_stride, (const uint32_t*)scratch, phase_out, chunks);
    return t2v_check_launch();
}
