// Time-scale modification of a ragged batch of polar spectrograms: the phase vocoder behind t2v_hip.time_stretch and
// pitch_shift, and the magnitude-only stretch of the synthesis path (GriffinLimVocoder(speed=, pitch=)).
//
// mag, phase: (B, 513, t_stride) as t2v_stft_polar writes them (time contiguous), row b of n[b] frames.  The rate is num / den;
// row b gets n_out[b] = ceil(n[b] den / num) output frames.  For output frame j
//   i = (j num) / den,  a = ((j num) % den) / den                      integers, so every precision agrees on i
//   mag_out[j, k]   = (1 - a) mag[i, k] + a mag[i + 1, k]              frame i + 1 == n[b] counts as magnitude 0
//   phase_out[j, k] = phase[0, k] + sum_{j' < j} d[j', k]              d = wrap(phase[i' + 1] - phase[i'] - pi k / 2) + pi k / 2
// (librosa.effects.time_stretch with exact positions); past the end d is the expected advance pi k / 2 alone.
//
// The sum is an exclusive prefix sum along the contiguous axis (k_pv_scan): one wave owns one (b, k) row and walks it in chunks
// of 64 output frames, a Hillis-Steele scan over the lanes per chunk and one carry between chunks.  What is summed is not
// radians.  Only the phase modulo 2 pi reaches the inverse transform, and modulo a turn wrap(x - e) + e = x, so a term is
// phase[i + 1] - phase[i] as a 32-bit fixed-point fraction of a turn: round(p 2^32 / 2 pi), made in fp64 from the fp32 input
// (at most 2^-33 turn off per conversion), subtracted and added as uint32, where the wrap is the overflow.  The expected
// advance is (k mod 4) quarter turns, (k & 3) << 30.  Integer addition is associative: a row gives the same bits alone, in any
// batch, at any stride and for any chunking, and the error of output j is at most 2 (j + 1) conversions, far inside the
// fp32 figure a float accumulator would need.  The accumulator goes back to radians in [-pi, pi) with one fp32 rounding.
//
// phase_lock (identity phase locking, feed-forward): k_pv_scan leaves the accumulators, still fixed point, in the caller's
// scratch, and k_pv_lock writes phase_out.  Peaks are the bins of ANALYSIS frame i with mag[i, k] > mag[i, k +-1], mag[i, k +-2]
// (neighbours outside 0..512 are not compared), so the decision reads exact inputs.  A peak keeps its accumulator; any other
// bin takes that of its nearest peak kp (a tie goes to the lower one) plus phase[i, k] - phase[i, kp]; a frame without a peak
// is left as it is.  The accumulators are never locked, so the scan stays a scan.  A workgroup takes 64 output frames (the
// lanes, contiguous in memory) and all 513 bins, in eight chunks of 65 bins, a wave each: a walk up the chunk finds the peaks
// and the last peak at or below every bin (a byte in LDS: its offset in the chunk), the waves exchange their chunks' first and last peaks, and a walk
// down finds the next peak at or above, picks the nearer and writes.
//
// Nothing at or past frame n[b] of a row is read, and both outputs are +0 from n_out[b] to out_stride.
#include <math.h>

#include "t2v_common.h"
#include "t2v_kernels.h"

#define PV_BINS T2V_TSM_BINS
#define PV_ROWS 4                                  // k_pv_scan: (b, k) rows, a wave each, per workgroup
#define PV_LW 8                                    // k_pv_lock: waves, a chunk of bins each
#define PV_LC 65                                   // bins per chunk
static_assert(PV_LW * PV_LC >= PV_BINS && (PV_LW - 1) * PV_LC < PV_BINS, "every wave has a chunk, the chunks cover the bins");
static_assert(PV_LC <= 127, "a peak's offset in its chunk is stored in an int8");

#define PV_TURN 6.283185307179586476925286766559

// radians -> 32-bit fraction of a turn (the conversion saturates far outside any phase; the cut to 32 bits is the wrap)
__device__ __forceinline__ uint32_t pv_turns(float p) { return (uint32_t)__double2ll_rn((double)p * (4294967296.0 / PV_TURN)); }
// fraction of a turn -> radians in [-pi, pi), one fp32 rounding
__device__ __forceinline__ float pv_radians(uint32_t t) { return (float)((double)(int32_t)t * (PV_TURN / 4294967296.0)); }

__device__ __forceinline__ int pv_out_frames(int n, int num, int den, int out_stride) {
    return min((int)(((unsigned)n * (unsigned)den + (unsigned)num - 1u) / (unsigned)num), out_stride);   // n den < 2^30
}

// PHASE: the scan runs (else magnitudes only); LOCK: the accumulators go to `acc` as they are, for k_pv_lock
template <bool PHASE, bool LOCK>
__global__ __launch_bounds__(64 * PV_ROWS) void k_pv_scan(const float* __restrict__ mag, const float* __restrict__ phase,
                                                          const int32_t* __restrict__ n_frames, int T, int t_stride, int num, int den,
                                                          double inv_den, float* __restrict__ mag_out, float* __restrict__ phase_out,
                                                          uint32_t* __restrict__ acc, int out_stride, int rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * PV_ROWS + (threadIdx.x >> 6);
    if (row >= rows) return;                                           // the whole wave
    const int b = row / PV_BINS, k = row - b * PV_BINS;
    const int n = min(max(n_frames[b], 0), T);                         // no count addresses outside the row
    const int n_out = pv_out_frames(n, num, den, out_stride);
    const float* mr = mag + (size_t)row * t_stride;
    const float* pr = PHASE ? phase + (size_t)row * t_stride : nullptr;
    const size_t o0 = (size_t)row * out_stride;
    const uint32_t expect = (uint32_t)(k & 3) << 30;                   // pi k / 2 in turns
    uint32_t carry = 0;
    if (PHASE && n > 0) carry = pv_turns(pr[0]);
    for (int j0 = 0; j0 < out_stride; j0 += 64) {
        const int j = j0 + lane;
        float m = 0.f;
        uint32_t d = 0;
        if (j < n_out) {
            const unsigned p = (unsigned)j * (unsigned)num;            // < n den < 2^30
            const int i = (int)(p / (unsigned)den), r = (int)(p - (unsigned)i * (unsigned)den);
            const bool end = i + 1 >= n;
            const float m0 = mr[i], m1 = end ? 0.f : mr[i + 1];
            const float a = (float)((double)r * inv_den), w0 = (float)((double)(den - r) * inv_den);
            m = fmaf(a, m1, w0 * m0);
            if (PHASE) d = end ? expect : pv_turns(pr[i + 1]) - pv_turns(pr[i]);
        }
        if (j < out_stride) mag_out[o0 + j] = m;
        if (PHASE) {
            uint32_t mine = 0;
            if (j0 < n_out) {                                          // the whole wave
                uint32_t s = d;                                        // inclusive scan over the lanes
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t v = __shfl_up(s, o, 64);
                    if (lane >= o) s += v;
                }
                mine = carry + (s - d);
                carry += __shfl(s, 63, 64);
            }
            if (j < out_stride) {
                if (LOCK)
                    acc[o0 + j] = mine;
                else
                    phase_out[o0 + j] = j < n_out ? pv_radians(mine) : 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(64 * PV_LW) void k_pv_lock(const float* __restrict__ mag, const float* __restrict__ phase,
                                                        const int32_t* __restrict__ n_frames, int T, int t_stride, int num, int den,
                                                        const uint32_t* __restrict__ acc, float* __restrict__ phase_out,
                                                        int out_stride) {
    __shared__ int8_t LO[PV_LW * PV_LC][64];                           // the chunk's last peak at or below bin k of lane's frame, as
                                                                       // its offset in the chunk; -1: none yet
    __shared__ int16_t TAIL[PV_LW][64], HEAD[PV_LW][64];               // a chunk's last and first peak
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.y, j = blockIdx.x * 64 + lane;
    const int n = min(max(n_frames[b], 0), T);
    const int n_out = pv_out_frames(n, num, den, out_stride);
    const bool live = j < n_out;
    const int i = live ? (int)((unsigned)j * (unsigned)num / (unsigned)den) : 0;          // <= n - 1
    const int k0 = w * PV_LC, k1 = min(k0 + PV_LC, PV_BINS);
    const float* mb = mag + (size_t)b * PV_BINS * t_stride + i;
    const float* pb = phase + (size_t)b * PV_BINS * t_stride + i;
    int last = -1, first = -1;
    if (live) {
        // a bin that does not exist loses every comparison
        float m2 = k0 >= 2 ? mb[(size_t)(k0 - 2) * t_stride] : -INFINITY, m1 = k0 >= 1 ? mb[(size_t)(k0 - 1) * t_stride] : -INFINITY;
        float c = mb[(size_t)k0 * t_stride], p1 = k0 + 1 < PV_BINS ? mb[(size_t)(k0 + 1) * t_stride] : -INFINITY;
        for (int k = k0; k < k1; ++k) {
            const float p2 = k + 2 < PV_BINS ? mb[(size_t)(k + 2) * t_stride] : -INFINITY;
            if (c > m2 && c > m1 && c > p1 && c > p2) {
                last = k;
                if (first < 0) first = k;
            }
            LO[k][lane] = (int8_t)(last < 0 ? -1 : last - k0);
            m2 = m1; m1 = c; c = p1; p1 = p2;
        }
    }
    TAIL[w][lane] = (int16_t)last;
    HEAD[w][lane] = (int16_t)first;
    __syncthreads();
    int below = -1, hi = -1;                                           // the nearest peaks in the chunks under and over this one
    for (int v = 0; v < w; ++v)
        if (TAIL[v][lane] >= 0) below = TAIL[v][lane];
    for (int v = PV_LW - 1; v > w; --v)
        if (HEAD[v][lane] >= 0) hi = HEAD[v][lane];
    if (j >= out_stride) return;
    const size_t ob = (size_t)b * PV_BINS * out_stride + j;
    for (int k = k1 - 1; k >= k0; --k) {
        float out = 0.f;
        if (live) {
            const int l = LO[k][lane];
            const int lo = l < 0 ? below : k0 + l;
            if (lo == k) hi = k;
            const int kp = lo < 0 ? hi : hi < 0 ? lo : (k - lo <= hi - k ? lo : hi);
            uint32_t v = acc[ob + (size_t)k * out_stride];
            if (kp >= 0 && kp != k)
                v = acc[ob + (size_t)kp * out_stride] + (pv_turns(pb[(size_t)k * t_stride]) - pv_turns(pb[(size_t)kp * t_stride]));
            out = pv_radians(v);
        }
        phase_out[ob + (size_t)k * out_stride] = out;
    }
}

static bool pv_sizes_ok(int B, int T, int out_stride) {
    return B >= 1 && T >= 1 && T <= T2V_TSM_MAX_FRAMES && out_stride >= 1 && out_stride <= (1 << 30) &&
           (long long)B * PV_BINS <= 0x7fffffffLL - PV_ROWS;
}

extern "C" size_t t2v_phase_vocoder_scratch_bytes(int B, int out_stride, int phase_lock) {
    if (B < 1 || out_stride < 1 || out_stride > (1 << 30) || !phase_lock) return 0;
    return sizeof(uint32_t) * (size_t)B * PV_BINS * (size_t)out_stride;
}

extern "C" int t2v_phase_vocoder(const float* mag, const float* phase, const int32_t* n_frames, int B, int T, int t_stride, int num,
                                 int den, int phase_lock, float* mag_out, float* phase_out, int out_stride, void* scratch,
                                 void* stream_) {
    if (!mag || !n_frames || !mag_out || (phase == nullptr) != (phase_out == nullptr)) return T2V_ERR_ARG;
    if (num < 1 || num > T2V_TSM_MAX_RATIO || den < 1 || den > T2V_TSM_MAX_RATIO) return T2V_ERR_DIMS;
    if (!pv_sizes_ok(B, T, out_stride) || t_stride < T) return T2V_ERR_ARG;
    if ((long long)out_stride < ((long long)T * den + num - 1) / num) return T2V_ERR_ARG;
    const bool lock = phase && phase_lock;
    if (lock && (!scratch || B > 65535)) return T2V_ERR_ARG;          // k_pv_lock has the batch in grid.y
    hipStream_t s = (hipStream_t)stream_;
    const int rows = B * PV_BINS, blocks = (rows + PV_ROWS - 1) / PV_ROWS;
    const double inv_den = 1.0 / (double)den;
    uint32_t* acc = (uint32_t*)scratch;
    if (!phase)
        k_pv_scan<false, false><<<blocks, 64 * PV_ROWS, 0, s>>>(mag, nullptr, n_frames, T, t_stride, num, den, inv_den, mag_out,
                                                                nullptr, nullptr, out_stride, rows);
    else if (!lock)
        k_pv_scan<true, false><<<blocks, 64 * PV_ROWS, 0, s>>>(mag, phase, n_frames, T, t_stride, num, den, inv_den, mag_out,
                                                               phase_out, nullptr, out_stride, rows);
    else {
        k_pv_scan<true, true><<<blocks, 64 * PV_ROWS, 0, s>>>(mag, phase, n_frames, T, t_stride, num, den, inv_den, mag_out,
                                                              phase_out, acc, out_stride, rows);
        k_pv_lock<<<dim3((out_stride + 63) / 64, B), 64 * PV_LW, 0, s>>>(mag, phase, n_frames, T, t_stride, num, den, acc, phase_out,
                                                                        out_stride);
    }
    return t2v_check_launch();
}
