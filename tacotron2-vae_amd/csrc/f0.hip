// YIN pitch tracker (de Cheveigne & Kawahara 2002, steps 1-5) on the front end's grid: 16 kHz, hop 256, integration window
// W = 1024, for scoring the prosody of free-running synthesis (Synthesizer.evaluate(prosody=True), Synthesizer.pitch).
//
// Measure (row b: y[0..n), every sample index outside [0, n) counts as 0 and is never read; n // 256 + 1 frames):
//   d_t(tau)  = sum_{j=0}^{1023} (x[s+j] - x[s+j+tau])^2,  s = 256 t - 512,  tau = 1..tau_max       (from the differences)
//   d'_t(tau) = d(tau) tau / sum_{k<=tau} d(k), 1 where that sum is 0
//   tau*: the smallest tau in [tau_min, tau_max] with d' < threshold, then downhill while d'(tau+1) < d'(tau); none: unvoiced
//   f0 = 16000 / (tau* + delta), delta the vertex of the parabola through d'(tau*-1 .. tau*+1), clamped to +-1 (0 when a
//   neighbour lies outside 1..tau_max or the parabola is not convex);  aperiodicity = d'(tau*), 1 where unvoiced.
//
// k_f0_yin: B x ceil(frames / 13) workgroups of 256 threads.  A workgroup owns F0_F = 13 consecutive frames of one row.  The
// 256-sample block partial p_k(tau) = sum_{i in [256k, 256k+256)} (x_i - x_{i+tau})^2 serves four frames:
// d_t = ((p_{t-2} + p_{t-1}) + p_t) + p_{t+1}, so 13 frames cost 16 partials instead of 52, and every one of them is this
// workgroup's own: a frame's bits depend on (t, tau) alone, never on the batch or on a neighbouring workgroup.
//   phase 1: the samples [256 (t0-2), 256 (t0+14) + lags) go to LDS, zeros outside [0, n).
//   phase 2: work units (block k, group of 128 lags), dealt round-robin to the 4 waves.  Lane l owns the lags 128 g + 2l and
//            + 1 as one packed pair: per 8 samples, two broadcast 16-byte reads of x[j..j+7] and four 8-byte reads that slide
//            x[j+tau..] along (9 values serve 16 differences), then 8 packed subtracts and 8 packed fmas on two accumulator
//            chains (even / odd j, added at the end).  The partials go to LDS.
//   phase 3: one wave per frame: lane l adds the four partials of the lags 7l+1..7l+7, the running sum of d is a serial sum
//            in the lane on top of a shuffle scan of the lane totals, d' goes to LDS, the first lag under the threshold is a
//            wave minimum, the descent and the parabola are uniform.  Plain vector stores write f0 and the aperiodicity.
#include "t2v_common.h"
#include "t2v_kernels.h"

#define F0_HOP 256
#define F0_W 1024
#define F0_F 13                                   // frames per workgroup
#define F0_NBLK (F0_F + 3)                        // block partials per workgroup
#define F0_NT 256
#define F0_NW (F0_NT / 64)
#define F0_LG 128                                 // lags per work unit: 64 lanes x 2
#define F0_NG_MAX ((T2V_F0_MAX_LAG + F0_LG) / F0_LG)             // groups that cover the lags 0..T2V_F0_MAX_LAG
#define F0_XLEN (F0_NBLK * F0_HOP + F0_NG_MAX * F0_LG + 8)      // samples in LDS: the blocks, the largest lag, the sliding read
#define F0_LP ((T2V_F0_MAX_LAG + 4) / 4 * 4)      // lag stride of a row of partials
#define F0_CH 7                                   // lags per lane in phase 3
static_assert(64 * F0_CH >= T2V_F0_MAX_LAG, "phase 3: one wave covers every lag");
static_assert(F0_LP >= T2V_F0_MAX_LAG + 2, "a lane stores the pair (tau0, tau0 + 1) with tau0 <= tau_max");
static_assert(4 * (F0_XLEN + (F0_NBLK + F0_NW) * F0_LP) <= 65536, "static LDS");

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(F0_NT) void k_f0_yin(const float* __restrict__ y, const int32_t* __restrict__ n_samples, int y_stride,
                                                  int chunks, int tau_min, int tau_max, float threshold,
                                                  float* __restrict__ f0, float* __restrict__ aper, int out_stride) {
    __shared__ __attribute__((aligned(16))) float X[F0_XLEN];          // x[w0 + i]
    __shared__ __attribute__((aligned(16))) float P[F0_NBLK * F0_LP];  // p_{t0-2+k}(tau) at [k][tau]
    __shared__ float DP[F0_NW * F0_LP];                                // d'(tau) of the frame a wave works on
    const int b = blockIdx.x / chunks, t0 = (blockIdx.x - b * chunks) * F0_F, tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = min(max(n_samples[b], 0), y_stride);                 // no length addresses outside the row
    const int frames = n > 0 ? n / F0_HOP + 1 : 0;
    const int t_end = min(y_stride / F0_HOP + 1, t0 + F0_F);           // frames past the row's own are padding: 0 / 1
    const int nf = min(frames - t0, F0_F);                             // frames of this workgroup that exist
    float* f0_row = f0 + (size_t)b * out_stride;
    float* ap_row = aper + (size_t)b * out_stride;
    for (int t = t0 + max(nf, 0) + tid; t < t_end; t += F0_NT) {
        f0_row[t] = 0.f;
        ap_row[t] = 1.f;
    }
    if (nf <= 0) return;

    const int ng = (tau_max + F0_LG) / F0_LG;                          // lag groups: lags 0..tau_max
    const int nblk = nf + 3;
    {   // phase 1
        const float* yb = y + (size_t)b * y_stride;
        const int w0 = (t0 - 2) * F0_HOP, len = nblk * F0_HOP + ng * F0_LG + 8;
        for (int i = tid; i < len; i += F0_NT) {
            const int g = w0 + i;
            X[i] = g >= 0 && g < n ? yb[g] : 0.f;
        }
    }
    __syncthreads();

    // phase 2
    for (int u = wave; u < nblk * ng; u += F0_NW) {
        const int k = u / ng, g = u - k * ng;
        const int tau0 = g * F0_LG + 2 * lane;
        const float* xa = X + k * F0_HOP;                              // x[256 k' + j], the same address in every lane
        const float* xb = xa + tau0;                                   // x[256 k' + j + tau0]: 8-byte aligned, 64 lanes on 64 banks
        f2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
        f2 w01 = *(const f2*)xb;
#pragma unroll 2
        for (int j = 0; j < F0_HOP; j += 8) {
            const f4 a0 = *(const f4*)(xa + j), a1 = *(const f4*)(xa + j + 4);
            const f2 w23 = *(const f2*)(xb + j + 2), w45 = *(const f2*)(xb + j + 4), w67 = *(const f2*)(xb + j + 6),
                     w89 = *(const f2*)(xb + j + 8);
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float w[9] = {w01.x, w01.y, w23.x, w23.y, w45.x, w45.y, w67.x, w67.y, w89.x};
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                const f2 e0 = f2{a[q], a[q]} - f2{w[q], w[q + 1]};
                const f2 e1 = f2{a[q + 1], a[q + 1]} - f2{w[q + 1], w[q + 2]};
                acc0 = __builtin_elementwise_fma(e0, e0, acc0);
                acc1 = __builtin_elementwise_fma(e1, e1, acc1);
            }
            w01 = w89;
        }
        if (tau0 <= tau_max) *(f2*)(P + k * F0_LP + tau0) = acc0 + acc1;
    }
    __syncthreads();

    // phase 3
    float* dp = DP + wave * F0_LP;
    for (int i = wave; i < nf; i += F0_NW) {
        const float* p0 = P + i * F0_LP;                               // frame t0 + i: blocks i .. i + 3 of this workgroup
        float d[F0_CH], run[F0_CH], s = 0.f;
#pragma unroll
        for (int c = 0; c < F0_CH; ++c) {
            const int tau = F0_CH * lane + 1 + c;
            d[c] = 0.f;
            if (tau <= tau_max) d[c] = ((p0[tau] + p0[F0_LP + tau]) + p0[2 * F0_LP + tau]) + p0[3 * F0_LP + tau];
            s += d[c];
            run[c] = s;
        }
        float incl = s;                                                // inclusive scan of the lane totals, fixed order
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        float before = __shfl_up(incl, 1, 64);
        if (lane == 0) before = 0.f;
        int first = 0x7fffffff;
#pragma unroll
        for (int c = F0_CH - 1; c >= 0; --c) {
            const int tau = F0_CH * lane + 1 + c;
            const float cum = before + run[c];
            const float v = cum > 0.f ? d[c] * (float)tau / cum : 1.f;
            if (tau <= tau_max) {
                dp[tau] = v;
                if (tau >= tau_min && v < threshold) first = tau;
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float hz = 0.f, ap = 1.f;
        if (first <= tau_max) {
            int tau = __builtin_amdgcn_readfirstlane(first);
            float cur = dp[tau];
            while (tau + 1 <= tau_max) {
                const float nxt = dp[tau + 1];
                if (!(nxt < cur)) break;
                cur = nxt;
                ++tau;
            }
            float delta = 0.f;
            if (tau >= 2 && tau + 1 <= tau_max) {
                const float a = dp[tau - 1], c = dp[tau + 1];
                const float den = a - 2.f * cur + c;
                if (den > 0.f) delta = fminf(fmaxf(0.5f * (a - c) / den, -1.f), 1.f);
            }
            hz = 16000.f / ((float)tau + delta);
            ap = cur;
        }
        if (lane == 0) {
            f0_row[t0 + i] = hz;
            ap_row[t0 + i] = ap;
        }
        __builtin_amdgcn_wave_barrier();                               // dp is rewritten by the wave's next frame
    }
}

extern "C" int t2v_f0_yin(const float* y, const int32_t* n, int y_stride, int B, int tau_min, int tau_max, float threshold,
                          float* f0, float* aperiodicity, int out_stride, void* stream_) {
    if (!y || !n || !f0 || !aperiodicity || B < 1 || y_stride < 1 || out_stride < 1) return T2V_ERR_ARG;
    if (tau_min < 1 || tau_min >= tau_max || tau_max > T2V_F0_MAX_LAG) return T2V_ERR_DIMS;
    const int frames = y_stride / F0_HOP + 1;
    const int chunks = (frames + F0_F - 1) / F0_F;
    if (out_stride < frames || (long long)B * chunks > 0x7fffffffLL) return T2V_ERR_ARG;
    k_f0_yin<<<B * chunks, F0_NT, 0, (hipStream_t)stream_>>>(y, n, y_stride, chunks, tau_min, tau_max, threshold, f0, aperiodicity,
                                                            out_stride);
    return t2v_check_launch();
}
