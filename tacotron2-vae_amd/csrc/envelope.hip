// Spectral envelope of STFT magnitudes and the warp of a spectrum's envelope: the primitive behind t2v_hip.spectral_envelope,
// warp_envelope, formant_shift and pitch_shift(preserve_formants=True).  The definition is in include/t2vae.h.
//
// mag: (B, 513, t_stride) as t2v_stft_polar writes it (time contiguous), row b of n[b] frames.  Per frame, with
// floor = max(1e-7 max_k m[k], 1e-10) and L[k] = log(max(m[k], floor)):
//   lifter(x) = Re DFT1024(keep(DFT1024(even extension of x) / 1024))     keep: cepstral bins n <= order and n >= 1024 - order
//   A = L;  iters + 1 times:  E = lifter(A), A = max(L, E)                the true envelope of Roebel and Rodet, a fixed count
//   Ew[k] = (1 - a) E[i] + a E[i + 1],  i = (k p) / q,  a = ((k p) % q) / q   integers; i >= 512 reads E[512]
//   mag_out[k] = m[k] exp(Ew[k] - E[k])                                    p == q: m[k] itself
//
// One launch, k_spectral_envelope.  A workgroup owns ENV_W consecutive frames of one row, a wave per frame.  The layout has
// time contiguous, so a frame's 513 bins are 513 separate sectors: the workgroup stages the (513 x ENV_W) tile through LDS,
// global reads and writes running along T, and each wave works on its own column, repacked bin-contiguous (row pitch ENV_LD:
// the transposing accesses of a wave fall on distinct banks).  A frame's state is its own: L and m sit in registers (bins
// lane + 64 r, and bin 512 in every lane), the sequence on its way into a transform in the wave's row of S, the transform in
// the wave's 512 complex points of Z.  Both transforms of a lifter are the forward real 1024-point FFT of a real even sequence:
// the packed 512-point Stockham FFT of t2v_fft.h and the real-spectrum split, imaginary parts dropped.  The twiddles are made
// in LDS by each workgroup (fp64 sincospi, rounded once), so the call needs no table and no scratch.  No wave reads another's
// frame: a frame's bits depend on that frame alone.  The transforms run on L less the frame's mean (see the kernel): the
// lifter passes a constant through, and sums of a few units round finer than sums around the log spectrum's offset.
//
// Nothing at or past frame n[b] of a row is read, and the outputs are +0 from n[b] to out_stride.
#include <math.h>

#include "t2v_common.h"
#include "t2v_kernels.h"
#include "t2v_fft.h"

#define ENV_BINS T2V_ENV_BINS
#define ENV_W 8                                    // frames, a wave each, per workgroup
#define ENV_LD 516                                 // floats per frame in LDS.  A 4-byte LDS access is served in groups of 32 lanes
                                                   // over 32 banks; in the staging a group is 8 frames x 4 bins at words
                                                   // 516 f + k: 516 mod 32 = 4 puts them on 32 different banks
static_assert(ENV_LD >= ENV_BINS && ENV_LD % 32 == 32 / ENV_W, "the staging transposes without bank conflicts");
static_assert(ENV_W * ENV_LD * sizeof(float) <= ENV_W * 512 * sizeof(c32), "the staging tile fits in the FFT workspace");

// log of a normal x > 0 to within an ulp of the result at any size: x = m 2^e with m in [sqrt(1/2), sqrt(2)), and
// e ln 2 + log m with ln 2 in two parts, the upper of 9 bits so that its product with e is exact.  logf alone was 1.7 ulp
// off at the floor's own logarithm, -23.03, the value of every bin of a silent frame.
__device__ __forceinline__ float env_log(float x) {
    int e;
    float m = frexpf(x, &e);                       // [0.5, 1)
    if (m < 0.70710678f) {
        m *= 2.f;
        e -= 1;
    }
    const float fe = (float)e;
    return fmaf(fe, 0.693359375f, fmaf(fe, -2.12194440e-4f, logf(m)));
}

__global__ __launch_bounds__(64 * ENV_W) void k_spectral_envelope(const float* __restrict__ mag, const int32_t* __restrict__ n_frames,
                                                                  int T, int t_stride, int order, int iters, int p, int q,
                                                                  double inv_q, float* __restrict__ log_env_out,
                                                                  float* __restrict__ mag_out, int out_stride, int tiles) {
    __shared__ c32 Z[ENV_W][512];                  // a wave's FFT workspace; before and after the transforms, the magnitude tile
    __shared__ float S[ENV_W][ENV_LD];             // a wave's real sequence, less the frame's mean mu: A, the cepstrum, E
    __shared__ float MU[ENV_W];
    __shared__ c32 TW512[512], TW1024[257];        // exp(-2 pi i k / 512), exp(-2 pi i k / 1024)
    float (*M)[ENV_LD] = (float (*)[ENV_LD])&Z[0][0];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * ENV_W;
    const int n = min(max(n_frames[b], 0), T);     // no count addresses outside the row
    const size_t row0 = (size_t)b * ENV_BINS;
    if (t0 < n) {                                  // the whole workgroup
        for (int i = tid; i < 512 + 257; i += 64 * ENV_W) {
            double sn, cs;
            if (i < 512) {
                sincospi((double)i * (1.0 / 256.0), &sn, &cs);
                TW512[i] = {(float)cs, (float)-sn};
            } else {
                sincospi((double)(i - 512) * (1.0 / 512.0), &sn, &cs);
                TW1024[i - 512] = {(float)cs, (float)-sn};
            }
        }
        for (int i = tid; i < ENV_BINS * ENV_W; i += 64 * ENV_W) {
            const int f = i % ENV_W, k = i / ENV_W, t = t0 + f;
            M[f][k] = t < n ? mag[(row0 + k) * t_stride + t] : 0.f;
        }
        __syncthreads();
        float m[8], L[8], E[8];
        float m512 = M[w][512], mx = m512;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            m[r] = M[w][lane + 64 * r];
            mx = fmaxf(mx, m[r]);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        __syncthreads();                           // the tile is in registers: Z is free for the transforms
        const bool warp = mag_out && p != q;
        if (log_env_out || warp) {
            const float floor_ = fmaxf(1e-7f * mx, 1e-10f);
            float* s = S[w];
            float L512 = env_log(fmaxf(m512, floor_)), sum = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                L[r] = env_log(fmaxf(m[r], floor_));
                sum += L[r];
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);          // a + b on both sides: every lane the same bits
            // The lifter keeps cepstral bin 0, so lifter(x - mu) + mu = lifter(x) for any constant: the transforms run on
            // L - mu, mu the frame's mean log magnitude (a sum in a fixed order), and mu comes back once, at the end.  A log
            // spectrum is an offset of some -10 with a spread of a few units; without this every sum in the transforms
            // rounds at the offset's size.
            const float mu = (sum + L512) * (1.f / ENV_BINS);
            L512 -= mu;
            float E512 = L512;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                L[r] -= mu;
                s[lane + 64 * r] = L[r];
            }
            if (lane == 0) {
                s[512] = L512;
                MU[w] = mu;
            }
            __builtin_amdgcn_wave_barrier();
            for (int it = 0; it <= iters; ++it) {
                even_transform(s, Z[w], TW512, TW1024, order, 1.f / 1024.f, lane);    // the liftered cepstrum
                even_transform(s, Z[w], TW512, TW1024, 512, 1.f, lane);               // E - mu
#pragma unroll
                for (int r = 0; r < 8; ++r) E[r] = s[lane + 64 * r];
                E512 = s[512];
                if (it < iters) {
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int r = 0; r < 8; ++r) s[lane + 64 * r] = fmaxf(L[r], E[r]);
                    if (lane == 0) s[512] = fmaxf(L512, E512);
                    __builtin_amdgcn_wave_barrier();
                }
            }
            if (warp) {
                auto warped = [&](int k, float mk, float ek) {
                    const unsigned pos = (unsigned)k * (unsigned)p;                    // <= 512 * 1023
                    const int i = (int)(pos / (unsigned)q), rem = (int)(pos - (unsigned)i * (unsigned)q);
                    float ew = E512;
                    if (i < 512) {
                        const float a = (float)((double)rem * inv_q), w0 = (float)((double)(q - rem) * inv_q);
                        ew = fmaf(a, s[i + 1], w0 * s[i]);
                    }
                    return mk * expf(ew - ek);                                         // mu cancels in Ew - E
                };
#pragma unroll
                for (int r = 0; r < 8; ++r) m[r] = warped(lane + 64 * r, m[r], E[r]);
                m512 = warped(512, m512, E512);                                        // every lane the same value
            }
        }
        __syncthreads();                           // every wave is through with Z: it takes the magnitudes on their way out
        if (mag_out) {
#pragma unroll
            for (int r = 0; r < 8; ++r) M[w][lane + 64 * r] = m[r];
            if (lane == 0) M[w][512] = m512;
        }
        __syncthreads();
    }
    for (int i = tid; i < ENV_BINS * ENV_W; i += 64 * ENV_W) {
        const int f = i % ENV_W, k = i / ENV_W, t = t0 + f;
        if (t < out_stride) {
            const size_t o = (row0 + k) * out_stride + t;
            if (log_env_out) log_env_out[o] = t < n ? S[f][k] + MU[f] : 0.f;
            if (mag_out) mag_out[o] = t < n ? M[f][k] : 0.f;
        }
    }
}

extern "C" int t2v_spectral_envelope(const float* mag, const int32_t* n_frames, int B, int T, int t_stride, int order, int iters,
                                     int p, int q, float* log_env_out, float* mag_out, int out_stride, void* stream_) {
    if (order < 1 || order > T2V_ENV_MAX_ORDER || iters < 0 || iters > T2V_ENV_MAX_ITERS || p < 1 || p > T2V_TSM_MAX_RATIO ||
        q < 1 || q > T2V_TSM_MAX_RATIO || B < 1 || T < 1 || T > T2V_TSM_MAX_FRAMES)
        return T2V_ERR_DIMS;
    if (!mag || !n_frames || (!log_env_out && !mag_out) || t_stride < T || out_stride < T || t_stride > (1 << 30) ||
        out_stride > (1 << 30))
        return T2V_ERR_ARG;
    const int tiles = (out_stride + ENV_W - 1) / ENV_W;
    if ((long long)B * tiles > 0x7fffffffLL) return T2V_ERR_DIMS;
    k_spectral_envelope<<<B * tiles, 64 * ENV_W, 0, (hipStream_t)stream_>>>(mag, n_frames, T, t_stride, order, iters, p, q,
                                                                          1.0 / (double)q, log_env_out, mag_out, out_stride,
                                                                          tiles);
    return t2v_check_launch();
}
