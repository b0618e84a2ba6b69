// Voice quality of a ragged batch of 16 kHz waveforms: the spectral-balance descriptors of eGeMAPS (alpha ratio, Hammarberg
// index, spectral slope) and the cepstral peak prominence of Hillenbrand et al., per frame of the front end's grid
// (t2v_hip.voice_quality, evaluate.py --voice).  The definition is in include/t2vae.h.
//
// Frame t of row b covers the samples [256 t - 512, 256 t + 512), 0 outside [0, n[b]) and never read there.  With w the periodic
// Hann window, P[k] = |DFT1024(x w)[k]|^2 for k = 0..512, fl = max(1e-9 max_k P, FLT_MIN) and dB(v) = 10 log10 v:
//   level_db      dB(max(sum_{k=4..319} P, fl))
//   alpha_db      dB(max(sum_{k=64..319} P, fl) / max(sum_{k=4..63} P, fl))
//   hammarberg_db dB(max(max_{k<128} P, fl) / max(max_{k=128..319} P, fl))
//   slope_db_khz  least-squares slope of L[k] = dB(max(P[k], fl)) on 15.625 k / 1000 over k = 32..96: sum (k - 64) L / 357.5
//   c[q]          Re DFT1024(even extension of L)[q] / 1024;  C[q] = 20 log10 max(|c[q]|, 1e-3 max_{16..266} |c|, 1e-4)
//   cpp_db        C[q*] less the least-squares line of C over q = 16..266 at q*, q* the lowest q in 32..266 with the largest C
//   cpp_lag       q*
//
// One launch, k_voice_quality.  A workgroup owns VQ_W consecutive frames of one row, a wave per frame.  Neighbouring frames share
// three quarters of their samples: the 1024 + 256 (VQ_W - 1) samples under the workgroup's frames go to LDS once, read along the
// row, and a wave packs its frame from there (lane l reads the 8 bytes at 256 f + 2 l + 128 r: 64 lanes on 64 different banks).
// With VQ_W = 8 a sample is read from memory 2.9 times less often than frame by frame and the tables below are built once per 8
// frames; the 113 KB of LDS make it one workgroup, 8 waves, per CU (16 frames would read 3.4 times less and need 190 KB).
// Everything behind the staging is the wave's own: the packed 512-point FFT of t2v_fft.h in its 512 complex points of Z, the
// real-spectrum split, and the sequence on its way into and out of the second transform (even_transform, as the spectral
// envelope's lifter) in its row of S.  No wave reads another's row, so the row pitch needs no bank argument like ENV_LD's:
// VQ_LD = 516 holds the 513 bins and keeps the rows 16-byte aligned.  Twiddles and window are made in LDS by the workgroup
// (fp64; rounded once where they are used in fp32): no table, no scratch.  Only the first quadrant of the 1024th roots, 257
// sincospi, is computed; the 512th roots and the window's cosines follow by symmetry.
//
// The first transform runs in fp64, the rest in fp32.  An fp32 FFT is off by about a quarter ulp of the frame's largest bin in
// every bin, and the descriptors read bins 50 to 90 dB under it: the 2 - 5 kHz peak of a row with a DC offset came out 4.6e-5 dB
// off and the slope and the cepstral peak of a 70 Hz 1 / k^2 tone 4.2e-5 dB/kHz and 2.2e-4 dB, at or past four times what numpy's
// own fp32 arithmetic loses on the same rows (tests/voice_ref.py).  Taking the frame's mean out first mended the DC row and
// cost the slope a factor of three.  In fp64 x w is exact and each P[k] is rounded once; L, the cepstrum and every sum are
// fp32: they work on dB values of a few tens, not on a spectrum of nine decades.
//
// A lane holds the bins lane + 64 r.  Every sum is the lane's own terms in ascending r, then the fixed butterfly of wave_sum;
// a maximum is exact in any order, and the arg max breaks ties to the lower index at every step.  The second transform and
// the slope run on L less the frame's mean (c[0] is not used, and sum (k - 64) = 0): sums of a few dB round finer than sums
// around the spectrum's offset.  No float atomics, and nothing a frame computes depends on another frame: a row gives the
// same bits alone, in any batch and at any stride.
#include <math.h>

#include "t2v_common.h"
#include "t2v_kernels.h"
#include "t2v_fft.h"

#define VQ_W T2V_VOICE_FRAMES                      // frames, a wave each, per workgroup
#define VQ_NT (64 * VQ_W)
#define VQ_HOP 256
#define VQ_X (1024 + VQ_HOP * (VQ_W - 1))          // samples under the workgroup's frames
#define VQ_LD 516                                  // floats per frame in S: the 513 bins, rows 16-byte aligned
#define VQ_K_LO 4                                  // 50 Hz in bins of 15.625 Hz; 1, 2 and 5 kHz are the bins 64, 128 and 320, whole
#define VQ_K_HI 320                                // registers of a lane's bins lane + 64 r
#define VQ_S0 32                                   // the slope's band, 500..1500 Hz, and its centre
#define VQ_S1 96
#define VQ_SC 64
#define VQ_Q0 16                                   // the regression's quefrencies, the peak's (60..500 Hz), the centre of the former
#define VQ_QP 32
#define VQ_Q1 266
#define VQ_QC 141
static_assert(VQ_LD >= 513 && VQ_LD % 4 == 0, "a row of S holds bins 0..512");
static_assert(VQ_Q1 < 64 * 5 && VQ_K_HI <= 64 * 5, "the bins lane + 64 r, r < 5, cover the bands and the quefrencies");
static_assert(2 * VQ_SC == VQ_S0 + VQ_S1 && 2 * VQ_QC == VQ_Q0 + VQ_Q1, "centred abscissae");
static_assert(sizeof(float) * (VQ_X + VQ_W * (2048 + VQ_LD) + 1024 + 6 * VQ_W) + 24 * (512 + 257) <= 160 * 1024,
              "the LDS of a CU");

// 10 log10 x of a normal x > 0 to within an ulp or so of the result at any size: x = m 2^e with m in [sqrt(1/2), sqrt(2)), and
// e 10 log10 2 + (10 / ln 10) log m, 10 log10 2 in two parts, the upper of 9 bits so that its product with e is exact
__device__ __forceinline__ float vq_db(float x) {
    int e;
    float m = frexpf(x, &e);                       // [0.5, 1)
    if (m < 0.70710678f) {
        m *= 2.f;
        e -= 1;
    }
    const float fe = (float)e;
    return fmaf(fe, 3.0078125f, fmaf(fe, 2.48745663e-3f, 4.34294482f * logf(m)));
}

// (v, i) of the lane with the largest v, the lowest i among equals, in every lane
__device__ __forceinline__ void vq_argmax(float& v, int& i) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

// exp(-2 pi i m / 1024) for m = 0..1023 from q[k] = exp(-2 pi i k / 1024), k = 0..256: cos and sin of pi - a and of pi + a
__device__ __forceinline__ c64 vq_unit(const c64* q, int m) {
    const int h = m & 511;                         // the angle less a half turn
    const c64 t = q[h <= 256 ? h : 512 - h];
    const c64 u = {h <= 256 ? t.x : -t.x, t.y};
    return m < 512 ? u : c64{-u.x, -u.y};
}

__global__ __launch_bounds__(VQ_NT) void k_voice_quality(const float* __restrict__ y, const int32_t* __restrict__ n_samples,
                                                         int y_stride, float* __restrict__ out, int t_stride, int tiles) {
    __shared__ c64 Z[VQ_W][512];                   // a wave's FFT workspace: c64 for the first transform, its head c32 for the second
    __shared__ float S[VQ_W][VQ_LD];               // a wave's real sequence: P, then L less its mean, then c
    __shared__ __attribute__((aligned(16))) float X[VQ_X];             // sample 256 t0 - 512 + i of the row
    __shared__ __attribute__((aligned(16))) float WIN[1024];
    __shared__ c64 TWD512[512], TWD1024[257];      // exp(-2 pi i k / 512), exp(-2 pi i k / 1024)
    __shared__ c32 TW512[512], TW1024[257];        // the same, rounded once
    __shared__ float OUT[T2V_VOICE_FEATS][VQ_W];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * VQ_W;
    const int n = min(max(n_samples[b], 0), y_stride);                 // no length addresses outside the row
    const int frames = n > 0 ? n / VQ_HOP + 1 : 0;
    if (t0 < frames) {                             // the whole workgroup; 256 t0 <= n <= 2^30
        if (tid < 257) {                           // the first quadrant in fp64: the only sines and cosines of the workgroup
            double sn, cs;
            sincospi((double)tid * (1.0 / 512.0), &sn, &cs);
            TWD1024[tid] = {cs, -sn};
            TW1024[tid] = {(float)cs, (float)-sn};
        }
        const float* yb = y + (size_t)b * y_stride;
        const int g0 = VQ_HOP * t0 - 512;
        for (int i = tid; i < VQ_X; i += VQ_NT) {
            const int g = g0 + i;
            X[i] = g >= 0 && g < n ? yb[g] : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < 512 + 1024; i += VQ_NT) {                // the other tables by symmetry, exact in fp64
            if (i < 512) {
                const c64 u = vq_unit(TWD1024, 2 * i);
                TWD512[i] = u;
                TW512[i] = {(float)u.x, (float)u.y};
            } else {
                WIN[i - 512] = (float)(0.5 - 0.5 * vq_unit(TWD1024, i - 512).x);
            }
        }
        __syncthreads();
        if (t0 + w < frames) {                     // the wave's frame; wave barriers only from here on
            float* s = S[w];
            const float* x = X + VQ_HOP * w;
            {   // P: the transform of x w in fp64 (see the head of the file), each power rounded once
                c64* z = Z[w];
                c64 v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int j = 2 * (lane + 64 * r);
                    const float2 xx = *(const float2*)(x + j), ww = *(const float2*)(WIN + j);
                    v[r] = {(double)xx.x * (double)ww.x, (double)xx.y * (double)ww.y};
                }
                fft512(v, z, TWD512, lane);
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = lane + 64 * r;
                    c64 xk, xc;
                    untangle(z[k], z[(512 - k) & 511], TWD1024[k], xk, xc);
                    s[k] = (float)fma(xk.x, xk.x, xk.y * xk.y);
                    s[512 - k] = (float)fma(xc.x, xc.x, xc.y * xc.y);
                }
                if (lane == 0) {
                    c64 xk, xc;
                    untangle(z[256], z[256], TWD1024[256], xk, xc);
                    s[256] = (float)fma(xk.x, xk.x, xk.y * xk.y);
                }
            }
            c32* z = (c32*)Z[w];
            __builtin_amdgcn_wave_barrier();
            float p[8], p512 = s[512], mx = p512;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                p[r] = s[lane + 64 * r];
                mx = fmaxf(mx, p[r]);
            }
            mx = wave_max(mx);
            float f[T2V_VOICE_FEATS] = {(float)T2V_VOICE_SILENT_DB, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (mx > 0.f) {                        // sum_k P > 0; the whole wave
                const float fl = fmaxf(1e-9f * mx, 1.17549435e-38f);
                // the bands: bins lane + 64 r, r = 0 is 0..63, r = 1..4 is 64..319, r = 0..1 is 0..127, r = 2..4 is 128..319
                const float lo = wave_sum(lane >= VQ_K_LO ? p[0] : 0.f);
                const float hi = wave_sum(((p[1] + p[2]) + p[3]) + p[4]);
                const float m_lo = wave_max(fmaxf(p[0], p[1])), m_hi = wave_max(fmaxf(fmaxf(p[2], p[3]), p[4]));
                f[0] = vq_db(fmaxf(lo + hi, fl));
                f[1] = vq_db(fmaxf(hi, fl) / fmaxf(lo, fl));             // one logarithm of the ratio: a difference of two would
                f[2] = vq_db(fmaxf(m_lo, fl) / fmaxf(m_hi, fl));         // round at their size, not at its own
                float L[8], L512 = vq_db(fmaxf(p512, fl)), sum = 0.f;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    L[r] = vq_db(fmaxf(p[r], fl));
                    sum += L[r];
                }
                const float mu = (wave_sum(sum) + L512) * (1.f / 513.f);
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    L[r] -= mu;
                    s[lane + 64 * r] = L[r];
                }
                if (lane == 0) s[512] = L512 - mu;
                // slope: bins 32..63 are r = 0 of lanes 32..63, bins 64..96 r = 1 of lanes 0..32
                const float sl = (lane >= VQ_S0 ? (float)(lane - VQ_SC) * L[0] : 0.f) + (lane <= VQ_S1 - 64 ? (float)lane * L[1] : 0.f);
                f[3] = wave_sum(sl) * (1.f / 357.5f);                  // sum (k - 64)^2 = 22 880 bins^2, a bin 0.015625 kHz
                __builtin_amdgcn_wave_barrier();
                even_transform(s, z, TW512, TW1024, 512, 1.f / 1024.f, lane);          // the cepstrum of L - mu
                float a[5], amax = 0.f;
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    const int q = lane + 64 * r;
                    a[r] = fabsf(s[q]);
                    if (q >= VQ_Q0 && q <= VQ_Q1) amax = fmaxf(amax, a[r]);
                }
                amax = wave_max(amax);
                const float cfl = fmaxf(1e-3f * amax, 1e-4f);
                float C[5], csum = 0.f, best = -INFINITY;
                int qbest = 0x7fffffff;
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    const int q = lane + 64 * r;
                    const bool in = q >= VQ_Q0 && q <= VQ_Q1;
                    C[r] = in ? 2.f * vq_db(fmaxf(a[r], cfl)) : 0.f;
                    csum += C[r];
                    if (in && q >= VQ_QP && C[r] > best) {             // ascending q: the lowest stays
                        best = C[r];
                        qbest = q;
                    }
                }
                const float mean = wave_sum(csum) * (1.f / 251.f);
                float cs = 0.f;
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    const int q = lane + 64 * r;
                    if (q >= VQ_Q0 && q <= VQ_Q1) cs = fmaf((float)(q - VQ_QC), C[r] - mean, cs);
                }
                const float slope = wave_sum(cs) * (1.f / 1317750.f);  // sum (q - 141)^2 over 16..266
                vq_argmax(best, qbest);
                f[4] = best - fmaf(slope, (float)(qbest - VQ_QC), mean);
                f[5] = (float)qbest;
            }
            if (lane == 0)
#pragma unroll
                for (int c = 0; c < T2V_VOICE_FEATS; ++c) OUT[c][w] = f[c];
        }
        __syncthreads();
    }
    if (tid < T2V_VOICE_FEATS * VQ_W) {
        const int c = tid / VQ_W, fr = tid - c * VQ_W, t = t0 + fr;
        if (t < t_stride) out[((size_t)b * T2V_VOICE_FEATS + c) * t_stride + t] = t < frames ? OUT[c][fr] : 0.f;
    }
}

extern "C" int t2v_voice_quality(const float* y, const int32_t* n, int y_stride, int B, float* out, int t_stride, void* stream_) {
    if (!y || !n || !out || B < 1 || y_stride < 1 || y_stride > (1 << 30) || t_stride < y_stride / VQ_HOP + 1) return T2V_ERR_ARG;
    const long long tiles = ((long long)t_stride + VQ_W - 1) / VQ_W;
    if ((long long)B * tiles > 0x7fffffffLL) return T2V_ERR_DIMS;
    k_voice_quality<<<(int)(B * tiles), VQ_NT, 0, (hipStream_t)stream_>>>(y, n, y_stride, out, t_stride, (int)tiles);
    return t2v_check_launch();
}
