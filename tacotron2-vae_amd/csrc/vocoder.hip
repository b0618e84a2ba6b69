// Griffin-Lim vocoder and the reference's STFT.transform / STFT.inverse (reference stft.py:77-140,
// audio_processing.py:52-68), for the front end's geometry n_fft = win = 1024, hop = 256, periodic Hann.
//
// The reference's inverse is conv_transpose1d with pinv(scale * F) (F: the stacked [Re; Im] DFT rows k = 0..512) followed by
// x (n_fft / hop).  That product is exactly the inverse real FFT with the imaginary parts of bins 0 and 512 ignored: each
// frame here is irfft(X) x window, overlap-added, divided by window_sumsquare wherever it is > FLT_MIN (tiny(float32)),
// 512 samples trimmed from each end.  Every FFT is the front end's packed 512-point Stockham scheme (one wave per frame, LDS
// exchange inside the wave); the inverse runs the same forward passes on the conjugate.
//
// Kernels (one wave = one frame unless noted):
//   k_stft_polar       wav -> |X|, atan2 phase (B,513,T)
//   k_spec_to_frames   (magnitude, phase) -> windowed time-domain frames (B,T,1024); optionally M transposed to (B,T,513)
//   k_gl_iter          one Griffin-Lim iteration, frames -> frames: gather + overlap-add of frames t-3..t+3, reflect,
//                      window, FFT, magnitude replaced by M (phase kept), inverse FFT, window
//   k_ola              frames -> signal (B, (T-1)*256): overlap-add / window_sumsquare, trimmed (256 threads, one per sample)
//   k_mel_to_mag       M = max(P exp(mel), 0), P = pinv(mel_basis) (513 x 80)  (256 threads, 16 frames)
//   k_gl_iter_fast     k_gl_iter with the momentum step of fast Griffin-Lim between the transform and the projection
//   k_mel_to_mag_nnls  k_mel_to_mag followed by n_iters projected-gradient steps of min ||B M - m||, M >= 0, in LDS
#include "t2v_common.h"
#include "t2v_kernels.h"
#include "t2v_fft.h"

#define VC_NFFT 1024
#define VC_HOP 256
#define VC_NBIN 513
#define VC_FLT_MIN 1.17549435e-38f

namespace {

// M times the unit phasor of X; (M, 0) where |X| = 0, as cos/sin of atan2(0, 0) = 0
__device__ __forceinline__ c32 with_magnitude(c32 x, float m) {
    const float r2 = x.x * x.x + x.y * x.y;
    if (r2 > 0.f) {
        const float s = m / sqrtf(r2);
        return {x.x * s, x.y * s};
    }
    return {m, 0.f};
}

// Spectrum -> windowed time frame.  ypair(k, yk, yc) gives Y[k] and Y[512-k] for k = 0..256 (k = 256: both the same bin).
// The imaginary parts of bins 0 and 512 are ignored (what pinv of the stacked basis does).  Writes window * irfft(Y) to
// frame[0..1024).  z: the wave's LDS buffer; each lane owns its (k, 512-k) pairs, so the in-place update needs no barrier.
template <class YPair>
__device__ __forceinline__ void spectrum_to_frame(YPair ypair, c32* z, const float* window, const c32* tw512,
                                                  const c32* tw1024, float* frame, int lane) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = lane + 64 * r;
        c32 yk, yc;
        ypair(k, yk, yc);
        if (k == 0) { yk.y = 0.f; yc.y = 0.f; }
        c32 zk, zc;
        retangle(yk, yc, tw1024[k], zk, zc);
        z[k] = zk;
        if (k != 0) z[512 - k] = zc;
    }
    if (lane == 0) {
        c32 yk, yc;
        ypair(256, yk, yc);
        c32 zk, zc;
        retangle(yk, yk, tw1024[256], zk, zc);
        z[256] = zk;
    }
    // inverse 512-point FFT by the conjugate trick: z = conj(FFT(conj Z)) / 512 = x[2j] + i x[2j+1]
    c32 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const c32 q = z[lane + 64 * r];
        v[r] = {q.x, -q.y};
    }
    fft512(v, z, tw512, lane);
    const float s = 1.f / 512.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int j = lane + 64 * r;
        const c32 q = z[j];
        const float2 w2 = ((const float2*)window)[j];
        ((float2*)frame)[j] = make_float2(q.x * s * w2.x, -q.y * s * w2.y);
    }
}

// overlap-add of the windowed frames at OLA position m (0 <= m < 1024 + 256 (T-1)): sum and window sum-square over the
// frames tp that cover m, in increasing tp (the reference's window_sumsquare order)
__device__ __forceinline__ float ola_at(const float* fr, const float* window, int m, int T) {
    const int lo = max(0, (m - (VC_NFFT - VC_HOP)) >> 8), hi = min(T - 1, m >> 8);
    float s = 0.f, wss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int tp = lo + i;
        if (tp <= hi) {
            const int n = m - VC_HOP * tp;
            s += fr[(size_t)tp * VC_NFFT + n];
            const float w = window[n];
            wss += w * w;
        }
    }
    return wss > VC_FLT_MIN ? s / wss : s;
}

// the same for m (even) and m + 1, which lie in the same frames: one 8-byte load per frame
__device__ __forceinline__ float2 ola_pair(const float* fr, const float* window, int m, int T) {
    const int lo = max(0, (m - (VC_NFFT - VC_HOP)) >> 8), hi = min(T - 1, m >> 8);
    float2 s = {0.f, 0.f}, wss = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int tp = lo + i;
        if (tp <= hi) {
            const int n = m - VC_HOP * tp;
            const float2 f = *(const float2*)(fr + (size_t)tp * VC_NFFT + n);
            const float2 w = *(const float2*)(window + n);
            s.x += f.x; s.y += f.y;
            wss.x += w.x * w.x; wss.y += w.y * w.y;
        }
    }
    return make_float2(wss.x > VC_FLT_MIN ? s.x / wss.x : s.x, wss.y > VC_FLT_MIN ? s.y / wss.y : s.y);
}

// sample q (0 <= q < N + 1024) of the reflect-padded signal, as its OLA position: F.pad(mode='reflect') excludes the edge
__device__ __forceinline__ int reflect_to_ola(int q, int N) {
    int j = q - VC_NFFT / 2;
    if (j < 0) j = -j;
    if (j >= N) j = 2 * (N - 1) - j;
    j = min(max(j, 0), max(N - 1, 0));       // N <= 512 is refused by the host; never leave the frames anyway
    return j + VC_NFFT / 2;
}

__device__ __forceinline__ int frames_of(const int32_t* n_frames, int b, int t_stride) {
    return min(n_frames[b], t_stride);
}

}  // namespace

struct VocoderTables {
    const float* window;     // (1024) periodic Hann
    const c32* tw512;        // (512)  exp(-2 pi i k/512)
    const c32* tw1024;       // (513)  exp(-2 pi i k/1024)
};

// ---------------------------------------------------------------- STFT.transform: magnitude and phase
__global__ __launch_bounds__(64) void k_stft_polar(const float* wav, const int64_t* n_samples, int n_stride,
                                                   VocoderTables tb, float* mag, float* phase, int t_stride) {
    __shared__ c32 z[512];
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int64_t n = n_samples[b];
    const int T = n > 0 ? (int)(n / VC_HOP) + 1 : 0;
    float* mg = mag + (size_t)b * VC_NBIN * t_stride + t;
    float* ph = phase + (size_t)b * VC_NBIN * t_stride + t;
    if (t >= T) {            // past this utterance
        for (int k = lane; k < VC_NBIN; k += 64) { mg[(size_t)k * t_stride] = 0.f; ph[(size_t)k * t_stride] = 0.f; }
        return;
    }
    c32 v[8];
    const int64_t base = (int64_t)t * VC_HOP - VC_NFFT / 2;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int nn = lane + 64 * k;
        float s[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            int64_t p = base + 2 * nn + c;
            if (p < 0) p = -p;
            if (p >= n) p = 2 * (n - 1) - p;
            p = p < 0 ? 0 : (p >= n ? n - 1 : p);
            s[c] = wav[(size_t)b * n_stride + (size_t)p] * tb.window[2 * nn + c];
        }
        v[k] = {s[0], s[1]};
    }
    fft512(v, z, tb.tw512, lane);
    auto put = [&](int k, c32 x) {
        mg[(size_t)k * t_stride] = sqrtf(x.x * x.x + x.y * x.y);
        ph[(size_t)k * t_stride] = (x.x == 0.f && x.y == 0.f) ? 0.f : atan2f(x.y, x.x);
    };
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = lane + 64 * r;
        c32 xk, xc;
        untangle(z[k], z[(512 - k) & 511], tb.tw1024[k], xk, xc);
        put(k, xk);
        put(512 - k, xc);
    }
    if (lane == 0) {
        c32 xk, xc;
        untangle(z[256], z[256], tb.tw1024[256], xk, xc);
        put(256, xk);
    }
}

// ---------------------------------------------------------------- (magnitude, phase) -> windowed frames
__global__ __launch_bounds__(64) void k_spec_to_frames(const float* mag, const float* phase, const int32_t* n_frames,
                                                       int t_stride, VocoderTables tb, float* frames, float* mt) {
    __shared__ c32 z[512];
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (t >= frames_of(n_frames, b, t_stride)) return;
    const float* mg = mag + (size_t)b * VC_NBIN * t_stride + t;
    const float* ph = phase + (size_t)b * VC_NBIN * t_stride + t;
    float* mrow = mt ? mt + ((size_t)b * t_stride + t) * VC_NBIN : nullptr;
    auto bin = [&](int k) {
        const float m = mg[(size_t)k * t_stride];
        float sn, cs;
        sincosf(ph[(size_t)k * t_stride], &sn, &cs);
        if (mrow) mrow[k] = m;
        return c32{m * cs, m * sn};
    };
    auto ypair = [&](int k, c32& yk, c32& yc) {
        yk = bin(k);
        yc = k == 256 ? yk : bin(512 - k);
    };
    spectrum_to_frame(ypair, z, tb.window, tb.tw512, tb.tw1024, frames + ((size_t)b * t_stride + t) * VC_NFFT, lane);
}

// ---------------------------------------------------------------- one Griffin-Lim iteration
__global__ __launch_bounds__(64) void k_gl_iter(const float* fin, const float* mt, const int32_t* n_frames, int t_stride,
                                                VocoderTables tb, float* fout) {
    __shared__ c32 z[512];
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int T = frames_of(n_frames, b, t_stride);
    if (t >= T) return;
    const int N = VC_HOP * (T - 1);
    const float* fr = fin + (size_t)b * t_stride * VC_NFFT;
    // previous iterate's signal under this frame's reflect-padded window, windowed again, packed as 512 complex points
    c32 v[8];
    if (t >= 2 && t + 3 <= T) {         // no reflection: padded sample 256 t + n is OLA position 256 t + n
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nn = lane + 64 * k;
            const float2 y = ola_pair(fr, tb.window, VC_HOP * t + 2 * nn, T);
            const float2 w2 = ((const float2*)tb.window)[nn];
            v[k] = {y.x * w2.x, y.y * w2.y};
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nn = lane + 64 * k;
            const int q = VC_HOP * t + 2 * nn;
            const float y0 = ola_at(fr, tb.window, reflect_to_ola(q, N), T);
            const float y1 = ola_at(fr, tb.window, reflect_to_ola(q + 1, N), T);
            v[k] = {y0 * tb.window[2 * nn], y1 * tb.window[2 * nn + 1]};
        }
    }
    fft512(v, z, tb.tw512, lane);
    // keep the phase, take the target magnitude
    const float* mrow = mt + ((size_t)b * t_stride + t) * VC_NBIN;
    auto ypair = [&](int k, c32& yk, c32& yc) {
        c32 xk, xc;
        untangle(z[k], z[(512 - k) & 511], tb.tw1024[k], xk, xc);
        yk = with_magnitude(xk, mrow[k]);
        yc = k == 256 ? yk : with_magnitude(xc, mrow[512 - k]);
    };
    spectrum_to_frame(ypair, z, tb.window, tb.tw512, tb.tw1024, fout + ((size_t)b * t_stride + t) * VC_NFFT, lane);
}

// ---------------------------------------------------------------- one fast Griffin-Lim iteration
// k_gl_iter with the momentum step of Perraudin, Balazs, Soendergaard 2013 between the transform and the projection.  tprev
// holds each frame's previous transform (B, t_stride, 513); a lane reads and writes only the bins it owns, so one buffer
// serves.  first: tprev counts as 0 and is not read.  A kernel of its own, so that k_gl_iter keeps its instructions.
__global__ __launch_bounds__(64) void k_gl_iter_fast(const float* fin, const float* mt, const int32_t* n_frames,
                                                     int t_stride, VocoderTables tb, float* fout, float alpha, c32* tprev,
                                                     int first) {
    __shared__ c32 z[512];
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int T = frames_of(n_frames, b, t_stride);
    if (t >= T) return;
    const int N = VC_HOP * (T - 1);
    const float* fr = fin + (size_t)b * t_stride * VC_NFFT;
    // previous iterate's signal under this frame's reflect-padded window, windowed again, packed as 512 complex points
    c32 v[8];
    if (t >= 2 && t + 3 <= T) {         // no reflection: padded sample 256 t + n is OLA position 256 t + n
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nn = lane + 64 * k;
            const float2 y = ola_pair(fr, tb.window, VC_HOP * t + 2 * nn, T);
            const float2 w2 = ((const float2*)tb.window)[nn];
            v[k] = {y.x * w2.x, y.y * w2.y};
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nn = lane + 64 * k;
            const int q = VC_HOP * t + 2 * nn;
            const float y0 = ola_at(fr, tb.window, reflect_to_ola(q, N), T);
            const float y1 = ola_at(fr, tb.window, reflect_to_ola(q + 1, N), T);
            v[k] = {y0 * tb.window[2 * nn], y1 * tb.window[2 * nn + 1]};
        }
    }
    fft512(v, z, tb.tw512, lane);
    // a = X - alpha tprev, tprev <- X; keep the phase of a, take the target magnitude
    const float* mrow = mt + ((size_t)b * t_stride + t) * VC_NBIN;
    c32* tp = tprev + ((size_t)b * t_stride + t) * VC_NBIN;
    auto momentum = [&](int j, c32& x) {
        const c32 p = first ? c32{0.f, 0.f} : tp[j];
        tp[j] = x;
        x = {x.x - alpha * p.x, x.y - alpha * p.y};
    };
    auto ypair = [&](int k, c32& yk, c32& yc) {
        c32 xk, xc;
        untangle(z[k], z[(512 - k) & 511], tb.tw1024[k], xk, xc);
        momentum(k, xk);
        if (k != 256) momentum(512 - k, xc);
        yk = with_magnitude(xk, mrow[k]);
        yc = k == 256 ? yk : with_magnitude(xc, mrow[512 - k]);
    };
    spectrum_to_frame(ypair, z, tb.window, tb.tw512, tb.tw1024, fout + ((size_t)b * t_stride + t) * VC_NFFT, lane);
}

// ---------------------------------------------------------------- frames -> signal
__global__ __launch_bounds__(256) void k_ola(const float* frames, const int32_t* n_frames, int t_stride,
                                             const float* window, float* out, int out_stride) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= out_stride) return;
    const int T = frames_of(n_frames, b, t_stride);
    const int N = VC_HOP * (T - 1);
    out[(size_t)b * out_stride + j] =
        j < N ? ola_at(frames + (size_t)b * t_stride * VC_NFFT, window, j + VC_NFFT / 2, T) : 0.f;
}

// ---------------------------------------------------------------- mel -> linear magnitude
#define VC_MEL_FR 16
__global__ __launch_bounds__(256) void k_mel_to_mag(const float* mel, const float* pinv, const int32_t* n_frames,
                                                    int t_stride, int n_mel, float* mag) {
    __shared__ float e[T2V_NMEL][VC_MEL_FR];
    const int b = blockIdx.y, t0 = blockIdx.x * VC_MEL_FR;
    const int T = frames_of(n_frames, b, t_stride);
    for (int i = threadIdx.x; i < n_mel * VC_MEL_FR; i += 256) {
        const int m = i / VC_MEL_FR, tt = i % VC_MEL_FR, t = t0 + tt;
        e[m][tt] = t < T ? expf(mel[((size_t)b * n_mel + m) * t_stride + t]) : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < VC_NBIN * VC_MEL_FR; i += 256) {
        const int k = i / VC_MEL_FR, tt = i % VC_MEL_FR, t = t0 + tt;
        if (t >= t_stride) continue;
        float acc = 0.f;
        for (int m = 0; m < n_mel; ++m) acc = fmaf(pinv[k * n_mel + m], e[m][tt], acc);
        mag[((size_t)b * VC_NBIN + k) * t_stride + t] = t < T ? fmaxf(acc, 0.f) : 0.f;
    }
}

// ---------------------------------------------------------------- mel -> linear magnitude, non-negative least squares
// The filterbank in two-tap form: bin k lies in the filters lo[k] and lo[k] + 1 only, with the weights w0[k] and w1[k];
// filter f covers the bins start[f] .. start[f] + len[f] - 1.  The host builds it from the basis and checks that it
// reproduces the basis exactly; the kernel clamps the indices, so no table addresses outside LDS.
struct NnlsTaps {
    const int32_t* lo;       // (513) 0..78
    const float* w0;         // (513)
    const float* w1;         // (513)
    const int32_t* start;    // (80)
    const int32_t* len;      // (80)
};

// A workgroup owns VC_MEL_FR frames: m = exp(mel), M = max(P m, 0) as k_mel_to_mag, then n_iters times r = B M - m and
// M <- max(M - B^T r / L, 0), with M and r in LDS throughout.  Thread i handles the frame i % 16 of every element it touches,
// and every sum runs in an order that depends on the filter or the bin alone: a frame's bits depend on that frame alone.
__global__ __launch_bounds__(256) void k_mel_to_mag_nnls(const float* mel, const float* pinv, NnlsTaps tp,
                                                         const int32_t* n_frames, int t_stride, int n_iters, float inv_l,
                                                         float* mag) {
    __shared__ float M[VC_NBIN][VC_MEL_FR];
    __shared__ float e[T2V_NMEL][VC_MEL_FR];
    __shared__ float r[T2V_NMEL][VC_MEL_FR];
    __shared__ float w0[VC_NBIN], w1[VC_NBIN];
    __shared__ int lo[VC_NBIN], fs[T2V_NMEL], fl[T2V_NMEL];
    const int b = blockIdx.y, t0 = blockIdx.x * VC_MEL_FR;
    const int T = frames_of(n_frames, b, t_stride);
    for (int i = threadIdx.x; i < T2V_NMEL * VC_MEL_FR; i += 256) {
        const int m = i / VC_MEL_FR, tt = i % VC_MEL_FR, t = t0 + tt;
        e[m][tt] = t < T ? expf(mel[((size_t)b * T2V_NMEL + m) * t_stride + t]) : 0.f;
    }
    for (int k = threadIdx.x; k < VC_NBIN; k += 256) {
        lo[k] = min(max(tp.lo[k], 0), T2V_NMEL - 2);
        w0[k] = tp.w0[k];
        w1[k] = tp.w1[k];
    }
    if (threadIdx.x < T2V_NMEL) {
        const int s = min(max(tp.start[threadIdx.x], 0), VC_NBIN);
        fs[threadIdx.x] = s;
        fl[threadIdx.x] = min(max(tp.len[threadIdx.x], 0), VC_NBIN - s);
    }
    __syncthreads();
#pragma unroll 1
    for (int i = threadIdx.x; i < VC_NBIN * VC_MEL_FR; i += 256) {
        const int k = i / VC_MEL_FR, tt = i % VC_MEL_FR;
        float acc = 0.f;
#pragma unroll 8
        for (int m = 0; m < T2V_NMEL; ++m) acc = fmaf(pinv[k * T2V_NMEL + m], e[m][tt], acc);
        M[k][tt] = t0 + tt < T ? fmaxf(acc, 0.f) : 0.f;
    }
    __syncthreads();
    for (int it = 0; it < n_iters; ++it) {
#pragma unroll 1
        for (int i = threadIdx.x; i < T2V_NMEL * VC_MEL_FR; i += 256) {
            const int f = i / VC_MEL_FR, tt = i % VC_MEL_FR;
            const int k0 = fs[f], k1 = k0 + fl[f];
            float acc = 0.f;
            for (int k = k0; k < k1; ++k) acc = fmaf(lo[k] == f ? w0[k] : w1[k], M[k][tt], acc);
            r[f][tt] = acc - e[f][tt];
        }
        __syncthreads();
#pragma unroll 4
        for (int i = threadIdx.x; i < VC_NBIN * VC_MEL_FR; i += 256) {
            const int k = i / VC_MEL_FR, tt = i % VC_MEL_FR;
            const int f = lo[k];
            const float g = fmaf(w1[k], r[f + 1][tt], w0[k] * r[f][tt]);
            M[k][tt] = fmaxf(fmaf(-g, inv_l, M[k][tt]), 0.f);
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < VC_NBIN * VC_MEL_FR; i += 256) {
        const int k = i / VC_MEL_FR, tt = i % VC_MEL_FR, t = t0 + tt;
        if (t < t_stride) mag[((size_t)b * VC_NBIN + k) * t_stride + t] = t < T ? M[k][tt] : 0.f;
    }
}

// ---------------------------------------------------------------- C ABI
namespace {
size_t round_floats(size_t n) { return (n + 63) / 64 * 64; }      // 256-byte aligned regions

int tables(const float* window, const float* tw512, const float* tw1024, VocoderTables& tb) {
    if (!window || !tw512 || !tw1024) return T2V_ERR_ARG;
    tb.window = window; tb.tw512 = (const c32*)tw512; tb.tw1024 = (const c32*)tw1024;
    return T2V_OK;
}

int ola(const float* frames, const int32_t* n_frames, int B, int t_stride, const float* window, float* out,
        int out_stride, hipStream_t stream) {
    if (out_stride < 1) return T2V_OK;
    dim3 grid((out_stride + 255) / 256, B);
    k_ola<<<grid, 256, 0, stream>>>(frames, n_frames, t_stride, window, out, out_stride);
    return t2v_check_launch();
}
}  // namespace

extern "C" int t2v_stft_polar(const float* wav, const int64_t* n_samples, int B, int n_stride, int n_fft, int hop,
                              const float* window, const float* tw512, const float* tw1024, float* mag, float* phase,
                              int t_stride, void* stream_) {
    if (n_fft != VC_NFFT || hop != VC_HOP) return T2V_ERR_DIMS;
    VocoderTables tb;
    if (tables(window, tw512, tw1024, tb) || !wav || !n_samples || !mag || !phase || B < 1 || t_stride < 1 || n_stride < 1)
        return T2V_ERR_ARG;
    k_stft_polar<<<dim3(t_stride, B), 64, 0, (hipStream_t)stream_>>>(wav, n_samples, n_stride, tb, mag, phase, t_stride);
    return t2v_check_launch();
}

extern "C" size_t t2v_istft_scratch_bytes(int B, int t_stride) {
    return 4 * round_floats((size_t)B * t_stride * VC_NFFT);
}

extern "C" int t2v_istft(const float* mag, const float* phase, const int32_t* n_frames, int B, int t_stride, int n_fft,
                         int hop, const float* window, const float* tw512, const float* tw1024, void* scratch,
                         float* out, int out_stride, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_fft != VC_NFFT || hop != VC_HOP) return T2V_ERR_DIMS;
    VocoderTables tb;
    if (tables(window, tw512, tw1024, tb) || !mag || !phase || !n_frames || !scratch || (!out && out_stride > 0) || B < 1 ||
        t_stride < 1)
        return T2V_ERR_ARG;
    float* frames = (float*)scratch;
    k_spec_to_frames<<<dim3(t_stride, B), 64, 0, stream>>>(mag, phase, n_frames, t_stride, tb, frames, nullptr);
    if (int rc = t2v_check_launch()) return rc;
    return ola(frames, n_frames, B, t_stride, window, out, out_stride, stream);
}

extern "C" size_t t2v_griffin_lim_scratch_bytes(int B, int t_stride) {
    const size_t fr = round_floats((size_t)B * t_stride * VC_NFFT);
    return 4 * (2 * fr + round_floats((size_t)B * t_stride * VC_NBIN));
}

extern "C" int t2v_griffin_lim(const float* mag, const float* angles, const int32_t* n_frames, int B, int t_stride,
                               int n_fft, int hop, int n_iters, const float* window, const float* tw512,
                               const float* tw1024, void* scratch, float* out, int out_stride, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_fft != VC_NFFT || hop != VC_HOP) return T2V_ERR_DIMS;
    VocoderTables tb;
    if (tables(window, tw512, tw1024, tb) || !mag || !angles || !n_frames || !scratch || !out || B < 1 || t_stride < 1 ||
        n_iters < 0)
        return T2V_ERR_ARG;
    const size_t fr = round_floats((size_t)B * t_stride * VC_NFFT);
    float* frames[2] = {(float*)scratch, (float*)scratch + fr};
    float* mt = (float*)scratch + 2 * fr;
    const dim3 grid(t_stride, B);
    // signal = inverse(M, angles); n_iters x (phase of transform(signal), signal = inverse(M, phase)), all on the stream
    k_spec_to_frames<<<grid, 64, 0, stream>>>(mag, angles, n_frames, t_stride, tb, frames[0], mt);
    if (int rc = t2v_check_launch()) return rc;
    for (int i = 0; i < n_iters; ++i) {
        k_gl_iter<<<grid, 64, 0, stream>>>(frames[i & 1], mt, n_frames, t_stride, tb, frames[(i + 1) & 1]);
        if (int rc = t2v_check_launch()) return rc;
    }
    return ola(frames[n_iters & 1], n_frames, B, t_stride, window, out, out_stride, stream);
}

extern "C" int t2v_mel_to_magnitude(const float* mel, const float* pinv_basis, const int32_t* n_frames, int B,
                                    int t_stride, int n_mel, float* mag, void* stream_) {
    if (n_mel != T2V_NMEL) return T2V_ERR_DIMS;
    if (!mel || !pinv_basis || !n_frames || !mag || B < 1 || t_stride < 1) return T2V_ERR_ARG;
    dim3 grid((t_stride + VC_MEL_FR - 1) / VC_MEL_FR, B);
    k_mel_to_mag<<<grid, 256, 0, (hipStream_t)stream_>>>(mel, pinv_basis, n_frames, t_stride, n_mel, mag);
    return t2v_check_launch();
}

extern "C" size_t t2v_griffin_lim_fast_scratch_bytes(int B, int t_stride) {
    return t2v_griffin_lim_scratch_bytes(B, t_stride) + 4 * round_floats((size_t)B * t_stride * VC_NBIN * 2);
}

extern "C" int t2v_griffin_lim_fast(const float* mag, const float* angles, const int32_t* n_frames, int B, int t_stride,
                                    int n_fft, int hop, int n_iters, float momentum, const float* window,
                                    const float* tw512, const float* tw1024, void* scratch, float* out, int out_stride,
                                    void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_fft != VC_NFFT || hop != VC_HOP) return T2V_ERR_DIMS;
    VocoderTables tb;
    if (tables(window, tw512, tw1024, tb) || !mag || !angles || !n_frames || !scratch || !out || B < 1 || t_stride < 1 ||
        n_iters < 0 || !(momentum >= 0.f && momentum < 1.f))
        return T2V_ERR_ARG;
    if (momentum == 0.f)
        return t2v_griffin_lim(mag, angles, n_frames, B, t_stride, n_fft, hop, n_iters, window, tw512, tw1024, scratch, out,
                               out_stride, stream_);
    const size_t fr = round_floats((size_t)B * t_stride * VC_NFFT);
    float* frames[2] = {(float*)scratch, (float*)scratch + fr};
    float* mt = (float*)scratch + 2 * fr;
    c32* tprev = (c32*)(mt + round_floats((size_t)B * t_stride * VC_NBIN));
    const float alpha = momentum / (1.f + momentum);
    const dim3 grid(t_stride, B);
    k_spec_to_frames<<<grid, 64, 0, stream>>>(mag, angles, n_frames, t_stride, tb, frames[0], mt);
    if (int rc = t2v_check_launch()) return rc;
    for (int i = 0; i < n_iters; ++i) {
        k_gl_iter_fast<<<grid, 64, 0, stream>>>(frames[i & 1], mt, n_frames, t_stride, tb, frames[(i + 1) & 1], alpha, tprev,
                                                i == 0);
        if (int rc = t2v_check_launch()) return rc;
    }
    return ola(frames[n_iters & 1], n_frames, B, t_stride, window, out, out_stride, stream);
}

extern "C" int t2v_mel_to_magnitude_nnls(const float* mel, const float* pinv_basis, const int32_t* tap_lo,
                                         const float* tap_w0, const float* tap_w1, const int32_t* filt_start,
                                         const int32_t* filt_len, float lipschitz, int n_iters, const int32_t* n_frames,
                                         int B, int t_stride, int n_mel, float* mag, void* stream_) {
    if (n_mel != T2V_NMEL) return T2V_ERR_DIMS;
    if (!mel || !pinv_basis || !tap_lo || !tap_w0 || !tap_w1 || !filt_start || !filt_len || !n_frames || !mag || B < 1 ||
        t_stride < 1 || n_iters < 0 || !(lipschitz > 0.f))
        return T2V_ERR_ARG;
    const NnlsTaps tp = {tap_lo, tap_w0, tap_w1, filt_start, filt_len};
    dim3 grid((t_stride + VC_MEL_FR - 1) / VC_MEL_FR, B);
    k_mel_to_mag_nnls<<<grid, 256, 0, (hipStream_t)stream_>>>(mel, pinv_basis, tp, n_frames, t_stride, n_iters,
                                                              1.f / lipschitz, mag);
    return t2v_check_launch();
}
