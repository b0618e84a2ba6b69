// Complex helpers, the in-register 8-point DFT and the packed 512-point FFT of a real 1024-point frame, shared by the STFT
// kernels (frontend.hip, vocoder.hip), and the forward transform of a real even sequence on top of it, shared by the spectral
// envelope (envelope.hip) and the voice-quality descriptors (voice.hip).  The helpers take either complex type: c32 everywhere
// but in voice.hip's first transform, which runs in c64.
#pragma once
#include <hip/hip_runtime.h>

struct c32 { float x, y; };
struct c64 { double x, y; };
template <class C> __device__ __forceinline__ C cmul(C a, C b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <class C> __device__ __forceinline__ C cadd(C a, C b) { return {a.x + b.x, a.y + b.y}; }
template <class C> __device__ __forceinline__ C csub(C a, C b) { return {a.x - b.x, a.y - b.y}; }
template <class C> __device__ __forceinline__ C mul_mi(C a) { return {a.y, -a.x}; }   // a * (-i)

// in-place 8-point DFT (forward, e^{-2 pi i/8}), outputs in natural order
template <class C> __device__ __forceinline__ void dft8(C* v) {
    const decltype(v[0].x) h = 0.70710678118654752440;
    C a0 = cadd(v[0], v[4]), a1 = csub(v[0], v[4]);
    C a2 = cadd(v[2], v[6]), a3 = mul_mi(csub(v[2], v[6]));
    C a4 = cadd(v[1], v[5]), a5 = csub(v[1], v[5]);
    C a6 = cadd(v[3], v[7]), a7 = mul_mi(csub(v[3], v[7]));
    C b0 = cadd(a0, a2), b2 = csub(a0, a2), b1 = cadd(a1, a3), b3 = csub(a1, a3);
    C b4 = cadd(a4, a6), b6 = mul_mi(csub(a4, a6)), b5 = cadd(a5, a7), b7 = csub(a5, a7);
    // twiddles W8^1 = h(1 - i), W8^3 = -h(1 + i)
    C t5 = {h * (b5.x + b5.y), h * (b5.y - b5.x)};
    C t7 = {h * (-b7.x + b7.y), h * (-b7.y - b7.x)};
    v[0] = cadd(b0, b4); v[4] = csub(b0, b4);
    v[2] = cadd(b2, b6); v[6] = csub(b2, b6);
    v[1] = cadd(b1, t5); v[5] = csub(b1, t5);
    v[3] = cadd(b3, t7); v[7] = csub(b3, t7);
}

// 512-point complex FFT of one wave's packed frame: v[r] holds point lane + 64 r on entry; z (LDS, 512) holds the
// spectrum in natural order on exit (three radix-8 Stockham passes, Ns = 1, 8, 64; thread j = lane)
template <class C> __device__ __forceinline__ void fft512(C* v, C* z, const C* tw512, int lane) {
    dft8(v);
#pragma unroll
    for (int r = 0; r < 8; ++r) z[lane * 8 + r] = v[r];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = z[lane + 64 * r];
    const int k = lane & 7;
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw512[8 * k * r]);
    dft8(v);
    const int j0 = (lane >> 3) * 64 + k;
#pragma unroll
    for (int r = 0; r < 8; ++r) z[j0 + 8 * r] = v[r];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = z[lane + 64 * r];
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw512[lane * r]);
    dft8(v);
#pragma unroll
    for (int r = 0; r < 8; ++r) z[lane + 64 * r] = v[r];
}

// real spectrum bins k and 512 - k from the packed FFT Z: X[k] = E - i W^k O, X[512-k] = conj(E) - i conj(W^k O)
template <class C> __device__ __forceinline__ void untangle(C zk, C zc, C w, C& xk, C& xc) {
    const decltype(zk.x) half = 0.5;
    const C e = {half * (zk.x + zc.x), half * (zk.y - zc.y)};
    const C o = {half * (zk.x - zc.x), half * (zk.y + zc.y)};
    const C wo = cmul(w, o);
    xk = {e.x + wo.y, e.y - wo.x};
    xc = {e.x - wo.y, -e.y - wo.x};
}

// the inverse: packed Z[k] and Z[512-k] from Y[k], Y[512-k] (Fe = (Y + conj Yc)/2, Fo = (Y - conj Yc)/2 conj(W^k), Z = Fe + i Fo)
__device__ __forceinline__ void retangle(c32 yk, c32 yc, c32 w, c32& zk, c32& zc) {
    const c32 fe = {0.5f * (yk.x + yc.x), 0.5f * (yk.y - yc.y)};
    const c32 d = {0.5f * (yk.x - yc.x), 0.5f * (yk.y + yc.y)};
    const c32 fo = cmul(d, c32{w.x, -w.y});
    zk = {fe.x - fo.y, fe.y + fo.x};
    zc = {fe.x + fo.y, -fe.y + fo.x};       // conj(Fe) + i conj(Fo)
}

// sample n (0..1023) of the even extension of x[0..512]
__device__ __forceinline__ int fold1024(int n) { return n <= 512 ? n : 1024 - n; }

// Re of the forward 1024-point DFT of the even extension of s[0..512], times `scale`, bins n <= keep (the others 0), back
// into s.  One wave; z: its 512 complex points.
__device__ __forceinline__ void even_transform(float* s, c32* z, const c32* tw512, const c32* tw1024, int keep, float scale,
                                              int lane) {
    c32 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int j = lane + 64 * r;
        v[r] = {s[fold1024(2 * j)], s[fold1024(2 * j + 1)]};
    }
    __builtin_amdgcn_wave_barrier();
    fft512(v, z, tw512, lane);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = lane + 64 * r;
        c32 xk, xc;
        untangle(z[k], z[(512 - k) & 511], tw1024[k], xk, xc);
        s[k] = k <= keep ? xk.x * scale : 0.f;
        s[512 - k] = 512 - k <= keep ? xc.x * scale : 0.f;
    }
    if (lane == 0) {
        c32 xk, xc;
        untangle(z[256], z[256], tw1024[256], xk, xc);
        s[256] = 256 <= keep ? xk.x * scale : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
}
