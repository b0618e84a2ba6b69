// Complex helpers, the in-register 8-point DFT and the packed 512-point FFT of a real 1024-point frame, shared by the STFT
// kernels (frontend.hip, vocoder.hip) and the spectral envelope (envelope.hip).
#pragma once
#include <hip/hip_runtime.h>

struct c32 { float x, y; };
__device__ __forceinline__ c32 cmul(c32 a, c32 b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ c32 cadd(c32 a, c32 b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ c32 csub(c32 a, c32 b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ c32 mul_mi(c32 a) { return {a.y, -a.x}; }   // a * (-i)

// in-place 8-point DFT (forward, e^{-2 pi i/8}), outputs in natural order
__device__ __forceinline__ void dft8(c32* v) {
    const float h = 0.70710678118654752440f;
    c32 a0 = cadd(v[0], v[4]), a1 = csub(v[0], v[4]);
    c32 a2 = cadd(v[2], v[6]), a3 = mul_mi(csub(v[2], v[6]));
    c32 a4 = cadd(v[1], v[5]), a5 = csub(v[1], v[5]);
    c32 a6 = cadd(v[3], v[7]), a7 = mul_mi(csub(v[3], v[7]));
    c32 b0 = cadd(a0, a2), b2 = csub(a0, a2), b1 = cadd(a1, a3), b3 = csub(a1, a3);
    c32 b4 = cadd(a4, a6), b6 = mul_mi(csub(a4, a6)), b5 = cadd(a5, a7), b7 = csub(a5, a7);
    // twiddles W8^1 = h(1 - i), W8^3 = -h(1 + i)
    c32 t5 = {h * (b5.x + b5.y), h * (b5.y - b5.x)};
    c32 t7 = {h * (-b7.x + b7.y), h * (-b7.y - b7.x)};
    v[0] = cadd(b0, b4); v[4] = csub(b0, b4);
    v[2] = cadd(b2, b6); v[6] = csub(b2, b6);
    v[1] = cadd(b1, t5); v[5] = csub(b1, t5);
    v[3] = cadd(b3, t7); v[7] = csub(b3, t7);
}

// 512-point complex FFT of one wave's packed frame: v[r] holds point lane + 64 r on entry; z (LDS, 512) holds the
// spectrum in natural order on exit (three radix-8 Stockham passes, Ns = 1, 8, 64; thread j = lane)
__device__ __forceinline__ void fft512(c32* v, c32* z, const c32* tw512, int lane) {
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
__device__ __forceinline__ void untangle(c32 zk, c32 zc, c32 w, c32& xk, c32& xc) {
    const c32 e = {0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y)};
    const c32 o = {0.5f * (zk.x - zc.x), 0.5f * (zk.y + zc.y)};
    const c32 wo = cmul(w, o);
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
