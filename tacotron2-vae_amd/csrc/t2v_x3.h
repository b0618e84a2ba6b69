// The x3 path (gemm.hip, conv_x3.hip): every fp32 operand is cut EXACTLY into three bf16 planes a = a0 + a1 + a2 and fed to the
// bf16 matrix cores; tiles of the planes travel global -> LDS by LDS-DMA with hand-counted waits.
#pragma once
#include "t2v_common.h"

// 8 consecutive-k fp32 values of one operand row -> the row's 16-byte word in each of the three planes
__device__ __forceinline__ void t2v_split8(const float (&v)[8], uint4& p0, uint4& p1, uint4& p2) {
    unsigned q0[4], q1[4], q2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float x = v[2 * c], y = v[2 * c + 1];
        const unsigned h = t2v_pack_bf16x2(x, y);
        const float r1x = x - __uint_as_float(h << 16), r1y = y - __uint_as_float(h & 0xffff0000u);
        const unsigned m = t2v_pack_bf16x2(r1x, r1y);
        const float r2x = r1x - __uint_as_float(m << 16), r2y = r1y - __uint_as_float(m & 0xffff0000u);
        q0[c] = h; q1[c] = m; q2[c] = t2v_pack_bf16x2(r2x, r2y);
    }
    p0 = make_uint4(q0[0], q0[1], q0[2], q0[3]);
    p1 = make_uint4(q1[0], q1[1], q1[2], q1[3]);
    p2 = make_uint4(q2[0], q2[1], q2[2], q2[3]);
}

// 16 bytes per lane global -> LDS without a destination register (lane i lands at lds_addr + 16 i; lds_addr wave-uniform, in an SGPR).
// Inline asm on purpose: hipcc counts the builtin form as an LDS write and puts `s_waitcnt vmcnt(0)` in front of EVERY later ds_read —
// the prefetch issued at the top of a stage was waited for before the stage's own MFMAs (first version of the conv kernels: 1.9 us per
// step of 0.35 us of MFMA work).  The asm form is invisible to its bookkeeping; the waits are counted by hand (t2v_wait_vmcnt).
__device__ __forceinline__ void t2v_dma16(const void* gsrc, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_addr) : "memory");
}

// 4 bytes per lane: lane i lands at lds_addr + 4 i, and every lane brings its own source address (a gather; rows that are not
// 16-byte aligned).  Same reasons for the inline-asm form as t2v_dma16.
__device__ __forceinline__ void t2v_dma4(const void* gsrc, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_addr) : "memory");
}

// wait until at most N of this wave's memory requests are outstanding (N a compile-time constant)
template <int N>
__device__ __forceinline__ void t2v_wait_vmcnt() {
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if constexpr (N == 11) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 13) asm volatile("s_waitcnt vmcnt(13)" ::: "memory");
    else if constexpr (N == 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
    else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else static_assert(N == 0, "add the literal");
}
