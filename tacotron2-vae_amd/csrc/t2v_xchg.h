// Cross-workgroup exchange of the persistent decoder kernels (decoder_persist.hip, decoder_train_persist.hip,
// decoder_train_bwd_persist.hip and their bf16 forms).  All 256 workgroups stay resident for a whole pass and hand their
// results from CU to CU through global exchange buffers:
//   - every exchanged value is produced exactly once per pass, so the buffers are pre-filled with T2V_SENT (a NaN pattern,
//     t2v_fill_sentinel) and a word that is no longer the sentinel IS the data: no tags, no flags, no ordering;
//   - every access is a raw buffer operation with the sc1 cache-policy bit (T2V_SC1): loads bypass the CU's vector L1,
//     stores are write-through, so a value reaches a consumer on another XCD (the XCD L2s are not coherent with each
//     other).  As builtins, not inline asm, the compiler tracks their vmcnt itself (an inline-asm load is invisible to its
//     scoreboard — the result registers can be read or copied before the data has landed);
//   - every wait is bounded: on a timeout (or when another workgroup has already given up) t2v_give_up sets the pass's
//     error word and clears the caller's LDS flag, and the engine skips the update and re-runs the step.
// Offsets are BYTES from the buffer base (< 2 GiB).
#pragma once
#include "t2v_common.h"

#define T2V_SENT 0xFFFFFFFFu
#define T2V_SC1 16
#define T2V_LDS_MAX (160 * 1024)     // dynamic-LDS limit the persistent kernels are raised to (t2v_persist_resident)

// raw buffer resource over the whole 31-bit range (word 3: DATA_FORMAT 32); also the split-K scratch of gemm.hip / conv_x3.hip
__device__ __forceinline__ __amdgpu_buffer_rsrc_t t2v_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}

__device__ __forceinline__ unsigned t2v_ld_b32(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, T2V_SC1);
}
__device__ __forceinline__ u32x2 t2v_ld_b64(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, T2V_SC1);
}
__device__ __forceinline__ u32x4 t2v_ld_b128(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, T2V_SC1);
}
__device__ __forceinline__ f32x2 t2v_ld_f32x2(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, T2V_SC1));
}
__device__ __forceinline__ f32x4 t2v_ld_f32x4(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, T2V_SC1));
}

__device__ __forceinline__ void t2v_st(__amdgpu_buffer_rsrc_t r, unsigned off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)off, 0, T2V_SC1);
}
__device__ __forceinline__ void t2v_st(__amdgpu_buffer_rsrc_t r, unsigned off, u32x2 v) {
    __builtin_amdgcn_raw_buffer_store_b64(v, r, (int)off, 0, T2V_SC1);
}
__device__ __forceinline__ void t2v_st(__amdgpu_buffer_rsrc_t r, unsigned off, f32x2 v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (int)off, 0, T2V_SC1);
}
__device__ __forceinline__ void t2v_st(__amdgpu_buffer_rsrc_t r, unsigned off, u32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)off, 0, T2V_SC1);
}
__device__ __forceinline__ void t2v_st(__amdgpu_buffer_rsrc_t r, unsigned off, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)off, 0, T2V_SC1);
}

// "written" tests: the word is no longer the sentinel; all four; the first nw (1..4) of four
__device__ __forceinline__ bool t2v_ok(unsigned v) { return v != T2V_SENT; }
__device__ __forceinline__ bool t2v_ok(float v) { return __float_as_uint(v) != T2V_SENT; }
__device__ __forceinline__ bool t2v_ok4(u32x4 v) { return v[0] != T2V_SENT && v[1] != T2V_SENT && v[2] != T2V_SENT && v[3] != T2V_SENT; }
__device__ __forceinline__ bool t2v_ok4(f32x4 v) { return t2v_ok(v[0]) && t2v_ok(v[1]) && t2v_ok(v[2]) && t2v_ok(v[3]); }
__device__ __forceinline__ bool t2v_ok_n(f32x4 v, int nw) {
    bool ok = __float_as_uint(v[0]) != T2V_SENT;
    ok = ok && (nw < 2 || __float_as_uint(v[1]) != T2V_SENT);
    ok = ok && (nw < 3 || __float_as_uint(v[2]) != T2V_SENT);
    ok = ok && (nw < 4 || __float_as_uint(v[3]) != T2V_SENT);
    return ok;
}

// One failed round of a bounded wait: counts it, and once `limit` rounds have failed or another workgroup has already
// set the error word, sets the error word and clears *flag (an LDS int, 1 while the pass is healthy).  True: stop waiting.
template <typename C>
__device__ __forceinline__ bool t2v_give_up(C& rounds, C limit, unsigned* err, int* flag) {
    if (++rounds > limit || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = 0;
        return true;
    }
    return false;
}
