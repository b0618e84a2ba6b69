// Hand-written BPTT of the teacher-forced decoder loop as ONE persistent launch, fp32 weights (reference: autograd over
// Decoder.decode, model.py:346-389 / train.py:225).  The launch-per-step backward (decoder_bwd.hip: 2 launches and a 67 MB
// transposed weight stream per reverse step) stays the general path; this file serves B <= 6, T_in <= 576
// (t2v_decoder_bwd_persist_supported); decoder_train_bwd_persist16.hip is its bf16 counterpart for B <= 16.
//
// k_achain_bwd<NB, LONG, DAL> runs the whole reverse recurrence on 256 resident workgroups in three roles (details at PBAArgs and
// at pba_na below):
//   T  attention(t) backward of one item and one slice of encoder positions (t2v_attn_role_bwd.h, shared with the bf16 kernel),
//   A  attention_rnn: dga(t+1) -> Wcat_att^T -> [d h_att(t) | d ctx(t)] -> (T role) -> dq(t) -> W_q^T -> cell backward -> dga(t)
//      — the per-step dependency chain,
//   D  decoder_rnn: dgd(t+1) -> W_hh_dec^T -> dh_dec(t) -> cell backward -> dgd(t).  Nothing of the attention path enters it
//      (teacher forcing: h_dec feeds only the projection and its own next step), so it free-runs ahead of the A chain and
//      leaves E(t) = Wcat_dec[:, :1536]^T dgd(t), its contribution to d h_att(t) / d ctx(t), for the A workgroups.
// All transposed LSTM weight columns live in registers, read once per pass from the nn.LSTMCell tensors.
// In front of the pass two small kernels turn the forward pass's saved activations into per-step factor arrays
// (k_pb_factors, k_pb_cellpre); they and the sentinel fills are the "preparation", which a training step issues right behind
// the decoder forward (t2v_decoder_bwd_achain_prepare / _prepared; t2v_decoder_bwd_achain does both).
// Host side at the end of the file: pba_layout() is the one description of the scratch buffer's sections.
// Hand-offs as in decoder_train_persist.hip: every exchanged value is produced exactly once per pass, so the exchange
// buffers are pre-filled with a NaN sentinel (T2V_SENT, t2v_xchg.h) and a word that is no longer the sentinel IS the data — 4 bytes
// per value on the wire, sc1 (write-through) stores, sc1 loads, no flags, no ordering.
#include "t2v_common.h"
#include "t2v_kernels.h"
#include "t2v_xchg.h"
#include "gemm_x3_tile.h"
#include "t2v_attn_role_bwd.h"

#define PB_THREADS T2V_AB_THREADS
#define PB_MAXB 6
#define PB_MAXT T2V_AB_MAXT           // 16- / 32-position attention slices up to here
#define PB_MAXT_LONG 576              // 96-position slices on eight waves beyond (k_achain_bwd<.., true>): at most six per item
#define PB_SPIN 400000
#define PB_KJ (T2V_G / PB_THREADS)          // 8 gate rows per thread: k = tid + 512 j
// floats of LDS of an LSTM role (the attention_rnn role's carve, the larger one) with NBS = 4 / 6 item slots
#define PBA_LROLE_FLOATS(NBS) ((NBS) * T2V_G + 6 * 1024 + 192 + 128 + 512 + 16 * T2V_A + 8 * T2V_A + 2048 + 256 + 64 + 512)

// ---- a gate-gradient row (4096 gate rows x B items) in the exchange buffer / in LDS:
//   plane 0: k -> 16 bytes (items 0..3) at byte 16 k          (64 KB)
//   plane 1: k -> 8 bytes (items 4, 5)  at byte 65536 + 8 k   (32 KB, B > 4 only)
#define PB_ROW_BYTES(NB) ((NB) > 4 ? 98304u : 65536u)

// ---- the one-launch reverse pass exchanges (d c, d h) of a cell instead of its four gate gradients: a row is
//   plane 0: unit U -> 32 bytes [dc items 0..3 | dh items 0..3] at byte 32 U          (32 KB)
//   plane 1: unit U -> 16 bytes [dc items 4, 5 | dh items 4, 5] at byte 32768 + 16 U  (16 KB, B > 4 only)
// and the gate gradient of row k = r*1024 + U is F[k] * (r == 3 ? dh[U] : dc[U]) with the factor F a function of the
// forward activations alone (k_pb_factors, before the pass): half the bytes on the wire, and since thread tid consumes
// exactly the gate rows tid + 512 j — units tid and tid + 512 — it polls its own 96 bytes and nobody else's.
#define PB_DROW_BYTES(NB) ((NB) > 4 ? 49152u : 32768u)
// The factors do not wait for anybody: a phase early (their latency hides behind the wait for the other role) the row is
// copied global -> LDS as it lies (planes 0 and 1 are contiguous in both), by LDS-DMA — 1 KB per wave instruction, no
// staging registers (the 168 weight registers leave room for only a few loads in flight).  pb_build_row multiplies in
// place; a barrier must lie between the two.
// a 4-byte word per lane global -> LDS (lane i lands at ldsbase + 4 i) without a destination register; aux: cache policy
__device__ __forceinline__ void pb_dma4(const void* g, float* ldsbase, const int aux_sc1) {
    if (aux_sc1)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)ldsbase, 4, 0, T2V_SC1);
    else
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)ldsbase, 4, 0, 0);
}

template <int NB>
__device__ __forceinline__ void pb_park_factors(float* ldsX, const float* Frow) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NCH = PB_ROW_BYTES(NB) / 1024;
#pragma unroll
    for (int i = 0; i < NCH / 8; ++i) {
        const int c = wave + 8 * i;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Frow + 256 * c + 4 * lane),
                                         (__attribute__((address_space(3))) void*)(ldsX + 256 * c), 16, 0, 0);
    }
}
template <int NB>
__device__ __forceinline__ int pb_build_row(f32x4* X0, f32x2* X1, __amdgpu_buffer_rsrc_t r, unsigned row_off, int B,
                                            int nap, unsigned* err, int* flag) {
    const int tid = threadIdx.x;
    for (int i = 0; i < nap; i += 8) __builtin_amdgcn_s_sleep(8);
    f32x4 dc[2], dh[2], dx[2];
    int rounds = 0;
    const int nw0 = min(B, 4), nw1 = B - 4;
    for (;;) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned U = (unsigned)(tid + PB_THREADS * h);
            dc[h] = t2v_ld_f32x4(r, row_off + 32u * U);
            dh[h] = t2v_ld_f32x4(r, row_off + 32u * U + 16u);
            if (NB > 4) dx[h] = t2v_ld_f32x4(r, row_off + 32768u + 16u * U);
        }
        bool ok = true;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            ok = ok && t2v_ok(dc[h][0]) && (nw0 < 2 || t2v_ok(dc[h][1])) && (nw0 < 3 || t2v_ok(dc[h][2])) && (nw0 < 4 || t2v_ok(dc[h][3]));
            ok = ok && t2v_ok(dh[h][0]) && (nw0 < 2 || t2v_ok(dh[h][1])) && (nw0 < 3 || t2v_ok(dh[h][2])) && (nw0 < 4 || t2v_ok(dh[h][3]));
            if (NB > 4) ok = ok && t2v_ok(dx[h][0]) && t2v_ok(dx[h][2]) && (nw1 < 2 || (t2v_ok(dx[h][1]) && t2v_ok(dx[h][3])));
        }
        if (__all(ok)) break;
        __builtin_amdgcn_s_sleep(2);
        if (t2v_give_up(rounds, PB_SPIN, err, flag)) break;
    }
#pragma unroll
    for (int j = 0; j < PB_KJ; ++j) {
        const int h = j & 1;
        const f32x4 d = (j >> 1) == 3 ? dh[h] : dc[h];
        X0[tid + PB_THREADS * j] = X0[tid + PB_THREADS * j] * d;
        if (NB > 4) X1[tid + PB_THREADS * j] = X1[tid + PB_THREADS * j] * ((j >> 1) == 3 ? f32x2{dx[h][2], dx[h][3]} : f32x2{dx[h][0], dx[h][1]});
    }
    return rounds;
}

// F[t][k][item] of one cell: the factor that turns (d c_t, d h_t) into the gate gradient of row k (layout of a gate row)
__global__ __launch_bounds__(256) void k_pb_factors(const float* __restrict__ G, const float* __restrict__ C, float* __restrict__ F,
                                                    int B, int T, int nb, float p, int stream_c, uint64_t seed0,
                                                    const t2v_step_params* step) {
    const uint64_t seed = t2v_step_seed(seed0, step);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)T * T2V_G) return;
    const int t = (int)(i / T2V_G), k = (int)(i % T2V_G), r = k >> 10, U = k & (T2V_H - 1);
    float f[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        f[b] = 0.f;
        if (b < B) {
            const float* gp = G + ((size_t)t * B + b) * T2V_G + U;
            const float gi = gp[0], gf = gp[T2V_H], gg = gp[2 * T2V_H], go = gp[3 * T2V_H];
            if (r == 0) f[b] = gg * gi * (1.0f - gi);
            else if (r == 2) f[b] = gi * (1.0f - gg * gg);
            else if (r == 3) f[b] = tanhf_(C[((size_t)(t + 1) * B + b) * T2V_H + U]) * go * (1.0f - go);
            else {
                float cprev = C[((size_t)t * B + b) * T2V_H + U];
                if (t > 0) cprev *= t2v_drop_scale(seed, stream_c, t - 1, (uint32_t)b * T2V_H + U, p);
                f[b] = cprev * gf * (1.0f - gf);
            }
        }
    }
    float* row = F + (size_t)t * (nb > 4 ? 6 : 4) * T2V_G;
    *(f32x4*)(row + 4 * (size_t)k) = f32x4{f[0], f[1], f[2], f[3]};
    if (nb > 4) *(f32x2*)(row + 4 * T2V_G + 2 * (size_t)k) = f32x2{f[4], f[5]};
}

// CP[t][U][item (nb slots)][8] of one cell: everything the cell backward of (unit U, item) needs at step t that is a function
// of the forward activations alone — {fh, fc, go (1 - tanh(c)^2), gf,  gg gi (1 - gi), c' gf (1 - gf), gi (1 - gg^2),
// tanh(c) go (1 - go)} (fh / fc: state-dropout scales of step t, c': the cell handed to step t, dropout applied).  Round 4:
// the attention_rnn workgroups used to compute these in the loop — three counter-based RNG draws and a tanh per
// (unit, item) and step, 1.5 us of every 12.9 us reverse step on the chain; now they copy 32 bytes.
__global__ __launch_bounds__(256) void k_pb_cellpre(const float* __restrict__ G, const float* __restrict__ C, float* __restrict__ CP,
                                                    int B, int T, int nb, float p, int stream_h, int stream_c, uint64_t seed0,
                                                    const t2v_step_params* step) {
    const uint64_t seed = t2v_step_seed(seed0, step);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)T * T2V_H * nb) return;
    const int b = (int)(i % nb), U = (int)((i / nb) % T2V_H), t = (int)(i / ((size_t)nb * T2V_H));
    float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0;
    if (b < B) {
        const float* gp = G + ((size_t)t * B + b) * T2V_G + U;
        const float gi = gp[0], gf = gp[T2V_H], gg = gp[2 * T2V_H], go = gp[3 * T2V_H];
        const float cc = C[((size_t)(t + 1) * B + b) * T2V_H + U];
        float cprev = C[((size_t)t * B + b) * T2V_H + U];
        const uint32_t idx = (uint32_t)b * T2V_H + U;
        const float fh = t2v_drop_scale(seed, stream_h, t, idx, p);
        const float fc = t2v_drop_scale(seed, stream_c, t, idx, p);
        if (t > 0) cprev *= t2v_drop_scale(seed, stream_c, t - 1, idx, p);
        const float tc = tanhf_(cc);
        c0 = make_float4(fh, fc, go * (1.0f - tc * tc), gf);
        c1 = make_float4(gg * gi * (1.0f - gi), cprev * gf * (1.0f - gf), gi * (1.0f - gg * gg), tc * go * (1.0f - go));
    }
    float4* o = (float4*)(CP + i * 8);
    o[0] = c0;
    o[1] = c1;
}

// acc[c][pair] += w[c][j] * x[k_j][pair] for NC output columns: packed FMAs (two items per op, weight broadcast through
// op_sel; even j = low word of the weight pair, odd j = high word) in volatile asm so the k loop keeps its shape.
template <bool ODD>
__device__ __forceinline__ void pb_pk3(f32x2& a01, f32x2& a23, f32x2& a45, f32x2 w, f32x2 x01, f32x2 x23, f32x2 x45) {
    if (ODD)
        asm volatile("v_pk_fma_f32 %0, %3, %4, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                     "v_pk_fma_f32 %1, %3, %5, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                     "v_pk_fma_f32 %2, %3, %6, %2 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                     : "+v"(a01), "+v"(a23), "+v"(a45) : "v"(w), "v"(x01), "v"(x23), "v"(x45));
    else
        asm volatile("v_pk_fma_f32 %0, %3, %4, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                     "v_pk_fma_f32 %1, %3, %5, %1 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                     "v_pk_fma_f32 %2, %3, %6, %2 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                     : "+v"(a01), "+v"(a23), "+v"(a45) : "v"(w), "v"(x01), "v"(x23), "v"(x45));
}

// Sum 16 per-thread values (2 columns x 8 item slots) over the 512 threads of the workgroup: 16-lane transposing butterfly,
// then the 32 row partials (8 waves x 4 rows) through LDS; the caller syncs and sums the partials it needs (pb_sum16).
// Twice the rounds of a 32-value reduction for the same number of DPP operations, but the GEMV's working set next to the weight registers halves
// (12 accumulator registers + 16 values instead of 24 + 32) — with 32-value rounds the role spilled loop-invariant offsets
// and every reload sat behind an s_waitcnt vmcnt(0) on the chain.  The first two levels write complementary register banks
// with bank-masked DPP adds (2 operations per output instead of select + select + add).  part[(wave * 4 + row) * 16 + idx].
__device__ __forceinline__ float pb_dpp_pair_add(float lo, float hi, const int level) {
    float t;
    if (level == 0)
        asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_mirror row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %0, %2, %2 row_mirror row_mask:0xf bank_mask:0xc" : "=&v"(t) : "v"(lo), "v"(hi));
    else
        asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %0, %2, %2 row_half_mirror row_mask:0xf bank_mask:0xa" : "=&v"(t) : "v"(lo), "v"(hi));
    return t;
}
__device__ __forceinline__ void pb_reduce16(float (&v)[16], float* part) {
    const int tid = threadIdx.x, lane = tid & 63;
    const bool b1 = lane & 2, b0 = lane & 1;
    float w8[8], w4[4], w2[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) w8[i] = pb_dpp_pair_add(v[i], v[8 + i], 0);          // lanes 0..7 of a row: values i, lanes 8..15: 8 + i
#pragma unroll
    for (int i = 0; i < 4; ++i) w4[i] = pb_dpp_pair_add(w8[i], w8[4 + i], 1);        // bit 2 of the lane picks the half
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float keep = b1 ? w4[2 + i] : w4[i], send = b1 ? w4[i] : w4[2 + i];
        w2[i] = keep + T2V_DPP_F(send, 0x4E);
    }
    const float keep = b0 ? w2[1] : w2[0], send = b0 ? w2[0] : w2[1];
    part[((tid >> 6) * 4 + (lane >> 4)) * 16 + (lane & 15)] = keep + T2V_DPP_F(send, 0xB1);
}
__device__ __forceinline__ float pb_sum16(const float* part, int idx) {
    float s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = (part[(4 * i) * 16 + idx] + part[(4 * i + 1) * 16 + idx]) + (part[(4 * i + 2) * 16 + idx] + part[(4 * i + 3) * 16 + idx]);
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

static size_t pb_row_bytes(int B) { return B > 4 ? 98304u : 65536u; }

extern "C" int t2v_decoder_bwd_persist_supported(int B, int T_in) {
    if (!(B >= 1 && B <= PB_MAXB && T_in >= 1 && T_in <= PB_MAXT_LONG)) return 0;
    return t2v_persist_cus_ok();
}

// ======================================================================= the reverse pass as one launch
// Roles (one workgroup per CU):
//   T : workgroups [0, B*S) — attention(t) backward of item b, encoder positions [s*JS, s*JS + JS) (the position-split
//       body of decoder_bwd.hip: softmax / tanh / fused-location-filter backward), operands that do not change over the
//       pass (memory rows, W_comb^T tile, v) resident in registers, the cumulative-weights gradient resident in LDS.
//       Runs on the first 256 threads; waves 4..7 only keep the barriers company.
//   A, D : the other NL = 256 - B*S workgroups, one set per LSTM cell (pba_na below): a workgroup owns a range of hidden
//       units and of context columns and keeps their columns of Wcat_att^T (A) or Wcat_dec^T (D) in registers (thread = 8
//       of the 4096 gate rows).  decoder_rnn's chain needs nothing of the attention path and free-runs ahead of it.
// Per reverse step the dependency chain is
//   all-gather dga(t+1) -> A-GEMV -> [d ctx(t)] -> hop -> attention(t) backward -> [dq(t)] -> hop -> W_q^T dq + cell A(t)
//   -> [dga(t)] -> all-gather ...
struct PBAArgs {
    // weights
    const float* w_ih_att; const float* w_hh_att; const float* w_ih_dec; const float* w_hh_dec;
    const float* wq;            // (128,1024)
    const float* wcomb;         // fused location filter (both copies)
    const float* v;             // (128)
    // saved by the forward pass
    const float* memory; const float* XS; const float* CA; const float* CD; const float* GA; const float* GD; const float* AL;
    float* S;                   // (T,B,T_in,128) in: tanh outputs, out: dpre
    const float* dHC;           // (T,B,1536)
    // outputs
    float* DGA; float* DGD; float* DCTX; float* DV;       // DV (B,S,128)
    // exchange (sentinel-filled): gate-gradient rows of both cells, context gradients, dq partials, window partials
    float* GXA; float* GXD; float* CX; float* DQX; float* GPX; float* EX;
    float* DQT;                 // (T,B,128) dq(t) summed over the position slices (published by slice 0 of each item)
    const float* CPA;           // (T,1024,NB,8) cell-layout factors of attention_rnn (k_pb_cellpre)
    const float* CPD;           // the same for decoder_rnn
    const float* FA; const float* FD;    // gate-gradient factors of both cells (k_pb_factors)      // EX (T,B,1536): E(t) = Wcat_dec[:, :1536]^T dgd(t)
    unsigned* err;
    int B, T_in, T, S_sl;
    float p_att, p_dec;
    uint64_t seed;
    const t2v_step_params* step;
    unsigned long long* prof;
    // weight-gradient epilogue of the decoder_rnn role (pba_dw_epilogue; dw_planes == nullptr: the role returns as before)
    uint4* dw_planes; float* dw_ih; float* dw_hh; unsigned* dw_ctr;
    int dw_ld_ih, dw_ld_hh, dw_accumulate, dw_cap, dw_margin;    // last, so that every field above sits where it sat before the operand existed
    const float* dAL;           // (T,B,T_in) upstream gradient of the alignments (the DAL kernels; nullptr in the others)
};
// phase profile (tools/dbg/persist_bwd_prof.py): slot I accumulates, over all steps, the cycles since the previous stamp
#define PBA_STAMP(COND, I) do { if (a.prof && (COND) && threadIdx.x == 0) { const unsigned long long now_ = __builtin_readcyclecounter(); \
        lprof_[(I)] += now_ - tprev_; tprev_ = now_; } } while (0)
// per-workgroup time line of ONE step (t = T/2) on the chip-wide 100 MHz counter: prof[64 + workgroup * 8 + slot]
#define PBA_RT(SLOT) do { if (a.prof && t == a.T / 2 && threadIdx.x == 0) a.prof[64 + blockIdx.x * 8 + (SLOT)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define PBA_PROF_INIT(FLAGP) unsigned long long* lprof_ = (unsigned long long*)((FLAGP) + 4); \
    if (threadIdx.x < 16) lprof_[threadIdx.x] = 0ull
#define PBA_PROF_FLUSH(COND, I0, N) do { if (a.prof && (COND) && threadIdx.x < (N)) a.prof[(I0) + threadIdx.x] = lprof_[(I0) + threadIdx.x]; } while (0)

// context-gradient row of a step in CX: [item (4 or 8 slots)][512 columns] — item-major (round 4): an attention_rnn workgroup
// publishes its <= 7 columns of an item as ONE 16-byte store (+ <= 3 words) instead of 4-byte stores 16 bytes apart, and an
// attention workgroup polls its item's 2 KB with 128 sixteen-byte loads instead of 512 four-byte loads spread over 8 KB
// (second form, round 4: [item][attention_rnn workgroup (128 slots)][8 floats] — every producer owns an aligned 32-byte slot,
// no cache line sector is ever written by two workgroups)
#define PB_CX_ROW_BYTES(NB) ((NB) > 4 ? 32768u : 16384u)

__host__ __device__ static inline int pba_na(int NL);
// The attention role is t2v_attn_role_bwd.h; here is what it takes from this kernel.  d ctx(t) of item b lies in CX as the NAw
// attention_rnn workgroups published it: threads [0, 2 NAw) poll their 16-byte slots, scatter by the producers' column ranges.
template <int NB>
struct PBAAttnHooks {
    static constexpr int SPIN = PB_SPIN;
    const PBAArgs& a;
    const int b, NAw;                     // NAw: attention_rnn workgroups, the producers of the context gradient
    const __amdgpu_buffer_rsrc_t rC;
    unsigned long long* lprof_;
    unsigned long long tprev_;
    __device__ __forceinline__ PBAAttnHooks(const PBAArgs& a_, int b_, int)
        : a(a_), b(b_), NAw(pba_na(T2V_NWG - a_.B * a_.S_sl)), rC(t2v_rsrc(a_.CX)), lprof_(nullptr), tprev_(0ull) {}
    __device__ __forceinline__ int dqt_items() const { return a.B; }
    __device__ __forceinline__ void dctx_early(int, int, int*) {}
    __device__ __forceinline__ void dctx_arrive(int t, int tid, float* dctx, int& nap, int* flag) {
        if (tid < 2 * NAw) {
            const unsigned off = (unsigned)t * PB_CX_ROW_BYTES(NB) + (unsigned)b * 4096u + 16u * (unsigned)tid;
            for (int i = 0; i < nap; i += 8) __builtin_amdgcn_s_sleep(8);
            // TWO polls in flight, half a round trip apart (round 4): with one, a row that lands just after a poll left is
            // only seen a full memory round trip later
            f32x4 x, x0 = t2v_ld_f32x4(rC, off);
            __builtin_amdgcn_s_sleep(4);
            f32x4 x1 = t2v_ld_f32x4(rC, off);
            int rounds = 0;
            for (;;) {
                if (__all(t2v_ok4(x0))) { x = x0; break; }
                x0 = t2v_ld_f32x4(rC, off);
                if (__all(t2v_ok4(x1))) { x = x1; break; }
                x1 = t2v_ld_f32x4(rC, off);
                if (t2v_give_up(rounds, PB_SPIN, a.err, flag)) { x = x0; break; }
            }
            nap = t2v_adapt_nap(nap, rounds);
            // slot (workgroup ja, half h) holds columns c0(ja) + 4 h .. of this item
            const int ja = tid >> 1, h4 = 4 * (tid & 1);
            const int cc0 = (ja * T2V_E) / NAw, ncc = ((ja + 1) * T2V_E) / NAw - cc0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (h4 + i < ncc) dctx[cc0 + h4 + i] = x[i];
        }
    }
    // phase profile of workgroup 0 (slots 8..11) + the time line of step T/2
    __device__ __forceinline__ void prof_init(int* flag) {
        lprof_ = (unsigned long long*)(flag + 4);
        if (threadIdx.x < 16) lprof_[threadIdx.x] = 0ull;
    }
    __device__ __forceinline__ void pass_begin() { tprev_ = __builtin_readcyclecounter(); }
    __device__ __forceinline__ void stamp(int t, int point) {
        PBA_STAMP(blockIdx.x == 0, 8 + point);
        if (point == T2V_AB_DCTX) PBA_RT(0);
        if (point == T2V_AB_DQ) PBA_RT(1);
    }
    __device__ __forceinline__ void pass_end() { PBA_PROF_FLUSH(blockIdx.x == 0, 8, 4); }
};
template <int JS, int NWV, int NB, bool DAL>
__device__ __forceinline__ void pba_attention(const PBAArgs& a, float* lds, const int b, const int s) {
    t2v_attn_role_bwd<JS, NWV, PBAAttnHooks<NB>, DAL>(a, lds, b, s);
}

// y[C0 + c][pair] = sum_j w[C0 + c][j] * x[k_j][pair] for NC <= 2 of the thread's columns into v[16] (two columns x 8 item
// slots); one LDS operand per gate row with three more in flight (the weight registers leave no room for all eight), and
// the operand rows are re-read per round
template <int NCT, int C0, int NC, int NB>
__device__ __forceinline__ void pb_gemv_cols16(const f32x2 (&w)[NCT][PB_KJ / 2], const f32x4* X0, const f32x2* X1, float (&v)[16]) {
    static_assert(NC >= 1 && NC <= 2, "one or two columns");
    const int tid = threadIdx.x;
    f32x2 acc[NC][3];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c][0] = acc[c][1] = acc[c][2] = f32x2{0.f, 0.f};
    constexpr int PF = 4;
    f32x4 xa[PF];
    f32x2 xb[PF];
#pragma unroll
    for (int d = 0; d < PF; ++d) {
        xa[d] = X0[tid + PB_THREADS * d];
        xb[d] = f32x2{0.f, 0.f};
        if (NB > 4) xb[d] = X1[tid + PB_THREADS * d];
    }
#pragma unroll
    for (int j = 0; j < PB_KJ; ++j) {
        const f32x4 xc = xa[j % PF];
        const f32x2 yc = xb[j % PF];
        const f32x2 x01 = {xc[0], xc[1]}, x23 = {xc[2], xc[3]};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (j & 1) pb_pk3<true>(acc[c][0], acc[c][1], acc[c][2], w[C0 + c][j / 2], x01, x23, yc);
            else pb_pk3<false>(acc[c][0], acc[c][1], acc[c][2], w[C0 + c][j / 2], x01, x23, yc);
        }
        if (j + PF < PB_KJ) {
            xa[j % PF] = X0[tid + PB_THREADS * (j + PF)];
            if (NB > 4) xb[j % PF] = X1[tid + PB_THREADS * (j + PF)];
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) { v[c * 8 + 2 * i] = acc[c][i][0]; v[c * 8 + 2 * i + 1] = acc[c][i][1]; }
}

// columns [C0, C0 + N) two at a time: round r leaves its 32 row partials x 16 values at part + 512 r
template <int NCT, int C0, int N, int NB, int R = 0>
__device__ __forceinline__ void pba_rounds16(const f32x2 (&w)[NCT][PB_KJ / 2], const f32x4* X0, const f32x2* X1, float* part) {
    if constexpr (2 * R < N) {
        float v[16];
        pb_gemv_cols16<NCT, C0 + 2 * R, (N - 2 * R >= 2 ? 2 : 1), NB>(w, X0, X1, v);
        pb_reduce16(v, part + 512 * R);
        pba_rounds16<NCT, C0, N, NB, R + 1>(w, X0, X1, part);
    }
}

// ---- role split of the LSTM workgroups (NL = 256 - B*S of them).  One workgroup set per cell halves the gate-gradient
// all-gather (a row of 4096 x B values goes to the workgroups of ITS cell only) and decouples the two chains:
//   A role, NA = 3/8 of NL workgroups: attention_rnn.  Workgroup ja owns hidden units [ja*1024/NA, ..) (<= 14) and context
//           columns [ja*512/NA, ..) (<= 7): their columns of Wcat_att^T in registers.  This is the per-step chain.
//   D role, ND = NL - NA workgroups: decoder_rnn.  Workgroup jd owns units [jd*1024/ND, ..) (<= 8, both the h_att-input
//           and the recurrent column of each) and context columns [jd*512/ND, ..) (<= 4): columns of Wcat_dec^T.  Its
//           loop needs only dHC and its own recurrence, so it FREE-RUNS ahead of the A chain and leaves
//           E(t) = Wcat_dec[:, :1536]^T dgd(t) — decoder_rnn's contribution to d h_att(t) / d ctx(t) — in a sentinel-filled
//           array the A workgroups read when they get there.
#define PBA_NUA 13
#define PBA_NCA 7
#define PBA_NUD 8
#define PBA_NCD 4
// (>= 79 workgroups: at most 13 units and 7 context columns each — 20 columns = 160 weight registers per thread)
// Round 4: the decoder_rnn role needs 128 workgroups to stay at 8 units + 4 context columns (20 columns) each; every other
// LSTM workgroup goes to the attention_rnn role, the per-step chain.  From 86 workgroups on it holds <= 12 units + 6 context
// columns (18 columns = 144 weight registers: the slim instantiation — one reduction round less per step and 16 registers
// fewer next to the GEMV's working set); below that the 13 + 7 form.
__host__ __device__ static inline int pba_na(int NL) {
    if (NL - 128 >= 86) return NL - 128;
    const int n = (3 * NL + 4) / 8;
    return n < 79 ? 79 : n;
}

// poll one word of a sentinel-filled array until it is written (bounded)
__device__ __forceinline__ float pba_wait_word(__amdgpu_buffer_rsrc_t r, unsigned off, unsigned* err, int* flag) {
    unsigned x;
    int spins = 0;
    for (;;) {
        x = t2v_ld_b32(r, off);
        if (x != T2V_SENT) break;
        __builtin_amdgcn_s_sleep(1);
        if (t2v_give_up(spins, PB_SPIN, err, flag)) break;
    }
    return __uint_as_float(x);
}

// stage[u][{dc, dh}][8 items] -> one 16-byte (+ one 8-byte) write-through store per unit and quantity
template <int NB>
__device__ __forceinline__ void pba_publish_rows(__amdgpu_buffer_rsrc_t r, unsigned row_off, const float* stage, int u0, int nu) {
    const int tid = threadIdx.x;
    if (tid < 2 * nu) {
        const int u = tid >> 1, q = tid & 1;
        const float* sp = stage + (u * 2 + q) * 8;
        t2v_st(r, row_off + 32u * (unsigned)(u0 + u) + 16u * (unsigned)q, f32x4{sp[0], sp[1], sp[2], sp[3]});
        if (NB > 4) t2v_st(r, row_off + 32768u + 16u * (unsigned)(u0 + u) + 8u * (unsigned)q, f32x2{sp[4], sp[5]});
    }
}


// ------------------------------------------------------------------------------------------------ D role, behind its time loop
// The decoder_rnn workgroups finish their chain T x (chain step - own step) before the attention_rnn chain ends (0.88 ms at B = 6,
// T = 400) and used to return.  Now they work on decoder_rnn's own weight gradients, [d_w_ih_dec | d_w_hh_dec] = DGD^T · x_cur — the
// larger of the two groups of the grouped launch behind the pass (t2v_gemm_f32_grouped_handed), which needs nothing but what this
// role has finished — with that launch's own code (gemm_x3_tile.h), so that a tile has the same bits whoever computes it:
//   1. barrier over the ND decoder_rnn workgroups (DGD left with plain stores: one release / acquire pair per workgroup and pass);
//   2. the split passes of DGD and x_cur into the grouped launch's planes, blocks dealt round robin; barrier;
//   3. 128 x 128 tiles, two side by side per workgroup (one per 256 threads, 48 KB of LDS each), taken in pairs from a counter.
// A workgroup stops taking tiles once the attention_rnn chain has published its (dc, dh) row of step dw_margin: the pass must never
// end later because of this.  The grouped launch reads the counter and computes the tiles from there on.
// A barrier that gives up (bounded spin) makes its workgroup return with the group's planes incomplete, and the grouped launch behind
// the pass — which issues no split launches for this group — then computes garbage from them: a.err, which the give-up sets and the
// host raises on, is the sole guard for that case, as for every other wait of this kernel.
// Control words in the pass's scratch (zeroed by the preparation): [0] tiles taken, [1], [2] the two barriers' arrivals.
// Profile (a.prof, workgroup jd = 0): [44] entry, [45] barrier 1 passed, [46] planes made + barrier 2 passed, [47] last tile done,
// [48] tile pairs of this workgroup; all on the 100 MHz counter.
struct PBADw {
    const float* DGD; const float* XC; uint4* planes; float* c_ih; float* c_hh; unsigned* ctr; const float* GXA; unsigned* err;
    unsigned long long* prof;
    int K, ld_ih, ld_hh, accumulate, cap, margin_off, jd, ND;
};
#define PBA_DW_CTL_SLOT (2 * GX_TILE_SLOTS(3, 2))       // control words in LDS behind the two tile buffers
static_assert(16 * (PBA_DW_CTL_SLOT + 1) <= 4 * PBA_LROLE_FLOATS(4), "the epilogue's LDS fits the LSTM roles' allocation");

// all threads of the workgroup; every store of this workgroup issued so far is visible to whoever passes.  False: gave up (a.err set).
// ONE wave per workgroup releases and acquires at agent scope (behind / in front of a workgroup barrier that covers the others): each
// such fence writes back resp. invalidates the XCD's L2 under the attention_rnn chain — with all eight waves at it the pass in the
// training step was 0.13 ms longer than without the epilogue, with one 0.08 ms
__device__ __forceinline__ bool pba_dw_barrier(unsigned* ctr, int n, unsigned* err, int* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        int rounds = 0;
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)n) {
            __builtin_amdgcn_s_sleep(8);
            if (t2v_give_up(rounds, PB_SPIN, err, flag)) break;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    return flag[0] == 1;
}

__device__ __noinline__ void pba_dw_epilogue(const PBADw d, float* lds) {
    const int tid = threadIdx.x, half = tid >> 8, t2 = tid & 255;
    uint4* const slots = (uint4*)lds;
    int* const flag = (int*)(slots + PBA_DW_CTL_SLOT);          // [0] healthy, [1] first tile of the pair taken (-1: stop)
    const bool prof = d.prof && d.jd == 0 && tid == 0;
    if (prof) d.prof[44] = __builtin_amdgcn_s_memrealtime();
    __syncthreads();                                            // (the time loop's last LDS reads)
    if (tid == 0) flag[0] = 1;
    if (!pba_dw_barrier(d.ctr + 1, d.ND, d.err, flag)) return;
    if (prof) d.prof[45] = __builtin_amdgcn_s_memrealtime();
    // ---- 2. planes: A = DGD as (4096 rows, K), B = x_cur as (2560 rows, K), both contiguous along their rows
    const long G = gx_groups(d.K);
    uint4* const Ap = d.planes;
    uint4* const Bp = Ap + gx_plane_slots(T2V_G, d.K);
    {
        uint4 (*sm)[4][64] = (uint4 (*)[4][64])(slots + half * (3 * 4 * 64));
        const int gy = (int)(G / 4), nA = (T2V_G / 64) * gy, total = nA + (T2V_XW / 64) * gy;
        const int W = 2 * d.ND, w = 2 * d.jd + half;
        for (int i0 = 0; i0 < total; i0 += W) {
            const bool on = i0 + w < total;
            const int i = on ? i0 + w : 0;
            const bool isA = i < nA;
            const int rows = isA ? T2V_G : T2V_XW, j = isA ? i : i - nA, nbx = rows / 64;
            gx_split_block<false, 3>(isA ? d.DGD : d.XC, 1, rows, rows, d.K, isA ? Ap : Bp, rows, G, j % nbx, j / nbx, t2, sm, on);
            __syncthreads();                                    // sm is free again
        }
    }
    if (!pba_dw_barrier(d.ctr + 2, d.ND, d.err, flag)) return;
    if (prof) d.prof[46] = __builtin_amdgcn_s_memrealtime();
    // ---- 3. tiles
    GemmX3Args ga;
    {
        GemmX3Prod& P = ga.pr[0];
        P.Ap = Ap; P.Bp = Bp; P.RpA = T2V_G; P.RpB = T2V_XW; P.N = T2V_XW; P.tiles_x = T2V_XW / GX_BN; P.tile0 = 0; P.nseg = 2;
        P.seg_col[0] = 0; P.seg_col[1] = T2V_KATT; P.seg_col[2] = 0x7fffffff;
        P.segC[0] = d.c_ih; P.segC[1] = d.c_hh; P.segC[2] = d.c_hh;
        P.seg_ldc[0] = d.ld_ih; P.seg_ldc[1] = d.ld_hh; P.seg_ldc[2] = d.ld_hh;
        ga.pr[1] = P;
        ga.nprod = 1; ga.ntiles = (T2V_G / GX_BM) * (T2V_XW / GX_BN); ga.G = G; ga.bias = nullptr; ga.M = T2V_G; ga.relu = 0;
        ga.accumulate = d.accumulate; ga.p_drop = 0.f; ga.seed = 0; ga.rng_stream = 0; ga.rng_t = 0; ga.step = nullptr;
        ga.st_chunk = 0; ga.part = nullptr; ga.tile_ctr = nullptr; ga.done_ctr = nullptr; ga.done_prod = 0; ga.done_cap = 0;
    }
    const int limit = min(ga.ntiles, d.cap);
    const __amdgpu_buffer_rsrc_t rA = t2v_rsrc(d.GXA);
    unsigned npair = 0;
    for (;;) {
        if (tid == 0) {
            int take = -1;
            // (margin_off < 0: a pass too short for a single pair)
            if (limit > 0 && d.margin_off >= 0 && t2v_ld_b32(rA, (unsigned)d.margin_off) == T2V_SENT) {
                const unsigned t = __hip_atomic_fetch_add(d.ctr, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (t < (unsigned)limit) take = (int)t;
            }
            flag[1] = take;
        }
        __syncthreads();
        const int take = flag[1];
        __syncthreads();
        if (take < 0) break;
        const int lin = take + half;
        gx_tile<3, 2, false>(ga, ga.pr[0], min(lin, limit - 1), t2, slots + half * GX_TILE_SLOTS(3, 2), 0, 1, lin < limit);
        ++npair;
    }
    if (prof) { d.prof[47] = __builtin_amdgcn_s_memrealtime(); d.prof[48] = npair; }
}

// ------------------------------------------------------------------------------------------------ D role (free-running)
template <int NB>
__device__ __forceinline__ void pba_decoder_role(const PBAArgs& a, float* lds, const int jd, const int ND) {
    const int B = a.B, T = a.T;
    f32x4* X0 = (f32x4*)lds;
    f32x2* X1 = (f32x2*)(lds + 4 * T2V_G);
    float* part = lds + (NB > 4 ? 6 : 4) * T2V_G;          // [10 rounds][32 row partials][16]
    float* stage = part + 10 * 512;                        // [8 units][2][8]
    float* cpd = stage + 256;                              // [2][64 rows][8] cell-layout factors of steps td, td-1 (k_pb_cellpre)
    float* dhcs = cpd + 1024;                              // [2][64] dHC words of the cell threads
    int* flag = (int*)(dhcs + 128);
    const int u0 = (jd * T2V_H) / ND, nu = ((jd + 1) * T2V_H) / ND - u0;      // <= 8 units
    const int c0 = (jd * T2V_E) / ND, nc = ((jd + 1) * T2V_E) / ND - c0;      // <= 4 context columns
    const __amdgpu_buffer_rsrc_t rD = t2v_rsrc(a.GXD), rE = t2v_rsrc(a.EX), rDG = t2v_rsrc(a.DGD);
    // columns: [0, 8) recurrent (W_hh_dec[k][U]), [8, 16) h_att input (W_ih_dec[k][U]), [16, 20) ctx input (W_ih_dec[k][1024 + C])
    f32x2 w[20][PB_KJ / 2];
    {
        const int tid = threadIdx.x;
#pragma unroll
        for (int jj = 0; jj < PB_KJ; ++jj) {
            const size_t k = (size_t)(tid + PB_THREADS * jj);
#pragma unroll
            for (int u = 0; u < PBA_NUD; ++u) {
                const bool on = u < nu;
                const int U = u0 + (on ? u : 0);
                w[u][jj / 2][jj & 1] = on ? a.w_hh_dec[k * T2V_H + U] : 0.f;
                w[8 + u][jj / 2][jj & 1] = on ? a.w_ih_dec[k * T2V_KATT + U] : 0.f;
            }
#pragma unroll
            for (int c = 0; c < PBA_NCD; ++c) {
                const bool on = c < nc;
                w[16 + c][jj / 2][jj & 1] = on ? a.w_ih_dec[k * T2V_KATT + T2V_H + c0 + (on ? c : 0)] : 0.f;
            }
        }
        if (tid == 0) flag[0] = 1;
    }
    float dcd = 0.f;
    int nap = 0;
    // cell-layout factors of the own units: nu * NB rows of 8 floats, contiguous per step (thread i < 2 nu NB moves float4 i)
    const int ncp4 = 2 * nu * NB;
    const float* cpd0 = a.CPD + (size_t)u0 * NB * 8;
    constexpr size_t CPSTEP = (size_t)T2V_H * NB * 8;
    {
        const int tid = threadIdx.x;
        if (tid < ncp4) *(float4*)(cpd + ((T - 1) & 1) * 512 + 4 * tid) = *(const float4*)(cpd0 + (size_t)(T - 1) * CPSTEP + 4 * tid);
        const int cu = tid >> 3, cb = tid & 7;
        if (tid < 64 && cu < nu && cb < B) dhcs[((T - 1) & 1) * 64 + tid] = a.dHC[((size_t)(T - 1) * B + cb) * (T2V_H + T2V_E) + u0 + cu];
    }
    pb_park_factors<NB>(lds, a.FD + (size_t)(T - 1) * (PB_ROW_BYTES(NB) / 4));
    __syncthreads();

    if (a.prof && jd == 0 && threadIdx.x == 0) a.prof[40] = __builtin_amdgcn_s_memrealtime();
    // iteration t: (t < T) gather (dc, dh)(t) and build dgd(t); the RECURRENT columns of Wcat_dec^T dgd(t) first — they feed cell
    // D(t-1), whose (dc, dh) row is this role's own chain — then, behind the hand-off, the 12 columns of E(t) for the other role
    // (round 4; before, all 20 columns and the in-loop RNG / tanh of the cell sat on the chain: 9.9 -> 8.5 us per step)
    for (int t = T; t >= 0; --t) {
        int tid_op = threadIdx.x;
        asm volatile("" : "+v"(tid_op));       // (see the attention_rnn role: nothing thread-derived is hoisted out of the loop)
        const int tid = tid_op;
        const int cu = tid >> 3, cb = tid & 7;
        const bool cell_thr = tid < 64 && cu < nu && cb < B;
        const int U = u0 + (cu < nu ? cu : 0);
        if (t < T) {
            const int rounds = pb_build_row<NB>(X0, X1, rD, (unsigned)t * PB_DROW_BYTES(NB), B, nap, a.err, flag);
            nap = t2v_adapt_nap(nap, rounds);
            pba_rounds16<20, 0, 8, NB>(w, X0, X1, part);
        }
        // prefetch for the NEXT cell (step t-2): its factors and its dHC words, straight into LDS
        if (t >= 2) {
            if (tid < ncp4)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(cpd0 + (size_t)(t - 2) * CPSTEP + 4 * tid),
                                                 (__attribute__((address_space(3))) void*)(cpd + ((t - 2) & 1) * 512 + 256 * (tid >> 6)), 16, 0, 0);
            if (cell_thr) pb_dma4(a.dHC + ((size_t)(t - 2) * B + cb) * (T2V_H + T2V_E) + U, dhcs + ((t - 2) & 1) * 64, 0);
        }
        __syncthreads();
        if (flag[0] != 1) return;
        f32x4 dg4 = {0.f, 0.f, 0.f, 0.f};
        if (t >= 1) {
            const int td = t - 1;
            if (cell_thr) {
                const float dh = dhcs[(td & 1) * 64 + tid] + (t < T ? pb_sum16(part + (cu >> 1) * 512, (cu & 1) * 8 + cb) : 0.f);
                const float* cp = cpd + (td & 1) * 512 + (cu * NB + cb) * 8;
                const float4 c0v = *(const float4*)cp, c1v = *(const float4*)(cp + 4);
                const float dht = dh * c0v.x;                         // fh
                const float dct = dcd * c0v.y + dht * c0v.z;          // fc, go (1 - tanh(c)^2)
                dg4 = f32x4{dct * c1v.x, dct * c1v.y, dct * c1v.z, dht * c1v.w};
                dcd = dct * c0v.w;                                    // gf
                float* sp = stage + (cu * 2) * 8 + cb;
                sp[0] = dct; sp[8] = dht;
            }
            // (stage is written and read by wave 0 only: LDS operations of one wave complete in order)
            if (tid < 64) pba_publish_rows<NB>(rD, (unsigned)td * PB_DROW_BYTES(NB), stage, u0, nu);
            if (cell_thr) {       // the saved gate gradients leave after the hand-off
                const unsigned o = (unsigned)((td * B + cb) * T2V_G + U) * 4u;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg4[0]), rDG, (int)o, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg4[1]), rDG, (int)(o + 4u * T2V_H), 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg4[2]), rDG, (int)(o + 8u * T2V_H), 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg4[3]), rDG, (int)(o + 12u * T2V_H), 0, 0);
            }
        }
        if (t < T) {
            // ---- off the chain: E(t) = Wcat_dec[:, :1536]^T dgd(t), the decoder_rnn contribution to d h_att(t) / d ctx(t)
            pba_rounds16<20, 8, 12, NB>(w, X0, X1, part + 4 * 512);
            __syncthreads();
            if (t > 0) pb_park_factors<NB>(lds, a.FD + (size_t)(t - 1) * (PB_ROW_BYTES(NB) / 4));
            // E(t): [h_att columns | ctx columns] of this workgroup, plain (T,B,1536) layout
            if (tid >= 64 && tid < 64 + 96) {
                const int i = tid - 64, col = i >> 3, b = i & 7;      // col 0..7: unit, 8..11: ctx column
                if (b < B) {
                    const float val = pb_sum16(part + (4 + (col >> 1)) * 512, (col & 1) * 8 + b);
                    if (col < 8) { if (col < nu) t2v_st(rE, (unsigned)(((t * B + b) * T2V_KATT) + u0 + col) * 4u, val); }
                    else if (col - 8 < nc) t2v_st(rE, (unsigned)(((t * B + b) * T2V_KATT) + T2V_H + c0 + col - 8) * 4u, val);
                }
            }
        }
        __syncthreads();
    }
    if (a.prof && jd == 0 && threadIdx.x == 0) a.prof[41] = __builtin_amdgcn_s_memrealtime();
    if (a.dw_planes) {
        PBADw d;
        d.DGD = a.DGD; d.XC = a.XS + (size_t)B * T2V_XW; d.planes = a.dw_planes; d.c_ih = a.dw_ih; d.c_hh = a.dw_hh; d.ctr = a.dw_ctr;
        d.GXA = a.GXA; d.err = a.err; d.prof = a.prof;
        d.K = T * B; d.ld_ih = a.dw_ld_ih; d.ld_hh = a.dw_ld_hh; d.accumulate = a.dw_accumulate; d.cap = a.dw_cap;
        d.margin_off = a.dw_margin >= 1 && a.dw_margin < T ? (int)((unsigned)a.dw_margin * PB_DROW_BYTES(NB)) : -1;
        d.jd = jd; d.ND = ND;
        pba_dw_epilogue(d, lds);
    }
}

// the activation-only part of attention_rnn's cell backward at step t -> cpre[row][8] = {fh, fc, go(1-tanh(c)^2), gf, e0..e3}.
// Two halves: the loads are issued BEFORE the factor-row DMA and consumed after it — behind the DMA they queued for the
// whole copy on the wave's in-order memory counter and in the CU's load pipe (1.7 us for six L2-warm loads).
struct PBACellIn { float gi, gf, gg, go, cac, cprev; };
__device__ __forceinline__ PBACellIn pba_cell_pre_load(const PBAArgs& a, bool cell_thr, int t, int cb, int U) {
    PBACellIn r = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!cell_thr) return r;
    const int B = a.B;
    const float* gp = a.GA + ((size_t)t * B + cb) * T2V_G + U;
    r.gi = gp[0]; r.gf = gp[T2V_H]; r.gg = gp[2 * T2V_H]; r.go = gp[3 * T2V_H];
    r.cac = a.CA[((size_t)(t + 1) * B + cb) * T2V_H + U];
    r.cprev = a.CA[((size_t)t * B + cb) * T2V_H + U];
    return r;
}
__device__ __forceinline__ void pba_cell_pre_finish(const PBAArgs& a, float* cpre, uint64_t seed, bool cell_thr, int rowi, int t, uint32_t idx,
                                                    const PBACellIn& r) {
    if (!cell_thr) return;
    const float gi = r.gi, gf = r.gf, gg = r.gg, go = r.go;
    float cprev = r.cprev;
    const float fh = t2v_drop_scale(seed, T2V_RNG_ATT_H, t, idx, a.p_att);
    const float fc = t2v_drop_scale(seed, T2V_RNG_ATT_C, t, idx, a.p_att);
    if (t > 0) cprev *= t2v_drop_scale(seed, T2V_RNG_ATT_C, t - 1, idx, a.p_att);
    const float tc = tanhf_(r.cac);
    *(float4*)(cpre + rowi * 8) = make_float4(fh, fc, go * (1.0f - tc * tc), gf);
    *(float4*)(cpre + rowi * 8 + 4) = make_float4(gg * gi * (1.0f - gi), cprev * gf * (1.0f - gf), gi * (1.0f - gg * gg), tc * go * (1.0f - go));
}
__device__ __forceinline__ void pba_cell_pre(const PBAArgs& a, float* cpre, uint64_t seed, bool cell_thr, int rowi, int t, int cb, int U,
                                             uint32_t idx) {
    const PBACellIn r = pba_cell_pre_load(a, cell_thr, t, cb, U);
    pba_cell_pre_finish(a, cpre, seed, cell_thr, rowi, t, idx, r);
}

// ------------------------------------------------------------------------------------------------ A role (the chain)
template <int NB, int NUA, int NCA>
__device__ __forceinline__ void pba_attention_rnn_role(const PBAArgs& a, float* lds, const int ja, const int NA) {
    constexpr int NCT = NUA + NCA;
    static_assert(NCA > 4 && NCA <= 8 && NUA > 8 && NUA <= 16, "two context rounds, three or four recurrent rounds");
    constexpr int NCR = (NCA + 1) / 2;                        // reduction rounds (2 columns each) of the context columns
    const uint64_t seed = t2v_step_seed(a.seed, a.step);
    const int tid = threadIdx.x;
    const int B = a.B, T = a.T, S = a.S_sl;
    f32x4* X0 = (f32x4*)lds;
    f32x2* X1 = (f32x2*)(lds + 4 * T2V_G);
    float* part = lds + (NB > 4 ? 6 : 4) * T2V_G;          // [6 groups][32 partials][32]
    float* ysum = part + 6 * 1024;                         // [21 cols -> 24][8]
    float* dhA = ysum + 192;                               // [14 units -> 16][8]  E_h(t) + ya_h(t+1)
    float* stage = dhA + 128;                              // [14 -> 16 units][4][8]
    float* wqs = stage + 512;                              // [14 -> 16][128] W_q^T rows of the own units
    float* dqs = wqs + 16 * T2V_A;                         // [8][128] dq(t) per item
    float* cpre = dqs + 8 * T2V_A;                         // [2][128 rows][8] activation-only factors of cell steps t, t-1
    float* eps = cpre + 2048;                              // [256] E(t) words / dHC words of the P2 threads (thread-private)
    int* flag = (int*)(eps + 256);                         // [4] + the phase profile (16 x 8 bytes)
    float* dump = eps + 256 + 64;                          // [8 waves][64] landing zone of the prefetch DMAs (never read)
    const int u0 = (ja * T2V_H) / NA, nu = ((ja + 1) * T2V_H) / NA - u0;      // <= 14 units
    const int c0 = (ja * T2V_E) / NA, nc = ((ja + 1) * T2V_E) / NA - c0;      // <= 7 context columns
    const __amdgpu_buffer_rsrc_t rA = t2v_rsrc(a.GXA), rC = t2v_rsrc(a.CX), rE = t2v_rsrc(a.EX);
    const __amdgpu_buffer_rsrc_t rQT = t2v_rsrc(a.DQT);
    const __amdgpu_buffer_rsrc_t rDC = t2v_rsrc(a.DCTX), rDG = t2v_rsrc(a.DGA);
    // columns: [0, NUA) W_hh_att[k][U], [NUA, NUA + NCA) W_ih_att[k][256 + C]
    f32x2 w[NCT][PB_KJ / 2];
#pragma unroll
    for (int jj = 0; jj < PB_KJ; ++jj) {
        const size_t k = (size_t)(tid + PB_THREADS * jj);
#pragma unroll
        for (int u = 0; u < NUA; ++u) {
            const bool on = u < nu;
            w[u][jj / 2][jj & 1] = on ? a.w_hh_att[k * T2V_H + u0 + (on ? u : 0)] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < NCA; ++c) {
            const bool on = c < nc;
            w[NUA + c][jj / 2][jj & 1] = on ? a.w_ih_att[k * (T2V_PRE + T2V_E) + T2V_PRE + c0 + (on ? c : 0)] : 0.f;
        }
    }
    for (int i = tid; i < 16 * T2V_A; i += PB_THREADS) {
        const int u = i >> 7, d = i & 127;
        wqs[i] = u < nu ? a.wq[(size_t)d * T2V_H + u0 + u] : 0.f;
    }
    for (int i = tid; i < 192; i += PB_THREADS) ysum[i] = 0.f;
    if (tid == 0) flag[0] = 1;
    float dca = 0.f;
    int napA = 0, napQ = 0;
    PBA_PROF_INIT(flag);
    if (a.prof && ja == 0 && tid == 0) a.prof[42] = __builtin_amdgcn_s_memrealtime();
    // cell-layout factors of the own units (k_pb_cellpre): nu * NB rows of 8 floats, contiguous per step -> thread i < 2 nu NB
    // moves float4 number i into cpre (row = i >> 1)
    const int ncp4 = 2 * nu * NB;
    const float* cpa0 = a.CPA + (size_t)u0 * NB * 8;
    constexpr size_t CPSTEP = (size_t)T2V_H * NB * 8;
    if (tid < ncp4) *(float4*)(cpre + ((T - 1) & 1) * 1024 + 4 * tid) = *(const float4*)(cpa0 + (size_t)(T - 1) * CPSTEP + 4 * tid);
    __syncthreads();
    unsigned long long tprev_ = __builtin_readcyclecounter();

    for (int t = T - 1; t >= 0; --t) {
        // Everything derived from the thread index is recomputed per step from an OPAQUE copy: hoisted out of the loop, the two
        // dozen offsets / addresses / predicates of this body live next to 144 weight registers for the whole pass, get
        // spilled, and every reload costs an s_waitcnt vmcnt(0) — a drain of this wave's whole memory queue — on the chain.
        int tid_op = threadIdx.x;
        asm volatile("" : "+v"(tid_op));
        const int tid = tid_op;
        // cell rows: row = tid >> 2 = u * NB + b (4 lanes per row, 32 attention dims each); lane 0 of a row owns (unit u, item b)
        const int rowi = tid >> 2, cu = rowi / NB, cb = rowi - cu * NB;
        const bool row_on = cu < nu;
        const bool cell_thr = (tid & 3) == 0 && cu < nu && cb < B;
        const int U = u0 + (cu < nu ? cu : 0);
        PBA_STAMP(ja == 0, 0);
        PBA_RT(0);
        // decoder_rnn's contribution E(t) was published long ago (that role runs ahead): fetched before the chain needs it
        // (LDS-DMA: no destination registers next to the weight registers; eps[tid] / eps[192 + tid] of the lanes that own a word)
        unsigned e_off = 0u;
        if (tid < 192) {
            const int wv = tid >> 6;
            if (tid < 56) {
                const int c = tid >> 3, b = tid & 7;
                if (c < nc && b < B) {
                    e_off = (unsigned)(((t * B + b) * T2V_KATT) + T2V_H + c0 + c) * 4u;
                    pb_dma4(a.EX + (e_off >> 2), eps + 64 * wv, 1);
                    pb_dma4(a.dHC + ((size_t)t * B + b) * (T2V_H + T2V_E) + T2V_H + c0 + c, eps + 192, 0);
                }
            } else if (tid >= 64 && tid < 64 + 112) {
                const int i = tid - 64, u = i >> 3, b = i & 7;
                if (u < nu && b < B) {
                    e_off = (unsigned)(((t * B + b) * T2V_KATT) + u0 + u) * 4u;
                    pb_dma4(a.EX + (e_off >> 2), eps + 64 * wv, 1);
                }
            }
        }
        // ---- P1a: the CONTEXT columns of ya = Wcat_att^T dga(t+1) first — they are what the attention workgroups wait for
        const bool have = t < T - 1;
        if (have) {
            const int rounds = pb_build_row<NB>(X0, X1, rA, (unsigned)(t + 1) * PB_DROW_BYTES(NB), B, napA, a.err, flag);
            napA = t2v_adapt_nap(napA, rounds);
            PBA_STAMP(ja == 0, 1);
            PBA_RT(1);
        }
        // (the poll has drained the memory queue: E / dHC are in LDS and cost no wait on the vector-memory counter later)
        if (have) {
            pba_rounds16<NCT, NUA, NCA, NB>(w, X0, X1, part);
            __syncthreads();
        }
        if (!have) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // first step: nothing else has waited for the E / dHC copies
        PBA_STAMP(ja == 0, 2);
        // ---- P2: context gradient of the own columns -> attention workgroups (E(t) comes from the decoder_rnn workgroups)
        if (tid < 64) {
            const int c = tid >> 3, b = tid & 7;
            float val = 0.f;
            const bool on = c < nc && b < B;
            if (on) {
                float e = eps[tid];
                if (__float_as_uint(e) == T2V_SENT) e = pba_wait_word(rE, e_off, a.err, flag);
                val = (e + eps[192 + tid]) + (have ? pb_sum16(part + (tid >> 4) * 512, tid & 15) : 0.f);        // column c: round c / 2
            }
            // lane b collects the columns of item b (lanes b + 8 c) and publishes them as one 16-byte store + the rest
            float g[NCA];
#pragma unroll
            for (int c2 = 0; c2 < NCA; ++c2) g[c2] = __shfl(val, (tid & 7) + 8 * c2, 64);
            if (tid < B) {
                const unsigned o = (unsigned)t * PB_CX_ROW_BYTES(NB) + (unsigned)tid * 4096u + 32u * (unsigned)ja;
                f32x4 hi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c2 = 4; c2 < NCA; ++c2) hi[c2 - 4] = g[c2];          // (columns past nc carry 0: val = 0 there)
                t2v_st(rC, o, f32x4{g[0], g[1], g[2], g[3]});
                t2v_st(rC, o + 16u, hi);
            }
            // (the saved copy for the d_memory GEMM goes out AFTER the hand-off, addressed off a scalar base: nothing the
            // attention workgroups wait for may sit behind a wait on this wave's memory counter)
            if (on) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), rDC, (int)((unsigned)((t * B + b) * T2V_E + c0 + c) * 4u), 0, 0);
        }
        PBA_STAMP(ja == 0, 3);
        PBA_RT(2);
        // ---- P1b: the recurrent columns (d h_att partial for the cell) while the attention workgroups work on step t
        if (have) {
            pba_rounds16<NCT, 0, NUA, NB>(w, X0, X1, part + 512 * NCR);
            __syncthreads();
        }
        if (tid >= 64 && tid < 64 + 112) {
            const int i = tid - 64, u = i >> 3, b = i & 7;
            if (u < nu && b < B) {
                float e = eps[tid];
                if (__float_as_uint(e) == T2V_SENT) e = pba_wait_word(rE, e_off, a.err, flag);
                dhA[i] = e + (have ? pb_sum16(part + 512 * NCR + (i >> 4) * 512, i & 15) : 0.f);                 // unit u: round u / 2
            }
        }
        PBA_STAMP(ja == 0, 5);
        PBA_RT(3);
        // (issued HERE, not right after the context hand-off: 768 line fetches from HBM in this CU's memory pipe in front of
        // the publishing store delayed its landing by more than a microsecond)
        // warm this XCD's L2 with the factor row that is parked one step from now (first touch comes from HBM): one word per
        // 128-byte line, consumed only at the end of the step
        // (LDS-DMA into a dump area: the touched words are never read, so they need no register either)
        {
            float* dmp = dump + 64 * (tid >> 6);
            if (tid >= 192 && t >= 2) {
                const float* fr = a.FA + (size_t)(t - 1) * (PB_ROW_BYTES(NB) / 4);
                const int i = tid - 192;
                constexpr int NLINE = PB_ROW_BYTES(NB) / 128;
                pb_dma4(fr + 32 * i, dmp, 0);
                if (i + 320 < NLINE) pb_dma4(fr + 32 * (i + 320), dmp, 0);
                if (i + 640 < NLINE) pb_dma4(fr + 32 * (i + 640), dmp, 0);
            } else if (tid >= 64 && tid < 64 + 24 && t >= 2) {
                // ... and with the cell-layout factor lines of step t-2 (copied into cpre at the end of the next step)
                const int i = tid - 64;
                if (32 * i < 4 * ncp4) pb_dma4(cpa0 + (size_t)(t - 2) * CPSTEP + 32 * i, dmp, 0);
            } else if (tid >= 100 && tid < 100 + B && t >= 1) {
                // ... and with the lines of dHC(t-1) the loop top of the next step reads (cold HBM otherwise, and the row poll
                // right behind them waits for every older load of its wave)
                const float* q = a.dHC + ((size_t)(t - 1) * B + (tid - 100)) * (T2V_H + T2V_E) + T2V_H + c0;
                pb_dma4(q, dmp, 0);
                pb_dma4(q + nc - 1, dmp, 0);
            }
        }

        // while dq(t) is on its way, prepare the next step: the factors of the next gather (row t) into the operand slots
        // (the recurrent GEMV was their last reader), and the part of cell A(t-1) that does not depend on d h_att
        if (t > 0) {
            // cell-layout factors of step t-1 straight into cpre (16 bytes per lane), issued BEFORE the big copy: small loads
            // behind it would queue for the whole copy on the wave's in-order memory counter
            if (tid < ncp4)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(cpa0 + (size_t)(t - 1) * CPSTEP + 4 * tid),
                                                 (__attribute__((address_space(3))) void*)(cpre + ((t - 1) & 1) * 1024 + 256 * (tid >> 6)), 16, 0, 0);
            pb_park_factors<NB>(lds, a.FA + (size_t)t * (PB_ROW_BYTES(NB) / 4));
            PBA_STAMP(ja == 0, 12);
            PBA_STAMP(ja == 0, 13);
        }
        // ---- P4: dq(t) of every item (sum of the position slices' partial rows)
        if (tid >= 320 && tid < 320 + B * 32) {
            const int i = tid - 320, b = i >> 5, q = i & 31;
            const unsigned off = (unsigned)((t * B + b) * T2V_A + 4 * q) * 4u;
            for (int n = 0; n < napQ; n += 8) __builtin_amdgcn_s_sleep(8);
            f32x4 sum = {0.f, 0.f, 0.f, 0.f};
            int rounds = 0;
            for (;;) {
                sum = t2v_ld_f32x4(rQT, off);
                const bool ok = t2v_ok(sum[0]) && t2v_ok(sum[1]) && t2v_ok(sum[2]) && t2v_ok(sum[3]);
                if (__all(ok)) break;
                __builtin_amdgcn_s_sleep(1);
                if (t2v_give_up(rounds, PB_SPIN, a.err, flag)) break;
            }
            napQ = t2v_adapt_nap(napQ, rounds);
            *(f32x4*)(dqs + b * T2V_A + 4 * q) = sum;
        }
        __syncthreads();
        if (flag[0] != 1) return;
        PBA_STAMP(ja == 0, 4);
        PBA_RT(4);
        // ---- W_q^T dq for the own units: row (u, b) x 4 lanes x 32 attention dims, quad sum; P5: cell A(t)
        f32x4 dg4 = {0.f, 0.f, 0.f, 0.f};
        {
            float acc = 0.f;
            if (row_on) {
                const float* wr = wqs + cu * T2V_A + 32 * (tid & 3);
                const float* dr = dqs + cb * T2V_A + 32 * (tid & 3);
#pragma unroll
                for (int i = 0; i < 32; i += 4) {
                    const float4 w4 = *(const float4*)(wr + i), d4 = *(const float4*)(dr + i);
                    acc = fmaf(w4.x, d4.x, acc); acc = fmaf(w4.y, d4.y, acc); acc = fmaf(w4.z, d4.z, acc); acc = fmaf(w4.w, d4.w, acc);
                }
            }
            acc = T2V_DPP_ADD(acc, 0xB1);
            acc = T2V_DPP_ADD(acc, 0x4E);
            if (cell_thr) {
                const float* cp = cpre + (t & 1) * 1024 + rowi * 8;
                const float4 c0v = *(const float4*)cp, c1v = *(const float4*)(cp + 4);
                const float dh = dhA[cu * 8 + cb] + acc;
                const float dht = dh * c0v.x;                         // cfh
                const float dct = dca * c0v.y + dht * c0v.z;          // cfc, go (1 - tanh(c)^2)
                const float d0 = dct * c1v.x, d1 = dct * c1v.y, d2 = dct * c1v.z, d3 = dht * c1v.w;
                dca = dct * c0v.w;                                    // gf
                float* sp = stage + (cu * 2) * 8 + cb;
                sp[0] = dct; sp[8] = dht;
                dg4 = f32x4{d0, d1, d2, d3};
            }
        }
        __syncthreads();
        if (t > 0) pba_publish_rows<NB>(rA, (unsigned)t * PB_DROW_BYTES(NB), stage, u0, nu);
        if (cell_thr) {       // the saved gate gradients (operands of the weight-gradient GEMMs) leave after the hand-off
            const unsigned o = (unsigned)((t * B + cb) * T2V_G + U) * 4u;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg4[0]), rDG, (int)o, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg4[1]), rDG, (int)(o + 4u * T2V_H), 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg4[2]), rDG, (int)(o + 8u * T2V_H), 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dg4[3]), rDG, (int)(o + 12u * T2V_H), 0, 0);
        }
        PBA_STAMP(ja == 0, 6);
        PBA_RT(5);
        __syncthreads();
        PBA_STAMP(ja == 0, 7);
    }
    if (a.prof && ja == 0 && tid == 0) a.prof[43] = __builtin_amdgcn_s_memrealtime();
    PBA_PROF_FLUSH(ja == 0, 0, 8);
    PBA_PROF_FLUSH(ja == 0, 12, 4);
}

// NB — 4: B <= 4, 6: B = 5, 6.  LONG — 224 < T_in <= 576: the attention role as 96-position slices on all eight waves (the form
// round 4 built for "one workgroup per item"; with S <= 6 slices an item of 555 symbols takes as many workgroups as the
// headline shape's 84 symbols in 16-position slices, so the LSTM roles keep their 4 / 5 units per workgroup).
// DAL — the attention role adds a.dAL (t2v_attn_role_bwd.h); the other roles are the same.
template <int NB, bool LONG, bool DAL>
__global__ __launch_bounds__(PB_THREADS) void k_achain_bwd(PBAArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wg = blockIdx.x;
    const int S = a.S_sl, NT = a.B * S, NL = T2V_NWG - NT, NA = pba_na(NL), ND = NL - NA;
    // (-DPBA_ONLY=1..4 builds ONE role into the kernel: `hipcc -Rpass-analysis=kernel-resource-usage` then reports that role's
    // own register pressure — the combined kernel always shows the maximum over the roles; tools/dbg/role_regs.sh)
#if defined(PBA_ONLY) && PBA_ONLY == 1
    pba_attention<16, 4, NB, DAL>(a, lds, wg / S, wg % S);
#elif defined(PBA_ONLY) && PBA_ONLY == 2
    pba_attention_rnn_role<NB, 12, 6>(a, lds, wg - NT, NA);
#elif defined(PBA_ONLY) && PBA_ONLY == 3
    pba_attention_rnn_role<NB, PBA_NUA, PBA_NCA>(a, lds, wg - NT, NA);
#elif defined(PBA_ONLY) && PBA_ONLY == 4
    pba_decoder_role<NB>(a, lds, wg - NT - NA, ND);
#else
    if (wg < NT) {
        if (LONG) pba_attention<96, 8, NB, DAL>(a, lds, wg / S, wg % S);
        else if (a.T_in <= 128) pba_attention<16, 4, NB, DAL>(a, lds, wg / S, wg % S);
        else pba_attention<32, 4, NB, DAL>(a, lds, wg / S, wg % S);
    } else if (wg < NT + NA) {
        if (NA >= 114) pba_attention_rnn_role<NB, 9, 5>(a, lds, wg - NT, NA);
        else if (NA >= 86) pba_attention_rnn_role<NB, 12, 6>(a, lds, wg - NT, NA);
        else pba_attention_rnn_role<NB, PBA_NUA, PBA_NCA>(a, lds, wg - NT, NA);
    } else {
        pba_decoder_role<NB>(a, lds, wg - NT - NA, ND);
    }
#endif
}

// slice geometry of the one-launch reverse pass: the launch-per-step geometry up to PB_MAXT symbols, 96-position slices beyond
static inline int pba_js(int T_in) { return T_in > PB_MAXT ? 96 : t2v_attn_bwd_js(T_in); }
static inline int pba_slices(int T_in) { const int js = pba_js(T_in); return (T_in + js - 1) / js; }
extern "C" int t2v_decoder_bwd_persist_slices(int T_in) { return T_in < 1 ? 0 : pba_slices(T_in); }

static size_t pba_lds_bytes(int B, int T_in) {
    const size_t lrole = PBA_LROLE_FLOATS(B > 4 ? 6 : 4);
    const size_t trole = t2v_attn_bwd_lds_floats(T_in, pba_js(T_in));
    return sizeof(float) * (lrole > trole ? lrole : trole);
}

// The sections of `scratch`, in floats and in this order (what every host function below reads):
//   GXA, GXD   n_gx each   (dc, dh) rows of attention_rnn / decoder_rnn: half a gate row per step (PB_DROW_BYTES)
//   CX         n_cx        context-gradient rows (PB_CX_ROW_BYTES)
//   GPX        n_gp        window partials of the attention slices
//   EX         n_ex        E(t) (T,B,1536), decoder_rnn's contribution to d h_att(t) / d ctx(t)
//   DQT        n_dqt       dq(t) summed over the slices, B padded to 8 (16-byte rows)
//   -- up to here exchange arrays: sentinel-filled by the preparation --
//   FA, FD     n_f each    gate-gradient factors of both cells (k_pb_factors): a gate row per step
//   CPA, CPD   n_cp each   cell-layout factors of both cells (k_pb_cellpre)
//   DWC        n_dwc       control words of the weight-gradient epilogue (pba_dw_epilogue): zeroed by the preparation
// The dq partials DQP (T,B,S,128), n_dq floats, are an OUTPUT (the caller passes them separately) and not part of scratch.
struct PBALayout {
    size_t n_gx, n_cx, n_gp, n_ex, n_dqt, n_f, n_cp, n_dwc, n_dq;
    size_t dqt_off() const { return 2 * n_gx + n_cx + n_gp + n_ex; }
    size_t n_exchange() const { return dqt_off() + n_dqt; }
    size_t dwc_off() const { return n_exchange() + 2 * n_f + 2 * n_cp; }
    size_t total() const { return dwc_off() + n_dwc; }
};
static PBALayout pba_layout(int B, int T_in, int T_out) {
    const size_t T = (size_t)T_out, S = (size_t)pba_slices(T_in), gpw = pba_js(T_in) + 30 <= 64 ? 64 : 128;
    const size_t rowf = pb_row_bytes(B) / 4, cxf = (size_t)(B > 4 ? 32768 : 16384) / 4;
    PBALayout l;
    l.n_gx = T * rowf / 2;
    l.n_cx = T * cxf;
    l.n_gp = T * B * S * 2 * gpw;
    l.n_ex = T * B * T2V_KATT;
    l.n_dqt = T * 8 * T2V_A;
    l.n_f = T * rowf;
    l.n_cp = T * T2V_H * (B > 4 ? 6 : 4) * 8;
    l.n_dwc = 16;
    l.n_dq = T * B * S * 128;
    return l;
}

extern "C" long t2v_decoder_bwd_achain_scratch_floats(int B, int T_in, int T_out) {
    if (B < 1 || B > PB_MAXB || T_in < 1 || T_in > PB_MAXT_LONG || T_out < 1) return 0;
    return (long)pba_layout(B, T_in, T_out).total();
}

// float offset, inside `scratch`, of dq(t) summed over the position slices — (T_out, B, 128), complete when the pass has ended:
// the d W_q product of the caller reads it there (the sum over the slice axis of DQP was a reduction launch behind the pass)
extern "C" long t2v_decoder_bwd_achain_dq_offset(int B, int T_in, int T_out) {
    if (!t2v_decoder_bwd_persist_supported(B, T_in) || T_out < 1) return -1;
    return (long)pba_layout(B, T_in, T_out).dqt_off();
}

// float offset, inside `scratch`, of the weight-gradient epilogue's control words; word 0 = the tiles of the decoder_rnn group it took
// (what t2v_gemm_f32_grouped_handed reads)
extern "C" long t2v_decoder_bwd_achain_dw_offset(int B, int T_in, int T_out) {
    if (!t2v_decoder_bwd_persist_supported(B, T_in) || T_out < 1) return -1;
    return (long)pba_layout(B, T_in, T_out).dwc_off();
}

// Reverse steps the attention_rnn chain must still have in front of it when a workgroup of the epilogue takes another pair of
// tiles, for K = T_out * B.  Measured (profiles/dw_epilogue_bwd_persist_timeline.txt, B = 6, T = 400, K = 2400): 227 .. 234 us per pair
// (two tiles side by side on one CU, 128 CUs at it), taken as 20 us + 0.09 us per unit of K; the chain advances one step per
// 10.58 .. 10.86 us.  A quarter of a pair on top for what the estimate misses at other shapes.
static int pba_dw_margin(int B, int T_out) {
    const double pair_us = 20.0 + 0.09 * (double)T_out * B;
    return (int)(1.25 * pair_us / 10.58) + 1;
}

template <int NB, bool LONG>
static void pba_launch_kernel(const PBAArgs& a, size_t lds, hipStream_t stream) {
    if (a.dAL) k_achain_bwd<NB, LONG, true><<<T2V_NWG, PB_THREADS, lds, stream>>>(a);
    else k_achain_bwd<NB, LONG, false><<<T2V_NWG, PB_THREADS, lds, stream>>>(a);
}

// do_prepare: error word, sentinel fills, the factor arrays of both cells (functions of the forward activations alone: they may
// run long before the reverse pass, next to the Postnet).  do_run: the pass itself.
static int pba_launch(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s,
                      const float* dHC, float* DGA, float* DGD, float* DCTX, float* DV, float* DQP, float* scratch,
                      uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed,
                      void* stream_, bool do_prepare, bool do_run, const t2v_achain_dw* dw = nullptr, const float* dAL = nullptr) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!s || !DQP || !scratch || !err_word) return T2V_ERR_ARG;
    if (do_run && (!w || !dHC || !DGA || !DGD || !DCTX || !DV)) return T2V_ERR_ARG;
    if (!t2v_decoder_bwd_persist_supported(B, T_in) || T_out < 1) return T2V_ERR_ARG;
    if (do_run && (!w->w_ih_att || !w->w_hh_att || !w->w_ih_dec || !w->w_hh_dec || !w->wq || !w->wcomb || !w->v)) return T2V_ERR_ARG;
    if (!s->memory || !s->XS || !s->CA || !s->CD || !s->GA || !s->GD || !s->AL || !s->S) return T2V_ERR_ARG;
    const PBALayout l = pba_layout(B, T_in, T_out);
    if (((uintptr_t)scratch & 15) || ((uintptr_t)DQP & 15) || l.n_gx * 4 >= 0x7fffffffull || l.n_dq * 4 >= 0x7fffffffull) return T2V_ERR_ARG;
    if (pba_lds_bytes(B, T_in) > T2V_LDS_MAX) return T2V_ERR_ARG;
    if (do_run && dw && (!dw->planes || ((uintptr_t)dw->planes & 15) || !dw->d_w_ih || !dw->d_w_hh || dw->ld_ih < T2V_KATT || dw->ld_hh < T2V_H ||
                         (long)T_out * B < 32))
        return T2V_ERR_ARG;
    static bool raised = false;
    if (!t2v_persist_raise_lds({(const void*)k_achain_bwd<4, false, false>, (const void*)k_achain_bwd<6, false, false>,
                                (const void*)k_achain_bwd<4, true, false>, (const void*)k_achain_bwd<6, true, false>,
                                (const void*)k_achain_bwd<4, false, true>, (const void*)k_achain_bwd<6, false, true>,
                                (const void*)k_achain_bwd<4, true, true>, (const void*)k_achain_bwd<6, true, true>}, raised))
        return t2v_check_launch();
    if (do_prepare) {
        (void)hipMemsetAsync(err_word, 0, sizeof(uint32_t), stream);
        t2v_fill_sentinel(scratch, l.n_exchange() / 4, 1024, stream);
        t2v_fill_sentinel(DQP, l.n_dq / 4, 256, stream);
        (void)hipMemsetAsync(scratch + l.dwc_off(), 0, l.n_dwc * sizeof(float), stream);
    }
    PBAArgs a;
    if (do_run) {
        a.w_ih_att = w->w_ih_att; a.w_hh_att = w->w_hh_att; a.w_ih_dec = w->w_ih_dec; a.w_hh_dec = w->w_hh_dec;
        a.wq = w->wq; a.wcomb = w->wcomb; a.v = w->v;
    }
    a.memory = s->memory; a.XS = s->XS; a.CA = s->CA; a.CD = s->CD; a.GA = s->GA; a.GD = s->GD; a.AL = s->AL; a.S = s->S;
    a.dHC = dHC; a.dAL = dAL; a.DGA = DGA; a.DGD = DGD; a.DCTX = DCTX; a.DV = DV; a.DQX = DQP;
    // the walk over the sections of pba_layout, in its order
    a.GXA = scratch;
    a.GXD = a.GXA + l.n_gx;
    a.CX = a.GXD + l.n_gx;
    a.GPX = a.CX + l.n_cx;
    a.EX = a.GPX + l.n_gp;
    a.DQT = a.EX + l.n_ex;
    float* FA = a.DQT + l.n_dqt;
    float* FD = FA + l.n_f;
    float* CPA = FD + l.n_f;
    float* CPD = CPA + l.n_cp;
    a.FA = FA; a.FD = FD; a.CPA = CPA; a.CPD = CPD;
    a.err = err_word;
    a.B = B; a.T_in = T_in; a.T = T_out; a.S_sl = pba_slices(T_in); a.p_att = p_att; a.p_dec = p_dec; a.seed = seed;
    a.step = t2v_step_for(stream);
    a.prof = g_t2v_prof;
    a.dw_planes = nullptr; a.dw_ih = a.dw_hh = nullptr; a.dw_ctr = (unsigned*)(scratch + l.dwc_off());
    a.dw_ld_ih = a.dw_ld_hh = a.dw_accumulate = a.dw_cap = a.dw_margin = 0;
    if (do_run && dw) {
        a.dw_planes = (uint4*)dw->planes; a.dw_ih = dw->d_w_ih; a.dw_hh = dw->d_w_hh; a.dw_ld_ih = dw->ld_ih; a.dw_ld_hh = dw->ld_hh;
        a.dw_accumulate = dw->accumulate ? 1 : 0;
        a.dw_cap = dw->tile_cap < 0 ? 0x7fffffff : dw->tile_cap;
        a.dw_margin = pba_dw_margin(B, T_out);
    }
    if (do_prepare) {
        const unsigned nblk = (unsigned)(((size_t)T_out * T2V_G + 255) / 256);
        k_pb_factors<<<nblk, 256, 0, stream>>>(s->GA, s->CA, FA, B, T_out, B, p_att, T2V_RNG_ATT_C, seed, a.step);
        k_pb_factors<<<nblk, 256, 0, stream>>>(s->GD, s->CD, FD, B, T_out, B, p_dec, T2V_RNG_DEC_C, seed, a.step);
        const int nbs = B > 4 ? 6 : 4;
        const unsigned ncp = (unsigned)(((size_t)T_out * T2V_H * nbs + 255) / 256);
        k_pb_cellpre<<<ncp, 256, 0, stream>>>(s->GA, s->CA, CPA, B, T_out, nbs, p_att, T2V_RNG_ATT_H, T2V_RNG_ATT_C, seed, a.step);
        k_pb_cellpre<<<ncp, 256, 0, stream>>>(s->GD, s->CD, CPD, B, T_out, nbs, p_dec, T2V_RNG_DEC_H, T2V_RNG_DEC_C, seed, a.step);
    }
    if (!do_run) return t2v_check_launch();
    const size_t lds = pba_lds_bytes(B, T_in);
    // without an alignment gradient the pass is the pointer-less kernel, as it always was
    if (T_in > PB_MAXT) {
        if (B > 4) pba_launch_kernel<6, true>(a, lds, stream);
        else pba_launch_kernel<4, true>(a, lds, stream);
    } else {
        if (B > 4) pba_launch_kernel<6, false>(a, lds, stream);
        else pba_launch_kernel<4, false>(a, lds, stream);
    }
    return t2v_check_launch();
}

// preparation + pass; dAL: upstream gradient of the alignments, contiguous (T_out, B, T_in), or NULL
extern "C" int t2v_decoder_bwd_achain_align(const t2v_dec_train_persist_weights* w, const t2v_achain_dw* dw, const t2v_dec_train_bufs* s,
                                            const float* dHC, const float* dAL, float* DGA, float* DGD, float* DCTX, float* DV, float* DQP,
                                            float* scratch, uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec,
                                            uint64_t seed, void* stream_) {
    return pba_launch(w, s, dHC, DGA, DGD, DCTX, DV, DQP, scratch, err_word, B, T_in, T_out, p_att, p_dec, seed, stream_, true, true, dw, dAL);
}
extern "C" int t2v_decoder_bwd_achain(const t2v_dec_train_persist_weights* w, const t2v_achain_dw* dw, const t2v_dec_train_bufs* s,
                                      const float* dHC, float* DGA, float* DGD, float* DCTX, float* DV, float* DQP, float* scratch,
                                      uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed,
                                      void* stream_) {
    return t2v_decoder_bwd_achain_align(w, dw, s, dHC, nullptr, DGA, DGD, DCTX, DV, DQP, scratch, err_word, B, T_in, T_out, p_att, p_dec, seed,
                                        stream_);
}

// The preparation on its own (everything it needs exists when the FORWARD pass has ended) ...
extern "C" int t2v_decoder_bwd_achain_prepare(const t2v_dec_train_bufs* s, float* DQP, float* scratch, uint32_t* err_word, int B, int T_in,
                                              int T_out, float p_att, float p_dec, uint64_t seed, void* stream_) {
    return pba_launch(nullptr, s, nullptr, nullptr, nullptr, nullptr, nullptr, DQP, scratch, err_word, B, T_in, T_out, p_att, p_dec, seed,
                      stream_, true, false);
}
// ... and the pass without it (same arguments as t2v_decoder_bwd_achain_align; scratch / DQP / err_word as handed to _prepare)
extern "C" int t2v_decoder_bwd_achain_prepared_align(const t2v_dec_train_persist_weights* w, const t2v_achain_dw* dw,
                                                     const t2v_dec_train_bufs* s, const float* dHC, const float* dAL, float* DGA, float* DGD,
                                                     float* DCTX, float* DV, float* DQP, float* scratch, uint32_t* err_word, int B, int T_in,
                                                     int T_out, float p_att, float p_dec, uint64_t seed, void* stream_) {
    return pba_launch(w, s, dHC, DGA, DGD, DCTX, DV, DQP, scratch, err_word, B, T_in, T_out, p_att, p_dec, seed, stream_, false, true, dw, dAL);
}
extern "C" int t2v_decoder_bwd_achain_prepared(const t2v_dec_train_persist_weights* w, const t2v_achain_dw* dw, const t2v_dec_train_bufs* s,
                                               const float* dHC, float* DGA, float* DGD, float* DCTX, float* DV, float* DQP, float* scratch,
                                               uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed,
                                               void* stream_) {
    return t2v_decoder_bwd_achain_prepared_align(w, dw, s, dHC, nullptr, DGA, DGD, DCTX, DV, DQP, scratch, err_word, B, T_in, T_out, p_att,
                                                 p_dec, seed, stream_);
}
