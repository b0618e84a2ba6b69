// Teacher-forced decoder recurrence, forward, as ONE persistent launch (reference Decoder.forward's time loop
// model.py:415-421 -> Decoder.decode 346-389 -> Attention.forward 67-88): 256 workgroups x 512 threads stay resident for
// all T_out steps, the 67 MB of LSTM weights live in registers, nothing is streamed per step.  The launch-per-step path
// (decoder_fwd.hip + attn_fwd.hip: 2 launches and a 67 MB weight stream per step) stays the general path; this kernel
// serves B <= 6 and T_in <= 224 — the headline training shape (B = 6 per GPU, T_in = 84).
//
// Roles (one workgroup per CU, all co-resident):
//   T  : workgroups [0, 8B)   — location-sensitive attention of item b = wg / 8, attention dims [16s, 16s + 16) and context
//        columns [64s, 64s + 64), s = wg % 8.  W_q slice, memory / processed-memory slices and the alignment window stay
//        in LDS for all steps (as in decoder_persist.hip).  The role's body is t2v_attn_role_fwd.inc, included below and
//        shared with k_dec_train_persist16; this file has what is its own: how h_att(t) arrives and how the context leaves.
//   L  : workgroups [8B, 256) — LSTM rows of BOTH cells: workgroup j owns hidden units [j*1024/NL, (j+1)*1024/NL) (4 or 5
//        units = 16 or 20 gate rows per cell), weights in VGPRs (thread = (gate, 1/128 of K): 60 + 100 registers).
// Teacher forcing takes decoder_rnn off the critical path: attention_rnn(t+1) needs only h_att(t) and ctx(t) (the Prenet
// term gpre is precomputed for all steps), so the per-step chain is
//     A-gemv(t) -> h_att hop -> attention(t) -> ctx hop -> A-gemv(t+1)
// while every L workgroup runs D-gemv(t-1) and its own gathers in the shadow of attention(t).
//
// Hand-off = the saved activations themselves.  Every recurrent value is produced exactly once per pass, so it needs no
// tag and no flag: the exchange buffer G (one row per step, laid out [plane][k][4 items] so that a consumer's 16-byte
// load is an LDS-ready operand) is pre-filled with a NaN sentinel (T2V_SENT, t2v_xchg.h: never produced by arithmetic); producers
// store with sc1 (write-through), consumers poll their own words with sc1 loads until none is the sentinel.  4 bytes per
// value on the wire instead of an 8-byte {value, tag} granule, 16-byte loads, no memory ordering needed (MI355X guide
// G16 form R2 with an implicit tag).  The partial energies of the 8 attention slices of an item travel the same way (EX).
// The backward pass reads the usual arena (XS, CA, CD, GA, GD, AL, ACUM, S), written here with plain stores.
#include "t2v_common.h"
#include "t2v_kernels.h"
#include "t2v_xchg.h"

#define PT_MAXB 6                    // (thread count, spin limit and the T_in bounds: T2V_AF_*, t2v_kernels.h)
#define PT_MAXU 5
#define PT_JA (T2V_KATT / 128)       // 12 k per thread, attention_rnn  [h_att | ctx]
#define PT_JD (T2V_XW / 128)         // 20 k per thread, decoder_rnn    [h_att | ctx | h_dec]

struct PTArgs {
    const float* w_ih_att; const float* w_hh_att; const float* w_ih_dec; const float* w_hh_dec;
    const float* bias_dec; const float* wq; const float* wcomb; const float* v;
    const float* gpre; const float* memory; const float* pm; const int32_t* lengths;
    float* XS; float* CA; float* CD; float* GA; float* GD; float* AL; float* ACUM; float* S;
    float* G;                 // (T+2) rows x NP planes x 2560 k x 4 items, sentinel-filled
    float* EX;                // T x B x 8 x Tcap partial energies, sentinel-filled
    unsigned* err;
    int B, T_in, T_out;
    float p_att, p_dec;
    uint64_t seed;
    const t2v_step_params* step;
    unsigned long long* prof;   // optional: stamps of step T_out/2 (L workgroup 8B: slots 0..7, T workgroup 0: slots 8..15)
};
// wall clock (100 MHz, the same counter on every CU): hop latencies between workgroups
#define PT_WALL(COND, I) do { if (a.prof && (COND) && tid == 0) a.prof[(I)] = wall_clock64(); } while (0)
#define PT_STAMP(COND, I) do { if (a.prof && (COND) && tid == 0) a.prof[(I)] = __builtin_readcyclecounter(); } while (0)

// Gather nk columns [k0, k0 + nk) of all planes of one G row (byte offset row_off) into the LDS state planes.  PER
// chunks per thread (NP * nk <= PER * 512).  A chunk is valid when the words of the items it carries are all written.
// Returns through *flag (LDS, stays 1 unless a spin timed out); the caller syncs before reading X.
template <int PER, int NP>
__device__ __forceinline__ int pt_gather(f32x4* X, __amdgpu_buffer_rsrc_t rG, unsigned row_off, int k0, int nk, int B, int nap,
                                         unsigned* err, int* flag, int gap_at = 1 << 30, int gap = 0) {
    const int tid = threadIdx.x;
    unsigned src[PER];
    int dsti[PER], nw[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        int c = tid + T2V_AF_THREADS * u;
        const bool on = c < NP * nk;
        c = on ? c : 0;
        const int pl = c / nk;
        int kk = k0 + (c - pl * nk);
        kk += kk >= gap_at ? gap : 0;            // two column segments in one pass: [k0, gap_at) and [gap_at + gap, ..)
        src[u] = row_off + (unsigned)(pl * T2V_XW + kk) * 16u;
        dsti[u] = on ? pl * T2V_XW + kk : -1;
        nw[u] = min(4, B - 4 * pl);
    }
    // nap first (s_sleep units of 64 clocks): the caller passes what the previous steps' waits suggested, so that a
    // known-long wait issues no load at all; then the payload itself is polled — the first round that finds every
    // word written IS the gather (no separate flag round trip).  Rounds are counted per wave (wave-uniform loop).
    for (int i = 0; i < nap; i += 8) __builtin_amdgcn_s_sleep(8);
    f32x4 v[PER];
    int rounds = 0;
    for (;;) {
#pragma unroll
        for (int u = 0; u < PER; ++u) v[u] = t2v_ld_f32x4(rG, src[u]);
        bool ok = true;
#pragma unroll
        for (int u = 0; u < PER; ++u) ok = ok && t2v_ok_n(v[u], nw[u]);
        if (__all(ok)) break;
        __builtin_amdgcn_s_sleep(2);
        if (t2v_give_up(rounds, (int)(T2V_AF_SPIN / 4), err, flag)) break;
    }
#pragma unroll
    for (int u = 0; u < PER; ++u)
        if (dsti[u] >= 0) X[dsti[u]] = v[u];
    return rounds;
}

// Sparse wait ahead of a bulk gather: threads [0, npoll) each watch ONE word (one per producing workgroup); everybody
// else parks at the block barrier.  Hundreds of threads per CU polling the payload itself cost the producers' stores and
// the other consumers' loads (MI355X guide: polling-cost row) — this way a CU issues npoll 4-byte loads per round.
// nap: s_sleep units (64 clocks each) to spend before the first look — the caller passes what the previous step's wait
// suggested, so that most of a known-long wait issues no load at all.  Returns the rounds it took.
__device__ __forceinline__ int pt_wait_words(__amdgpu_buffer_rsrc_t r, unsigned off, int npoll, int nap, unsigned* err, int* flag) {
    const int tid = threadIdx.x;
    if (tid < 64)
        for (int i = 0; i < nap; i += 16) __builtin_amdgcn_s_sleep(16);
    int rounds = 0;
    unsigned spins = 0;
    for (;;) {
        bool ok = true;
        if (tid < npoll) ok = t2v_ok(t2v_ld_b32(r, off));
        if (__syncthreads_and(ok)) break;
        ++rounds;
        if (tid == 0) t2v_give_up(spins, T2V_AF_SPIN / 8, err, flag);
        __syncthreads();
        if (*flag != 1) break;
    }
    return rounds;
}

// acc[u][pair] += w[u] * x[pair] for the 5 unit rows of a thread and the item PAIRS (0,1), (2,3)[, (4,5)] as ONE volatile
// asm block of packed FMAs.  (a) v_pk_fma_f32 does two fp32 FMAs per lane in the 4 cycles a plain v_fma_f32 needs for one
// — measured here: the scalar-FMA version of this loop ran at 4.8 cycles per FMA and SIMD — with the weight broadcast to
// both halves through op_sel (weights of two consecutive k share a register pair: even k = low word, odd k = high word);
// (b) volatile asm, because left to itself the compiler sinks the (pure) FMAs of the fully unrolled k loop to the end of
// the function, first loads all operand vectors (80 registers) and then walks one accumulator at a time as a dependent
// chain — with 160 weight registers live that spills, and the chains stall.
template <int NB>
struct PTAcc {
    static constexpr int NPAIR = NB > 4 ? 3 : 2;
    f32x2 p[PT_MAXU][NPAIR];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int u = 0; u < PT_MAXU; ++u)
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) p[u][i] = f32x2{0.f, 0.f};
    }
};
template <bool ODD>
__device__ __forceinline__ void pt_pkfma(PTAcc<6>& acc, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 w4, f32x2 x01, f32x2 x23, f32x2 x45) {
    if (ODD)
        asm volatile("v_pk_fma_f32 %0, %15, %20, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %1, %15, %21, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %2, %15, %22, %2 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %3, %16, %20, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %4, %16, %21, %4 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %5, %16, %22, %5 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %6, %17, %20, %6 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %7, %17, %21, %7 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %8, %17, %22, %8 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %9, %18, %20, %9 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %10, %18, %21, %10 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %11, %18, %22, %11 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %12, %19, %20, %12 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %13, %19, %21, %13 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %14, %19, %22, %14 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 : "+v"(acc.p[0][0]), "+v"(acc.p[0][1]), "+v"(acc.p[0][2]), "+v"(acc.p[1][0]), "+v"(acc.p[1][1]), "+v"(acc.p[1][2]), "+v"(acc.p[2][0]), "+v"(acc.p[2][1]), "+v"(acc.p[2][2]), "+v"(acc.p[3][0]), "+v"(acc.p[3][1]), "+v"(acc.p[3][2]), "+v"(acc.p[4][0]), "+v"(acc.p[4][1]), "+v"(acc.p[4][2])
                 : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "v"(x01), "v"(x23), "v"(x45));
    else
        asm volatile("v_pk_fma_f32 %0, %15, %20, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %1, %15, %21, %1 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %2, %15, %22, %2 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %3, %16, %20, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %4, %16, %21, %4 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %5, %16, %22, %5 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %6, %17, %20, %6 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %7, %17, %21, %7 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %8, %17, %22, %8 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %9, %18, %20, %9 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %10, %18, %21, %10 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %11, %18, %22, %11 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %12, %19, %20, %12 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %13, %19, %21, %13 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %14, %19, %22, %14 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 : "+v"(acc.p[0][0]), "+v"(acc.p[0][1]), "+v"(acc.p[0][2]), "+v"(acc.p[1][0]), "+v"(acc.p[1][1]), "+v"(acc.p[1][2]), "+v"(acc.p[2][0]), "+v"(acc.p[2][1]), "+v"(acc.p[2][2]), "+v"(acc.p[3][0]), "+v"(acc.p[3][1]), "+v"(acc.p[3][2]), "+v"(acc.p[4][0]), "+v"(acc.p[4][1]), "+v"(acc.p[4][2])
                 : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "v"(x01), "v"(x23), "v"(x45));
}
template <bool ODD>
__device__ __forceinline__ void pt_pkfma(PTAcc<4>& acc, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 w4, f32x2 x01, f32x2 x23, f32x2) {
    if (ODD)
        asm volatile("v_pk_fma_f32 %0, %10, %15, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %1, %10, %16, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %2, %11, %15, %2 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %3, %11, %16, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %4, %12, %15, %4 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %5, %12, %16, %5 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %6, %13, %15, %6 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %7, %13, %16, %7 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %8, %14, %15, %8 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 "v_pk_fma_f32 %9, %14, %16, %9 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
                 : "+v"(acc.p[0][0]), "+v"(acc.p[0][1]), "+v"(acc.p[1][0]), "+v"(acc.p[1][1]), "+v"(acc.p[2][0]), "+v"(acc.p[2][1]), "+v"(acc.p[3][0]), "+v"(acc.p[3][1]), "+v"(acc.p[4][0]), "+v"(acc.p[4][1])
                 : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "v"(x01), "v"(x23));
    else
        asm volatile("v_pk_fma_f32 %0, %10, %15, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %1, %10, %16, %1 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %2, %11, %15, %2 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %3, %11, %16, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %4, %12, %15, %4 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %5, %12, %16, %5 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %6, %13, %15, %6 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %7, %13, %16, %7 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %8, %14, %15, %8 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 "v_pk_fma_f32 %9, %14, %16, %9 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
                 : "+v"(acc.p[0][0]), "+v"(acc.p[0][1]), "+v"(acc.p[1][0]), "+v"(acc.p[1][1]), "+v"(acc.p[2][0]), "+v"(acc.p[2][1]), "+v"(acc.p[3][0]), "+v"(acc.p[3][1]), "+v"(acc.p[4][0]), "+v"(acc.p[4][1])
                 : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "v"(x01), "v"(x23));
}

// acc += sum_{j in [J0, J1)} w[.][j] * x[kp + 128 j][.]: per k one 16-byte (+ one 8-byte) LDS operand, PT_PF of them in
// flight; w2[u][j / 2] holds the weights of k-blocks j (even, low word) and j + 1 (high word)
#define PT_PF 3
template <int NJ2, int J0, int J1, int NB>
__device__ __forceinline__ void pt_fma_range(const f32x2 (&w2)[PT_MAXU][NJ2], const f32x4* X, int kp, PTAcc<NB>& acc) {
    f32x4 xq[PT_PF];
    f32x2 yq[PT_PF];
#pragma unroll
    for (int d = 0; d < PT_PF; ++d) {
        yq[d] = f32x2{0.f, 0.f};
        if (J0 + d < J1) {
            xq[d] = X[kp + 128 * (J0 + d)];
            if constexpr (NB > 4) yq[d] = *(const f32x2*)&X[T2V_XW + kp + 128 * (J0 + d)];
        }
    }
#pragma unroll
    for (int j = J0; j < J1; ++j) {
        const f32x4 xc = xq[(j - J0) % PT_PF];
        const f32x2 yc = yq[(j - J0) % PT_PF];
        const f32x2 x01 = {xc[0], xc[1]}, x23 = {xc[2], xc[3]};
        if (j & 1) pt_pkfma<true>(acc, w2[0][j / 2], w2[1][j / 2], w2[2][j / 2], w2[3][j / 2], w2[4][j / 2], x01, x23, yc);
        else pt_pkfma<false>(acc, w2[0][j / 2], w2[1][j / 2], w2[2][j / 2], w2[3][j / 2], w2[4][j / 2], x01, x23, yc);
        if (j + PT_PF < J1) {
            xq[(j - J0) % PT_PF] = X[kp + 128 * (j + PT_PF)];
            if constexpr (NB > 4) yq[(j - J0) % PT_PF] = *(const f32x2*)&X[T2V_XW + kp + 128 * (j + PT_PF)];
        }
    }
}

// 16-lane row sums of the 5 x NB accumulators as a TRANSPOSING butterfly: 32 values (index u * NB + b, zero padded) are
// halved four times — at every stage a lane keeps the half selected by one bit of its lane id and adds its partner's
// copy of that half (row_mirror, row_half_mirror, quad xor 2, quad xor 1: the partner always differs in the selector
// bit) — 30 DPP adds + 60 selects instead of 120 dependent DPP adds + 30 masked stores.  Lane c of a row ends with the
// row sums of values 2c and 2c + 1 and stores them as one float2: red[gate][partial = 2 waves x 4 rows][32].
template <int NB>
__device__ __forceinline__ void pt_reduce_store(const PTAcc<NB>& acc, float* red) {
    const int tid = threadIdx.x, lane = tid & 63, g = tid >> 7;
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = 0.f;
#pragma unroll
    for (int u = 0; u < PT_MAXU; ++u)
#pragma unroll
        for (int i = 0; i < PTAcc<NB>::NPAIR; ++i) {
            v[u * NB + 2 * i] = acc.p[u][i][0];
            v[u * NB + 2 * i + 1] = acc.p[u][i][1];
        }
    const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
    float w16[16], w8[8], w4[4], w2[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float keep = b3 ? v[16 + i] : v[i], send = b3 ? v[i] : v[16 + i];
        w16[i] = keep + T2V_DPP_F(send, 0x140);            // row_mirror
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float keep = b2 ? w16[8 + i] : w16[i], send = b2 ? w16[i] : w16[8 + i];
        w8[i] = keep + T2V_DPP_F(send, 0x141);             // row_half_mirror
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float keep = b1 ? w8[4 + i] : w8[i], send = b1 ? w8[i] : w8[4 + i];
        w4[i] = keep + T2V_DPP_F(send, 0x4E);              // quad_perm [2,3,0,1]
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float keep = b0 ? w4[2 + i] : w4[i], send = b0 ? w4[i] : w4[2 + i];
        w2[i] = keep + T2V_DPP_F(send, 0xB1);              // quad_perm [1,0,3,2]
    }
    const int part = ((tid >> 6) & 1) * 4 + (lane >> 4);
    *(float2*)(red + (g * 8 + part) * 32 + 2 * (lane & 15)) = make_float2(w2[0], w2[1]);
}

// NB — 4: B <= 4 (one item plane), 6: B = 5, 6 (two planes).  LONG — the attention role for 224 < T_in <= 560 (koemo's longest
// sentence has 555 symbols): the W_q slice and the processed-memory slice move from LDS into registers (32 + 20 per thread: an
// attention workgroup holds no LSTM weights), which leaves the 160 KB to the memory slice (560 x 64 floats = 140 KB); five
// position tiles per wave instead of two, two positions per thread in the softmax.
template <int NB, bool LONG>
__global__ __launch_bounds__(T2V_AF_THREADS) void k_dec_train_persist(PTArgs a) {
    constexpr int NP = NB > 4 ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint64_t seed = t2v_step_seed(a.seed, a.step);
    const int wg = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int B = a.B, Tp = a.T_in, T = a.T_out;
    const int NT = 8 * B, NL = T2V_NWG - NT;
    const unsigned grow_b = (unsigned)NP * T2V_XW * 16u;      // bytes per G row
    const __amdgpu_buffer_rsrc_t rG = t2v_rsrc(a.G), rE = t2v_rsrc(a.EX);
    const int Tcap = (Tp + 15) & ~15;

    if (wg >= NT) {
        // =========================================================================== L role: LSTM rows of both cells
        f32x4* X = (f32x4*)lds;                              // [NP][2560] state planes: X[pl*2560 + k] = items 4pl..4pl+3 of column k
        float* red = lds + (size_t)NP * T2V_XW * 4;          // [4 gates][8 partials][32]
        float* cst = red + 4 * 8 * 32;                       // [2 cells][32] cell states, [4][32] decoder_rnn biases
        float* fdrop = cst + 6 * 32;                         // [2][32] dropout factors (cell state, hidden state) of attention_rnn's coming step
        int* flag = (int*)(cst + 8 * 32);
        const int j = wg - NT;
        const int u0 = (j * T2V_H) / NL, nu = ((j + 1) * T2V_H) / NL - u0;      // 4 or 5 units
        const int g = tid >> 7, kp = tid & 127;
        f32x2 wa[PT_MAXU][PT_JA / 2], wd[PT_MAXU][PT_JD / 2];     // [u][j / 2][j & 1]: weight of k = kp + 128 j
#pragma unroll
        for (int u = 0; u < PT_MAXU; ++u) {
            const bool on = u < nu;
            const size_t row = (size_t)g * T2V_H + u0 + (on ? u : 0);
#pragma unroll
            for (int jj = 0; jj < PT_JA; ++jj) {          // [h_att | ctx]: weight_hh, then weight_ih columns 256..767
                const int k = kp + 128 * jj;
                const float w = jj < 8 ? a.w_hh_att[row * T2V_H + k] : a.w_ih_att[row * (T2V_PRE + T2V_E) + T2V_PRE + (k - T2V_H)];
                wa[u][jj / 2][jj & 1] = on ? w : 0.f;
            }
#pragma unroll
            for (int jj = 0; jj < PT_JD; ++jj) {          // [h_att | ctx | h_dec]: weight_ih, then weight_hh
                const int k = kp + 128 * jj;
                const float w = jj < 12 ? a.w_ih_dec[row * T2V_KATT + k] : a.w_hh_dec[row * T2V_H + (k - T2V_KATT)];
                wd[u][jj / 2][jj & 1] = on ? w : 0.f;
            }
        }
        for (int i = tid; i < NP * T2V_XW; i += T2V_AF_THREADS) X[i] = f32x4{0.f, 0.f, 0.f, 0.f};      // row 0: zero initial states
        if (tid == 0) flag[0] = 1;
        // cell threads: tid = u * NB + b (wave 0); each keeps its two cell states in registers for the whole pass
        const int cu = tid / NB, cb = tid - cu * NB;
        const bool cell_on = tid < PT_MAXU * NB && cu < nu && cb < B;
        const int U = u0 + (cu < nu ? cu : 0);
        if (tid < 64) { cst[tid] = 0.f; }
        if (cell_on) {
#pragma unroll
            for (int r = 0; r < 4; ++r) cst[64 + 32 * r + tid] = a.bias_dec[r * T2V_H + U];
        }
        __syncthreads();
        int ctx_nap = 0;
        PTAcc<NB> accA;
        accA.clear();                  // row 0 is zero: the h_att half of attention_rnn(0) is zero
        // State-dropout factors of attention_rnn's cell of the COMING step (round 6): two 64-bit counter hashes (~300 cycles each) that
        // depend on (seed, step, unit) alone.  They used to sit behind the gate sums, between "context arrived" and "h_att published";
        // now the cell threads evaluate them BEFORE they poll for the context and park them in LDS (as two more live registers next
        // to the 160 weight registers they spill into the FMA phases and the step gets slower: measured).  Same-box A/B of the whole
        // training step: 10.86-10.90 -> 10.75-10.79 ms.  (All four factors of a step on the idle wave 1 during the cell phases —
        // built, parity-green: 10.93-10.98 ms; the decoder_rnn cell is not on the chain and the extra scratch costs more.)
        if (cell_on) { fdrop[tid] = 1.0f; fdrop[32 + tid] = t2v_drop_scale(seed, T2V_RNG_ATT_H, 0, (uint32_t)cb * T2V_H + U, a.p_att); }

        for (int t = 0; t <= T; ++t) {
            const bool do_att = t < T, do_dec = t >= 1;
            const unsigned grow = (unsigned)(t + 1) * grow_b;      // row t+1 = [h_att(t) | ctx(t) | h_dec(t-1)] (byte offset)
            PT_STAMP(wg == NT && t == T / 2, 0);
            // ---- attention_rnn(t): X holds row t = [h_att(t-1) | ctx(t-1) | h_dec(t-2)]; the h_att half of the sum was
            // accumulated into accA before ctx(t-1) arrived (end of the previous iteration), the ctx half is left
            if (do_att) {
                float gp[4] = {0.f, 0.f, 0.f, 0.f};
                if (cell_on) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) gp[r] = a.gpre[((size_t)t * B + cb) * T2V_G + r * T2V_H + U];
                }
                pt_fma_range<PT_JA / 2, 8, PT_JA, NB>(wa, X, kp, accA);
                pt_reduce_store<NB>(accA, red);
                PT_STAMP(wg == NT && t == T / 2, 16);
                __syncthreads();
                PT_STAMP(wg == NT && t == T / 2, 17);
                if (wave == 0) {
                    float hd = 0.f;
                    if (cell_on) {
                        float s[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float* rp = red + (r * 8) * 32 + cu * NB + cb;
                            s[r] = ((rp[0] + rp[32]) + (rp[64] + rp[96])) + ((rp[128] + rp[160]) + (rp[192] + rp[224])) + gp[r];
                        }
                        const float gi = sigmoidf_(s[0]), gf = sigmoidf_(s[1]), gg = tanhf_(s[2]), go = sigmoidf_(s[3]);
                        float cprev = cst[tid];
                        if (t > 0) cprev *= fdrop[tid];
                        const float c = gf * cprev + gi * gg;
                        cst[tid] = c;
                        a.CA[((size_t)(t + 1) * B + cb) * T2V_H + U] = c;
                        if (a.GA) {
                            float* gs = a.GA + ((size_t)t * B + cb) * T2V_G + U;
                            gs[0] = gi; gs[T2V_H] = gf; gs[2 * T2V_H] = gg; gs[3 * T2V_H] = go;
                        }
                        hd = go * tanhf_(c) * fdrop[32 + tid];
                        a.XS[((size_t)(t + 1) * B + cb) * T2V_XW + U] = hd;
                    }
                    // publish FIRST (the write-through store is what attention(t) waits for): lane (u, plane) sends the 4
                    // items of its plane as one 16-byte store; the saved activations follow
                    const int pu = lane / NP, pp = lane - pu * NP;
                    f32x4 v4;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int bb = 4 * pp + i;
                        const float x = __shfl(hd, min(pu, PT_MAXU - 1) * NB + min(bb, NB - 1), 64);
                        v4[i] = bb < B ? x : 0.f;
                    }
                    if (lane < PT_MAXU * NP && pu < nu) t2v_st(rG, grow + (unsigned)(pp * T2V_XW + u0 + pu) * 16u, v4);
                    PT_WALL(wg == NT && t == T / 2, 20);
                }
            }
            PT_STAMP(wg == NT && t == T / 2, 1);
            // ---- decoder_rnn(t-1): same row (its h_dec(t-2) columns included)
            if (do_dec) {
                PTAcc<NB> accD;
                accD.clear();
                pt_fma_range<PT_JD / 2, 0, PT_JD, NB>(wd, X, kp, accD);
                __syncthreads();               // attention_rnn's cell threads are done with red
                pt_reduce_store<NB>(accD, red);
                __syncthreads();
                if (wave == 0) {
                    float hd = 0.f;
                    if (cell_on) {
                        float s[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float* rp = red + (r * 8) * 32 + cu * NB + cb;
                            s[r] = ((rp[0] + rp[32]) + (rp[64] + rp[96])) + ((rp[128] + rp[160]) + (rp[192] + rp[224])) + cst[64 + 32 * r + tid];
                        }
                        const float gi = sigmoidf_(s[0]), gf = sigmoidf_(s[1]), gg = tanhf_(s[2]), go = sigmoidf_(s[3]);
                        const uint32_t idx = (uint32_t)cb * T2V_H + U;
                        const int tt = t - 1;
                        float cprev = cst[32 + tid];
                        if (tt > 0) cprev *= t2v_drop_scale(seed, T2V_RNG_DEC_C, tt - 1, idx, a.p_dec);
                        const float c = gf * cprev + gi * gg;
                        cst[32 + tid] = c;
                        a.CD[((size_t)t * B + cb) * T2V_H + U] = c;
                        if (a.GD) {
                            float* gs = a.GD + ((size_t)tt * B + cb) * T2V_G + U;
                            gs[0] = gi; gs[T2V_H] = gf; gs[2 * T2V_H] = gg; gs[3 * T2V_H] = go;
                        }
                        hd = go * tanhf_(c) * t2v_drop_scale(seed, T2V_RNG_DEC_H, tt, idx, a.p_dec);
                        a.XS[((size_t)(t + 1) * B + cb) * T2V_XW + T2V_KATT + U] = hd;
                    }
                    const int pu = lane / NP, pp = lane - pu * NP;
                    f32x4 v4;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int bb = 4 * pp + i;
                        const float x = __shfl(hd, min(pu, PT_MAXU - 1) * NB + min(bb, NB - 1), 64);
                        v4[i] = bb < B ? x : 0.f;
                    }
                    if (t < T && lane < PT_MAXU * NP && pu < nu) t2v_st(rG, grow + (unsigned)(pp * T2V_XW + T2V_KATT + u0 + pu) * 16u, v4);
                }
            } else if (wave == 0) {
                // t = 0: h_dec(-1) = 0 (XS row 1 was cleared by the reset launch)
                const int pu = lane / NP, pp = lane - pu * NP;
                if (lane < PT_MAXU * NP && pu < nu)
                    t2v_st(rG, grow + (unsigned)(pp * T2V_XW + T2V_KATT + u0 + pu) * 16u, f32x4{0.f, 0.f, 0.f, 0.f});
            }
            if (t == T) break;
            PT_STAMP(wg == NT && t == T / 2, 2);
            __syncthreads();                   // every wave is done reading X (row t)
            // ---- row t+1 into X: h_att(t) is there (or about to be), h_dec(t-1) follows, ctx(t) comes last.  Each bulk
            // gather is preceded by a sparse wait on one word per producer (first unit of every L workgroup / last context
            // column of every T workgroup); the bulk loads then find their data on the first try almost always
            {
                // (both segments in ONE pass — 8 loads of 16 bytes in flight per thread — measured slower: the 32 extra
                // registers spill next to the 160 weight registers and the cell phases pay for it: 9.2 vs 8.7 us per step)
                pt_gather<(NP * T2V_H + T2V_AF_THREADS - 1) / T2V_AF_THREADS, NP>(X, rG, grow, 0, T2V_H, B, 0, a.err, flag);
                PT_STAMP(wg == NT && t == T / 2, 3);
                pt_gather<(NP * T2V_H + T2V_AF_THREADS - 1) / T2V_AF_THREADS, NP>(X, rG, grow, T2V_KATT, T2V_H, B, 0, a.err, flag);
                PT_STAMP(wg == NT && t == T / 2, 4);
                __syncthreads();
                if (flag[0] != 1) return;
                // the h_att(t) half of attention_rnn(t+1), in the shadow of attention(t)
                accA.clear();
                if (t + 1 < T) pt_fma_range<PT_JA / 2, 0, 8, NB>(wa, X, kp, accA);
                if (cell_on && t + 1 < T) {
                    const uint32_t idx = (uint32_t)cb * T2V_H + U;
                    fdrop[tid] = t2v_drop_scale(seed, T2V_RNG_ATT_C, t, idx, a.p_att);
                    fdrop[32 + tid] = t2v_drop_scale(seed, T2V_RNG_ATT_H, t + 1, idx, a.p_att);
                }
                PT_STAMP(wg == NT && t == T / 2, 6);
                const int rounds = pt_gather<(NP * T2V_E + T2V_AF_THREADS - 1) / T2V_AF_THREADS, NP>(X, rG, grow, T2V_H, T2V_E, B, ctx_nap, a.err, flag);
                // adaptive nap: wake up just before the context lands (a poll round is about 16 nap units long)
                ctx_nap = t2v_adapt_nap(ctx_nap, rounds);
                PT_WALL(wg == NT && t == T / 2, 23);
                if (a.prof && wg == NT && t == T / 2 && tid == 0) { a.prof[24] = (unsigned long long)rounds; a.prof[25] = (unsigned long long)ctx_nap; }
            }
            __syncthreads();
            if (flag[0] != 1) return;
            PT_STAMP(wg == NT && t == T / 2, 5);
        }
        return;
    }

    // =============================================================================== T role: attention slice (b, s)
    // t2v_attn_role_fwd.inc, shared with k_dec_train_persist16; what is this kernel's own: item ab is word myw of plane mypl of
    // a G row, h_att(t) arrives as 1024 of those words (two per thread), a context column leaves as one.
#define AF_TAIL 0
#define AF_SETUP const int mypl = ab >> 2, myw = ab & 3;
#define AF_GROW grow_b
#define AF_STAMP_STEP PT_STAMP(wg == 0 && t == T / 2, 8)
#define AF_STAMP_H PT_STAMP(wg == 0 && t == T / 2, 9)
#define AF_STAMP_Q PT_STAMP(wg == 0 && t == T / 2, 13)
#define AF_STAMP_E PT_STAMP(wg == 0 && t == T / 2, 10)
#define AF_STAMP_EX PT_STAMP(wg == 0 && t == T / 2, 14)
#define AF_STAMP_ALPHA PT_STAMP(wg == 0 && t == T / 2, 11)
#define AF_STAMP_END PT_WALL(wg == 0 && t == T / 2, 22); PT_STAMP(wg == 0 && t == T / 2, 12)
#define AF_H_INGEST {                                                                                                           \
            const unsigned s0 = grow + (unsigned)(mypl * T2V_XW + tid) * 16u + 4u * (unsigned)myw;                              \
            float v0, v1;                                                                                                       \
            for (int i = 0; i < h_nap; i += 8) __builtin_amdgcn_s_sleep(8);                                                     \
            int rounds = 0;                                                                                                     \
            for (;;) {                                                                                                          \
                v0 = __uint_as_float(t2v_ld_b32(rG, s0));                                                                       \
                v1 = __uint_as_float(t2v_ld_b32(rG, s0 + T2V_AF_THREADS * 16u));                                                \
                if (__all(t2v_ok(v0) && t2v_ok(v1))) break;                                                                     \
                __builtin_amdgcn_s_sleep(1);                                                                                    \
                if (t2v_give_up(rounds, (int)(T2V_AF_SPIN / 4), a.err, flag)) break;                                            \
            }                                                                                                                   \
            h_nap = t2v_adapt_nap(h_nap, rounds);                                                                               \
            PT_WALL(wg == 0 && t == T / 2, 21);                                                                                 \
            if (a.prof && wg == 0 && t == T / 2 && tid == 0) { a.prof[26] = (unsigned long long)rounds; a.prof[27] = (unsigned long long)h_nap; } \
            hx[tid] = v0;                                                                                                       \
            hx[tid + T2V_AF_THREADS] = v1;                                                                                      \
        }
#define AF_CTX_PUBLISH t2v_st(rG, grow + (unsigned)(mypl * T2V_XW + T2V_H + 64 * as + tid) * 16u + 4u * (unsigned)myw, acc);
#include "t2v_attn_role_fwd.inc"
#undef AF_TAIL
#undef AF_SETUP
#undef AF_GROW
#undef AF_STAMP_STEP
#undef AF_STAMP_H
#undef AF_STAMP_Q
#undef AF_STAMP_E
#undef AF_STAMP_EX
#undef AF_STAMP_ALPHA
#undef AF_STAMP_END
#undef AF_H_INGEST
#undef AF_CTX_PUBLISH
}

static size_t pt_lds_bytes(int B, int T_in) {
    const size_t np = B > 4 ? 2 : 1;
    const size_t lrole = np * T2V_XW * 4 + 4 * 8 * 32 + 8 * 32 + 4;
    const size_t trole = t2v_attn_fwd_lds_floats(T_in, 0);
    return sizeof(float) * (lrole > trole ? lrole : trole);
}
static size_t pt_g_floats(int B, int T_out) { return (size_t)(T_out + 2) * (B > 4 ? 2 : 1) * T2V_XW * 4; }
static size_t pt_ex_floats(int B, int T_in, int T_out) { return (size_t)T_out * B * 8 * t2v_tcap(T_in); }

static const void* pt_kernel(int B, int T_in) {
    if (T_in > T2V_AF_MAXT) return B > 4 ? (const void*)k_dec_train_persist<6, true> : (const void*)k_dec_train_persist<4, true>;
    return B > 4 ? (const void*)k_dec_train_persist<6, false> : (const void*)k_dec_train_persist<4, false>;
}

extern "C" int t2v_decoder_train_persist_supported(int B, int T_in) {
    if (!(B >= 1 && B <= PT_MAXB && T_in >= 1 && T_in <= T2V_AF_MAXT_LONG && pt_lds_bytes(B, T_in) <= T2V_LDS_MAX)) return 0;
    static bool raised = false;
    return t2v_persist_resident(pt_kernel(B, T_in), T2V_AF_THREADS, pt_lds_bytes(B, T_in),
                                {pt_kernel(4, T2V_AF_MAXT), pt_kernel(4, T2V_AF_MAXT + 1), pt_kernel(6, T2V_AF_MAXT), pt_kernel(6, T2V_AF_MAXT + 1)}, raised);
}
extern "C" long t2v_decoder_train_persist_scratch_floats(int B, int T_in, int T_out) {
    if (B < 1 || B > PT_MAXB || T_in < 1 || T_out < 1) return 0;
    return (long)(pt_g_floats(B, T_out) + pt_ex_floats(B, T_in, T_out));
}

extern "C" int t2v_decoder_train_fwd_persistent(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s, float* scratch,
                                                int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!w || !s || !scratch || T_out < 1 || !t2v_decoder_train_persist_supported(B, T_in)) return T2V_ERR_ARG;
    if (pt_g_floats(B, T_out) * 4 >= 0x7fffffffull || pt_ex_floats(B, T_in, T_out) * 4 >= 0x7fffffffull) return T2V_ERR_ARG;   // 31-bit buffer offsets
    unsigned* sync = t2v_persist_fwd_begin(w, s, scratch, B, T_in, stream);
    if (!sync) return T2V_ERR_ARG;
    t2v_fill_sentinel(scratch, (pt_g_floats(B, T_out) + pt_ex_floats(B, T_in, T_out)) / 4, 1024, stream);
    PTArgs a;
    a.w_ih_att = w->w_ih_att; a.w_hh_att = w->w_hh_att; a.w_ih_dec = w->w_ih_dec; a.w_hh_dec = w->w_hh_dec;
    a.bias_dec = w->bias_dec; a.wq = w->wq; a.wcomb = w->wcomb; a.v = w->v;
    a.gpre = s->gpre; a.memory = s->memory; a.pm = s->pm; a.lengths = s->lengths;
    a.XS = s->XS; a.CA = s->CA; a.CD = s->CD; a.GA = s->GA; a.GD = s->GD; a.AL = s->AL; a.ACUM = s->ACUM; a.S = s->S;
    a.G = scratch;
    a.EX = scratch + pt_g_floats(B, T_out);
    a.err = sync + 31;
    a.B = B; a.T_in = T_in; a.T_out = T_out; a.p_att = p_att; a.p_dec = p_dec; a.seed = seed;
    a.step = t2v_step_for(stream);
    a.prof = g_t2v_prof;
    const size_t lds = pt_lds_bytes(B, T_in);
    if (T_in > T2V_AF_MAXT) {
        if (B > 4) k_dec_train_persist<6, true><<<T2V_NWG, T2V_AF_THREADS, lds, stream>>>(a);
        else k_dec_train_persist<4, true><<<T2V_NWG, T2V_AF_THREADS, lds, stream>>>(a);
    } else {
        if (B > 4) k_dec_train_persist<6, false><<<T2V_NWG, T2V_AF_THREADS, lds, stream>>>(a);
        else k_dec_train_persist<4, false><<<T2V_NWG, T2V_AF_THREADS, lds, stream>>>(a);
    }
    return t2v_check_launch();
}
