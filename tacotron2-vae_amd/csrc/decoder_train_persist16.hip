// Teacher-forced decoder recurrence, forward, for hparams.bf16_run (BASELINE configs[4]: B = 16 per GPU) as ONE persistent
// launch (reference Decoder.forward's time loop model.py:415-421 -> Decoder.decode 346-389 -> Attention.forward 67-88;
// replaces fp16_optimizer.py's fp16 model copy on this path: bf16 weight operands, fp32 accumulation / cell state /
// saved activations, exactly what the launch-per-step pair k_lstm_fwd256<true> + k_attn_fwd computes).
//
// Round 5.  decoder_train_persist.hip keeps the fp32 weights of 4-5 hidden units per workgroup in 160 VGPRs per thread and
// multiplies them with packed VALU FMAs: that is what limits it to B <= 6.  Here the weights are rounded to bf16 (the same
// RNE rounding as t2v_pack_lstm_weights_bf16), a workgroup owns EIGHT hidden units of both cells (two 16-row MFMA tiles per
// cell: 4 units x 4 gates, unit-major), and the batch is the N dimension of v_mfma_f32_16x16x32_bf16: B <= 16 is one tile.
//
// Roles (one 512-thread workgroup per CU, all co-resident):
//   T : workgroups [0, 8B)      — attention slice (item b = wg / 8, s = wg % 8): the role of decoder_train_persist.hip, the
//                                 same program text (t2v_attn_role_fwd.inc; fp32: bf16_run keeps the attention in fp32)
//   L : workgroups [128, 256)   — LSTM rows of both cells: workgroup j owns units [8j, 8j + 8).  K is split over the 8 waves:
//                                 wave w multiplies h_att k-blocks [4w, 4w+4), ctx k-blocks [32+2w, 32+2w+2) and h_dec
//                                 k-blocks [48+4w, 48+4w+4) (32 columns each) of both cells — 48 + 80 weight registers.
//   (workgroups [8B, 128) leave at once when B < 16)
//
// The state exchange IS the MFMA operand.  Row r of GH = [h_att(r-1) | ctx(r-1) | h_dec(r-2)] rounded to bf16, laid out
// [k / 8][item 0..15][8 consecutive k] — 16 bytes per (k-group, item) — so the B operand of k-block kb for lane l (item
// l & 15, k-group l >> 4) is the 16 bytes at kb * 1024 + 16 l: a wave polls ITS OWN k-blocks with fully coalesced 1-KB loads
// straight into the registers the MFMA reads.  No LDS staging of the state, no all-threads gather, no barrier between
// "arrived" and "multiplied"; what a workgroup pulls per step is 80 KB (B = 16) where the fp32 kernel pulls 61 KB at B = 6.
// Sentinel protocol as in decoder_train_persist.hip: rows are pre-filled with T2V_SENT (a pair of bf16 NaNs that rounding
// a finite fp32 never produces), producers store write-through (sc1), consumers poll the payload with sc1 loads.
// The attention slices read h_att(t) in fp32 from HX (T rows x 16 items x 1024) — the attention stays fp32 like the
// launch-per-step path — and publish their 64 context columns as eight 16-byte bf16 chunks.
//
// Per step the chain is  A-finish(ctx(t-1): 4 MFMAs) -> cross-wave reduce -> cell -> h_att hop -> attention(t) -> ctx hop;
// decoder_rnn(t-1) finishes behind the same barrier, everything else (h_att / h_dec parts of both products) runs in the shadow
// of attention(t).  Writes the same arena as the launch-per-step loop (XS, CA, CD, GA, GD, AL, ACUM, S), same counter-based
// dropout masks: either backward runs on it.
//
// Measured on the way (same-box A/B through a run-time switch, B = 16, T_in = 84, T = 400; none kept): TWO polls in flight on
// the ctx / h_att hand-offs 9.63 -> 10.2 / 9.9 us per step (the polling traffic is what stretches a look's round trip to ~1 us);
// re-polling only the k-blocks that are still missing 9.63 -> 9.65; partial energies as 16-byte stores + 16-byte polls through
// an LDS transpose 9.51 -> 9.63 (the extra barrier costs more than the narrower stores); a gentler nap rule: no change.
#include "t2v_common.h"
#include "t2v_kernels.h"
#include "t2v_xchg.h"

#define P16_MAXB 16                  // (thread count, spin limit and the T_in bounds: T2V_AF_*, t2v_kernels.h)
#define P16_NL 128
#define P16_L0 (T2V_NWG - P16_NL)
#define P16_GROW (T2V_XW / 8 * 16 * 16)        // bytes per GH row: 320 k-groups x 16 items x 16 B = 81 920
#define P16_HROW (16 * T2V_H * 4)              // bytes per HX row: 16 items x 1024 fp32 = 65 536

struct P16Args {
    const float* w_ih_att; const float* w_hh_att; const float* w_ih_dec; const float* w_hh_dec;
    const float* bias_dec; const float* wq; const float* wcomb; const float* v;
    const float* gpre; const float* memory; const float* pm; const int32_t* lengths;
    float* XS; float* CA; float* CD; float* GA; float* GD; float* AL; float* ACUM; float* S;
    void* GH;                 // (T+2) rows x 81 920 B, sentinel-filled: bf16 state rows in MFMA-operand order
    float* HX;                // T rows x 16 x 1024 fp32: h_att(t) for the attention slices
    float* EX;                // T x B x 8 x Tcap partial energies
    unsigned* err;
    int B, T_in, T_out;
    float p_att, p_dec;
    uint64_t seed;
    const t2v_step_params* step;
    unsigned long long* prof;
};
#define P16_STAMP(COND, I) do { if (a.prof && (COND) && (threadIdx.x & 63) == 0) a.prof[(I)] = __builtin_readcyclecounter(); } while (0)
#define P16_WALL(COND, I) do { if (a.prof && (COND) && (threadIdx.x & 63) == 0) a.prof[(I)] = wall_clock64(); } while (0)
// per-workgroup time line of ONE step (t = T/2) on the chip-wide 100 MHz counter: prof[64 + workgroup * 8 + slot]
// (tools/dbg/persist16_prof.py passes a buffer of 64 + 256 * 8 words)
#define P16_RT(SLOT) do { if (a.prof && t == a.T_out / 2 && threadIdx.x == 0) a.prof[64 + blockIdx.x * 8 + (SLOT)] = __builtin_amdgcn_s_memrealtime(); } while (0)

__device__ __forceinline__ f32x4 p16_mfma(u32x4 w, u32x4 x, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(t2v_bf16x8, w), __builtin_bit_cast(t2v_bf16x8, x), c, 0, 0, 0);
}

// Poll N consecutive k-blocks of one GH row straight into MFMA B operands.  off = row + kb0 * 1024 + 16 * lane.  A lane
// whose item does not exist (live == false) never waits and reads zeros.  Wave-uniform loop; returns the failed rounds.
template <int N>
__device__ __forceinline__ int p16_poll(u32x4 (&x)[N], __amdgpu_buffer_rsrc_t rG, unsigned off, bool live, int nap,
                                        unsigned* err, int* flag) {
    for (int i = 0; i < nap; i += 8) __builtin_amdgcn_s_sleep(8);
    int rounds = 0;
    for (;;) {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = t2v_ld_b128(rG, off + 1024u * (unsigned)i);
        bool ok = true;
#pragma unroll
        for (int i = 0; i < N; ++i) ok = ok && t2v_ok4(x[i]);
        if (__all(ok || !live)) break;
        __builtin_amdgcn_s_sleep(2);
        if (t2v_give_up(rounds, (int)(T2V_AF_SPIN / 4), err, flag)) break;
    }
    if (!live) {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = u32x4{0u, 0u, 0u, 0u};
    }
    return rounds;
}

// bf16x8 A operand of one (tile, k-block): 8 consecutive columns of one gate row, read from the nn.LSTMCell tensors
__device__ __forceinline__ u32x4 p16_wload(const float* p) {
    const float4 lo = *(const float4*)p, hi = *(const float4*)(p + 4);
    const uint4 u = t2v_pack_bf16x8(lo, hi);
    return u32x4{u.x, u.y, u.z, u.w};
}

template <bool LONG>          // the attention role for 224 < T_in <= 560, as in k_dec_train_persist<.., true>
__global__ __launch_bounds__(T2V_AF_THREADS) void k_dec_train_persist16(P16Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint64_t seed = t2v_step_seed(a.seed, a.step);
    const int wg = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int B = a.B, Tp = a.T_in, T = a.T_out;
    const int NT = 8 * B;
    const __amdgpu_buffer_rsrc_t rG = t2v_rsrc(a.GH), rH = t2v_rsrc(a.HX), rE = t2v_rsrc(a.EX);
    const int Tcap = (Tp + 15) & ~15;

#ifndef P16_ONLY_T     // (per-role register reports: tools/dbg/role_regs.sh builds the kernel with one role compiled out)
    if (wg >= P16_L0) {
        // =========================================================================== L role: 8 units of both cells
        f32x4* red = (f32x4*)lds;                            // [parity 2][cell 2][wave 8][tile 2][lane 64]
        float* hs = lds + 2 * 2 * 8 * 2 * 64 * 4;            // [cell wave 4][item 16][4 units]
        int* flag = (int*)(hs + 4 * 64);
        const int j = wg - P16_L0, u0 = 8 * j;
        const int n = lane & 15, g = lane >> 4;              // MFMA: item column / k-group (operands), unit of the tile (results)
        const bool live = n < B;
        // ---- weights: tile m, A row (lane & 15) = 4 * unit + gate -> gate row gate * 1024 + u0 + 4 m + unit; k-group g
        u32x4 wa[2][6], wd[2][10];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const size_t row = (size_t)(n & 3) * T2V_H + u0 + 4 * m + (n >> 2);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 32 * (4 * wave + i) + 8 * g;                       // h_att columns
                wa[m][i] = p16_wload(a.w_hh_att + row * T2V_H + k);
                wd[m][i] = p16_wload(a.w_ih_dec + row * T2V_KATT + k);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int k = 32 * (2 * wave + i) + 8 * g;                       // context columns
                wa[m][4 + i] = p16_wload(a.w_ih_att + row * (T2V_PRE + T2V_E) + T2V_PRE + k);
                wd[m][4 + i] = p16_wload(a.w_ih_dec + row * T2V_KATT + T2V_H + k);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 32 * (4 * wave + i) + 8 * g;                       // h_dec columns
                wd[m][6 + i] = p16_wload(a.w_hh_dec + row * T2V_H + k);
            }
        }
        if (tid == 0) flag[0] = 1;
        // cell waves: 0, 1 = attention_rnn tiles 0, 1; 2, 3 = decoder_rnn tiles 0, 1.  Lane (item n, unit g of the tile)
        const bool is_cell = wave < 4;
        const int cm = wave & 1, ccell = wave >> 1;          // tile, cell (0 att, 1 dec)
        const int U = u0 + 4 * cm + g;
        const bool cell_on = is_cell && live;
        float cst = 0.f;                                     // this lane's cell state (pre-dropout), whole pass
        float bias[4] = {0.f, 0.f, 0.f, 0.f};
        if (cell_on && ccell == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bias[r] = a.bias_dec[r * T2V_H + U];
        }
        if (is_cell) hs[wave * 64 + lane] = 0.f;
        __syncthreads();
        // byte offsets of this wave's k-blocks inside a GH row
        const unsigned off_h = (unsigned)(4 * wave) * 1024u + 16u * (unsigned)lane;
        const unsigned off_c = (unsigned)(32 + 2 * wave) * 1024u + 16u * (unsigned)lane;
        const unsigned off_d = (unsigned)(48 + 4 * wave) * 1024u + 16u * (unsigned)lane;
        u32x4 xc[2] = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};     // ctx(-1) = 0
        f32x4 pA[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};         // h_att part of attention_rnn(t)
        f32x4 pD[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};         // h_att + h_dec parts of decoder_rnn(t-1)
        int nap_h = 0, nap_c = 0;
        // state-dropout factors of the NEXT cell evaluation of this lane (counter-based: functions of (seed, t, unit, item) alone),
        // drawn in the shadow of attention(t) instead of on the chain: two 64-bit hash rounds per cell and step
        float f_c = 1.0f, f_h = 1.0f;
        if (cell_on && ccell == 0) f_h = t2v_drop_scale(seed, T2V_RNG_ATT_H, 0, (uint32_t)n * T2V_H + U, a.p_att);

        for (int t = 0; t <= T; ++t) {
            const bool do_att = t < T, do_dec = t >= 1;
            const unsigned grow = (unsigned)(t + 1) * (unsigned)P16_GROW;          // row t+1 = [h_att(t) | ctx(t) | h_dec(t-1)]
            f32x4* redp = red + (size_t)(t & 1) * (2 * 8 * 2 * 64);
            P16_STAMP(wg == P16_L0 && wave == 0 && t == T / 2, 0);
            P16_RT(0);
            // Prenet term of this step for the attention_rnn cell lanes (issued before the products: latency hidden)
            float gp[4] = {0.f, 0.f, 0.f, 0.f};
            if (cell_on && ccell == 0 && do_att) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gp[r] = a.gpre[((size_t)t * B + n) * T2V_G + r * T2V_H + U];
            }
            // ---- both cells finish with ctx(t-1): 4 + 4 MFMAs, partial tiles to LDS
            if (do_att) {
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    f32x4 acc = p16_mfma(wa[m][4], xc[0], pA[m]);
                    acc = p16_mfma(wa[m][5], xc[1], acc);
                    redp[((0 * 8 + wave) * 2 + m) * 64 + lane] = acc;
                }
            }
            if (do_dec) {
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    f32x4 acc = p16_mfma(wd[m][4], xc[0], pD[m]);
                    acc = p16_mfma(wd[m][5], xc[1], acc);
                    redp[((1 * 8 + wave) * 2 + m) * 64 + lane] = acc;
                }
            }
            P16_STAMP(wg == P16_L0 && wave == 0 && t == T / 2, 1);
            __syncthreads();
            if (flag[0] != 1) return;
            P16_STAMP(wg == P16_L0 && wave == 0 && t == T / 2, 2);
            P16_RT(1);
            // ---- cell update + publish (4 waves, one tile of one cell each)
            if (is_cell && (ccell == 0 ? do_att : do_dec)) {
                const f32x4* rp = redp + ((ccell * 8) * 2 + cm) * 64 + lane;       // wave stride: 2 * 64
                const f32x4 s4 = ((rp[0] + rp[128]) + (rp[256] + rp[384])) + ((rp[512] + rp[640]) + (rp[768] + rp[896]));
                P16_STAMP(wg == P16_L0 && wave == 0 && t == T / 2 && s4[0] != 123.f, 13);
                const int tt = ccell == 0 ? t : t - 1;
                float hd = 0.f, c = 0.f, gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f;
                if (cell_on) {
                    gi = sigmoidf_(s4[0] + (ccell == 0 ? gp[0] : bias[0]));
                    gf = sigmoidf_(s4[1] + (ccell == 0 ? gp[1] : bias[1]));
                    gg = tanhf_(s4[2] + (ccell == 0 ? gp[2] : bias[2]));
                    go = sigmoidf_(s4[3] + (ccell == 0 ? gp[3] : bias[3]));
                    c = gf * (cst * f_c) + gi * gg;
                    cst = c;
                    hd = go * tanhf_(c) * f_h;
                }
                P16_STAMP(wg == P16_L0 && wave == 0 && t == T / 2 && hd != 123.f, 14);
                // publish FIRST (the write-through store is what attention(t) waits for): lane b < B of this wave sends item b's
                // 4 units of the tile — 8 bytes of bf16 into the state row (+ 16 bytes of fp32 into HX for the attention slices);
                // the LDS round trip stays inside the wave (in-order), no barrier
                hs[wave * 64 + 4 * n + g] = hd;
                const float4 hv4 = *(const float4*)(hs + wave * 64 + 4 * (lane & 15));
                if (lane < B && (ccell == 0 || t < T)) {
                    const u32x2 pk = {t2v_pack_bf16x2(hv4.x, hv4.y), t2v_pack_bf16x2(hv4.z, hv4.w)};
                    const unsigned kg = (unsigned)((ccell == 0 ? 0 : T2V_KATT) / 8 + j);
                    t2v_st(rG, grow + (kg * 16u + (unsigned)lane) * 16u + 8u * (unsigned)cm, pk);
                    if (ccell == 0)
                        t2v_st(rH, (unsigned)t * (unsigned)P16_HROW + (unsigned)(lane * T2V_H + u0 + 4 * cm) * 4u,
                                 u32x4{__float_as_uint(hv4.x), __float_as_uint(hv4.y), __float_as_uint(hv4.z), __float_as_uint(hv4.w)});
                }
                P16_STAMP(wg == P16_L0 && wave == 0 && t == T / 2, 15);
                if (cell_on) {          // the saved activations follow (plain stores)
                    if (ccell == 0) a.CA[((size_t)(t + 1) * B + n) * T2V_H + U] = c;
                    else a.CD[((size_t)t * B + n) * T2V_H + U] = c;
                    float* gsv = ccell == 0 ? a.GA : a.GD;
                    if (gsv) {
                        float* gs = gsv + ((size_t)tt * B + n) * T2V_G + U;
                        gs[0] = gi; gs[T2V_H] = gf; gs[2 * T2V_H] = gg; gs[3 * T2V_H] = go;
                    }
                    a.XS[((size_t)(t + 1) * B + n) * T2V_XW + (ccell == 0 ? 0 : T2V_KATT) + U] = hd;
                }
            }
            if (t == T) break;
            P16_STAMP(wg == P16_L0 && wave == 0 && t == T / 2, 3);
            P16_RT(2);
            if (cell_on) {          // dropout factors of this lane's next cell evaluation: step tt' = t + 1 (attention_rnn) / t (decoder_rnn)
                const int ntt = ccell == 0 ? t + 1 : t;
                const uint32_t idx = (uint32_t)n * T2V_H + U;
                const float p = ccell == 0 ? a.p_att : a.p_dec;
                f_c = ntt > 0 ? t2v_drop_scale(seed, ccell == 0 ? T2V_RNG_ATT_C : T2V_RNG_DEC_C, ntt - 1, idx, p) : 1.0f;
                f_h = t2v_drop_scale(seed, ccell == 0 ? T2V_RNG_ATT_H : T2V_RNG_DEC_H, ntt, idx, p);
            }
            // ---- row t+1 in the shadow of attention(t): h_att(t) -> its share of attention_rnn(t+1) and decoder_rnn(t);
            // h_dec(t-1) -> decoder_rnn(t); ctx(t) last (the chain)
            {
                u32x4 xh[4];
                const int rounds = p16_poll<4>(xh, rG, grow + off_h, live, nap_h, a.err, flag);
                nap_h = t2v_adapt_nap(nap_h, rounds);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accD = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        accA = p16_mfma(wa[m][i], xh[i], accA);
                        accD = p16_mfma(wd[m][i], xh[i], accD);
                    }
                    pA[m] = accA;
                    pD[m] = accD;
                }
            }
            P16_STAMP(wg == P16_L0 && wave == 0 && t == T / 2, 4);
            P16_RT(3);
            if (t >= 1) {
                u32x4 xd[4];
                p16_poll<4>(xd, rG, grow + off_d, live, 0, a.err, flag);
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int i = 0; i < 4; ++i) pD[m] = p16_mfma(wd[m][6 + i], xd[i], pD[m]);
            }
            P16_STAMP(wg == P16_L0 && wave == 0 && t == T / 2, 5);
            P16_RT(4);
            {
                const int rounds = p16_poll<2>(xc, rG, grow + off_c, live, nap_c, a.err, flag);
                nap_c = t2v_adapt_nap(nap_c, rounds);
                if (a.prof && t == T / 2 && tid == 0) { a.prof[64 + wg * 8 + 6] = (unsigned long long)rounds; a.prof[64 + wg * 8 + 7] = (unsigned long long)nap_c; }
            }
            P16_RT(5);
            P16_WALL(wg == P16_L0 && wave == 0 && t == T / 2, 23);
        }
        return;
    }
#endif
#ifdef P16_ONLY_L
    return;
#else
    if (wg >= NT) return;

    // =============================================================================== T role: attention slice (b, s)
    // t2v_attn_role_fwd.inc, shared with k_dec_train_persist; what is this kernel's own: h_att(t) arrives as 4 KB of fp32 in HX (16
    // bytes per thread of waves 0..3), the 64 context columns leave as bf16: lanes 0..7 send 8 columns each as one 16-byte chunk
    // (k-group 128 + 8 as + lane, item ab) out of cfin[64], the finished columns; the LDS round trip stays inside wave 0.
#define AF_TAIL 64
#define AF_SETUP float* cfin = rss + 32;
#define AF_GROW (unsigned)P16_GROW
#define AF_STAMP_STEP P16_STAMP(wg == 0 && wave == 0 && t == T / 2, 8); P16_RT(0)
#define AF_STAMP_H P16_STAMP(wg == 0 && wave == 0 && t == T / 2, 9)
#define AF_STAMP_Q
#define AF_STAMP_E P16_STAMP(wg == 0 && wave == 0 && t == T / 2, 10); P16_RT(2)
#define AF_STAMP_EX P16_RT(3)
#define AF_STAMP_ALPHA P16_STAMP(wg == 0 && wave == 0 && t == T / 2, 11); P16_RT(4)
#define AF_STAMP_END P16_WALL(wg == 0 && wave == 0 && t == T / 2, 22); P16_STAMP(wg == 0 && wave == 0 && t == T / 2, 12); P16_RT(5)
#define AF_H_INGEST if (tid < 256) {                                                                                            \
            const unsigned s0 = (unsigned)t * (unsigned)P16_HROW + (unsigned)(ab * T2V_H + 4 * tid) * 4u;                       \
            u32x4 v;                                                                                                            \
            for (int i = 0; i < h_nap; i += 8) __builtin_amdgcn_s_sleep(8);                                                     \
            int rounds = 0;                                                                                                     \
            for (;;) {                                                                                                          \
                v = t2v_ld_b128(rH, s0);                                                                                        \
                if (__all(t2v_ok4(v))) break;                                                                                   \
                __builtin_amdgcn_s_sleep(1);                                                                                    \
                if (t2v_give_up(rounds, (int)(T2V_AF_SPIN / 4), a.err, flag)) break;                                            \
            }                                                                                                                   \
            h_nap = t2v_adapt_nap(h_nap, rounds);                                                                               \
            P16_WALL(wg == 0 && wave == 0 && t == T / 2, 21);                                                                   \
            P16_RT(1);                                                                                                          \
            if (a.prof && t == T / 2 && tid == 0) { a.prof[64 + wg * 8 + 6] = (unsigned long long)rounds; a.prof[64 + wg * 8 + 7] = (unsigned long long)h_nap; } \
            *(float4*)(hx + 4 * tid) = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])); \
        }
#define AF_CTX_PUBLISH                                                                                                          \
            cfin[tid] = acc;                                                                                                    \
            if (tid < 8) {                                                                                                      \
                const float4 c0 = *(const float4*)(cfin + 8 * tid), c1 = *(const float4*)(cfin + 8 * tid + 4);                  \
                const uint4 pk = t2v_pack_bf16x8(c0, c1);                                                                       \
                const unsigned kg = (unsigned)(T2V_H / 8 + 8 * as + tid);                                                       \
                t2v_st(rG, grow + (kg * 16u + (unsigned)ab) * 16u, u32x4{pk.x, pk.y, pk.z, pk.w});                              \
            }
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
#endif
}

static size_t p16_lds_bytes(int T_in) {
    const size_t lrole = 2 * 2 * 8 * 2 * 64 * 4 + 4 * 64 + 4;
    const size_t trole = t2v_attn_fwd_lds_floats(T_in, 64);         // cfin[64]
    return sizeof(float) * (lrole > trole ? lrole : trole);
}
static size_t p16_gh_floats(int T_out) { return (size_t)(T_out + 2) * (P16_GROW / 4); }
static size_t p16_hx_floats(int T_out) { return (size_t)T_out * (P16_HROW / 4); }
static size_t p16_ex_floats(int B, int T_in, int T_out) { return (size_t)T_out * B * 8 * t2v_tcap(T_in); }

static const void* p16_kernel(int T_in) {
    return T_in > T2V_AF_MAXT ? (const void*)k_dec_train_persist16<true> : (const void*)k_dec_train_persist16<false>;
}
extern "C" int t2v_decoder_train_persist16_supported(int B, int T_in) {
    if (!(B >= 1 && B <= P16_MAXB && T_in >= 1 && T_in <= T2V_AF_MAXT_LONG && p16_lds_bytes(T_in) <= T2V_LDS_MAX)) return 0;
    static bool raised = false;
    return t2v_persist_resident(p16_kernel(T_in), T2V_AF_THREADS, p16_lds_bytes(T_in), {p16_kernel(T2V_AF_MAXT), p16_kernel(T2V_AF_MAXT + 1)}, raised);
}
extern "C" long t2v_decoder_train_persist16_scratch_floats(int B, int T_in, int T_out) {
    if (B < 1 || B > P16_MAXB || T_in < 1 || T_out < 1) return 0;
    return (long)(p16_gh_floats(T_out) + p16_hx_floats(T_out) + p16_ex_floats(B, T_in, T_out));
}

extern "C" int t2v_decoder_train_fwd_persistent16(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s, float* scratch,
                                                  int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!w || !s || !scratch || T_out < 1 || !t2v_decoder_train_persist16_supported(B, T_in)) return T2V_ERR_ARG;
    if (p16_gh_floats(T_out) * 4 >= 0x7fffffffull || p16_hx_floats(T_out) * 4 >= 0x7fffffffull ||
        p16_ex_floats(B, T_in, T_out) * 4 >= 0x7fffffffull)
        return T2V_ERR_ARG;                                  // 31-bit buffer offsets
    unsigned* sync = t2v_persist_fwd_begin(w, s, scratch, B, T_in, stream);
    if (!sync) return T2V_ERR_ARG;
    t2v_fill_sentinel(scratch, (p16_gh_floats(T_out) + p16_hx_floats(T_out) + p16_ex_floats(B, T_in, T_out)) / 4, 1024, stream);
    P16Args a;
    a.w_ih_att = w->w_ih_att; a.w_hh_att = w->w_hh_att; a.w_ih_dec = w->w_ih_dec; a.w_hh_dec = w->w_hh_dec;
    a.bias_dec = w->bias_dec; a.wq = w->wq; a.wcomb = w->wcomb; a.v = w->v;
    a.gpre = s->gpre; a.memory = s->memory; a.pm = s->pm; a.lengths = s->lengths;
    a.XS = s->XS; a.CA = s->CA; a.CD = s->CD; a.GA = s->GA; a.GD = s->GD; a.AL = s->AL; a.ACUM = s->ACUM; a.S = s->S;
    a.GH = scratch;
    a.HX = scratch + p16_gh_floats(T_out);
    a.EX = a.HX + p16_hx_floats(T_out);
    a.err = sync + 31;
    a.B = B; a.T_in = T_in; a.T_out = T_out; a.p_att = p_att; a.p_dec = p_dec; a.seed = seed;
    a.step = t2v_step_for(stream);
    a.prof = g_t2v_prof;
    if (T_in > T2V_AF_MAXT) k_dec_train_persist16<true><<<T2V_NWG, T2V_AF_THREADS, p16_lds_bytes(T_in), stream>>>(a);
    else k_dec_train_persist16<false><<<T2V_NWG, T2V_AF_THREADS, p16_lds_bytes(T_in), stream>>>(a);
    return t2v_check_launch();
}
