// The attention role of the persistent reverse kernels (k_achain_bwd, decoder_train_bwd_persist.hip, and k_bwd_persist16,
// decoder_train_bwd_persist16.hip): attention(t) backward of item b, encoder positions [s JS, s JS + JS), for all steps of one
// pass — softmax / tanh / fused-location-filter backward, split over positions (the body of decoder_bwd.hip's k_attn_cell_bwd).
// Operands that do not change over the pass (memory rows, W_comb^T tile, v) stay in registers, the cumulative-weights gradient
// in LDS.  The arithmetic is fp32 in both kernels, so it exists once, here; what differs between the two comes in through a
// hooks type HK that each kernel defines next to its LSTM roles; the role constructs one object of it, HK(a, b, s):
//   static constexpr int SPIN             bound of the waits
//   int dqt_items()                       items per step of DQT (row stride of the summed dq rows)
//   void dctx_early(t, tid, flag)         before the window loop: fetch what of d ctx(t) does not wait for the chain (may be empty)
//   void dctx_arrive(t, tid, dctx, nap, flag)   at the hand-off: wait for d ctx(t) of item b (nap first, adapt nap) -> dctx[512]
//   void prof_init(flag) / pass_begin() / stamp(t, point) / pass_end()     profile stamps (T2V_AB_* points of a step); pass_begin
//                                         comes behind the barrier that ends the set-up, prof_init in front of it
// The order of memory operations is part of the design: the nap comes before the first poll, and the dpre rows (8 KB of plain
// stores) leave after the dq words that the next role waits for.
// JS: positions per slice (16 / 32: position-split slices on 4 waves; 96 (round 4): all 8 waves — one workgroup per item for
// T_in <= 96, at most six per item for the long texts).  NWV: waves that compute (4 or 8; with 4, waves 4..7 only keep the
// barriers company).  GPW: floats per channel of a slice's window-partial row in GPX.
#pragma once
#include "t2v_common.h"
#include "t2v_kernels.h"
#include "t2v_xchg.h"

#define T2V_AB_THREADS 512           // workgroup size of both reverse kernels
#define T2V_AB_MAXT 224              // 16- / 32-position slices up to here, 96-position slices on eight waves beyond
#define T2V_AB_SMAX (T2V_AB_MAXT / 16)   // 14 slices per item at most (the 96-position form has at most six)

enum { T2V_AB_BEGIN, T2V_AB_DCTX, T2V_AB_DQ, T2V_AB_END };

// floats of the role's LDS carve below for slices of JS positions
static inline size_t t2v_attn_bwd_lds_floats(int T_in, int js) {
    const size_t Tcap = t2v_tcap(T_in), JS = (size_t)js, NWV = JS == 96 ? 8 : 4;
    return 4 * Tcap + T2V_E + JS + (1 + JS / NWV) * 4 * NWV + T2V_A * (JS == 96 ? JS + 17 : JS + 1) + 64 * (JS + 1) +
           2 * 2 * NWV * T2V_A + 40 + (NWV == 8 ? 64 * 132 : 0);
}

// DAL: the pass has an upstream gradient of the alignments themselves, a.dAL (T,B,T_in) — a loss that reads the attention.  It is
// one more addend of the gradient wrt alpha(t), so it joins gp where that is assembled: from there it reaches the own positions'
// dalpha and the softmax's dot product, which are all that gfull0 feeds.  A plain load: the tensor is complete before the launch.
// Without DAL the role is the code it was (the kernels are at their register limit; the pointer-less form is what launches when
// the caller has no such gradient).
template <int JS, int NWV, class HK, bool DAL, class Args>
__device__ __forceinline__ void t2v_attn_role_bwd(const Args& a, float* lds, const int b, const int s) {
    constexpr int NJT = JS / 16;
    constexpr int PW = JS + 30;
    constexpr int GPW = PW <= 64 ? 64 : 128;
    constexpr int NRG = 2 * NWV;                     // row groups of 32 lanes in the dpre loop
    constexpr int DPS = JS == 96 ? JS + 17 : JS + 1; // row stride of dpT: = 17 mod 32, the four k-rows of an MFMA operand read land in
                                                     // disjoint banks (JS + 1 = 97 = 1 mod 32 made that read 4-way conflicted)
    static_assert(JS % NRG == 0 && JS % NWV == 0 && PW <= GPW, "slice geometry");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool act = tid < 64 * NWV;
    const int g = lane >> 4, c16 = lane & 15;
    const int B = a.B, Tp = a.T_in, T = a.T, S = a.S_sl, j0 = s * JS;
    const int Tcap = (Tp + 15) & ~15;
    const int nown = min(JS, Tp - j0);
    HK hk(a, b, s);
    // ---- LDS carve
    float* gfull0 = lds;                      // [Tcap]
    float* gfull1 = gfull0 + Tcap;            // [Tcap]
    float* alf = gfull1 + Tcap;               // [Tcap]
    float* gcum = alf + Tcap;                 // [Tcap] running cumulative-weights gradient (this workgroup's copy)
    float* dctx = gcum + Tcap;                // [512]
    float* de = dctx + T2V_E;                 // [JS]
    float* red = de + JS;                     // [1 + JS/NWV][4 NWV]
    float* dpT = red + (1 + JS / NWV) * 4 * NWV;     // [128][JS+1]
    float* Tl = dpT + T2V_A * DPS;            // [64][JS+1]
    float* rq = Tl + 64 * (JS + 1);           // [NRG][128] (also: the 32 row partials of the dot product)
    float* rv = rq + NRG * T2V_A;             // [NRG][128]
    int* flag = (int*)(rv + NRG * T2V_A);
    // (8-wave form: the W_comb^T operand tile of the location backward lives in LDS, not in 32 registers per thread — next to the
    // 96 registers of memory rows they spilled)
    constexpr bool AREG_LDS = NWV == 8;
    float* wcs = (float*)(flag + 40);         // [64 rows (c,k)][132] when AREG_LDS (flag + 4 .. + 36: the hooks' phase profile)
    const __amdgpu_buffer_rsrc_t rQ = t2v_rsrc(a.DQX), rP = t2v_rsrc(a.GPX), rQT = t2v_rsrc(a.DQT);
    // ---- operands resident for the whole pass
    float4 m0[JS / NWV], m1[JS / NWV];
    float areg[AREG_LDS ? 1 : 32];
    float4 vd4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int d4 = tid & 31;
    if (act) {
#pragma unroll
        for (int r = 0; r < JS / NWV; ++r) {
            const int jl = wave + NWV * r;
            const float* mrow = a.memory + ((size_t)b * Tp + j0 + (jl < nown ? jl : 0)) * T2V_E + lane * 4;
            m0[r] = *(const float4*)mrow;
            m1[r] = *(const float4*)(mrow + 256);
        }
        if (!AREG_LDS) {
            const float4* wp = (const float4*)(a.wcomb + T2V_A * 64 + (16 * (wave & 3) + c16) * 128 + 32 * g);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 w4 = wp[u];
                areg[4 * u + 0] = w4.x; areg[4 * u + 1] = w4.y; areg[4 * u + 2] = w4.z; areg[4 * u + 3] = w4.w;
            }
        }
        vd4 = *(const float4*)(a.v + 4 * d4);
    }
    if (AREG_LDS)
        for (int i = tid; i < 64 * 128; i += T2V_AB_THREADS)          // row stride 132, 33 floats per k-group: conflict-free operand reads
            wcs[(i >> 7) * 132 + ((i & 127) >> 5) * 33 + (i & 31)] = a.wcomb[T2V_A * 64 + i];
    for (int j = tid; j < Tcap; j += T2V_AB_THREADS) gcum[j] = 0.f;
    if (tid == 0) flag[0] = 1;
    float dvacc = 0.f;                          // tid < 128: running dv[tid] of this slice
    int nap = 0;
    hk.prof_init(flag);
    __syncthreads();
    hk.pass_begin();

    for (int t = T - 1; t >= 0; --t) {
        // (thread-derived indices are recomputed per step from an opaque copy: hoisted, they are spilled next to the 96 registers
        // of memory rows, and every reload is a drain of the wave's memory queue)
        int tid_op = threadIdx.x;
        asm volatile("" : "+v"(tid_op));
        const int tid = tid_op, lane = tid & 63, wave = tid >> 6;
        const bool act = tid < 64 * NWV;
        const int g = lane >> 4, c16 = lane & 15;
        const int d4 = tid & 31, rg = (tid >> 5) & (NRG - 1);
        hk.stamp(t, T2V_AB_BEGIN);
        // ---- operands that do not wait for the context gradient: tanh outputs, alpha(t), ctx(t), window partials of step t+1,
        // and whatever part of the context gradient the kernel can have early (hk.dctx_early)
        float4 sreg[JS / NRG];
        float2 ctx2 = make_float2(0.f, 0.f);
        if (act) {
            const float* sp = a.S + (((size_t)t * B + b) * Tp + j0) * T2V_A + 4 * d4;
#pragma unroll
            for (int i = 0; i < JS / NRG; ++i) {
                const int jl = rg + NRG * i;
                sreg[i] = *(const float4*)(sp + (size_t)min(jl, nown - 1) * T2V_A);
            }
            if (tid < 256) ctx2 = *(const float2*)(a.XS + ((size_t)(t + 1) * B + b) * T2V_XW + T2V_H + 2 * tid);
        }
        hk.dctx_early(t, tid, flag);
        float dot_g = 0.f;
        for (int j = tid; j < Tp; j += T2V_AB_THREADS) {
            float gp = 0.f, gc = gcum[j];
            if (t < T - 1) {
                const int lo = max(0, (j + 15 - PW + JS) / JS), hi = min(S - 1, (j + 15) / JS);
                for (int sp2 = lo; sp2 <= hi; ++sp2) {
                    const int jj = j - sp2 * JS + 15;
                    if (jj < 0 || jj >= PW) continue;
                    const unsigned off = (unsigned)((((t + 1) * B + b) * S + sp2) * (2 * GPW) + jj) * 4u;
                    unsigned x0, x1;
                    int spins = 0;
                    for (;;) {          // published at the end of the previous reverse step: almost always there
                        x0 = t2v_ld_b32(rP, off);
                        x1 = t2v_ld_b32(rP, off + 4u * GPW);
                        if (t2v_ok(x0) && t2v_ok(x1)) break;
                        __builtin_amdgcn_s_sleep(1);
                        if (t2v_give_up(spins, HK::SPIN, a.err, flag)) break;
                    }
                    gp += __uint_as_float(x0);
                    gc += __uint_as_float(x1);
                }
            }
            if (DAL) gp += a.dAL[((size_t)t * B + b) * Tp + j];
            gcum[j] = gc;
            gfull0[j] = gp;
            gfull1[j] = gc;
            const float al = a.AL[((size_t)(t + 1) * B + b) * Tp + j];
            alf[j] = al;
            dot_g = fmaf(al, gp + gc, dot_g);
        }
        // ---- the context gradient of this item into dctx[512], nap first — this hand-off is on the chain of every reverse step
        hk.dctx_arrive(t, tid, dctx, nap, flag);
        __syncthreads();
        if (flag[0] != 1) return;
        hk.stamp(t, T2V_AB_DCTX);
        // ---- dot = dctx·ctx_t + sum_j alpha_j (Gprev_j + Gcum_j); dalpha of the own positions = dctx·memory_j + G_j
        {
            float dotp = dot_g;
            if (tid < 256) dotp += dctx[2 * tid] * ctx2.x + dctx[2 * tid + 1] * ctx2.y;
            dotp = row16_sum(dotp);
            // 32 row partials (8 waves x 4 rows): waves 4..7 carry only their share of dot_g
            if (c16 == 0) rq[4 * wave + g] = dotp;
            if (act) {
                const float4 d0 = *(const float4*)(dctx + lane * 4), d1 = *(const float4*)(dctx + 256 + lane * 4);
#pragma unroll
                for (int r = 0; r < JS / NWV; ++r) {
                    float acc = m0[r].x * d0.x;
                    acc = fmaf(m0[r].y, d0.y, acc); acc = fmaf(m0[r].z, d0.z, acc); acc = fmaf(m0[r].w, d0.w, acc);
                    acc = fmaf(m1[r].x, d1.x, acc); acc = fmaf(m1[r].y, d1.y, acc);
                    acc = fmaf(m1[r].z, d1.z, acc); acc = fmaf(m1[r].w, d1.w, acc);
                    acc = row16_sum(acc);
                    if (c16 == 0) red[(1 + r) * 4 * NWV + 4 * wave + g] = acc;
                }
            }
        }
        __syncthreads();
        if (tid < JS) {
            float dsum = 0.f;
#pragma unroll
            for (int u = 0; u < 32; ++u) dsum += rq[u];
            const int wv = tid % NWV, r = tid / NWV;              // position tid = wv + NWV r
            const float* rr = red + (1 + r) * 4 * NWV + 4 * wv;
            const float dalv = ((rr[0] + rr[1]) + (rr[2] + rr[3])) + gfull0[j0 + min(tid, nown - 1)] + gfull1[j0 + min(tid, nown - 1)];
            de[tid] = tid < nown ? softmax_de(alf[j0 + tid], dalv, dsum) : 0.f;
        }
        __syncthreads();
        // ---- through v·tanh(.): dpre, partial dq / dv
        if (act) {
            float4 dq = make_float4(0.f, 0.f, 0.f, 0.f), dv = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int i = 0; i < JS / NRG; ++i) {
                const int jl = rg + NRG * i;
                const float dej = de[jl];
                const float4 sv = sreg[i];
                float4 dp;
                dp.x = dej * vd4.x * (1.0f - sv.x * sv.x); dp.y = dej * vd4.y * (1.0f - sv.y * sv.y);
                dp.z = dej * vd4.z * (1.0f - sv.z * sv.z); dp.w = dej * vd4.w * (1.0f - sv.w * sv.w);
                sreg[i] = dp;           // the saved copy (operand of the d W_comb / d memory_layer products) leaves AFTER the hand-off
                dq.x += dp.x; dq.y += dp.y; dq.z += dp.z; dq.w += dp.w;
                dv.x = fmaf(dej, sv.x, dv.x); dv.y = fmaf(dej, sv.y, dv.y); dv.z = fmaf(dej, sv.z, dv.z); dv.w = fmaf(dej, sv.w, dv.w);
                dpT[(4 * d4 + 0) * DPS + jl] = dp.x; dpT[(4 * d4 + 1) * DPS + jl] = dp.y;
                dpT[(4 * d4 + 2) * DPS + jl] = dp.z; dpT[(4 * d4 + 3) * DPS + jl] = dp.w;
            }
            *(float4*)&rq[rg * T2V_A + 4 * d4] = dq;
            *(float4*)&rv[rg * T2V_A + 4 * d4] = dv;
        }
        __syncthreads();
        if (tid < T2V_A) {
            const float* p = rq + tid;
            float q = ((p[0] + p[T2V_A]) + (p[2 * T2V_A] + p[3 * T2V_A])) + ((p[4 * T2V_A] + p[5 * T2V_A]) + (p[6 * T2V_A] + p[7 * T2V_A]));
            const float* p2 = rv + tid;
            float vv = ((p2[0] + p2[T2V_A]) + (p2[2 * T2V_A] + p2[3 * T2V_A])) + ((p2[4 * T2V_A] + p2[5 * T2V_A]) + (p2[6 * T2V_A] + p2[7 * T2V_A]));
            if (NRG > 8) {
                p += 8 * T2V_A; p2 += 8 * T2V_A;
                q += ((p[0] + p[T2V_A]) + (p[2 * T2V_A] + p[3 * T2V_A])) + ((p[4 * T2V_A] + p[5 * T2V_A]) + (p[6 * T2V_A] + p[7 * T2V_A]));
                vv += ((p2[0] + p2[T2V_A]) + (p2[2 * T2V_A] + p2[3 * T2V_A])) + ((p2[4 * T2V_A] + p2[5 * T2V_A]) + (p2[6 * T2V_A] + p2[7 * T2V_A]));
            }
            t2v_st(rQ, (unsigned)(((t * B + b) * S + s) * T2V_A + tid) * 4u, q);       // partial row (the d W_q GEMM reads them later)
            dvacc += vv;
            if (s == 0) {
                // Round 4: slice 0 of an item sums the S partial rows in slice order and publishes ONE row per item.  The ≥ 79
                // attention_rnn workgroups of the fp32 kernel used to pull all B*S partial rows each (18 KB per workgroup and step
                // through the ≈ 11 B/cycle a CU gets from beyond its L2: 2.7 us from "published" to "gathered"); now they pull B rows
                // (all partial rows are requested in ONE round: a round trip per slice would cost 0.45 us each)
                constexpr int SMAX = T2V_AB_SMAX;
                const unsigned off0 = (unsigned)(((t * B + b) * S) * T2V_A + tid) * 4u;
                unsigned x[SMAX];
                int spins = 0;
                for (;;) {
                    bool ok = true;
#pragma unroll
                    for (int s2 = 1; s2 < SMAX; ++s2) x[s2] = t2v_ld_b32(rQ, off0 + (unsigned)(min(s2, S - 1) * T2V_A) * 4u);
#pragma unroll
                    for (int s2 = 1; s2 < SMAX; ++s2) ok = ok && (s2 >= S || t2v_ok(x[s2]));
                    if (__all(ok)) break;
                    __builtin_amdgcn_s_sleep(1);
                    if (t2v_give_up(spins, HK::SPIN, a.err, flag)) break;
                }
                float tot = q;
#pragma unroll
                for (int s2 = 1; s2 < SMAX; ++s2) tot += s2 < S ? __uint_as_float(x[s2]) : 0.f;
                t2v_st(rQT, (unsigned)((t * hk.dqt_items() + b) * T2V_A + tid) * 4u, tot);     // the attention_rnn cells wait for this
            }
        }
        hk.stamp(t, T2V_AB_DQ);
        if (act) {      // dpre rows: 8 KB of stores that must not sit in this CU's memory pipe in front of the dq words above
            float* sp = a.S + (((size_t)t * B + b) * Tp + j0) * T2V_A + 4 * d4;
#pragma unroll
            for (int i = 0; i < JS / NRG; ++i) {
                const int jl = rg + NRG * i;
                if (jl < nown) *(float4*)(sp + (size_t)jl * T2V_A) = sreg[i];
            }
        }
        // ---- through the fused location filter on MFMA: T[(c,k)][jl] = sum_d W_comb[d][(c,k)] dpre[jl][d], K = 128
        if (act) {
#pragma unroll
            for (int jt = (wave >> 2); jt < NJT; jt += NWV / 4) {     // (8 waves: waves 4..7 take the odd position tiles)
                f32x4 ac4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) ac4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int st = 0; st < 32; ++st) {
                    const float av = AREG_LDS ? wcs[(16 * (wave & 3) + c16) * 132 + 33 * g + st] : areg[AREG_LDS ? 0 : st];
                    ac4[st & 3] = mfma16x4(av, dpT[(4 * st + g) * DPS + 16 * jt + c16], ac4[st & 3]);
                }
                const f32x4 acc = (ac4[0] + ac4[1]) + (ac4[2] + ac4[3]);
#pragma unroll
                for (int r = 0; r < 4; ++r) Tl[(16 * (wave & 3) + 4 * g + r) * (JS + 1) + 16 * jt + c16] = acc[r];
            }
        }
        __syncthreads();
        // ---- gradient wrt the alignment window of this slice -> the slices of step t-1 (their window partials)
        if (tid < 2 * GPW && t > 0) {
            const int c = tid / GPW, jj = tid % GPW;
            if (jj < PW) {
                float tt[T2V_KS];
#pragma unroll
                for (int k = 0; k < T2V_KS; ++k) {
                    const int jl = jj - k;
                    const float tv = Tl[(32 * c + k) * (JS + 1) + min(max(jl, 0), JS - 1)];
                    tt[k] = (jl >= 0 && jl < JS) ? tv : 0.f;
                }
                float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
#pragma unroll
                for (int k = 0; k + 3 < T2V_KS; k += 4) { acc0 += tt[k]; acc1 += tt[k + 1]; acc2 += tt[k + 2]; acc3 += tt[k + 3]; }
                acc0 += tt[28]; acc1 += tt[29]; acc2 += tt[30];
                t2v_st(rP, (unsigned)(((t * B + b) * S + s) * (2 * GPW) + c * GPW + jj) * 4u, (acc0 + acc1) + (acc2 + acc3));
            }
        }
        __syncthreads();
        hk.stamp(t, T2V_AB_END);
    }
    if (tid < T2V_A) a.DV[((size_t)b * S + s) * T2V_A + tid] = dvacc;
    hk.pass_end();
}
