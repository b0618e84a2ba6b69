// The attention role (T role) of the persistent forward kernels, k_dec_train_persist<NB, LONG> (decoder_train_persist.hip) and
// k_dec_train_persist16<LONG> (decoder_train_persist16.hip): location-sensitive attention of item ab = wg / 8, attention dims
// [16 as, 16 as + 16) and context columns [64 as, 64 as + 64), as = wg % 8, for all steps of one pass.  The arithmetic is fp32 in
// both kernels, so it exists once, here.  This is not a function but program text, #included INSIDE both kernel bodies where the
// role starts: the same tokens after preprocessing compile to the program each kernel had with its own copy (a function that
// takes the argument struct moved the L roles' register allocation in kernels that sit on the 256-VGPR ceiling; DESIGN.md 6).
// From the kernel's scope it uses a (wq, wcomb, v, memory, pm, lengths, S, AL, ACUM, XS, err), lds, LONG, wg, tid, wave, lane,
// B, Tp, T, Tcap, rG and rE.  What differs between the two the kernel #defines in front of the #include and #undefs behind it:
//   AF_TAIL            floats between rss and flag at the end of the carve (t2v_attn_fwd_lds_floats's `tail`, t2v_kernels.h)
//   AF_SETUP           declarations that the kernel's two blocks below share (may be empty)
//   AF_GROW            bytes per row of the state exchange (row t + 1 carries step t)
//   AF_H_INGEST        a block: wait for h_att(t) of item ab (nap h_nap first, adapt it from the rounds) -> hx[1024]
//   AF_CTX_PUBLISH     statements of threads tid < 64: context column 64 as + tid (acc) -> the state exchange
//   AF_STAMP_STEP / _H / _Q / _E / _EX / _ALPHA / _END     profile stamps: step begins, h_att(t) arrived, query done, energies
//                      sent, partials arrived, weights done, context published
// The order of memory operations is part of the design: the nap comes before the first poll, XS is stored after the publish.
    const int ab = wg >> 3, as = wg & 7;
    constexpr int NTI = LONG ? T2V_AF_NTI_LONG : 2;      // position tiles per wave: tile jt = wave + 8 i
    constexpr int NPP = LONG ? 2 : 1;                    // positions per thread in the softmax: tid + 512 u
    const int TW = Tcap + 32;
    // ---- LDS carve (its size for the launchers: t2v_attn_fwd_lds_floats, t2v_kernels.h)
    float* wq_s = lds;                                  // [16][1028]   (LONG: in registers)
    float* mem_s = wq_s + (LONG ? 0 : 16 * 1028);        // [Tcap][64]
    float* pm_s = mem_s + Tcap * 64;                     // [Tcap][16]   (LONG: in registers)
    float* win = pm_s + (LONG ? 0 : Tcap * 16);          // [2][TW]: alignment window, index x <-> position x - 15
    float* eall = win + 2 * TW;                          // [Tcap] (LONG: + T2V_CTX_PAD, zero from Tp on: t2v_ctx_partial)
    float* hx = eall + Tcap + (LONG ? T2V_CTX_PAD : 0);  // [1024] h_att(t) of this item
    float* qv = hx + T2V_H;                              // [16]
    float* qred = qv + 16;                               // [32][16]
    float* cred = qred + 32 * 16;                        // [8][64]
    float* rsm = cred + 8 * 64;                          // [32]
    float* rss = rsm + 32;                               // [32]
    int* flag = (int*)(rss + 32 + AF_TAIL);              // (AF_TAIL floats in between are the kernel's own)
    const int g = lane >> 4, c16 = lane & 15;
    float4 wqr[LONG ? 8 : 1], pmr[LONG ? NTI : 1];
    if constexpr (LONG) {
        // the operands of a thread's own part of the query product (dim tid >> 5, k = 4 (tid & 31) + 128 i) and of its tiles'
        // energies (position 16 jt + c16, dims 16 as + 4 g ..) never change over the pass
        const float* wrow = a.wq + (size_t)(16 * as + (tid >> 5)) * 1024 + 4 * (tid & 31);
#pragma unroll
        for (int i = 0; i < 8; ++i) wqr[i] = *(const float4*)(wrow + 128 * i);
#pragma unroll
        for (int i = 0; i < NTI; ++i) {
            const int jp = 16 * (wave + 8 * i) + c16;
            pmr[i] = *(const float4*)(a.pm + ((size_t)ab * Tp + min(jp, Tp - 1)) * T2V_A + 16 * as + 4 * g);
        }
    } else {
        for (int i = tid; i < 16 * 1024; i += T2V_AF_THREADS) wq_s[(i >> 10) * 1028 + (i & 1023)] = a.wq[(size_t)(16 * as) * 1024 + i];
    }
    for (int i = tid; i < Tp * 64; i += T2V_AF_THREADS) mem_s[i] = a.memory[((size_t)ab * Tp + (i >> 6)) * T2V_E + 64 * as + (i & 63)];
    if constexpr (!LONG)
        for (int i = tid; i < Tp * 16; i += T2V_AF_THREADS) pm_s[i] = a.pm[((size_t)ab * Tp + (i >> 4)) * T2V_A + 16 * as + (i & 15)];
    for (int i = tid; i < 2 * TW; i += T2V_AF_THREADS) win[i] = 0.f;
    if constexpr (LONG)
        for (int i = Tp + tid; i < Tcap + T2V_CTX_PAD; i += T2V_AF_THREADS) eall[i] = 0.f;
    if (tid == 0) flag[0] = 1;
    float areg[16];
    {
        const float4* wp = (const float4*)(a.wcomb + (16 * as + c16) * 64 + 16 * g);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 w4 = wp[u];
            areg[4 * u] = w4.x; areg[4 * u + 1] = w4.y; areg[4 * u + 2] = w4.z; areg[4 * u + 3] = w4.w;
        }
    }
    const float4 vr = *(const float4*)(a.v + 16 * as + 4 * g);
    const int len = a.lengths ? a.lengths[ab] : Tp;
    AF_SETUP
    __syncthreads();
    int h_nap = 0;

    for (int t = 0; t < T; ++t) {
        const unsigned grow = (unsigned)(t + 1) * AF_GROW;
        AF_STAMP_STEP;
        // ---- location features of this step's tiles (fused filter, K = 64): they depend on alpha(t-1) only, so they
        // are evaluated BEFORE h_att(t) arrives (wave -> tiles wave, wave + 8)
        f32x4 lacc[NTI];
#pragma unroll
        for (int i = 0; i < NTI; ++i) {
            const int jt = wave + 8 * i;
            lacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (16 * jt < Tp) {
                float bop[16];
#pragma unroll
                for (int st = 0; st < 16; ++st) {
                    const int kk = 4 * st + g;
                    bop[st] = win[(kk >> 5) * TW + 16 * jt + c16 + (kk & 31)];
                }
                f32x4 l0 = {0.f, 0.f, 0.f, 0.f}, l1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int st = 0; st < 16; st += 2) {
                    l0 = mfma16x4(areg[st], bop[st], l0);
                    l1 = mfma16x4(areg[st + 1], bop[st + 1], l1);
                }
                lacc[i] = l0 + l1;
            }
        }
        // ---- h_att(t) of this item -> hx: nap (h_nap, adapted), then poll the payload
        AF_H_INGEST
        __syncthreads();
        if (flag[0] != 1) return;
        AF_STAMP_H;
        // ---- query slice: thread = (dim d = tid >> 5, k part kq = tid & 31): k = 4 kq + 128 i, 16-byte LDS operands;
        // 32-lane sum = 16-lane DPP row sum + one cross-row exchange
        {
            const int d = tid >> 5, kq = tid & 31;
            const float* wrow = wq_s + d * 1028 + 4 * kq;
            const float* hp = hx + 4 * kq;
            float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 w4 = LONG ? wqr[LONG ? i : 0] : *(const float4*)(wrow + 128 * i);
                const float4 h4 = *(const float4*)(hp + 128 * i);
                acc0 = fmaf(w4.x, h4.x, acc0); acc1 = fmaf(w4.y, h4.y, acc1);
                acc0 = fmaf(w4.z, h4.z, acc0); acc1 = fmaf(w4.w, h4.w, acc1);
            }
            float q = row16_sum(acc0 + acc1);
            q += __shfl_xor(q, 16, 64);
            if (kq == 0) qv[d] = q;
        }
        __syncthreads();
        const float4 q4 = *(const float4*)(qv + 4 * g);
        AF_STAMP_Q;
        // ---- partial energies of this slice
        const unsigned exw = (unsigned)(((t * B + ab) * 8 + as) * Tcap) * 4u;
#pragma unroll
        for (int i = 0; i < NTI; ++i) {
            const int jt = wave + 8 * i;
            if (16 * jt < Tp) {
                const f32x4 acc = lacc[i];
                const int jp = 16 * jt + c16;
                const float4 pm4 = LONG ? pmr[LONG ? i : 0] : *(const float4*)(pm_s + min(jp, Tp - 1) * 16 + 4 * g);
                float4 sv;
                sv.x = tanhf_(q4.x + acc[0] + pm4.x); sv.y = tanhf_(q4.y + acc[1] + pm4.y);
                sv.z = tanhf_(q4.z + acc[2] + pm4.z); sv.w = tanhf_(q4.w + acc[3] + pm4.w);
                float esum = vr.x * sv.x + vr.y * sv.y + vr.z * sv.z + vr.w * sv.w;
                esum += __shfl_xor(esum, 16, 64);
                esum += __shfl_xor(esum, 32, 64);
                if (g == 0 && jp < Tp) t2v_st(rE, exw + 4u * (unsigned)jp, esum);
                if (a.S && jp < Tp) *(float4*)(a.S + (((size_t)t * B + ab) * Tp + jp) * T2V_A + 16 * as + 4 * g) = sv;
            }
        }
        AF_STAMP_E;
        // (two copies of the softmax: the one-position form is kept word for word so that the short kernels keep their instruction
        // stream — round 6 checked the ISA of <.., false> against the previous build, identical)
        if constexpr (!LONG) {
            // ---- the 8 partials of every position (fixed order), masked softmax
            float ev0 = -INFINITY;
            if (tid < Tp) {
                const unsigned e0 = (unsigned)((t * B + ab) * 8 * Tcap + tid) * 4u;
                unsigned p[8];
                unsigned spins = 0;
                for (;;) {
                    bool ok = true;
    #pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        p[i] = t2v_ld_b32(rE, e0 + (unsigned)(i * Tcap) * 4u);
                        ok = ok && t2v_ok(p[i]);
                    }
                    if (ok) break;
                    __builtin_amdgcn_s_sleep(1);
                    if (t2v_give_up(spins, T2V_AF_SPIN, a.err, flag)) break;
                }
                const float ev = ((__uint_as_float(p[0]) + __uint_as_float(p[1])) + (__uint_as_float(p[2]) + __uint_as_float(p[3]))) +
                                 ((__uint_as_float(p[4]) + __uint_as_float(p[5])) + (__uint_as_float(p[6]) + __uint_as_float(p[7])));
                ev0 = tid < len ? ev : -INFINITY;
            }
            AF_STAMP_EX;
            {
                float mloc = ev0;
                mloc = T2V_DPP_MAX(mloc, 0xB1); mloc = T2V_DPP_MAX(mloc, 0x4E);
                mloc = T2V_DPP_MAX(mloc, 0x141); mloc = T2V_DPP_MAX(mloc, 0x140);
                mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
                mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
                if (lane == 0) rsm[wave] = mloc;
            }
            __syncthreads();
            if (flag[0] != 1) return;
            float m;
            {
                const float4 a0 = *(const float4*)rsm, a1 = *(const float4*)(rsm + 4);
                m = fmaxf(fmaxf(fmaxf(a0.x, a0.y), fmaxf(a0.z, a0.w)), fmaxf(fmaxf(a1.x, a1.y), fmaxf(a1.z, a1.w)));
            }
            const float e0v = tid < Tp ? expf(ev0 - m) : 0.f;
            {
                float sloc = row16_sum(e0v);
                sloc += __shfl_xor(sloc, 16, 64);
                sloc += __shfl_xor(sloc, 32, 64);
                if (lane == 0) rss[wave] = sloc;
            }
            __syncthreads();
            float ssum;
            {
                const float4 a0 = *(const float4*)rss, a1 = *(const float4*)(rss + 4);
                ssum = ((a0.x + a0.y) + (a0.z + a0.w)) + ((a1.x + a1.y) + (a1.z + a1.w));
            }
            const float al = e0v * (1.0f / ssum);
            if (tid < Tp) {
                eall[tid] = al;
                win[15 + tid] = al;                                        // previous weights of the next step
                const float cum = win[TW + 15 + tid] + al;                 // cumulative weights
                win[TW + 15 + tid] = cum;
                if (as == 0) {
                    a.AL[((size_t)(t + 1) * B + ab) * Tp + tid] = al;
                    a.ACUM[((size_t)(t + 1) * B + ab) * Tp + tid] = cum;
                }
            }
        } else {
            // ---- the 8 partials of every position (fixed order), masked softmax; thread -> positions tid + 512 u
            float ev0[NPP];
    #pragma unroll
            for (int u = 0; u < NPP; ++u) ev0[u] = -INFINITY;
            if (tid < Tp) {
                const unsigned e0 = (unsigned)((t * B + ab) * 8 * Tcap + tid) * 4u;
                unsigned p[NPP][8];
                unsigned spins = 0;
                for (;;) {
                    bool ok = true;
    #pragma unroll
                    for (int u = 0; u < NPP; ++u) {
                        // (a second position past the end re-reads the first one's words: no branch around the loads)
                        const unsigned eu = e0 + ((u > 0 && tid + T2V_AF_THREADS * u < Tp) ? (unsigned)(T2V_AF_THREADS * u) * 4u : 0u);
    #pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            p[u][i] = t2v_ld_b32(rE, eu + (unsigned)(i * Tcap) * 4u);
                            ok = ok && t2v_ok(p[u][i]);
                        }
                    }
                    if (ok) break;
                    __builtin_amdgcn_s_sleep(1);
                    if (t2v_give_up(spins, T2V_AF_SPIN, a.err, flag)) break;
                }
    #pragma unroll
                for (int u = 0; u < NPP; ++u) {
                    const float ev = ((__uint_as_float(p[u][0]) + __uint_as_float(p[u][1])) + (__uint_as_float(p[u][2]) + __uint_as_float(p[u][3]))) +
                                     ((__uint_as_float(p[u][4]) + __uint_as_float(p[u][5])) + (__uint_as_float(p[u][6]) + __uint_as_float(p[u][7])));
                    ev0[u] = tid + T2V_AF_THREADS * u < len ? ev : -INFINITY;
                }
            }
            AF_STAMP_EX;
            {
                float mloc = ev0[0];
    #pragma unroll
                for (int u = 1; u < NPP; ++u) mloc = fmaxf(mloc, ev0[u]);
                mloc = T2V_DPP_MAX(mloc, 0xB1); mloc = T2V_DPP_MAX(mloc, 0x4E);
                mloc = T2V_DPP_MAX(mloc, 0x141); mloc = T2V_DPP_MAX(mloc, 0x140);
                mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
                mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
                if (lane == 0) rsm[wave] = mloc;
            }
            __syncthreads();
            if (flag[0] != 1) return;
            float m;
            {
                const float4 a0 = *(const float4*)rsm, a1 = *(const float4*)(rsm + 4);
                m = fmaxf(fmaxf(fmaxf(a0.x, a0.y), fmaxf(a0.z, a0.w)), fmaxf(fmaxf(a1.x, a1.y), fmaxf(a1.z, a1.w)));
            }
            float e0v[NPP];
    #pragma unroll
            for (int u = 0; u < NPP; ++u) e0v[u] = tid + T2V_AF_THREADS * u < Tp ? expf(ev0[u] - m) : 0.f;
            {
                float sloc = e0v[0];
    #pragma unroll
                for (int u = 1; u < NPP; ++u) sloc += e0v[u];
                sloc = row16_sum(sloc);
                sloc += __shfl_xor(sloc, 16, 64);
                sloc += __shfl_xor(sloc, 32, 64);
                if (lane == 0) rss[wave] = sloc;
            }
            __syncthreads();
            float ssum;
            {
                const float4 a0 = *(const float4*)rss, a1 = *(const float4*)(rss + 4);
                ssum = ((a0.x + a0.y) + (a0.z + a0.w)) + ((a1.x + a1.y) + (a1.z + a1.w));
            }
            const float rinv = 1.0f / ssum;
    #pragma unroll
            for (int u = 0; u < NPP; ++u) {
                const int pos = tid + T2V_AF_THREADS * u;
                const float al = e0v[u] * rinv;
                if (pos < Tp) {
                    eall[pos] = al;
                    win[15 + pos] = al;                                        // previous weights of the next step
                    const float cum = win[TW + 15 + pos] + al;                 // cumulative weights
                    win[TW + 15 + pos] = cum;
                    if (as == 0) {
                        a.AL[((size_t)(t + 1) * B + ab) * Tp + pos] = al;
                        a.ACUM[((size_t)(t + 1) * B + ab) * Tp + pos] = cum;
                    }
                }
            }
        }
        __syncthreads();
        AF_STAMP_ALPHA;
        // ---- context columns [64 as, 64 as + 64): thread = (column c = tid & 63, part = tid >> 6)
        {
            const int c = tid & 63, part = tid >> 6;
            if constexpr (LONG) {
                // (up to 70 positions per thread: eight per round, reads first — 8 000 -> 6 500 cycles at 555 symbols; at <= 224 symbols
                // the plain loop is as fast and the short kernels keep their instruction stream)
                cred[part * 64 + c] = t2v_ctx_partial<8>(eall, mem_s, part, c, Tp);
            } else {
                float acc = 0.f;
                for (int jj = part; jj < Tp; jj += 8) acc = fmaf(eall[jj], mem_s[jj * 64 + c], acc);
                cred[part * 64 + c] = acc;
            }
        }
        __syncthreads();
        if (tid < 64) {
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += cred[u * 64 + tid];
            AF_CTX_PUBLISH
            a.XS[((size_t)(t + 1) * B + ab) * T2V_XW + T2V_H + 64 * as + tid] = acc;       // (after the publish)
        }
        AF_STAMP_END;
    }
