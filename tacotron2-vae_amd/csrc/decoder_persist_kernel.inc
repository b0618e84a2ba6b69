// The frame loop of decoder_persist.hip, included once per kernel: PD_ITEMS 0 defines k_decode_persist, PD_ITEMS 1 the per-item variant
// k_decode_persist_items (batched synthesis: item b's first gate-fire frame -> it.stop_item[b]; item b's Prenet masks from
// it.item_seeds[b] with the element index of item 0, i.e. the masks of a B = 1 decode with that seed).  Preprocessor
// instances rather than a template: the PD_ITEMS 0 text is the kernel as it was, so its instructions stay the same.
// PD_WINDOW 1 (with either PD_ITEMS) adds the attention window of include/t2vae.h (t2v_dec_window): k_decode_persist_win and
// k_decode_persist_items_win.  With PD_WINDOW 0 the text is what it was before the window existed.
// PD_WINDOW 2 is the planned decode (include/t2vae.h t2v_decoder_infer_persistent_plan): k_decode_persist_plan and
// k_decode_persist_items_plan mask as PD_WINDOW 1 does, around a centre read from the plan instead of found by a scan.  With
// PD_WINDOW 0 or 1 the text is what it was before the plan existed.
#if PD_ITEMS && PD_WINDOW == 2
__global__ __launch_bounds__(PD_THREADS) void k_decode_persist_items_plan(PersistArgs a, PersistItems it, PersistPlan wn) {
#elif PD_WINDOW == 2
__global__ __launch_bounds__(PD_THREADS) void k_decode_persist_plan(PersistArgs a, PersistPlan wn) {
#elif PD_ITEMS && PD_WINDOW
__global__ __launch_bounds__(PD_THREADS) void k_decode_persist_items_win(PersistArgs a, PersistItems it, PersistWindow wn) {
#elif PD_WINDOW
__global__ __launch_bounds__(PD_THREADS) void k_decode_persist_win(PersistArgs a, PersistWindow wn) {
#elif PD_ITEMS
__global__ __launch_bounds__(PD_THREADS) void k_decode_persist_items(PersistArgs a, PersistItems it) {
#else
__global__ __launch_bounds__(PD_THREADS) void k_decode_persist(PersistArgs a) {
#endif
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wg = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int B = a.B, Tp = a.T_in;
    // ---- LDS carve (floats; sizes follow the runtime B and T_in: pd_lds_floats())
    const int Tcap = (Tp + 15) & ~15, TW = Tcap + 32;
    float* X = lds;                                      // [B][2816]
    float* red = X + B * PD_XW;                          // [8][16][MAXB]
    float* gst = red + 8 * 16 * PD_MAXB;                 // [MAXB][16] gate pre-activations
    float* cst = gst + PD_MAXB * 16;                     // [2][MAXB][4] cell states (attention_rnn, decoder_rnn)
    int* flag = (int*)(cst + 2 * PD_MAXB * 4);           // [4]
    float* role = (float*)(flag + 4);                    // role area
    // attention role
    float* wq_s = role;                                  // [16][1028]
    float* mem_s = wq_s + 16 * 1028;                     // [Tcap][64]
    float* pm_s = mem_s + Tcap * 64;                     // [Tcap][16]
    float* win = pm_s + Tcap * 16;                       // [2][TW]: alignment window, index x <-> position x - 15
    float* eall = win + 2 * TW;                          // [Tcap + T2V_CTX_PAD]: attention weights, zero from Tp on (t2v_ctx_partial)
    float* qv = eall + Tcap + T2V_CTX_PAD;               // [16]
    float* cred = qv + 16;                               // [8][64]   (round 6: a 2 KB reduction buffer nobody used any more sat here — three
                                                         //            utterances of 160 symbols now fit the 160 KB)
    float* rsm = cred + 8 * 64;                          // [32] row maxima
    float* rss = rsm + 32;                               // [32] row sums
    // projection / Prenet-1 roles (their own workgroups: alias the same area)
    float* prow_s = role;                                // [8][1536]
    float* w1_s = role;                                  // [8][256]

    const bool is_attn = wg < 8 * B;
    const int ab = wg >> 3, as = wg & 7;                 // attention item / slice
    const int gw = wg * 8 + wave;                        // global wave index
    const int prow = (wg >= PD_WG_PROJ && wg < PD_WG_PROJ + 43) ? (wg - PD_WG_PROJ) * 8 + wave : -1;      // projection row of this wave
    const bool is_proj = prow >= 0 && prow < PD_NROW;
    const bool wg_proj = prow >= 0;                       // whole workgroup (the last one has idle waves)
    const int p1row = (wg >= PD_WG_PRE1 && wg < PD_WG_PRE1 + 32) ? (wg - PD_WG_PRE1) * 8 + wave : -1;    // Prenet-1 row of this wave
    (void)gw;

    // ---- one-time loads: LSTM weights of this workgroup's 16 gate rows per cell into registers
    const int kq = lane & 3, r16 = lane >> 2;
    const int grow = (r16 & 3) * T2V_H + 4 * wg + (r16 >> 2);           // gate-major row of (unit 4wg + r16>>2, gate r16&3)
    float wa[PD_KATT / 32], wd[PD_KDEC / 32];
#pragma unroll
    for (int j = 0; j < PD_KATT / 32; ++j) {
        const int k = pd_ka(wave, j, kq);                                // [h_att | ctx | pre1]
        wa[j] = k < T2V_H ? a.w_hh_att[(size_t)grow * T2V_H + k]
                          : (k < T2V_KATT ? a.w_ih_att[(size_t)grow * 768 + T2V_PRE + (k - T2V_H)] : a.w_ih_att[(size_t)grow * 768 + (k - T2V_KATT)]);
    }
#pragma unroll
    for (int j = 0; j < PD_KDEC / 32; ++j) {
        const int k = pd_kd(wave, j, kq);                                // [h_att | ctx | h_dec]
        wd[j] = k < T2V_KATT ? a.w_ih_dec[(size_t)grow * T2V_KATT + k] : a.w_hh_dec[(size_t)grow * T2V_H + (k - T2V_KATT)];
    }
    float bias_a = 0.f, bias_d = 0.f;                                   // wave 0: thread (row r = tid & 15, item) holds the bias of row r
    if (tid < 64) {
        const int row = (tid & 3) * T2V_H + 4 * wg + ((tid & 15) >> 2);
        bias_a = a.bias_att[row];
        bias_d = a.bias_dec[row];
    }
    for (int i = tid; i < B * PD_XW; i += PD_THREADS) X[i] = 0.f;
    if (tid < 2 * PD_MAXB * 4) cst[tid] = 0.f;
    if (tid == 0) flag[0] = 1;
#if PD_WINDOW == 2
    // the plan row of this attention workgroup's item, the last frame the plan names and the item's length: uniform over the
    // workgroup (wave-uniform values, no vector register per lane).  The window centre of frame 0 is the plan's first symbol.
    const int32_t* plan_row = wn.plan + (size_t)(wg < 8 * B ? wg >> 3 : 0) * wn.plan_stride;
    const int plan_last = min(max(wn.n_plan[wg < 8 * B ? wg >> 3 : 0], 1), wn.plan_stride) - 1;
    const int plan_len = a.lengths ? a.lengths[wg < 8 * B ? wg >> 3 : 0] : Tp;
    if (tid == 0) flag[1] = min(max(plan_row[0], 0), plan_len - 1);
#elif PD_WINDOW
    if (tid == 0) flag[1] = 0;          // the window centre of frame 0
#endif
    // role operands
    // (round 4: the fused location filter's MFMA operand lives in LDS — 16 registers per lane that only the attention
    // workgroups used, next to 136 weight registers and the carried partial gate sums, made the kernel spill)
    float* areg_s = rss + 32;                              // [16 steps][64 lanes]
    float4 vr = make_float4(0.f, 0.f, 0.f, 0.f);
    if (is_attn) {
        for (int i = tid; i < 16 * 1024; i += PD_THREADS) wq_s[(i >> 10) * 1028 + (i & 1023)] = a.wq[(size_t)(16 * as) * 1024 + i];
        for (int i = tid; i < Tp * 64; i += PD_THREADS) mem_s[i] = a.memory[((size_t)ab * Tp + (i >> 6)) * T2V_E + 64 * as + (i & 63)];
        for (int i = tid; i < Tp * 16; i += PD_THREADS) pm_s[i] = a.pm[((size_t)ab * Tp + (i >> 4)) * T2V_A + 16 * as + (i & 15)];
        for (int i = tid; i < 2 * TW; i += PD_THREADS) win[i] = 0.f;
        for (int i = Tp + tid; i < Tcap + T2V_CTX_PAD; i += PD_THREADS) eall[i] = 0.f;
        const int g = lane >> 4, c16 = lane & 15;
        const float4* wp = (const float4*)(a.wcomb + (16 * as + c16) * 64 + 16 * g);
        if (wave == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 w4 = wp[u];
                areg_s[(4 * u) * 64 + lane] = w4.x; areg_s[(4 * u + 1) * 64 + lane] = w4.y;
                areg_s[(4 * u + 2) * 64 + lane] = w4.z; areg_s[(4 * u + 3) * 64 + lane] = w4.w;
            }
        }
        vr = *(const float4*)(a.v + 16 * as + 4 * g);
    } else if (prow >= 0) {
        if (is_proj)
            for (int i = lane; i < 1536; i += 64) prow_s[wave * 1536 + i] = a.proj_w[(size_t)prow * 1536 + i];
    } else if (p1row >= 0) {
        for (int i = lane; i < 256; i += 64) w1_s[wave * 256 + i] = a.w1[(size_t)p1row * 256 + i];
    }
    const float pbias = is_proj ? a.proj_b[prow] : 0.f;
#if PD_ITEMS
    // per-item dropout seeds: loaded once here, so the mask hashes below stay off the frames' dependent chains
    uint64_t iseed[PD_MAXB];
#pragma unroll
    for (int b = 0; b < PD_MAXB; ++b) iseed[b] = b < B ? it.item_seeds[b] : a.seed;
#endif
    // Prenet of the go frame (frame 0 input)
    for (int i = tid; i < B * T2V_PRE; i += PD_THREADS) X[(i >> 8) * PD_XW + PD_X_P1 + (i & 255)] = a.pre_first[i];
    __syncthreads();

    const __amdgpu_buffer_rsrc_t rx = t2v_rsrc(a.xg);
    int nap_e = 0, nap_h = 0, nap_x = 0, nap_c = 0, nap_p = 0, nap_q = 0;      // adaptive naps in front of the polls (64-cycle units)
    // partial gate sums carried from where their inputs appear to where the gates are needed (see pd_gemv_part); frame 0
    // starts from h_att = ctx = h_dec = 0, i.e. from zero partial sums
    float ea[PD_MAXB], ed[PD_MAXB];
#pragma unroll
    for (int b = 0; b < PD_MAXB; ++b) ea[b] = ed[b] = 0.f;
    for (int t = 0; t < a.t_end; ++t) {
        const unsigned xcur = (unsigned)t * pd_row(B), xprev = xcur - pd_row(B);      // float offsets of this / the previous frame's row
        // ---- frame entry (t > 0): stop decision of the previous frame, Prenet output of the new frame's input
        if (t > 0) {
            // Prenet output of the new frame's input + stop decision of the previous frame.  Every workgroup of the chip wants
            // the same 1 KB (+ one word) at the same moment: with all 8 waves of all 256 workgroups polling it, the eight cache
            // lines behind it were a hot spot that took ~4 us to hand the values over (time line of tools/dbg_persist.py).  So
            // ONE wave per item polls (one 16-byte load per lane) and thread 0 alone watches the stop word.
            if (tid < 64 * B) {
                u32x4 pv = {0u, 0u, 0u, 0u};
                unsigned spins = 0, sx = 0u;
                for (int i = 0; i < nap_e; i += 4) __builtin_amdgcn_s_sleep(4);
                for (;;) {
                    pv = t2v_ld_b128(rx, (xprev + pd_pre1(B) + 4u * (unsigned)tid) * 4u);          // [b][256] is contiguous
                    if (tid == 0) sx = t2v_ld_b32(rx, (xprev + pd_stop(B)) * 4u);
                    if (tid == 0 && sx == 2u) flag[0] = 2;              // the gate fired on the previous frame: nothing runs after it
                    if (__all(pv[0] != T2V_SENT && pv[1] != T2V_SENT && pv[2] != T2V_SENT && pv[3] != T2V_SENT && sx != T2V_SENT)) break;
                    if (__any(tid == 0 && sx == 2u)) break;
                    __builtin_amdgcn_s_sleep(1);
                    if (t2v_give_up(spins, PD_SPIN, a.err, flag)) break;
                }
                nap_e = pd_adapt(nap_e, (int)spins);
                const int i = 4 * tid;
                *(float4*)(X + (size_t)(i >> 8) * PD_XW + PD_X_P1 + (i & 255)) =
                    make_float4(__uint_as_float(pv[0]), __uint_as_float(pv[1]), __uint_as_float(pv[2]), __uint_as_float(pv[3]));
            }
            __syncthreads();
            if (flag[0] != 1) return;                          // stopped on the gate (2) or timed out (0)
        }
        PD_STAMP(0, 0); PD_STAMP(64, 10); PD_STAMP(128, 14);
        PD_RT(0);
        if (a.prof && wg == 0 && tid == 0 && (t == 100 || t == 600)) {       // steady-state frame period: 500 frames between two stamps
            a.prof[t == 100 ? 20 : 22] = __builtin_readcyclecounter();
            a.prof[t == 100 ? 21 : 23] = __builtin_amdgcn_s_memrealtime();
        }
        // ---- 1. attention_rnn(t): gates of this workgroup's 4 units, cell update, publish h_att
        pd_gemv_part<PD_KATT / 32, 48, 56, false>(wa, X, B, ea);      // the Prenet columns; [h_att | ctx] were added during frame t-1
        pd_gemv_finish(ea, B, red);
        __syncthreads();
        if (tid < 16 * B) {                                    // thread = (row r = tid & 15, item b = tid >> 4)
            const int r = tid & 15, b = tid >> 4;
            float s = 0.f;
#pragma unroll
            for (int w8 = 0; w8 < 8; ++w8) s += red[(w8 * 16 + r) * PD_MAXB + b];
            gst[b * 16 + r] = s + bias_a;                      // pre-activation where the unit's thread finds its four gates
        }
        __syncthreads();
        if (tid < 4 * B) {                                     // thread = (unit u = tid & 3, item b = tid >> 2)
            const int u = tid & 3, b = tid >> 2;
            const float* gp = gst + b * 16 + 4 * u;
            const float gi = sigmoidf_(gp[0]), gf = sigmoidf_(gp[1]), gg = tanhf_(gp[2]), go = sigmoidf_(gp[3]);
            const float c = gf * cst[b * 4 + u] + gi * gg;
            cst[b * 4 + u] = c;
            // the four units of an item leave as ONE 16-byte store (round 4: four 4-byte stores from four lanes were four
            // write-through transactions into the same 32-byte sector)
            const float h = go * tanhf_(c);
            const float h1 = T2V_DPP_QUAD_F(h, 1), h2 = T2V_DPP_QUAD_F(h, 2), h3 = T2V_DPP_QUAD_F(h, 3);      // (used by lane u == 0 only)
            // (offset rebuilt from an opaque copy of the thread index: hoisted out of the frame loop it was spilled, and its reload from
            // scratch — a vector-memory load + s_waitcnt vmcnt(0) — sat in front of this store on every frame's chain; round 6)
            if (u == 0) t2v_st(rx, (xcur + pd_hatt(B) + (unsigned)((pd_opaque(threadIdx.x) >> 2) * 1024 + 4 * wg)) * 4u, u32x4{__float_as_uint(h), __float_as_uint(h1), __float_as_uint(h2), __float_as_uint(h3)});
        }
        PD_STAMP(0, 1);
        PD_RT(1);
        // ---- 2. h_att(t) for everyone (attention slices need it now, the others for decoder_rnn)
        // location features of this frame's tiles (fused filter, K = 64): they depend on the PREVIOUS frame's weights only,
        // so the attention workgroups evaluate them while h_att(t) is still on its way (round 3, from the training kernel)
        f32x4 lacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (is_attn) {
            const int g = lane >> 4, c16 = lane & 15;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int jt = wave + 8 * i;
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
                        l0 = mfma16x4(areg_s[st * 64 + lane], bop[st], l0);
                        l1 = mfma16x4(areg_s[(st + 1) * 64 + lane], bop[st + 1], l1);
                    }
                    lacc[i] = l0 + l1;
                }
            }
        }
        {
            // (only the attention workgroups need h_att(t) NOW; everybody else uses it for decoder_rnn microseconds later and
            // comes for it late, with a fixed nap — 256 workgroups polling the same 32 lines the moment they land made this the
            // longest hand-off of the frame)
            const int rounds = pd_gather_items(X + PD_X_HA, rx, xcur + pd_hatt(B), 1024u, 1024, B, is_attn ? nap_h : 80, a.err, flag);
            if (is_attn) nap_h = pd_adapt(nap_h, rounds);
        }
        __syncthreads();
        if (flag[0] != 1) return;
        PD_STAMP(0, 2);
        PD_RT(2);
        // decoder_rnn(t), part 2: the h_att(t) columns — now, while the attention workgroups are busy (they do theirs behind
        // their context hand-off, in the shadow of the context gather)
        if (!is_attn) {
            pd_gemv_part<PD_KDEC / 32, 0, 32, true>(wd, X, B, ed);
            // ... and the h_dec(t-1) columns: the other workgroups fetch that row only now, a frame after it was published and
            // long after the projection workgroups (who needed it at once) are done with it
            if (t > 0 && !wg_proj) {
                (void)pd_gather_items(X + PD_X_HD, rx, xprev + pd_hdec(B), 1024u, 1024, B, 0, a.err, flag);
                __syncthreads();
                if (flag[0] != 1) return;
                pd_gemv_part<PD_KDEC / 32, 32, 64, true>(wd, X, B, ed);
            }
        }
        if (is_attn) {
            const int g = lane >> 4, c16 = lane & 15;
            const int len = a.lengths ? a.lengths[ab] : Tp;
            // query slice: thread = (dim d = tid >> 5, k part kq = tid & 31): k = 4 kq + 128 i, 16-byte LDS operands; 32-lane
            // sum = 16-lane DPP row sum + one cross-row exchange (one barrier instead of two and a 32-way tree)
            {
                const int d = tid >> 5, kq = tid & 31;
                const float* wrow = wq_s + d * 1028 + 4 * kq;
                const float* hx = X + (size_t)ab * PD_XW + PD_X_HA + 4 * kq;
                float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float4 w4 = *(const float4*)(wrow + 128 * i);
                    const float4 h4 = *(const float4*)(hx + 128 * i);
                    acc0 = fmaf(w4.x, h4.x, acc0); acc1 = fmaf(w4.y, h4.y, acc1);
                    acc0 = fmaf(w4.z, h4.z, acc0); acc1 = fmaf(w4.w, h4.w, acc1);
                }
                float q = row16_sum(acc0 + acc1);
                q = rows2_sum(q);
                if (kq == 0) qv[d] = q;
            }
            __syncthreads();
            const float4 q4 = make_float4(qv[4 * g], qv[4 * g + 1], qv[4 * g + 2], qv[4 * g + 3]);
            // partial energies of this slice: wave -> position tiles wave, wave + 8
            const unsigned exw = xcur + pd_ex(B) + (unsigned)((ab * 8 + as) * 256);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int jt = wave + 8 * i;
                if (16 * jt < Tp) {
                    const f32x4 acc = lacc[i];
                    const int j = 16 * jt + c16;
                    const float4 pm4 = *(const float4*)(pm_s + min(j, Tp - 1) * 16 + 4 * g);
                    const float s0 = tanhf_(q4.x + acc[0] + pm4.x), s1 = tanhf_(q4.y + acc[1] + pm4.y);
                    const float s2 = tanhf_(q4.z + acc[2] + pm4.z), s3 = tanhf_(q4.w + acc[3] + pm4.w);
                    float esum = vr.x * s0 + vr.y * s1 + vr.z * s2 + vr.w * s3;
                    esum += __shfl_xor(esum, 16, 64);
                    esum += __shfl_xor(esum, 32, 64);
                    if (g == 0 && j < Tp) pd_put(rx, exw + (unsigned)j, esum);
                }
            }
            PD_STAMP(0, 3);
            PD_RT(3);
            // gather the 8 partials of every position, masked softmax
            float ev0 = -INFINITY;
            if (tid < Tp) {
                const unsigned e0 = xcur + pd_ex(B) + (unsigned)(ab * 8 * 256 + tid);
                float p[8];
                unsigned spins = 0;
#if PD_WINDOW
                const int wlo = flag[1] - wn.back, whi = flag[1] + wn.ahead;      // (read ahead of the wait, not behind it)
#endif
                for (int i = 0; i < nap_x; i += 4) __builtin_amdgcn_s_sleep(4);
                for (;;) {
                    bool ok = true;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const unsigned x = t2v_ld_b32(rx, (e0 + (unsigned)(i * 256)) * 4u);
                        p[i] = __uint_as_float(x);
                        ok = ok && x != T2V_SENT;
                    }
                    if (__all(ok)) break;
                    __builtin_amdgcn_s_sleep(1);
                    if (t2v_give_up(spins, PD_SPIN, a.err, flag)) break;
                }
                nap_x = pd_adapt(nap_x, (int)spins);
                const float ev = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
#if PD_WINDOW
                ev0 = (tid < len && tid >= wlo && tid <= whi) ? ev : -INFINITY;
#else
                ev0 = tid < len ? ev : -INFINITY;
#endif
            }
            {
                float mloc = ev0;
                mloc = T2V_DPP_MAX(mloc, 0xB1); mloc = T2V_DPP_MAX(mloc, 0x4E);
                mloc = T2V_DPP_MAX(mloc, 0x141); mloc = T2V_DPP_MAX(mloc, 0x140);
                mloc = rows4_max(mloc);
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
                const float sloc = rows4_sum(row16_sum(e0v));
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
                win[15 + tid] = al;                                         // previous weights of the next frame
                win[TW + 15 + tid] += al;                                   // cumulative weights
            }
            __syncthreads();
            PD_STAMP(0, 4);
            PD_RT(4);
            // context columns 64 as .. 64 as + 63: thread = (column c = tid & 63, part = tid >> 6)
            {
                const int c = tid & 63, part = tid >> 6;
                cred[part * 64 + c] = t2v_ctx_partial_v<PD_CTXW>(eall, mem_s, part, c, Tp);
            }
            __syncthreads();
            if (tid < 64) {
                float acc = 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += cred[u * 64 + tid];
                pd_put(rx, xcur + pd_ctx(B) + (unsigned)(ab * 512 + 64 * as + tid), acc);
            }
            // (the saved alignment row leaves AFTER the context hand-off: nothing sits in this CU's memory pipe in front of it)
            if (as == 0 && tid < Tp) a.AL[((size_t)(t + 1) * B + ab) * Tp + tid] = al;
        }
        PD_STAMP(0, 5); PD_STAMP(64, 11);
        PD_RT(5);
        if (is_attn) pd_gemv_part<PD_KDEC / 32, 0, 32, true>(wd, X, B, ed);      // (the context of the other items is in flight meanwhile)
        // ---- 3. ctx(t) for everyone, the context columns of decoder_rnn(t)
        {
            const int rounds = pd_gather_items(X + PD_X_CX, rx, xcur + pd_ctx(B), 512u, 512, B, nap_c, a.err, flag);
            nap_c = pd_adapt(nap_c, rounds);
        }
        __syncthreads();
        if (flag[0] != 1) return;
        PD_STAMP(0, 6);
        PD_RT(6);
        pd_gemv_part<PD_KDEC / 32, 64, 80, true>(wd, X, B, ed);
        pd_gemv_finish(ed, B, red);
        __syncthreads();
        if (tid < 16 * B) {
            const int r = tid & 15, b = tid >> 4;
            float s = 0.f;
#pragma unroll
            for (int w8 = 0; w8 < 8; ++w8) s += red[(w8 * 16 + r) * PD_MAXB + b];
            gst[b * 16 + r] = s + bias_d;
        }
        __syncthreads();
        if (tid < 4 * B) {
            const int u = tid & 3, b = tid >> 2;
            const float* gp = gst + b * 16 + 4 * u;
            const float gi = sigmoidf_(gp[0]), gf = sigmoidf_(gp[1]), gg = tanhf_(gp[2]), go = sigmoidf_(gp[3]);
            const float c = gf * cst[PD_MAXB * 4 + b * 4 + u] + gi * gg;
            cst[PD_MAXB * 4 + b * 4 + u] = c;
            const float h = go * tanhf_(c);
            const float h1 = T2V_DPP_QUAD_F(h, 1), h2 = T2V_DPP_QUAD_F(h, 2), h3 = T2V_DPP_QUAD_F(h, 3);      // (used by lane u == 0 only)
            if (u == 0) t2v_st(rx, (xcur + pd_hdec(B) + (unsigned)((pd_opaque(threadIdx.x) >> 2) * 1024 + 4 * wg)) * 4u, u32x4{__float_as_uint(h), __float_as_uint(h1), __float_as_uint(h2), __float_as_uint(h3)});
        }
        PD_STAMP(0, 7); PD_STAMP(64, 12);
        PD_RT(7);
        // attention_rnn(t+1), the [h_att(t) | ctx(t)] columns: in the shadow of the projection / Prenet stages (the projection
        // workgroups do theirs once their rows are out)
        if (!wg_proj) pd_gemv_part<PD_KATT / 32, 0, 48, false>(wa, X, B, ea);
        // ---- 4. projection rows (mel, gate, folded Prenet layer 0)
        if (prow >= 0) {            // whole workgroup takes the branch: barriers inside are uniform
            // the context columns of the rows first: h_dec(t) is still on its way
            float pacc[PD_MAXB];
#pragma unroll
            for (int b = 0; b < PD_MAXB; ++b) pacc[b] = 0.f;
            if (is_proj) {
                const float* wr = prow_s + wave * 1536;
#pragma unroll
                for (int b = 0; b < PD_MAXB; ++b) {
                    if (b < B) {
                        const float* xb = X + (size_t)b * PD_XW;
                        float acc = 0.f;
#pragma unroll
                        for (int i = 16; i < 24; ++i) acc = fmaf(wr[lane + 64 * i], xb[PD_X_CX + (lane + 64 * i - T2V_H)], acc);
                        pacc[b] = acc;
                    }
                }
            }
            // (round 6: the Prenet-0 dropout factors of this wave's row — a 64-bit counter hash per item, a function of (seed, frame, row)
            // alone — are evaluated HERE, in the shadow of the h_dec hand-off, not behind the dot product on the frame's chain)
            float drop0[PD_MAXB];
#pragma unroll
            for (int b = 0; b < PD_MAXB; ++b)
                drop0[b] = (is_proj && prow > T2V_NMEL && b < B)
#if PD_ITEMS
                               ? t2v_drop_scale(iseed[b], T2V_RNG_PRENET0, t + 1, (uint32_t)(prow - (T2V_NMEL + 1)), a.p_prenet) : 0.f;
#else
                               ? t2v_drop_scale(a.seed, T2V_RNG_PRENET0, t + 1, (uint32_t)(b * T2V_PRE + (prow - (T2V_NMEL + 1))), a.p_prenet) : 0.f;
#endif
            {
                const int rounds = pd_gather_items(X + PD_X_HD, rx, xcur + pd_hdec(B), 1024u, 1024, B, nap_p, a.err, flag);
                nap_p = pd_adapt(nap_p, rounds);
            }
            __syncthreads();
            if (flag[0] != 1) return;
            if (is_proj) {
                const float* wr = prow_s + wave * 1536;
                bool all_fired = true;
                // (an opaque copy of the row number: the output addresses derived from it are rebuilt per frame instead of being
                // hoisted out of the frame loop, spilled, and reloaded from scratch in front of every store)
                int prow_o = prow;
                asm volatile("" : "+v"(prow_o));
                const int prow = prow_o;
#pragma unroll
                for (int b = 0; b < PD_MAXB; ++b) {
                    if (b >= B) continue;
                    const float* xb = X + (size_t)b * PD_XW;
                    float acc = pacc[b];
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc = fmaf(wr[lane + 64 * i], xb[PD_X_HD + lane + 64 * i], acc);      // the h_dec columns
                    acc = wave_sum_rl(acc) + pbias;
                    if (lane == 0) {
                        if (prow < T2V_NMEL) a.MEL[((size_t)t * B + b) * T2V_NMEL + prow] = acc;
#if PD_ITEMS
                        else if (prow == T2V_NMEL) {
                            a.GATE[(size_t)t * B + b] = acc;
                            if (acc > a.gate_logit_thr) atomicMin(it.stop_item + b, t);     // item b's own stop frame
                        }
#else
                        else if (prow == T2V_NMEL) a.GATE[(size_t)t * B + b] = acc;
#endif
                        else {
                            const float pv = fmaxf(acc, 0.f) * drop0[b];
                            gst[b * 8 + wave] = pv;         // published below, eight rows with ONE store instruction
                        }
                    }
                    all_fired = all_fired && acc > a.gate_logit_thr;
                }
                if (prow == T2V_NMEL && lane == 0) {
                    // stop rule sigmoid(gate) > threshold for every item (model.py:453; B == 1 in the reference)
                    if (all_fired) atomicMin(a.stop_flag, t);
                    pd_put(rx, xcur + pd_stop(B), __uint_as_float(all_fired ? 2u : 1u));
                }
            }
            __syncthreads();        // X[HD] now holds h_dec(t): the next frame's decoder_rnn input for this workgroup
            // Prenet layer-0 rows of this workgroup: one coalesced 32-byte write per item instead of eight 4-byte writes from
            // eight waves — 32 single-word writes per cache line from all over the chip took microseconds to land
            if (tid < 8 * B) {
                const int b = tid >> 3, row = (wg - PD_WG_PROJ) * 8 + (tid & 7);
                if (row > T2V_NMEL && row < PD_NROW) {
                    const int to = pd_opaque(threadIdx.x);
                    pd_put(rx, xcur + pd_pre0(B) + (unsigned)((to >> 3) * 256 + (wg - PD_WG_PROJ) * 8 + (to & 7) - (T2V_NMEL + 1)), gst[b * 8 + (tid & 7)]);
                }
            }
            pd_gemv_part<PD_KATT / 32, 0, 48, false>(wa, X, B, ea);
        } else if (is_attn && t + 1 < a.t_end) {
            // decoder_rnn(t+1), part 1 (the h_dec(t) columns) of the ATTENTION workgroups: in the tail of this frame — at the top
            // of the next one they go straight from "h_att published" to their gather of it and the attention (the chain).  The
            // projection workgroups are gathering the same row right now and ARE the chain: let them go first.
#if PD_WINDOW == 2
            // window centre of the NEXT frame: the plan's symbol of frame t + 1 (its last one behind the plan's end), clamped to
            // the item.  It is data, so nothing of it waits for this frame: one load in the idle tail, where PD_WINDOW 1 scans the
            // weights, left in flag[1] for the softmax threads of frame t + 1 behind the barrier below.  (Issued a frame earlier
            // and carried in a register, so that no round trip to memory sits in this tail, it measured the same and spilled 8
            // bytes more: DESIGN 7w.)  The 8 slices of an item read the same word.
            {
                const int q = plan_row[min(t + 1, plan_last)];
                if (tid == 0) flag[1] = min(max(q, 0), plan_len - 1);
            }
#elif PD_WINDOW
            // attention window of the NEXT frame: p = position of the largest weight of this frame (lowest index on a tie; frame 0
            // starts from p = 0, as the all-zero initial weights give), energies outside [p - back, p + ahead] count as -inf.  It
            // depends on this frame's weights alone, so it is found here, where the attention workgroups idle: wave 0 scans
            // win[15 ..] and leaves p in flag[1], which the softmax threads of frame t + 1 read behind the barrier below.  (In front
            // of the h_att(t + 1) gather, next to the location features, the same scan cost 1.1 us per frame: DESIGN 7n.)  Every
            // slice of an item derives p from its own copy of the weights: the copies are bit-identical (the same 8 partial
            // energies summed in the same order, the same maximum and sum), so the 8 slices take the same window without
            // exchanging anything.
            if (wave == 0) {
                float bv = -1.f;
                int bj = 0;
#pragma unroll
                for (int i = 0; i < (PD_MAXT + 63) / 64; ++i) {
                    const int j = lane + 64 * i;
                    const float v = j < Tp ? win[15 + j] : -1.f;
                    if (v > bv) { bv = v; bj = j; }
                }
                pd_argmax_wave(bv, bj);
                if (lane == 0) flag[1] = bj;
            }
#endif
            __builtin_amdgcn_s_sleep(48);
            (void)pd_gather_items(X + PD_X_HD, rx, xcur + pd_hdec(B), 1024u, 1024, B, 0, a.err, flag);
            __syncthreads();
            if (flag[0] != 1) return;
        }
        if ((is_attn || wg_proj) && t + 1 < a.t_end) pd_gemv_part<PD_KDEC / 32, 32, 64, true>(wd, X, B, ed);
        PD_STAMP(64, 13); PD_STAMP(128, 15);
        PD_RT(8);
        // ---- 5. Prenet layer 1 rows: wave 0 fetches pre0 for the whole workgroup (256 waves polling the same 1 KB were the
        //         other hot spot of the frame)
        if (p1row >= 0) {
            float* p0_s = w1_s + 8 * 256;                                  // [B][256]
            // (what does not depend on pre0 goes in front of the wait for it: the row's weights and its dropout factors)
            const float4 w4 = *(const float4*)(w1_s + wave * 256 + 4 * lane);
            float drop1[PD_MAXB];
#pragma unroll
            for (int b = 0; b < PD_MAXB; ++b)
#if PD_ITEMS
                drop1[b] = b < B ? t2v_drop_scale(iseed[b], T2V_RNG_PRENET1, t + 1, (uint32_t)p1row, a.p_prenet) : 0.f;
#else
                drop1[b] = b < B ? t2v_drop_scale(a.seed, T2V_RNG_PRENET1, t + 1, (uint32_t)(b * T2V_PRE + p1row), a.p_prenet) : 0.f;
#endif
            if (wave == 0) {
                unsigned spins = 0;
                for (int i = 0; i < nap_q; i += 4) __builtin_amdgcn_s_sleep(4);
                if (B == 1) {
                    const unsigned gq = xcur + pd_pre0(B) + (unsigned)(4 * lane);
                    u32x4 x;
                    for (;;) {
                        x = t2v_ld_b128(rx, gq * 4u);
                        if (__all(x[0] != T2V_SENT && x[1] != T2V_SENT && x[2] != T2V_SENT && x[3] != T2V_SENT)) break;
                        __builtin_amdgcn_s_sleep(1);
                        if (t2v_give_up(spins, PD_SPIN, a.err, flag)) break;
                    }
                    *(float4*)(p0_s + 4 * lane) = make_float4(__uint_as_float(x[0]), __uint_as_float(x[1]), __uint_as_float(x[2]), __uint_as_float(x[3]));
                } else {
                    // (all items in one polling pass, their loads in flight together: item by item every item paid its own round trip)
                    u32x4 x[PD_MAXB];
                    for (;;) {
                        bool ok = true;
    #pragma unroll
                        for (int b = 0; b < PD_MAXB; ++b) {
                            if (b < B || b == 0) x[b] = t2v_ld_b128(rx, (xcur + pd_pre0(B) + (unsigned)(min(b, B - 1) * 256 + 4 * lane)) * 4u);
                            else x[b] = x[0];
                            ok = ok && x[b][0] != T2V_SENT && x[b][1] != T2V_SENT && x[b][2] != T2V_SENT && x[b][3] != T2V_SENT;
                        }
                        if (__all(ok)) break;
                        __builtin_amdgcn_s_sleep(1);
                        if (t2v_give_up(spins, PD_SPIN, a.err, flag)) break;
                    }
    #pragma unroll
                    for (int b = 0; b < PD_MAXB; ++b)
                        if (b < B)
                            *(float4*)(p0_s + b * 256 + 4 * lane) =
                                make_float4(__uint_as_float(x[b][0]), __uint_as_float(x[b][1]), __uint_as_float(x[b][2]), __uint_as_float(x[b][3]));
                }
                nap_q = pd_adapt(nap_q, (int)spins);
            }
            __syncthreads();
            if (flag[0] != 1) return;
#pragma unroll
            for (int b = 0; b < PD_MAXB; ++b) {
                if (b >= B) continue;
                const float4 xv = *(const float4*)(p0_s + b * 256 + 4 * lane);
                float acc = w4.x * xv.x;
                acc = fmaf(w4.y, xv.y, acc); acc = fmaf(w4.z, xv.z, acc); acc = fmaf(w4.w, xv.w, acc);
                acc = wave_sum_rl(acc);
                if (lane == 0) {
                    acc = fmaxf(acc, 0.f) * drop1[b];
                    gst[b * 8 + wave] = acc;
                }
            }
            __syncthreads();
            if (tid < 8 * B) {
                const int to = pd_opaque(threadIdx.x);
                pd_put(rx, xcur + pd_pre1(B) + (unsigned)((to >> 3) * 256 + (wg - PD_WG_PRE1) * 8 + (to & 7)), gst[tid]);
            }
        }
        PD_STAMP(128, 16); PD_STAMP(0, 8);
        PD_RT(9);
    }
}

