// k_proj_prenet of decoder_infer.hip, included twice: PP_ITEMS 0 defines k_proj_prenet, PP_ITEMS 1 the per-item variant
// k_proj_prenet_items (batched synthesis): item b's own first gate-fire frame -> stop_item[b], and item b's Prenet masks from
// item_seeds[b] with the element index of item 0 (the masks of a B = 1 decode with that seed).  Two preprocessor instances
// rather than a template: the PP_ITEMS 0 text is the kernel as it was, so its instructions stay the same.
#if PP_ITEMS
__global__ __launch_bounds__(256) void k_proj_prenet_items(ProjPrenetArgs a, int* stop_item, const uint64_t* item_seeds) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // the seeds once, in front of every wait: the mask hashes stay off the frame's chain
    __shared__ uint64_t sseed[8];
    if (tid < a.B) sseed[tid] = item_seeds[tid];
    __syncthreads();
#else
__global__ __launch_bounds__(256) void k_proj_prenet(ProjPrenetArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#endif
    const int gw = blockIdx.x * 4 + wave;                 // global wave index 0..255
    const int HC = T2V_H + T2V_E;
    const int nrows = a.pre_next ? T2V_NMEL + 1 + T2V_PRE : T2V_NMEL + 1;
    // stage-2 operands requested up front: this wave's row of W1 (4 floats per lane)
    float4 w1r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.pre_next) w1r = *(const float4*)(a.w1 + (size_t)gw * T2V_PRE + 4 * lane);
    // ---- stage 1: rows gw, gw + 256 (the second pass only for the first 81 waves)
    for (int o = gw; o < nrows; o += 4 * PP_NWG) {
        const float4* wr = (const float4*)(a.proj_w + (size_t)o * HC);
        float4 wv[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) wv[i] = wr[lane + 64 * i];
        const float bias = a.proj_b[o];
        bool all_fired = true;
        for (int b = 0; b < a.B; ++b) {
            // (the Prenet-0 dropout factor of this row: a counter hash that needs none of the operands below — evaluated while
            // their loads are in flight, not behind the wave sum; round 6, as in the persistent decode kernel)
#if PP_ITEMS
            const float drop0 = o > T2V_NMEL ? t2v_drop_scale(sseed[b], T2V_RNG_PRENET0, a.t + 1, (uint32_t)(o - (T2V_NMEL + 1)), a.p_prenet) : 0.f;
#else
            const float drop0 = o > T2V_NMEL ? t2v_drop_scale(a.seed, T2V_RNG_PRENET0, a.t + 1, (uint32_t)(b * T2V_PRE + (o - (T2V_NMEL + 1))), a.p_prenet) : 0.f;
#endif
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int k = 4 * (lane + 64 * i);               // [h_dec_t (1024) | ctx_t (512)]
                const float* src = k < T2V_H ? a.xs_next + (size_t)b * T2V_XW + T2V_KATT + k : a.xs_cur + (size_t)b * T2V_XW + k;
                const float4 xv = *(const float4*)src;
                acc = fmaf(wv[i].x, xv.x, acc); acc = fmaf(wv[i].y, xv.y, acc);
                acc = fmaf(wv[i].z, xv.z, acc); acc = fmaf(wv[i].w, xv.w, acc);
            }
            acc = wave_sum(acc) + bias;
            if (o < T2V_NMEL) {
                if (lane == 0) a.mel_t[(size_t)b * T2V_NMEL + o] = acc;
            } else if (o == T2V_NMEL) {
                if (lane == 0) a.gate_t[b] = acc;
                // stop rule sigmoid(gate) > threshold (model.py:453; B == 1 in the reference): all items must fire.
                // This wave sees every item's gate in turn, so it can decide alone.
                all_fired = all_fired && acc > a.gate_logit_thr;
#if PP_ITEMS
                if (lane == 0 && acc > a.gate_logit_thr) atomicMin(stop_item + b, a.t);      // item b's own stop frame
#endif
            } else if (lane == 0) {
                const int r = o - (T2V_NMEL + 1);
                float v = fmaxf(acc, 0.f) * drop0;
                __hip_atomic_store(a.xchg + (size_t)b * T2V_PRE + r, ((t2v_u64)a.epoch << 32) | (t2v_u64)__float_as_uint(v),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (o == T2V_NMEL && lane == 0 && all_fired) atomicMin(a.stop_flag, a.t);
    }
    if (!a.pre_next) return;
    // ---- stage 2: Prenet layer 1, row gw (dropout always on)
    for (int b = 0; b < a.B; ++b) {
        const t2v_u64* gq = a.xchg + (size_t)b * T2V_PRE + 4 * lane;
#if PP_ITEMS
        const float drop1 = t2v_drop_scale(sseed[b], T2V_RNG_PRENET1, a.t + 1, (uint32_t)gw, a.p_prenet);      // (in front of the wait)
#else
        const float drop1 = t2v_drop_scale(a.seed, T2V_RNG_PRENET1, a.t + 1, (uint32_t)(b * T2V_PRE + gw), a.p_prenet);      // (in front of the wait)
#endif
        float xv[4];
        unsigned spins = 0;
        for (;;) {
            bool ok = true;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const t2v_u64 x = __hip_atomic_load(gq + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                xv[i] = __uint_as_float((unsigned)x);
                ok = ok && (unsigned)(x >> 32) == a.epoch;
            }
            if (__all(ok)) break;
            __builtin_amdgcn_s_sleep(2);
            if (++spins > 4000000u || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
        }
        float acc = w1r.x * xv[0];
        acc = fmaf(w1r.y, xv[1], acc); acc = fmaf(w1r.z, xv[2], acc); acc = fmaf(w1r.w, xv[3], acc);
        acc = wave_sum(acc);
        if (lane == 0) {
            acc = fmaxf(acc, 0.f) * drop1;
            a.pre_next[(size_t)b * T2V_PRE + gw] = acc;
        }
    }
}
