// Fused multi-tensor optimiser step over ONE flat fp32 arena (params / grads / exp_avg /
// exp_avg_sq laid out back to back in reference parameter order).
// Replaces torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step of the reference train loop
// (train.py:226-229; Adam(lr, weight_decay) at train.py:171-172 — L2-in-grad weight decay).
// HBM-bound: 16 B read + 12 B written per element, two launches regardless of tensor count.
// With a weight average (t2v_clip_adam_ema_step_guarded) the same launch also carries an exponential moving average of the
// parameters in a fifth arena: 4 B more read and 4 B more written per element (28 -> 36), still two launches.
#include "t2v_common.h"
#include "t2v_kernels.h"

#define T2V_NORM_BLOCKS 1024

__global__ __launch_bounds__(256) void k_sumsq(const float4* __restrict__ g, size_t n4, const float* __restrict__ tail,
                                               int ntail, float inv_world, float* __restrict__ partials) {
    __shared__ float red[4];
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        float4 v = g[i];
        v.x *= inv_world; v.y *= inv_world; v.z *= inv_world; v.w *= inv_world;
        acc = fmaf(v.x, v.x, acc);
        acc = fmaf(v.y, v.y, acc);
        acc = fmaf(v.z, v.z, acc);
        acc = fmaf(v.w, v.w, acc);
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) { const float t = tail[threadIdx.x] * inv_world; acc = fmaf(t, t, acc); }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct AdamArgs {
    float* p; float* g; float* m; float* v;
    size_t n;
    const float* partials;
    float* norm_out;          // [0] = total grad norm (after the 1/world scaling)
    float lr, b1, b2, eps, wd, max_norm, inv_world, bc1, bc2s;   // bc1 = 1-b1^t, bc2s = sqrt(1-b2^t)
    const t2v_step_params* step;     // device-side lr / bc1 / bc2s (graph replay) or NULL
    const uint32_t* guard;           // optional: error words of the step's cooperative / persistent kernels
    int guard_n;
};

struct EmaArgs {
    float* s;                 // the shadow arena (n floats), updated in place
    float rate;               // 1 - decay
    int warmup;               // rate_t = max(rate, 9 / (10 + t)): TensorFlow's min(decay, (1 + t) / (10 + t)) as a rate
    uint64_t t;               // number of updates so far; a.step->epoch replaces it when a device record is bound
};

// One body, two instantiations: k_clip_adam<false> is the step as it always was (instruction for instruction: the body
// is the kernel, not a function inlined into two wrappers, which the compiler schedules differently), k_clip_adam<true>
// folds the shadow update in behind the parameter update, from the register that holds the parameter just before it is
// stored.
template <bool EMA>
__global__ __launch_bounds__(256) void k_clip_adam(AdamArgs a, EmaArgs e) {
    __shared__ float red[4];
    __shared__ float s_coef;
    __shared__ int s_skip;
    // Guarded step (round 4): a bounded spin that gave up inside one of the step's persistent / cooperative kernels leaves a
    // non-zero error word and gradients that mean nothing.  The update is then SKIPPED on the device — parameters and both
    // moment arenas stay untouched, norm_out reads NaN — so the host, when it reads the error ledger at its next sync, can
    // switch that kernel family off and simply run the iteration again (train.TrainEngine.recover).
    if (a.guard) {
        if (threadIdx.x == 0) {
            int bad = 0;
            for (int i = 0; i < a.guard_n; ++i) bad |= (a.guard[i] != 0u);
            s_skip = bad;
        }
        __syncthreads();
        if (s_skip) {
            if (blockIdx.x == 0 && threadIdx.x == 0) a.norm_out[0] = __uint_as_float(0x7fc0beefu);     // a NaN with a payload the host recognises
            return;                                                                                     // (the shadow stays as well)
        }
    }
    // every block re-reduces the 1024 partials in the same order -> identical clip coefficient
    float acc = 0.f;
    for (int i = threadIdx.x; i < T2V_NORM_BLOCKS; i += 256) acc += a.partials[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float total = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
        float coef = a.max_norm / (total + 1e-6f);
        coef = coef < 1.0f ? coef : 1.0f;
        if (a.max_norm <= 0.f) coef = 1.0f;
        s_coef = coef * a.inv_world;
        if (blockIdx.x == 0) a.norm_out[0] = total;
    }
    __syncthreads();
    const float gs = s_coef;
    const float lr = a.step ? a.step->lr : a.lr, bc1 = a.step ? a.step->bc1 : a.bc1;
    const float bc2s = a.step ? a.step->bc2s : a.bc2s;
    const float step_size = lr / bc1;
    float rate = 0.f;
    if constexpr (EMA) {
        const uint64_t t = a.step ? a.step->epoch : e.t;
        rate = e.warmup ? fmaxf(e.rate, 9.0f / (10.0f + (float)t)) : e.rate;
    }
    const size_t n4 = a.n >> 2;
    float4* p4 = (float4*)a.p; const float4* g4 = (const float4*)a.g; float4* m4 = (float4*)a.m; float4* v4 = (float4*)a.v;
    float4* s4 = (float4*)e.s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        float4 p = p4[i], g = g4[i], m = m4[i], v = v4[i];
        float4 s;
        if constexpr (EMA) s = s4[i];
#define UPD(c)                                                        \
        {                                                             \
            const float gg = fmaf(a.wd, p.c, g.c * gs);              \
            m.c = a.b1 * m.c + (1.0f - a.b1) * gg;                    \
            v.c = a.b2 * v.c + (1.0f - a.b2) * gg * gg;               \
            p.c -= step_size * (m.c / (sqrtf(v.c) / bc2s + a.eps)); \
        }
        UPD(x) UPD(y) UPD(z) UPD(w)
#undef UPD
        p4[i] = p; m4[i] = m; v4[i] = v;
        if constexpr (EMA) {            // s += rate * (p_new - s), p_new being the very fp32 value that went to params
            s.x = fmaf(rate, p.x - s.x, s.x); s.y = fmaf(rate, p.y - s.y, s.y);
            s.z = fmaf(rate, p.z - s.z, s.z); s.w = fmaf(rate, p.w - s.w, s.w);
            s4[i] = s;
        }
    }
    if (blockIdx.x == 0) {
        for (size_t i = (n4 << 2) + threadIdx.x; i < a.n; i += 256) {
            const float gg = fmaf(a.wd, a.p[i], a.g[i] * gs);
            const float m = a.b1 * a.m[i] + (1.0f - a.b1) * gg;
            const float v = a.b2 * a.v[i] + (1.0f - a.b2) * gg * gg;
            a.m[i] = m; a.v[i] = v;
            const float p = a.p[i] - step_size * (m / (sqrtf(v) / bc2s + a.eps));
            a.p[i] = p;
            if constexpr (EMA) { const float s = e.s[i]; e.s[i] = fmaf(rate, p - s, s); }
        }
    }
}

// the argument checks and the two launches of every entry point; ema == nullptr: the plain step
static int clip_adam_launch(float* params, float* grads, float* exp_avg, float* exp_avg_sq, uint64_t n, float lr, float beta1,
                            float beta2, float eps, float weight_decay, float max_norm, float inv_world, float bc1, float bc2,
                            float* partials, float* norm_out, const uint32_t* guard, int guard_n, const EmaArgs* ema,
                            hipStream_t stream) {
    if (guard_n < 0 || (guard_n > 0 && !guard)) return T2V_ERR_ARG;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !partials || !norm_out || !(bc1 > 0.f) || !(bc2 > 0.f)) return T2V_ERR_ARG;
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return T2V_ERR_ARG;
    if (ema && (!ema->s || ((uintptr_t)ema->s & 15) || !(ema->rate > 0.f && ema->rate <= 1.0f))) return T2V_ERR_ARG;
    const size_t n4 = n >> 2;
    k_sumsq<<<T2V_NORM_BLOCKS, 256, 0, stream>>>((const float4*)grads, n4, grads + (n4 << 2), (int)(n & 3), inv_world, partials);
    AdamArgs a;
    a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
    a.partials = partials; a.norm_out = norm_out;
    a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.wd = weight_decay; a.max_norm = max_norm;
    a.inv_world = inv_world;
    a.bc1 = bc1;
    a.bc2s = sqrtf(bc2);
    a.step = t2v_step_for(stream);
    a.guard = guard_n > 0 ? guard : nullptr;
    a.guard_n = guard_n;
    if (ema) k_clip_adam<true><<<2048, 256, 0, stream>>>(a, *ema);
    else k_clip_adam<false><<<2048, 256, 0, stream>>>(a, EmaArgs{nullptr, 0.f, 0, 0});
    return t2v_check_launch();
}

extern "C" int t2v_clip_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, uint64_t n,
                                  float lr, float beta1, float beta2, float eps, float weight_decay,
                                  float max_norm, float inv_world, float bc1, float bc2, float* partials,
                                  float* norm_out, void* stream_) {
    return clip_adam_launch(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, max_norm, inv_world,
                            bc1, bc2, partials, norm_out, nullptr, 0, nullptr, (hipStream_t)stream_);
}

extern "C" int t2v_clip_adam_step_guarded(float* params, float* grads, float* exp_avg, float* exp_avg_sq, uint64_t n,
                                          float lr, float beta1, float beta2, float eps, float weight_decay,
                                          float max_norm, float inv_world, float bc1, float bc2, float* partials,
                                          float* norm_out, const uint32_t* guard, int guard_n, void* stream_) {
    return clip_adam_launch(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, max_norm, inv_world,
                            bc1, bc2, partials, norm_out, guard, guard_n, nullptr, (hipStream_t)stream_);
}

extern "C" int t2v_clip_adam_ema_step_guarded(float* params, float* grads, float* exp_avg, float* exp_avg_sq, uint64_t n,
                                              float lr, float beta1, float beta2, float eps, float weight_decay,
                                              float max_norm, float inv_world, float bc1, float bc2, float* partials,
                                              float* norm_out, const uint32_t* guard, int guard_n, float* ema, float ema_rate,
                                              int ema_warmup, uint64_t ema_t, void* stream_) {
    const EmaArgs e{ema, ema_rate, ema_warmup, ema_t};
    return clip_adam_launch(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, max_norm, inv_world,
                            bc1, bc2, partials, norm_out, guard, guard_n, &e, (hipStream_t)stream_);
}
