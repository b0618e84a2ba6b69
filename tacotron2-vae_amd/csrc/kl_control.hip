// KL control: Tacotron2Loss_VAE with free bits (Kingma et al. 2016) and a KL capacity target (Burgess et al. 2018), value and
// gradients in one launch, plus a running per-dimension record of the posterior (the collapse monitor).
//   kl[b][d] = 0.5 (mu^2 + e^logvar - logvar - 1)        k[d] = (1/B) sum_b kl[b][d]        KL = sum_b sum_d kl[b][d]
//   K' = B sum_d max(k[d], lambda)     dimension d is floored when lambda > 0 and k[d] <= lambda: it adds B lambda, its gradients are 0
//   T  = |K' - B C|, s = sign(K' - B C) (0 at equality)  when C >= 0, else T = K', s = 1
//   total = recon + w T      dmu = w s g[d] mu      dlogvar = w s g[d] 0.5 (e^logvar - 1)      g[d] = 0 floored, else 1
// k_loss_klc is k_loss (refenc.hip) in its mel and gate part: grid-stride, one fp32 partial per block, the last block to arrive adds
// the partials in index order.  The latent part needs k[d], then K' and s, before a latent gradient can be written, and is a few
// thousand elements at most (D <= 256): workgroup 0 does it alone, in two phases through LDS.  Phase one: thread (r, d) adds the
// fp32 terms of rows r, r + R, ... of column d in fp64, thread d adds the R partials in order, thread 0 adds the D columns in order.
// Phase two: the gradients.  No float atomics, nothing read back, an order fixed by B and D: the same bits from run to run, eagerly
// or replayed from a graph.
// Monitor (optional, 3 D + 2 doubles): [0] rows seen n, [1] launches seen, then per dimension the running mean of mu[:, d], its M2
// (sum of squared deviations; the batch joins the aggregate by Chan's merge) and sum kl[:, d].
#include "t2v_common.h"
#include "t2v_kernels.h"

#define KLC_THREADS 256
#define KLC_MAX_DIMS 256

struct KlcArgs {
    const float* mel; const float* post; const float* mel_t; const float* gate; const float* gate_t;
    const float* mu; const float* logvar;
    float* dmel; float* dpost; float* dgate; float* dmu; float* dlogvar;
    float* part;     // (nblk, 2)
    float* out;      // (8) total, recon, KL, w, K', T, floored dimensions, s
    double* monitor; // (3 D + 2) or NULL
    size_t n_mel; int n_gate, B, D, nblk;
    float klw, free_bits, capacity;
    const t2v_step_params* step;   // device-side KL weight (graph replay) or NULL
    unsigned* ticket;
};

// the latent part: workgroup 0, all 256 threads
__device__ __forceinline__ void klc_latent(const KlcArgs& a, float klw) {
    __shared__ double s_a[KLC_THREADS], s_b[KLC_THREADS];   // phase-one partials, then per-dimension sum kl / batch mean of mu
    __shared__ double s_c[KLC_MAX_DIMS];                    // per-dimension contribution to K'
    __shared__ float s_g[KLC_MAX_DIMS];                     // g[d]
    __shared__ float s_coef;                                // w s
    const int tid = threadIdx.x, B = a.B, D = a.D;
    const int R = KLC_THREADS / D;                          // rows in flight (>= 1: D <= 256)
    const int r = tid / D, d = tid - r * D;
    const bool lane = r < R;                                // threads past R D sit phase one out
    double acc_kl = 0.0, acc_mu = 0.0;
    if (lane)
        for (int b = r; b < B; b += R) {
            const size_t i = (size_t)b * D + d;
            const float m = a.mu[i], lv = a.logvar[i], e = expf(lv);
            acc_kl += (double)(-0.5f * (1.f + lv - m * m - e));
            acc_mu += (double)m;
        }
    s_a[tid] = acc_kl;
    s_b[tid] = acc_mu;
    __syncthreads();
    double klsum = 0.0, mean_b = 0.0;
    if (tid < D) {
        double mu_sum = 0.0;
        for (int q = 0; q < R; ++q) {
            klsum += s_a[q * D + tid];
            mu_sum += s_b[q * D + tid];
        }
        mean_b = mu_sum / (double)B;
    }
    __syncthreads();
    if (tid < D) {
        s_a[tid] = klsum;
        s_b[tid] = mean_b;
        const double floor_sum = (double)B * (double)a.free_bits;
        const bool floored = a.free_bits > 0.f && klsum <= floor_sum;       // k[d] <= lambda
        s_c[tid] = floored ? floor_sum : klsum;
        s_g[tid] = floored ? 0.f : 1.f;
    }
    __syncthreads();
    if (tid == 0) {
        double kl = 0.0, kp = 0.0;
        int nfl = 0;
        for (int q = 0; q < D; ++q) {
            kl += s_a[q];
            kp += s_c[q];
            nfl += s_g[q] == 0.f;
        }
        double T = kp, s = 1.0;
        if (a.capacity >= 0.f) {
            const double diff = kp - (double)B * (double)a.capacity;
            T = fabs(diff);
            s = diff > 0.0 ? 1.0 : diff < 0.0 ? -1.0 : 0.0;
        }
        a.out[2] = (float)kl;
        a.out[3] = klw;
        a.out[4] = (float)kp;
        a.out[5] = (float)T;
        a.out[6] = (float)nfl;
        a.out[7] = (float)s;
        s_coef = klw * (float)s;
    }
    __syncthreads();
    // phase two: the gradients (w s = w when the capacity term is off: k_loss's products)
    const float coef = s_coef;
    const size_t n_lat = (size_t)B * D;
    for (size_t i = tid; i < n_lat; i += KLC_THREADS) {
        const int q = (int)(i % (size_t)D);
        if (s_g[q] == 0.f) {
            a.dmu[i] = 0.f;
            a.dlogvar[i] = 0.f;
        } else {
            const float m = a.mu[i], e = expf(a.logvar[i]);
            a.dmu[i] = coef * m;
            a.dlogvar[i] = coef * -0.5f * (1.f - e);
        }
    }
    if (!a.monitor) return;
    // the batch's M2 about its own mean (second pass: no cancellation), then Chan's merge into the aggregate
    double acc_m2 = 0.0;
    if (lane) {
        const double mb = s_b[d];
        for (int b = r; b < B; b += R) {
            const double x = (double)a.mu[(size_t)b * D + d] - mb;
            acc_m2 += x * x;
        }
    }
    __syncthreads();            // (s_a[d] = sum kl is read below: keep it, the partials go to s_c)
    s_c[tid] = acc_m2;          // KLC_MAX_DIMS == KLC_THREADS
    __syncthreads();
    const double n_a = a.monitor[0];
    __syncthreads();            // every thread holds the old row count before thread 0 replaces it
    if (tid < D) {
        double m2_b = 0.0;
        for (int q = 0; q < R; ++q) m2_b += s_c[q * D + tid];
        double* mean = a.monitor + 2 + tid;
        double* m2 = a.monitor + 2 + D + tid;
        double* skl = a.monitor + 2 + 2 * (size_t)D + tid;
        const double n_b = (double)B, n = n_a + n_b;
        const double delta = s_b[tid] - *mean;
        *mean += delta * (n_b / n);
        *m2 += m2_b + delta * delta * (n_a * n_b / n);
        *skl += s_a[tid];
    }
    if (tid == 0) {
        a.monitor[0] = n_a + (double)B;
        a.monitor[1] += 1.0;
    }
}

__global__ __launch_bounds__(KLC_THREADS) void k_loss_klc(KlcArgs a) {
    __shared__ float scr[4];
    __shared__ int last;
    const int tid = threadIdx.x;
    const float klw = a.step ? a.step->kl_weight : a.klw;
    float s_mel = 0.f, s_gate = 0.f;
    const float cm = 2.0f / (float)a.n_mel;
    for (size_t i = (size_t)blockIdx.x * KLC_THREADS + tid; i < a.n_mel; i += (size_t)gridDim.x * KLC_THREADS) {
        const float t = a.mel_t[i];
        const float d0 = a.mel[i] - t, d1 = a.post[i] - t;
        s_mel = fmaf(d0, d0, s_mel);
        s_mel = fmaf(d1, d1, s_mel);
        a.dmel[i] = cm * d0;
        a.dpost[i] = cm * d1;
    }
    for (int i = blockIdx.x * KLC_THREADS + tid; i < a.n_gate; i += gridDim.x * KLC_THREADS) {
        const float x = a.gate[i], y = a.gate_t[i];
        s_gate += fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
        a.dgate[i] = (1.0f / (1.0f + expf(-x)) - y) / (float)a.n_gate;
    }
    if (blockIdx.x == 0) klc_latent(a, klw);        // writes out[2..7] before this block takes its ticket
    const float v[2] = {s_mel, s_gate};
    for (int k = 0; k < 2; ++k) {
        float x = wave_sum(v[k]);
        __syncthreads();
        if ((tid & 63) == 0) scr[tid >> 6] = x;
        __syncthreads();
        if (tid == 0) a.part[(size_t)blockIdx.x * 2 + k] = (scr[0] + scr[1]) + (scr[2] + scr[3]);
    }
    // last block to finish reduces the partials in index order and joins them with workgroup 0's T
    __threadfence();
    if (tid == 0) last = (atomicAdd(a.ticket, 1u) == gridDim.x - 1);
    __syncthreads();
    if (last && tid == 0) {
        __threadfence();
        double m = 0.0, g = 0.0;
        for (int i = 0; i < a.nblk; ++i) {
            m += (double)__hip_atomic_load(a.part + (size_t)i * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            g += (double)__hip_atomic_load(a.part + (size_t)i * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const float T = __hip_atomic_load(a.out + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float recon = (float)(m / (double)a.n_mel + g / (double)a.n_gate);
        a.out[1] = recon;
        a.out[0] = recon + klw * T;
        *a.ticket = 0;
    }
}

extern "C" int t2v_loss_fwd_bwd_klc(const float* mel, const float* post, const float* mel_t, const float* gate,
                                    const float* gate_t, const float* mu, const float* logvar, float* dmel, float* dpost,
                                    float* dgate, float* dmu, float* dlogvar, float* part128, float* out8, uint32_t* ticket,
                                    double* monitor, uint64_t n_mel, int n_gate, int B, int D, float kl_weight,
                                    float free_bits, float capacity, void* stream_) {
    if (!mel || !post || !mel_t || !gate || !gate_t || !mu || !logvar || !dmel || !dpost || !dgate || !dmu || !dlogvar ||
        !part128 || !out8 || !ticket)
        return T2V_ERR_ARG;
    if (B < 1 || D < 1 || D > KLC_MAX_DIMS || n_gate < 1 || n_mel < 1 || !(free_bits >= 0.f) || capacity != capacity)
        return T2V_ERR_ARG;
    KlcArgs a;
    a.mel = mel; a.post = post; a.mel_t = mel_t; a.gate = gate; a.gate_t = gate_t; a.mu = mu; a.logvar = logvar;
    a.dmel = dmel; a.dpost = dpost; a.dgate = dgate; a.dmu = dmu; a.dlogvar = dlogvar; a.part = part128; a.out = out8;
    a.monitor = monitor; a.n_mel = n_mel; a.n_gate = n_gate; a.B = B; a.D = D; a.nblk = 64; a.klw = kl_weight;
    a.free_bits = free_bits; a.capacity = capacity; a.ticket = ticket; a.step = t2v_step_for((hipStream_t)stream_);
    k_loss_klc<<<64, KLC_THREADS, 0, (hipStream_t)stream_>>>(a);
    return t2v_check_launch();
}
