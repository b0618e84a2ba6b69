// Exact (all-pairs) t-SNE of N points to 2 dimensions: the map of the VAE latents that the reference README's "Visualization"
// section shows (tsne.png).  Affinities once, then a fixed number of gradient-descent iterations queued on the caller's
// stream without a host synchronisation.
//
// k_tsne_cond: one workgroup per row i.  Squared Euclidean distances to every j from the differences (a duplicate of x_i is
//   at distance 0 exactly), kept in LDS (4 N bytes, 64 KB at the cap); then the binary search of the precision beta_i for the
//   requested perplexity: at most 100 steps, |H - log(perplexity)| <= 1e-5 ends it, doubling / halving while a bound is
//   infinite, p_i|i = 0, a vanished sum replaced by 1e-8.  The search sums exp(-d beta) in fp64: its one discrete decision,
//   "stop here or halve once more", moves a row's p by far more than an fp32 rounding does, so it is taken on sums as good
//   as the fp64 reference's.  The row p_j|i is stored in fp32.
// k_tsne_sym: P_ij = (p_j|i + p_i|j) / (2N) in place, a pair of mirrored 32 x 32 tiles per workgroup.  Both elements of a
//   mirrored pair are the same fp32 sum of the same two numbers, so P is symmetric to the bit -- the pair pass relies on it.
// k_tsne_pairs: thread t of workgroup (bx, by) owns point i = 256 bx + t and visits j in [by jr, (by + 1) jr).  y_j comes
//   from an LDS tile (one broadcast read per pair), P_ij is read as P[j][i]: the 64 lanes of a wave read 256 contiguous
//   bytes of row j, which is the pass's HBM stream.  Per pair: w = 1 / (1 + |y_i - y_j|^2), attraction += P w (y_i - y_j),
//   repulsion += w^2 (y_i - y_j), Z += w.  The four force sums go out per (by, i), the workgroup's Z (and, in a pass that
//   reports the KL divergence, sum P' log(P' (1 + d^2)) and sum P', with P' = exaggeration * P) per workgroup.  jr is chosen from N alone so that
//   about 2048 workgroups exist at every N (tsne_geom): N = 1232 gives 5 x 39, N = 12000 gives 47 x 42.
// k_tsne_finish: every workgroup sums the per-workgroup Z in the same fixed order (fp64), then its 256 points sum their
//   per-split forces in split order, form grad = 4 (ex * attraction - repulsion / Z) and apply the update rule: gains + 0.2
//   where update and gradient differ in sign, * 0.8 elsewhere, floor 0.01; update = momentum * update - lr * gains * grad.
//   Workgroup 0 writes KL = A + log(Z) S when asked.
// No floating-point atomics; every sum has a fixed order that depends on N alone, so a run repeats to the bit.
#include "t2v_common.h"
#include "t2v_kernels.h"

#define TSNE_NT 256
#define TSNE_MAX_D 64
#define TSNE_TJ 512                 // y_j tile in LDS
#define TSNE_TARGET_WGS 2048        // 8 workgroups of 256 threads per CU
#define TSNE_MIN_JR 32
#define TSNE_UNROLL 8               // P loads in flight per thread
#define TSNE_EXAG_ITERS T2V_TSNE_EXAG_ITERS
#define TSNE_EXAG 12.0f
#define TSNE_KL_EVERY 50
#define TSNE_EPS 2.220446049250313e-16

namespace {

struct TsneGeom {
    int iblocks, jr, splits, nwg;
};

// the pair pass's grid: a function of N alone (not of the device), so that the order of every sum is too
TsneGeom tsne_geom(int N) {
    TsneGeom g;
    g.iblocks = (N + TSNE_NT - 1) / TSNE_NT;
    const int want = (TSNE_TARGET_WGS + g.iblocks - 1) / g.iblocks;
    int jr = (N + want - 1) / want;
    jr = (jr + 31) / 32 * 32;
    g.jr = jr < TSNE_MIN_JR ? TSNE_MIN_JR : jr;
    g.splits = (N + g.jr - 1) / g.jr;
    g.nwg = g.iblocks * g.splits;
    return g;
}

// scratch, in floats: [splits * N * 4] force partials | [3 * nwg] workgroup Z, A, S | [2N] update | [2N] gains
struct TsneScratch {
    float4* part;
    float *wgz, *wga, *wgs;
    float2 *upd, *gains;
};
size_t tsne_scratch_floats(int N, const TsneGeom& g) {
    return (size_t)g.splits * N * 4 + ((size_t)3 * g.nwg + 3) / 4 * 4 + (size_t)4 * N;
}
TsneScratch tsne_carve(void* scratch, int N, const TsneGeom& g) {
    TsneScratch s;
    float* p = (float*)scratch;
    s.part = (float4*)p;
    p += (size_t)g.splits * N * 4;
    s.wgz = p;
    s.wga = p + g.nwg;
    s.wgs = p + 2 * (size_t)g.nwg;
    p += ((size_t)3 * g.nwg + 3) / 4 * 4;
    s.upd = (float2*)p;
    s.gains = (float2*)(p + 2 * (size_t)N);
    return s;
}

// sum over the workgroup's 256 threads in a fixed order, returned to every thread (sh: 4 slots; two barriers)
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

}  // namespace

__global__ __launch_bounds__(TSNE_NT) void k_tsne_cond(const float* __restrict__ X, int N, int D, float perplexity,
                                                       float* __restrict__ Cnd) {
    extern __shared__ __attribute__((aligned(16))) float tsne_dist[];       // [N]
    __shared__ float xi[TSNE_MAX_D];
    __shared__ double sh[2][4];
    const int i = blockIdx.x, t = threadIdx.x;
    if (t < D) xi[t] = X[(size_t)i * D + t];
    __syncthreads();
    for (int j = t; j < N; j += TSNE_NT) {
        const float* xj = X + (size_t)j * D;
        float acc = 0.f;
        for (int c = 0; c < D; ++c) {
            const float df = xi[c] - xj[c];
            acc = fmaf(df, df, acc);
        }
        tsne_dist[j] = acc;
    }
    __syncthreads();
    const double target = log((double)perplexity), inf = __builtin_inf();
    double beta = 1.0, bmin = -inf, bmax = inf, beta_eval = 1.0, sum_eval = 1.0;
    for (int step = 0; step < 100; ++step) {
        double sp = 0.0, sd = 0.0;
        for (int j = t; j < N; j += TSNE_NT) {
            if (j == i) continue;
            const double d = (double)tsne_dist[j], e = exp(-d * beta);
            sp += e;
            sd = fma(d, e, sd);
        }
        sp = block_sum(sp, sh[0]);
        sd = block_sum(sd, sh[1]);
        if (sp == 0.0) sp = 1e-8;
        beta_eval = beta;
        sum_eval = sp;
        const double diff = log(sp) + beta * (sd / sp) - target;       // the same bits in every thread: uniform control flow
        if (fabs(diff) <= 1e-5) break;
        if (diff > 0.0) {
            bmin = beta;
            beta = bmax == inf ? beta * 2.0 : (beta + bmax) * 0.5;
        } else {
            bmax = beta;
            beta = bmin == -inf ? beta * 0.5 : (beta + bmin) * 0.5;
        }
    }
    float* row = Cnd + (size_t)i * N;
    for (int j = t; j < N; j += TSNE_NT)
        row[j] = j == i ? 0.f : (float)(exp(-(double)tsne_dist[j] * beta_eval) / sum_eval);
}

__global__ __launch_bounds__(TSNE_NT) void k_tsne_sym(float* __restrict__ P, int N) {
    __shared__ float A[32][33], B[32][33];
    const int a = blockIdx.y, b = blockIdx.x;
    if (a > b) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int ra = a * 32, rb = b * 32;
    for (int r = ty; r < 32; r += 8) {
        A[r][tx] = ra + r < N && rb + tx < N ? P[(size_t)(ra + r) * N + rb + tx] : 0.f;
        B[r][tx] = rb + r < N && ra + tx < N ? P[(size_t)(rb + r) * N + ra + tx] : 0.f;
    }
    __syncthreads();
    const float two_n = 2.f * (float)N;
    for (int r = ty; r < 32; r += 8) {
        if (ra + r < N && rb + tx < N) P[(size_t)(ra + r) * N + rb + tx] = (A[r][tx] + B[tx][r]) / two_n;
        if (rb + r < N && ra + tx < N) P[(size_t)(rb + r) * N + ra + tx] = (B[r][tx] + A[tx][r]) / two_n;
    }
}

namespace {

template <bool KL>
__device__ __forceinline__ void tsne_pair(float p, f32x2 yi, f32x2 yj, bool self, float ex, f32x2& fa, f32x2& fr, float& z,
                                          float& a, float& s) {
    const f32x2 d = yi - yj;
    const float q = 1.f + fmaf(d.x, d.x, d.y * d.y);
    const float w = self ? 0.f : fast_rcp(q);
    fa = __builtin_elementwise_fma(f32x2{p * w, p * w}, d, fa);
    fr = __builtin_elementwise_fma(f32x2{w * w, w * w}, d, fr);
    z += w;
    if (KL) {
        const float pe = ex * p;
        s += pe;
        if (pe > 0.f) a = fmaf(pe, logf(fmaxf(pe, (float)TSNE_EPS) * q), a);
    }
}

}  // namespace

template <bool KL>
__global__ __launch_bounds__(TSNE_NT) void k_tsne_pairs(const float* __restrict__ P, const float2* __restrict__ Y, int N, int jr,
                                                        float ex, float4* __restrict__ part, float* __restrict__ wgz,
                                                        float* __restrict__ wga, float* __restrict__ wgs) {
    __shared__ float2 ty[TSNE_TJ];
    __shared__ float sh[3][4];
    const int t = threadIdx.x, i = blockIdx.x * TSNE_NT + t;
    const int jbeg = blockIdx.y * jr, jend = min(N, jbeg + jr);
    const bool live = i < N;
    f32x2 yi = {0.f, 0.f};
    if (live) {
        const float2 v = Y[i];
        yi = f32x2{v.x, v.y};
    }
    f32x2 fa = {0.f, 0.f}, fr = {0.f, 0.f};
    float z = 0.f, a = 0.f, s = 0.f;
    for (int j0 = jbeg; j0 < jend; j0 += TSNE_TJ) {
        const int n = min(TSNE_TJ, jend - j0);
        __syncthreads();
        for (int k = t; k < n; k += TSNE_NT) ty[k] = Y[j0 + k];
        __syncthreads();
        if (live) {
            const float* p = P + (size_t)j0 * N + i;       // P[j][i] = P[i][j]: a wave reads 256 contiguous bytes of row j
            int k = 0;
            for (; k + TSNE_UNROLL <= n; k += TSNE_UNROLL) {
                float pv[TSNE_UNROLL];
#pragma unroll
                for (int u = 0; u < TSNE_UNROLL; ++u) pv[u] = p[(size_t)(k + u) * N];
#pragma unroll
                for (int u = 0; u < TSNE_UNROLL; ++u) {
                    const float2 v = ty[k + u];
                    tsne_pair<KL>(pv[u], yi, f32x2{v.x, v.y}, j0 + k + u == i, ex, fa, fr, z, a, s);
                }
            }
            for (; k < n; ++k) {
                const float2 v = ty[k];
                tsne_pair<KL>(p[(size_t)k * N], yi, f32x2{v.x, v.y}, j0 + k == i, ex, fa, fr, z, a, s);
            }
        }
    }
    if (live) part[(size_t)blockIdx.y * N + i] = make_float4(fa.x, fa.y, fr.x, fr.y);
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    z = block_sum(z, sh[0]);
    if (t == 0) wgz[wg] = z;
    if (KL) {
        a = block_sum(a, sh[1]);
        s = block_sum(s, sh[2]);
        if (t == 0) {
            wga[wg] = a;
            wgs[wg] = s;
        }
    }
}

// upd / gains / Y are touched only with do_update; grad_out and kl_out are optional
__global__ __launch_bounds__(TSNE_NT) void k_tsne_finish(const float4* __restrict__ part, const float* __restrict__ wgz,
                                                         const float* __restrict__ wga, const float* __restrict__ wgs, int nwg,
                                                         int N, int splits, float ex, float momentum, float lr, int do_update,
                                                         float2* __restrict__ Y, float2* __restrict__ upd,
                                                         float2* __restrict__ gains, float2* __restrict__ grad_out,
                                                         float* __restrict__ kl_out) {
    __shared__ double sh[3][4];
    const int t = threadIdx.x, i = blockIdx.x * TSNE_NT + t;
    double z = 0.0;
    for (int k = t; k < nwg; k += TSNE_NT) z += (double)wgz[k];
    const double Z = block_sum(z, sh[0]);
    if (kl_out && blockIdx.x == 0) {
        double a = 0.0, s = 0.0;
        for (int k = t; k < nwg; k += TSNE_NT) {
            a += (double)wga[k];
            s += (double)wgs[k];
        }
        a = block_sum(a, sh[1]);
        s = block_sum(s, sh[2]);
        if (t == 0) *kl_out = (float)(a + log(Z) * s);
    }
    if (i >= N) return;
    double ax = 0.0, ay = 0.0, rx = 0.0, ry = 0.0;
    for (int sp = 0; sp < splits; ++sp) {
        const float4 v = part[(size_t)sp * N + i];
        ax += (double)v.x;
        ay += (double)v.y;
        rx += (double)v.z;
        ry += (double)v.w;
    }
    const float g[2] = {(float)(4.0 * ((double)ex * ax - rx / Z)), (float)(4.0 * ((double)ex * ay - ry / Z))};
    if (grad_out) grad_out[i] = make_float2(g[0], g[1]);
    if (!do_update) return;
    const float2 u0 = upd[i], g0 = gains[i], y0 = Y[i];
    float u[2] = {u0.x, u0.y}, gn[2] = {g0.x, g0.y}, y[2] = {y0.x, y0.y};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        gn[c] = fmaxf(u[c] * g[c] < 0.f ? gn[c] + 0.2f : gn[c] * 0.8f, 0.01f);
        u[c] = momentum * u[c] - lr * (gn[c] * g[c]);
        y[c] += u[c];
    }
    upd[i] = make_float2(u[0], u[1]);
    gains[i] = make_float2(gn[0], gn[1]);
    Y[i] = make_float2(y[0], y[1]);
}

__global__ __launch_bounds__(TSNE_NT) void k_tsne_state_init(float2* __restrict__ upd, float2* __restrict__ gains, int N) {
    const int i = blockIdx.x * TSNE_NT + threadIdx.x;
    if (i < N) {
        upd[i] = make_float2(0.f, 0.f);
        gains[i] = make_float2(1.f, 1.f);
    }
}

namespace {

void tsne_pass(const float* P, const float* Y, int N, const TsneGeom& g, const TsneScratch& s, float ex, bool kl, hipStream_t stream) {
    const dim3 grid(g.iblocks, g.splits);
    if (kl)
        k_tsne_pairs<true><<<grid, TSNE_NT, 0, stream>>>(P, (const float2*)Y, N, g.jr, ex, s.part, s.wgz, s.wga, s.wgs);
    else
        k_tsne_pairs<false><<<grid, TSNE_NT, 0, stream>>>(P, (const float2*)Y, N, g.jr, ex, s.part, s.wgz, s.wga, s.wgs);
}

int tsne_dims_ok(int N) { return N >= 4 && N <= T2V_TSNE_MAX_POINTS; }

}  // namespace

extern "C" size_t t2v_tsne_scratch_bytes(int N, int D) {
    if (!tsne_dims_ok(N) || D < 2 || D > TSNE_MAX_D) return 0;
    return 4 * tsne_scratch_floats(N, tsne_geom(N));
}

extern "C" int t2v_tsne_affinities(const float* X, int N, int D, float perplexity, float* P, void* scratch, void* stream_) {
    (void)scratch;      // the conditional rows are written into P and symmetrised in place
    if (!tsne_dims_ok(N) || D < 2 || D > TSNE_MAX_D) return T2V_ERR_DIMS;
    if (!X || !P || !(perplexity > 0.f) || !(3.f * perplexity < (float)N)) return T2V_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute((const void*)k_tsne_cond, hipFuncAttributeMaxDynamicSharedMemorySize,
                                4 * T2V_TSNE_MAX_POINTS) != hipSuccess) {
            const int rc = t2v_check_launch();
            return rc ? rc : T2V_ERR_LAUNCH;
        }
        raised = true;
    }
    k_tsne_cond<<<N, TSNE_NT, 4 * (size_t)((N + 3) / 4 * 4), stream>>>(X, N, D, perplexity, P);
    const int tiles = (N + 31) / 32;
    k_tsne_sym<<<dim3(tiles, tiles), TSNE_NT, 0, stream>>>(P, N);
    return t2v_check_launch();
}

extern "C" int t2v_tsne_gradient(const float* P, const float* Y, int N, float exaggeration, float* grad, float* kl_or_null,
                                 void* scratch, void* stream_) {
    if (!tsne_dims_ok(N)) return T2V_ERR_DIMS;
    if (!P || !Y || !grad || !scratch || !(exaggeration > 0.f)) return T2V_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    const TsneGeom g = tsne_geom(N);
    const TsneScratch s = tsne_carve(scratch, N, g);
    tsne_pass(P, Y, N, g, s, exaggeration, kl_or_null != nullptr, stream);
    k_tsne_finish<<<g.iblocks, TSNE_NT, 0, stream>>>(s.part, s.wgz, s.wga, s.wgs, g.nwg, N, g.splits, exaggeration, 0.f, 0.f, 0,
                                                     nullptr, nullptr, nullptr, (float2*)grad, kl_or_null);
    return t2v_check_launch();
}

extern "C" int t2v_tsne_run(const float* P, float* Y, int N, int n_iter, float learning_rate, float* kl_trace, void* scratch,
                            void* stream_) {
    if (!tsne_dims_ok(N)) return T2V_ERR_DIMS;
    if (!P || !Y || !kl_trace || !scratch || n_iter < 1 || !(learning_rate > 0.f)) return T2V_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    const TsneGeom g = tsne_geom(N);
    const TsneScratch s = tsne_carve(scratch, N, g);
    k_tsne_state_init<<<g.iblocks, TSNE_NT, 0, stream>>>(s.upd, s.gains, N);
    // pass `it` sees the map after `it` updates; the one after the last update only reports the KL divergence
    for (int it = 0; it <= n_iter; ++it) {
        const bool exag = it < TSNE_EXAG_ITERS;
        const float ex = exag ? TSNE_EXAG : 1.f;
        const bool last = it == n_iter;
        float* kl = nullptr;
        if (it > 0 && (last || it % TSNE_KL_EVERY == 0)) kl = kl_trace + (it + TSNE_KL_EVERY - 1) / TSNE_KL_EVERY - 1;
        tsne_pass(P, Y, N, g, s, ex, kl != nullptr, stream);
        k_tsne_finish<<<g.iblocks, TSNE_NT, 0, stream>>>(s.part, s.wgz, s.wga, s.wgs, g.nwg, N, g.splits, ex, exag ? 0.5f : 0.8f,
                                                         learning_rate, last ? 0 : 1, (float2*)Y, s.upd, s.gains, nullptr, kl);
    }
    return t2v_check_launch();
}
