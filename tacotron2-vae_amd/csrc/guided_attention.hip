// Guided attention loss (Tachibana et al., DCTTS; ESPnet's GuidedAttentionLoss for Tacotron 2): a penalty on attention weight far
// from the diagonal, value and gradient from one read of the alignments.
//   W[b][t][j] = 1 - exp(-(j / N_b - t / T_b)^2 / (2 sigma^2))   for t < T_b and j < N_b, else 0
//   D = sum_b T_b N_b,   L = sum A W / D,   dL/dA = W / D
// k_guided_rows: one workgroup per (t, b) row reads the row of A in the strides it has, writes the row of W / D in (T, B, T_in)
// storage — what the reverse passes of the decoder take as dAL without a copy — and one fp64 partial of sum A W.
// k_guided_sum: one workgroup adds the T B partials and writes L.  Products are fp32, every sum is fp64 in an order fixed by the
// shapes (strided per thread, then a tree), so L has the same bits from run to run.  D comes from the two length vectors on the
// device: nothing is read back, and both launches can be captured in a graph.
#include "t2v_common.h"
#include "t2v_kernels.h"

#define GA_THREADS 256

__device__ __forceinline__ long long ga_len(const int64_t* p, int b, int cap) {
    const long long v = (long long)p[b];
    return v < 0 ? 0 : v > cap ? cap : v;
}
// D, the same in every thread of every workgroup (integer sum: no order to fix)
__device__ __forceinline__ double ga_denominator(const int64_t* in_len, const int64_t* out_len, int B, int T, int T_in) {
    long long d = 0;
    for (int b = 0; b < B; ++b) d += ga_len(in_len, b, T_in) * ga_len(out_len, b, T);
    return (double)d;
}
// the sum of the workgroup's 256 per-thread values, in tree order, in red[0]
__device__ __forceinline__ void ga_tree_sum(double* red, double v) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int w = GA_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
}

__global__ __launch_bounds__(GA_THREADS) void k_guided_rows(const float* __restrict__ A, long sb, long st, long sj,
                                                            const int64_t* __restrict__ in_len, const int64_t* __restrict__ out_len,
                                                            float* __restrict__ G, double* __restrict__ part, int B, int T, int T_in,
                                                            float sigma) {
    __shared__ double red[GA_THREADS];
    const int row = blockIdx.x, t = row / B, b = row % B, tid = threadIdx.x;
    const int N = (int)ga_len(in_len, b, T_in), Tb = (int)ga_len(out_len, b, T);
    const float Df = (float)ga_denominator(in_len, out_len, B, T, T_in);
    const float* arow = A + (long)b * sb + (long)t * st;
    float* grow = G + ((size_t)t * B + b) * T_in;
    const bool live = t < Tb;
    const float tf = live ? (float)t / (float)Tb : 0.f;
    const float den = 2.f * sigma * sigma;
    double acc = 0.0;
    for (int j = tid; j < T_in; j += GA_THREADS) {
        float g = 0.f;
        if (live && j < N) {
            const float x = (float)j / (float)N - tf;
            const float w = 1.f - expf(-(x * x) / den);
            acc += (double)(arow[(long)j * sj] * w);
            g = w / Df;
        }
        grow[j] = g;
    }
    ga_tree_sum(red, acc);
    if (tid == 0) part[row] = red[0];
}

__global__ __launch_bounds__(GA_THREADS) void k_guided_sum(const double* __restrict__ part, const int64_t* __restrict__ in_len,
                                                           const int64_t* __restrict__ out_len, float* __restrict__ loss, int B, int T,
                                                           int T_in) {
    __shared__ double red[GA_THREADS];
    const int n = T * B;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += GA_THREADS) acc += part[i];
    ga_tree_sum(red, acc);
    if (threadIdx.x == 0) {
        const double D = ga_denominator(in_len, out_len, B, T, T_in);
        loss[0] = D > 0.0 ? (float)(red[0] / D) : 0.f;
    }
}

extern "C" long t2v_guided_attention_part_doubles(int B, int T) { return B < 1 || T < 1 ? 0 : (long)B * T; }

extern "C" int t2v_guided_attention(const float* A, long sb, long st, long sj, const int64_t* in_len, const int64_t* out_len,
                                    float* loss, float* G, double* part, int B, int T, int T_in, float sigma, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!A || !in_len || !out_len || !loss || !G || !part || B < 1 || T < 1 || T_in < 1 || !(sigma > 0.f)) return T2V_ERR_ARG;
    if (sb < 0 || st < 0 || sj < 0 || (long long)T * B > 0x7fffffffll) return T2V_ERR_ARG;
    k_guided_rows<<<(unsigned)(T * B), GA_THREADS, 0, stream>>>(A, sb, st, sj, in_len, out_len, G, part, B, T, T_in, sigma);
    k_guided_sum<<<1, GA_THREADS, 0, stream>>>(part, in_len, out_len, loss, B, T, T_in);
    return t2v_check_launch();
}
