// Length regulator: symbol durations -> the frame-by-frame plan of the planned free-running decode.
// (t2v_hip.duration_plan, Decoder.inference(plan=), Synthesizer.synthesize(durations= / rhythm_from=); include/t2vae.h states
// the measure in full.)
//
//   q_j = llrint((double)dur_j * (double)rate_j * 65536.0), C_j = q_0 + ... + q_j in int64, E_j = (C_j + 32768) >> 16;
//   symbol j owns the frames E_{j-1} <= t < E_j;  n_plan = min(E_last, T_max);  behind n_plan the plan holds its last value.
//
// k_duration_plan: one workgroup of 256 threads per row, in two phases.
//   1. The symbols 256 at a time: thread i takes symbol 256 c + i, the inclusive prefix sum of q is a scan over the 64 lanes
//      of each wave (six shuffles of an int64), the four wave totals meet in LDS and the chunk's total is carried to the next
//      chunk.  E_j, clamped to T_max (the clamp keeps the order and no frame >= T_max is ever looked up), goes to LDS.
//   2. The frames 256 at a time: the symbol of frame t is the first j with E_j > t, a binary search over E in LDS (a symbol
//      with an empty range has E_j = E_{j-1} and is never the first).
// Everything is integer arithmetic on exactly representable products (two 24-bit mantissas, then a power of two), so a row
// gives the same plan alone, in any batch and at any stride.  No atomics, no host round trip.
#include "t2v_common.h"
#include "t2v_kernels.h"

#define PLAN_NT 256
#define PLAN_MAX_FRAMES_PER_SYMBOL 1048576.0      // 2^20: 4096 symbols of it stay far inside int64 in 16.16 fixed point

// first j in [0, L) with E[j] > t; L when there is none
__device__ __forceinline__ int plan_owner(const int32_t* E, int L, int t) {
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (E[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(PLAN_NT) void k_duration_plan(const float* __restrict__ dur, int dur_stride,
                                                           const int32_t* __restrict__ n_ids, const float* __restrict__ rate,
                                                           int rate_stride_b, int rate_stride_j, int S, int T_max,
                                                           int32_t* __restrict__ plan, int plan_stride,
                                                           int32_t* __restrict__ n_plan) {
    __shared__ int32_t E[T2V_PLAN_MAX_SYMBOLS];
    __shared__ long long wtot[PLAN_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = min(max(n_ids[b], 0), S);                                        // no length addresses outside the row
    const float* d = dur + (size_t)b * dur_stride;
    const float* r = rate ? rate + (size_t)b * rate_stride_b : nullptr;
    int32_t* out = plan + (size_t)b * plan_stride;

    long long carry = 0;                                                           // C of the last symbol of the previous chunk
    int bad = 0;
    for (int j0 = 0; j0 < L; j0 += PLAN_NT) {                                      // uniform over the workgroup
        const int j = j0 + tid;
        long long q = 0;
        if (j < L) {
            const double x = (double)d[j] * (r ? (double)r[(size_t)j * rate_stride_j] : 1.0);
            if (!(x >= 0.0) || !(x <= PLAN_MAX_FRAMES_PER_SYMBOL)) bad = 1;        // negative, NaN, inf, too long
            else q = llrint(x * 65536.0);
        }
        long long c = q;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const long long o = __shfl_up(c, m, 64);
            if (lane >= m) c += o;
        }
        if (lane == 63) wtot[wave] = c;
        __syncthreads();
        long long base = carry;
#pragma unroll
        for (int w = 0; w < PLAN_NT / 64; ++w) {
            const long long wt = wtot[w];
            if (w < wave) base += wt;
            carry += wt;
        }
        if (j < L) E[j] = (int32_t)min((base + c + 32768) >> 16, (long long)T_max);
        __syncthreads();                                                           // wtot is rewritten by the next chunk
    }
    bad = __syncthreads_or(bad);                                                   // (also: E complete)
    if (bad) {
        for (int t = tid; t < T_max; t += PLAN_NT) out[t] = 0;
        if (tid == 0) n_plan[b] = -1;
        return;
    }
    const int n = L > 0 ? E[L - 1] : 0;                                            // min(E_last, T_max)
    const int last = n > 0 ? plan_owner(E, L, n - 1) : 0;
    for (int t = tid; t < T_max; t += PLAN_NT) out[t] = t < n ? plan_owner(E, L, t) : last;
    if (tid == 0) n_plan[b] = n;
}

extern "C" int t2v_duration_plan(const float* dur, int dur_stride, const int32_t* n_ids, const float* rate, int rate_stride_b,
                                 int rate_stride_j, int B, int S, int T_max, int32_t* plan, int plan_stride, int32_t* n_plan,
                                 void* stream_) {
    if (!dur || !n_ids || !plan || !n_plan) return T2V_ERR_ARG;
    if (B < 1 || S < 1 || T_max < 1 || dur_stride < S || plan_stride < T_max || rate_stride_b < 0 || rate_stride_j < 0)
        return T2V_ERR_ARG;
    if (S > T2V_PLAN_MAX_SYMBOLS) return T2V_ERR_DIMS;
    k_duration_plan<<<B, PLAN_NT, 0, (hipStream_t)stream_>>>(dur, dur_stride, n_ids, rate, rate_stride_b, rate_stride_j, S,
                                                            T_max, plan, plan_stride, n_plan);
    return t2v_check_launch();
}
