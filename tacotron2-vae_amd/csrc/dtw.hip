// Mel-spectral distortion with dynamic time warping: the distance between two log-mels of different lengths, for scoring
// free-running synthesis against its ground truth (Synthesizer.evaluate).
//
// Measure (X: 80 x Tx, Y: 80 x Ty):  d(i, j) = ||x_i - y_j||_2 from the differences;  Sakoe-Chiba "symmetric2", no band:
//   D(0, 0) = 2 d(0, 0),   D(i, j) = min(D(i-1, j) + d, D(i, j-1) + d, D(i-1, j-1) + 2 d);   dist = D(Tx-1, Ty-1) / (Tx + Ty).
// Every path has total weight Tx + Ty, so the normalisation needs no back-tracking and no stored matrix.
//
// k_mel_dtw: one workgroup of 256 threads per pair, one launch per batch.  X is cut into strips of at most 512 rows; in a
// strip thread t keeps rows 2t, 2t+1 of X in registers (160 VGPRs) and at step s works on column j = s - t: one y_j read
// from LDS serves two local costs (packed fp32 subtract / fma, two accumulators per row), then two cells of the recurrence.
// Thread t hands D(2t+1, j) to thread t+1 through a double-buffered LDS slot, one workgroup barrier per step.  (Four rows
// per thread halve the steps but need 320 VGPRs for X alone: the compiler spilled 210 of them.)  Y streams
// through an LDS ring of 320 columns (256 in use by the skewed threads + the 64 of the chunk being fetched): every 64 steps
// the next 64 columns are loaded into registers while the steps run, and stored when the chunk ends.  The last row of a strip
// goes to the caller's scratch (Ty floats per pair) and comes back as the row above the next strip, 64 columns per chunk;
// column j of it is written only after it was fetched, so one row per pair is enough.  No float atomics and nothing depends
// on B or blockIdx beyond the pair's own pointers: a pair gives the same bits alone and in any batch.
#include "t2v_common.h"
#include "t2v_kernels.h"

#define DTW_NT 256
#define DTW_R 2
#define DTW_STRIP (DTW_NT * DTW_R)
#define DTW_C 64                        // steps per chunk = Y columns fetched per chunk
#define DTW_W (DTW_NT + DTW_C)          // ring columns
#define DTW_PRE (T2V_NMEL * DTW_C / DTW_NT)
#define DTW_LDS_FLOATS (T2V_NMEL * DTW_W + 2 * DTW_NT + DTW_C)
static_assert(DTW_W % 64 == 0, "64 skewed lanes read 64 distinct banks across the ring's wrap");
static_assert(T2V_NMEL * DTW_C % DTW_NT == 0 && DTW_C <= DTW_NT, "chunk fetch: whole rounds of the workgroup");
static_assert(T2V_DTW_MAX_FRAMES % DTW_R == 0, "strip rows are rounded up to whole threads");

typedef float f2 __attribute__((ext_vector_type(2)));

namespace {

// the chunk of Y columns [s0, s0 + 64) and of the row above the strip: global -> registers (nothing at or past Ty is read)
__device__ __forceinline__ void chunk_fetch(const float* Yb, int y_stride, int Ty, const float* above, int s0, int t,
                                            float* pre, float& pre_top) {
#pragma unroll
    for (int k = 0; k < DTW_PRE; ++k) {
        const int idx = t + k * DTW_NT, c = idx / DTW_C, j = s0 + idx % DTW_C;
        pre[k] = j < Ty ? Yb[(size_t)c * y_stride + j] : 0.f;
    }
    pre_top = __builtin_inff();
    if (above && t < DTW_C && s0 + t < Ty) pre_top = above[s0 + t];
}

__device__ __forceinline__ void chunk_store(float* ring, float* top, int s0, int t, const float* pre, float pre_top) {
#pragma unroll
    for (int k = 0; k < DTW_PRE; ++k) {
        const int idx = t + k * DTW_NT, c = idx / DTW_C, j = s0 + idx % DTW_C;
        ring[c * DTW_W + j % DTW_W] = pre[k];
    }
    if (t < DTW_C) top[t] = pre_top;
}

}  // namespace

__global__ __launch_bounds__(DTW_NT) void k_mel_dtw(const float* __restrict__ X, const int32_t* __restrict__ nx, int x_stride,
                                                    const float* __restrict__ Y, const int32_t* __restrict__ ny, int y_stride,
                                                    float* __restrict__ dist, float* __restrict__ rows, int row_stride) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ring = lds;                              // [80][DTW_W]: y_j[c] at ring[c * W + j % W]
    float* hand = lds + T2V_NMEL * DTW_W;           // [2][NT]: D(2t+1, j) of thread t's last step
    float* top = hand + 2 * DTW_NT;                 // [C]: D(row0 - 1, s0 + k), the row above the strip
    const int b = blockIdx.x, t = threadIdx.x;
    const int Tx = nx[b], Ty = ny[b];
    // the host checks the lengths; a pair that got past it is refused here before any array is touched
    if (Tx < 1 || Ty < 1 || Tx > x_stride || Ty > y_stride || Tx > T2V_DTW_MAX_FRAMES || Ty > T2V_DTW_MAX_FRAMES || Ty > row_stride) {
        if (t == 0) dist[b] = __builtin_nanf("");
        return;
    }
    const float* Xb = X + (size_t)b * T2V_NMEL * x_stride;
    const float* Yb = Y + (size_t)b * T2V_NMEL * y_stride;
    float* row = rows + (size_t)b * row_stride;
    const float inf = __builtin_inff();
    const int nstrips = (Tx + DTW_STRIP - 1) / DTW_STRIP;
    const int strip_rows = ((Tx + nstrips - 1) / nstrips + DTW_R - 1) / DTW_R * DTW_R;     // balanced, whole threads

    for (int strip = 0; strip < nstrips; ++strip) {
        const int row0 = strip * strip_rows;
        const int n_rows = min(strip_rows, Tx - row0);
        const int t_last = (n_rows - 1) / DTW_R, r_last = (n_rows - 1) % DTW_R;
        const bool last_strip = strip == nstrips - 1;
        const float* above = strip ? row : nullptr;
        // rows past Tx hold zeros: they sit below every real row of their thread and feed nothing
        f2 xa[T2V_NMEL];
        if (t <= t_last) {
            const int i0 = row0 + DTW_R * t;
#pragma unroll
            for (int c = 0; c < T2V_NMEL; ++c) {
                const float* xc = Xb + (size_t)c * x_stride + i0;
                xa[c] = f2{xc[0], i0 + 1 < Tx ? xc[1] : 0.f};
            }
        } else {
#pragma unroll
            for (int c = 0; c < T2V_NMEL; ++c) xa[c] = f2{0.f, 0.f};
        }
        float left[DTW_R] = {inf, inf};               // D(i0 + r, j - 1)
        float upleft = strip == 0 && t == 0 ? 0.f : inf;        // D(i0 - 1, j - 1); the virtual D(-1, -1) = 0 makes D(0, 0) = 2 d
        int p = 0;                                              // j % DTW_W of this thread's next column
        const int n_steps = Ty + t_last;

        float pre[DTW_PRE], pre_top;
        chunk_fetch(Yb, y_stride, Ty, above, 0, t, pre, pre_top);
        chunk_store(ring, top, 0, t, pre, pre_top);
        __syncthreads();
        for (int s0 = 0; s0 < n_steps; s0 += DTW_C) {
            const bool more = s0 + DTW_C < n_steps;
            if (more) chunk_fetch(Yb, y_stride, Ty, above, s0 + DTW_C, t, pre, pre_top);
            const int s1 = min(s0 + DTW_C, n_steps);
            for (int s = s0; s < s1; ++s) {
                const int j = s - t;
                if (t <= t_last && j >= 0 && j < Ty) {
                    f2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
                    const float* yp = ring + p;
#pragma unroll
                    for (int c = 0; c < T2V_NMEL; c += 2) {
                        const float y0 = yp[c * DTW_W], y1 = yp[(c + 1) * DTW_W];
                        const f2 da0 = xa[c] - y0, da1 = xa[c + 1] - y1;
                        a0 = __builtin_elementwise_fma(da0, da0, a0);
                        a1 = __builtin_elementwise_fma(da1, da1, a1);
                    }
                    const f2 sa = a0 + a1;
                    const float d[DTW_R] = {sqrtf(sa.x), sqrtf(sa.y)};
                    const float up = t == 0 ? top[s - s0] : hand[((s - 1) & 1) * DTW_NT + t - 1];     // D(i0 - 1, j)
                    float u = up, ul = upleft;
#pragma unroll
                    for (int r = 0; r < DTW_R; ++r) {
                        const float nd = fminf(fminf(u, left[r]) + d[r], ul + 2.f * d[r]);
                        ul = left[r];
                        left[r] = nd;
                        u = nd;
                    }
                    upleft = up;
                    hand[(s & 1) * DTW_NT + t] = left[DTW_R - 1];
                    if (t == t_last) {
                        const float bottom = r_last == 0 ? left[0] : left[1];
                        if (!last_strip) row[j] = bottom;
                        else if (j == Ty - 1) dist[b] = bottom / (float)(Tx + Ty);
                    }
                    p = p + 1 == DTW_W ? 0 : p + 1;
                }
                __syncthreads();
            }
            if (more) {
                chunk_store(ring, top, s0 + DTW_C, t, pre, pre_top);
                __syncthreads();
            }
        }
        __threadfence_block();      // the strip's last row: written by one thread, fetched by others in the next strip
        __syncthreads();
    }
}

extern "C" size_t t2v_mel_dtw_scratch_bytes(int B, int tx_max, int ty_max) {
    (void)tx_max;
    if (B < 1 || ty_max < 1) return 0;
    const size_t row = ((size_t)(ty_max < T2V_DTW_MAX_FRAMES ? ty_max : T2V_DTW_MAX_FRAMES) + 63) / 64 * 64;
    return 4 * (size_t)B * row;
}

extern "C" int t2v_mel_dtw(const float* X, const int32_t* nx, int x_stride, const float* Y, const int32_t* ny, int y_stride,
                           int B, int n_mel, float* dist, void* scratch, void* stream_) {
    if (n_mel != T2V_NMEL) return T2V_ERR_DIMS;
    if (!X || !nx || !Y || !ny || !dist || !scratch || B < 1 || x_stride < 1 || y_stride < 1) return T2V_ERR_ARG;
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute((const void*)k_mel_dtw, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * DTW_LDS_FLOATS) !=
            hipSuccess) {
            const int rc = t2v_check_launch();
            return rc ? rc : T2V_ERR_LAUNCH;
        }
        raised = true;
    }
    const int row_stride = (int)(t2v_mel_dtw_scratch_bytes(1, x_stride, y_stride) / 4);
    k_mel_dtw<<<B, DTW_NT, 4 * DTW_LDS_FLOATS, (hipStream_t)stream_>>>(X, nx, x_stride, Y, ny, y_stride, dist, (float*)scratch,
                                                                       row_stride);
    return t2v_check_launch();
}
