// Frame-aligned scores of prosody transfer: the mel cepstrum of an 80-band log-mel, a DTW over 13 cepstral coefficients that
// keeps its decisions, the warping path walked back through them, and the MCD / F0 sums taken along a path
// (Synthesizer.evaluate(aligned=True)).  The measure is stated in include/t2vae.h.
//
// k_mel_cepstrum: one thread per frame, the 80 log-mel values of the frame read once (coalesced along t), 13 accumulators,
// the table read at wave-uniform addresses.  Each coefficient adds its 80 terms in index order.
//
// k_cep_dtw_fwd: one workgroup of 256 threads per pair.  Thread t keeps rows 8t .. 8t+7 of X in registers (13 x 8 = 104
// VGPRs), so 256 threads cover the 2048 rows of the longest pair in one strip; all of Y's cepstra sit in LDS (13 x 2048 x 4 B),
// loaded once.  At step s thread t works on column j = s - t: 13 LDS reads serve 8 local costs, then 8 cells of the
// recurrence.  Thread t hands D(8t+7, j) to thread t+1 through a double-buffered LDS slot, one workgroup barrier per step.
// Each cell leaves its 2-bit decision (0: from (i-1, j-1), 1: from (i-1, j), 2: from (i, j-1)); a thread's 8 decisions of a
// step are one 16-bit word at dirs[s][t], so a step is one coalesced store.  The step loop runs Ty + (Tx - 1) / 8 times.
//
// k_cep_dtw_back: one workgroup per pair.  s = j + i / 8 never grows along the walk from (Tx-1, Ty-1) to (0, 0), so the
// table is staged in LDS 64 steps at a time by the whole workgroup, and thread 0 walks through the staged words: a bounded
// `for` (Tx + Ty - 1 points at most over the whole kernel, i and j clamped at 0), never a loop on what the table holds.  The
// points collect in LDS in walk order; the workgroup then writes them reversed, start to end, as (i, j) int32 pairs.
//
// k_path_scores: one workgroup per pair, thread t takes the points t, t + 256, ... in order, and every total is a tree over
// the 256 partial sums in LDS.  No float atomics; nothing depends on B or on a stride, so a pair gives the same bits alone
// and in any batch.
#include "t2v_common.h"
#include "t2v_kernels.h"

#define CD_NT 256
#define CD_R 8                          // rows of X per thread
#define CD_YW T2V_DTW_MAX_FRAMES        // LDS row of one coefficient of Y
#define CD_CHUNK 64                     // steps of the table staged at a time by the walk
#define CD_FWD_LDS_FLOATS (T2V_NCEP * CD_YW + 2 * CD_NT)
#define CD_MAX_POINTS (2 * T2V_DTW_MAX_FRAMES - 1)
static_assert(CD_NT * CD_R >= T2V_DTW_MAX_FRAMES, "one strip covers the longest pair");
static_assert(2 * CD_R == 16, "a thread's decisions of one step are one 16-bit word");
static_assert(T2V_DTW_MAX_FRAMES <= 65536, "a path point packs into 2 x 16 bits in LDS");
static_assert(CD_NT % 2 == 0, "a step of the table is whole 32-bit words");

namespace {

__device__ __forceinline__ bool cd_bad_lengths(int Tx, int Ty, int x_stride, int y_stride) {
    return Tx < 1 || Ty < 1 || Tx > x_stride || Ty > y_stride || Tx > T2V_DTW_MAX_FRAMES || Ty > T2V_DTW_MAX_FRAMES;
}

// steps of the forward kernel for a pair: columns 0 .. Ty-1 skewed over the threads 0 .. (Tx-1)/R
__host__ __device__ __forceinline__ int cd_steps(int Tx, int Ty) { return Ty + (Tx - 1) / CD_R; }

// ||x_i - y_j||_2 from the differences, coefficients in index order (the forward kernel's arithmetic)
__device__ __forceinline__ float cd_cost(const float* __restrict__ Xb, int x_stride, int i, const float* __restrict__ Yb,
                                         int y_stride, int j) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < T2V_NCEP; ++c) {
        const float df = Xb[(size_t)c * x_stride + i] - Yb[(size_t)c * y_stride + j];
        a = fmaf(df, df, a);
    }
    return sqrtf(a);
}

// the sum of v over the workgroup, the same in every thread: a tree in LDS whose order depends on the thread index alone
template <class T>
__device__ __forceinline__ T cd_block_sum(T v, T* buf, int t) {
    __syncthreads();                    // the previous total has been read by everyone
    buf[t] = v;
    __syncthreads();
#pragma unroll
    for (int off = CD_NT / 2; off >= 1; off >>= 1) {
        if (t < off) buf[t] += buf[t + off];
        __syncthreads();
    }
    return buf[0];
}

}  // namespace

__global__ __launch_bounds__(CD_NT) void k_mel_cepstrum(const float* __restrict__ M, const int32_t* __restrict__ n, int m_stride,
                                                        const float* __restrict__ table, float* __restrict__ out, int out_stride) {
    const int b = blockIdx.y, t = blockIdx.x * CD_NT + threadIdx.x;
    if (t >= out_stride) return;
    float* ob = out + (size_t)b * T2V_NCEP * out_stride;
    const int len = min(max(n[b], 0), m_stride);
    if (t >= len) {
#pragma unroll
        for (int k = 0; k < T2V_NCEP; ++k) ob[(size_t)k * out_stride + t] = 0.f;
        return;
    }
    const float* Mb = M + (size_t)b * T2V_NMEL * m_stride + t;
    float acc[T2V_NCEP];
#pragma unroll
    for (int k = 0; k < T2V_NCEP; ++k) acc[k] = 0.f;
    for (int c = 0; c < T2V_NMEL; ++c) {
        const float m = Mb[(size_t)c * m_stride];
#pragma unroll
        for (int k = 0; k < T2V_NCEP; ++k) acc[k] = fmaf(table[k * T2V_NMEL + c], m, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < T2V_NCEP; ++k) ob[(size_t)k * out_stride + t] = acc[k];
}

__global__ __launch_bounds__(CD_NT) void k_cep_dtw_fwd(const float* __restrict__ X, const int32_t* __restrict__ nx, int x_stride,
                                                       const float* __restrict__ Y, const int32_t* __restrict__ ny, int y_stride,
                                                       float* __restrict__ dist, uint16_t* __restrict__ dirs, int max_steps) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ylds = lds;                              // [13][CD_YW]: coefficient c of y_j at ylds[c * CD_YW + j]
    float* hand = lds + T2V_NCEP * CD_YW;           // [2][NT]: D(8t+7, j) of thread t's last step
    const int b = blockIdx.x, t = threadIdx.x;
    const int Tx = nx[b], Ty = ny[b];
    // the host checks the lengths; a pair that got past it is refused here before any array is touched and before any barrier
    if (cd_bad_lengths(Tx, Ty, x_stride, y_stride) || cd_steps(Tx, Ty) > max_steps) {
        if (t == 0) dist[b] = __builtin_nanf("");
        return;
    }
    const float* Xb = X + (size_t)b * T2V_NCEP * x_stride;
    const float* Yb = Y + (size_t)b * T2V_NCEP * y_stride;
    uint16_t* dir = dirs + (size_t)b * max_steps * CD_NT;
    const float inf = __builtin_inff();
    const int t_last = (Tx - 1) / CD_R, r_last = (Tx - 1) % CD_R;
    const int n_steps = cd_steps(Tx, Ty);

#pragma unroll
    for (int c = 0; c < T2V_NCEP; ++c)
        for (int j = t; j < Ty; j += CD_NT) ylds[c * CD_YW + j] = Yb[(size_t)c * y_stride + j];
    // rows past Tx hold zeros: they sit below every real row of their thread and feed nothing
    float x[T2V_NCEP][CD_R];
    const int i0 = CD_R * t;
#pragma unroll
    for (int c = 0; c < T2V_NCEP; ++c)
#pragma unroll
        for (int r = 0; r < CD_R; ++r) x[c][r] = i0 + r < Tx ? Xb[(size_t)c * x_stride + i0 + r] : 0.f;
    float left[CD_R];                               // D(i0 + r, j - 1)
#pragma unroll
    for (int r = 0; r < CD_R; ++r) left[r] = inf;
    float upleft = t == 0 ? 0.f : inf;              // D(i0 - 1, j - 1); the virtual D(-1, -1) = 0 makes D(0, 0) = 2 d
    __syncthreads();

    for (int s = 0; s < n_steps; ++s) {
        const int j = s - t;
        if (t <= t_last && j >= 0 && j < Ty) {
            float a[CD_R];
#pragma unroll
            for (int r = 0; r < CD_R; ++r) a[r] = 0.f;
#pragma unroll
            for (int c = 0; c < T2V_NCEP; ++c) {
                const float y = ylds[c * CD_YW + j];
#pragma unroll
                for (int r = 0; r < CD_R; ++r) {
                    const float df = x[c][r] - y;
                    a[r] = fmaf(df, df, a[r]);
                }
            }
            const float up = t == 0 ? inf : hand[((s - 1) & 1) * CD_NT + t - 1];        // D(i0 - 1, j)
            float u = up, ul = upleft;
            uint32_t word = 0;
#pragma unroll
            for (int r = 0; r < CD_R; ++r) {
                const float d = sqrtf(a[r]);
                float best = ul + 2.f * d;          // ties: the diagonal, then (i-1, j), then (i, j-1)
                uint32_t from = 0;
                const float cu = u + d, cl = left[r] + d;
                if (cu < best) { best = cu; from = 1; }
                if (cl < best) { best = cl; from = 2; }
                ul = left[r];
                left[r] = best;
                u = best;
                word |= from << (2 * r);
            }
            upleft = up;
            hand[(s & 1) * CD_NT + t] = left[CD_R - 1];
            dir[(size_t)s * CD_NT + t] = (uint16_t)word;
            if (t == t_last && j == Ty - 1) {
                float bottom = left[0];
#pragma unroll
                for (int r = 1; r < CD_R; ++r) bottom = r == r_last ? left[r] : bottom;
                dist[b] = bottom / (float)(Tx + Ty);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(CD_NT) void k_cep_dtw_back(const int32_t* __restrict__ nx, int x_stride, const int32_t* __restrict__ ny,
                                                        int y_stride, const uint16_t* __restrict__ dirs, int max_steps,
                                                        int32_t* __restrict__ K, int32_t* __restrict__ path, int path_stride) {
    __shared__ uint32_t stage[CD_CHUNK * CD_NT / 2];        // the decision words of up to 64 steps, as they lie in memory
    __shared__ uint32_t pts[CD_MAX_POINTS];                 // (i << 16) | j in walk order, end first
    __shared__ int n_pts;
    const int b = blockIdx.x, t = threadIdx.x;
    const int Tx = nx[b], Ty = ny[b];
    if (cd_bad_lengths(Tx, Ty, x_stride, y_stride) || cd_steps(Tx, Ty) > max_steps || Tx + Ty - 1 > path_stride) {
        if (t == 0) K[b] = 0;
        return;
    }
    const uint32_t* dir32 = (const uint32_t*)(dirs + (size_t)b * max_steps * CD_NT);
    const uint16_t* stage16 = (const uint16_t*)stage;
    const int words_used = (Tx - 1) / CD_R / 2 + 1;         // 32-bit words of a step that hold a thread of this pair
    const int n_steps = cd_steps(Tx, Ty);
    int i = Tx - 1, j = Ty - 1, n = 0, left_to_go = Tx + Ty - 1;
    bool done = false;
    for (int s_hi = n_steps - 1; s_hi >= 0; s_hi -= CD_CHUNK) {
        const int s_lo = max(s_hi - CD_CHUNK + 1, 0);
        const int n_words = (s_hi - s_lo + 1) * (CD_NT / 2);
        for (int w = t; w < n_words; w += CD_NT)
            if (w % (CD_NT / 2) < words_used) stage[w] = dir32[(size_t)s_lo * (CD_NT / 2) + w];
        __syncthreads();
        if (t == 0 && !done) {
            for (; left_to_go > 0; --left_to_go) {
                const int s = j + i / CD_R;
                if (s < s_lo) break;                        // the next chunk holds it
                pts[n++] = (uint32_t)i << 16 | (uint32_t)j;
                if (i == 0 && j == 0) { done = true; break; }
                const uint32_t from = stage16[(s - s_lo) * CD_NT + i / CD_R] >> (2 * (i % CD_R)) & 3u;
                i = max(i - (from != 2u ? 1 : 0), 0);
                j = max(j - (from != 1u ? 1 : 0), 0);
            }
        }
        __syncthreads();
    }
    if (t == 0) n_pts = n;
    __syncthreads();
    const int k = n_pts;
    int32_t* pb = path + (size_t)b * 2 * path_stride;
    for (int p = t; p < k; p += CD_NT) {
        const uint32_t v = pts[k - 1 - p];
        pb[2 * p] = (int32_t)(v >> 16);
        pb[2 * p + 1] = (int32_t)(v & 0xffffu);
    }
    if (t == 0) K[b] = k;
}

__global__ __launch_bounds__(CD_NT) void k_path_scores(const int32_t* __restrict__ path, const int32_t* __restrict__ K, int path_stride,
                                                       const float* __restrict__ X, const int32_t* __restrict__ nx, int x_stride,
                                                       const float* __restrict__ Y, const int32_t* __restrict__ ny, int y_stride,
                                                       const float* __restrict__ fx, int fx_stride, const float* __restrict__ fy,
                                                       int fy_stride, int32_t* __restrict__ counts, float* __restrict__ sums) {
    __shared__ float fbuf[CD_NT];
    __shared__ int ibuf[CD_NT];
    const int b = blockIdx.x, t = threadIdx.x;
    const int Tx = nx[b], Ty = ny[b], k = K[b];
    int32_t* cb = counts + (size_t)b * T2V_ALIGNED_COUNTS;
    float* sb = sums + (size_t)b * T2V_ALIGNED_SUMS;
    if (cd_bad_lengths(Tx, Ty, x_stride, y_stride) || k < 1 || k > path_stride || (fx && Tx > fx_stride) || (fy && Ty > fy_stride)) {
        if (t < T2V_ALIGNED_COUNTS) cb[t] = 0;
        if (t < T2V_ALIGNED_SUMS) sb[t] = __builtin_nanf("");
        return;
    }
    const float* Xb = X + (size_t)b * T2V_NCEP * x_stride;
    const float* Yb = Y + (size_t)b * T2V_NCEP * y_stride;
    const float* fxb = fx ? fx + (size_t)b * fx_stride : nullptr;
    const float* fyb = fy ? fy + (size_t)b * fy_stride : nullptr;
    const int32_t* pb = path + (size_t)b * 2 * path_stride;
    const float wx = (float)max(Tx - 1, 1), wy = (float)max(Ty - 1, 1);

    int n_both = 0, n_vde = 0, n_gpe = 0;
    float s_d = 0.f, s_e = 0.f, s_e2 = 0.f, s_lx = 0.f, s_ly = 0.f, s_w = 0.f;
    for (int p = t; p < k; p += CD_NT) {
        const int i = min(max(pb[2 * p], 0), Tx - 1), j = min(max(pb[2 * p + 1], 0), Ty - 1);      // a foreign path addresses nothing outside
        s_d += cd_cost(Xb, x_stride, i, Yb, y_stride, j);
        s_w += fabsf((float)i / wx - (float)j / wy);
        const float a = fxb ? fxb[i] : 0.f, c = fyb ? fyb[j] : 0.f;
        const bool va = a > 0.f, vc = c > 0.f;
        if (va && vc) {
            ++n_both;
            n_gpe += fabsf(a - c) > 0.2f * c ? 1 : 0;
            const float e = 1200.f * log2f(a / c);
            s_e += e;
            s_e2 = fmaf(e, e, s_e2);
            s_lx += log2f(a);
            s_ly += log2f(c);
        } else if (va != vc) {
            ++n_vde;
        }
    }
    n_both = cd_block_sum(n_both, ibuf, t);
    n_vde = cd_block_sum(n_vde, ibuf, t);
    n_gpe = cd_block_sum(n_gpe, ibuf, t);
    s_d = cd_block_sum(s_d, fbuf, t);
    s_e = cd_block_sum(s_e, fbuf, t);
    s_e2 = cd_block_sum(s_e2, fbuf, t);
    s_lx = cd_block_sum(s_lx, fbuf, t);
    s_ly = cd_block_sum(s_ly, fbuf, t);
    s_w = cd_block_sum(s_w, fbuf, t);

    // second pass: the centred second moments of (log2 fx, log2 fy) around the means of the first
    float s_xx = 0.f, s_yy = 0.f, s_xy = 0.f;
    if (n_both > 0) {
        const float mx = s_lx / (float)n_both, my = s_ly / (float)n_both;
        for (int p = t; p < k; p += CD_NT) {
            const int i = min(max(pb[2 * p], 0), Tx - 1), j = min(max(pb[2 * p + 1], 0), Ty - 1);
            const float a = fxb ? fxb[i] : 0.f, c = fyb ? fyb[j] : 0.f;
            if (a > 0.f && c > 0.f) {
                const float dx = log2f(a) - mx, dy = log2f(c) - my;
                s_xx = fmaf(dx, dx, s_xx);
                s_yy = fmaf(dy, dy, s_yy);
                s_xy = fmaf(dx, dy, s_xy);
            }
        }
    }
    s_xx = cd_block_sum(s_xx, fbuf, t);
    s_yy = cd_block_sum(s_yy, fbuf, t);
    s_xy = cd_block_sum(s_xy, fbuf, t);
    if (t == 0) {
        cb[0] = k; cb[1] = n_both; cb[2] = n_vde; cb[3] = n_gpe;
        sb[0] = s_d; sb[1] = s_e; sb[2] = s_e2; sb[3] = s_xx; sb[4] = s_yy; sb[5] = s_xy; sb[6] = s_w; sb[7] = 0.f;
    }
}

extern "C" int t2v_mel_cepstrum(const float* M, const int32_t* n, int m_stride, int B, int n_mel, int n_cep, const float* table,
                                float* out, int out_stride, void* stream_) {
    if (n_mel != T2V_NMEL || n_cep != T2V_NCEP) return T2V_ERR_DIMS;
    if (!M || !n || !table || !out || B < 1 || B > 65535 || m_stride < 1 || out_stride < 1) return T2V_ERR_ARG;
    k_mel_cepstrum<<<dim3((out_stride + CD_NT - 1) / CD_NT, B), CD_NT, 0, (hipStream_t)stream_>>>(M, n, m_stride, table, out,
                                                                                                 out_stride);
    return t2v_check_launch();
}

static int cd_max_steps(int tx_max, int ty_max) {
    const int tx = tx_max < T2V_DTW_MAX_FRAMES ? tx_max : T2V_DTW_MAX_FRAMES, ty = ty_max < T2V_DTW_MAX_FRAMES ? ty_max : T2V_DTW_MAX_FRAMES;
    return cd_steps(tx, ty);
}

extern "C" size_t t2v_cep_dtw_scratch_bytes(int B, int tx_max, int ty_max) {
    if (B < 1 || tx_max < 1 || ty_max < 1) return 0;
    return (size_t)B * cd_max_steps(tx_max, ty_max) * CD_NT * sizeof(uint16_t);
}

extern "C" int t2v_cep_dtw_forward(const float* X, const int32_t* nx, int x_stride, const float* Y, const int32_t* ny, int y_stride,
                                   int B, int n_cep, float* dist, void* scratch, void* stream_) {
    if (n_cep != T2V_NCEP) return T2V_ERR_DIMS;
    if (!X || !nx || !Y || !ny || !dist || !scratch || B < 1 || x_stride < 1 || y_stride < 1) return T2V_ERR_ARG;
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute((const void*)k_cep_dtw_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * CD_FWD_LDS_FLOATS) !=
            hipSuccess) {
            const int rc = t2v_check_launch();
            return rc ? rc : T2V_ERR_LAUNCH;
        }
        raised = true;
    }
    k_cep_dtw_fwd<<<B, CD_NT, 4 * CD_FWD_LDS_FLOATS, (hipStream_t)stream_>>>(X, nx, x_stride, Y, ny, y_stride, dist, (uint16_t*)scratch,
                                                                             cd_max_steps(x_stride, y_stride));
    return t2v_check_launch();
}

extern "C" int t2v_cep_dtw_walk(const int32_t* nx, int x_stride, const int32_t* ny, int y_stride, int B, const void* scratch,
                                int32_t* K, int32_t* path, int path_stride, void* stream_) {
    if (!nx || !ny || !scratch || !K || !path || B < 1 || x_stride < 1 || y_stride < 1 || path_stride < 1) return T2V_ERR_ARG;
    k_cep_dtw_back<<<B, CD_NT, 0, (hipStream_t)stream_>>>(nx, x_stride, ny, y_stride, (const uint16_t*)scratch,
                                                          cd_max_steps(x_stride, y_stride), K, path, path_stride);
    return t2v_check_launch();
}

extern "C" int t2v_cep_dtw_path(const float* X, const int32_t* nx, int x_stride, const float* Y, const int32_t* ny, int y_stride,
                                int B, int n_cep, float* dist, int32_t* K, int32_t* path, int path_stride, void* scratch,
                                void* stream_) {
    if (n_cep != T2V_NCEP) return T2V_ERR_DIMS;
    if (!K || !path || path_stride < 1) return T2V_ERR_ARG;
    const int rc = t2v_cep_dtw_forward(X, nx, x_stride, Y, ny, y_stride, B, n_cep, dist, scratch, stream_);
    return rc ? rc : t2v_cep_dtw_walk(nx, x_stride, ny, y_stride, B, scratch, K, path, path_stride, stream_);
}

extern "C" int t2v_path_scores(const int32_t* path, const int32_t* K, int path_stride, const float* X, const int32_t* nx, int x_stride,
                               const float* Y, const int32_t* ny, int y_stride, const float* fx, int fx_stride, const float* fy,
                               int fy_stride, int B, int n_cep, int32_t* counts, float* sums, void* stream_) {
    if (n_cep != T2V_NCEP) return T2V_ERR_DIMS;
    if (!path || !K || !X || !nx || !Y || !ny || !counts || !sums || B < 1 || path_stride < 1 || x_stride < 1 || y_stride < 1 ||
        (fx && fx_stride < 1) || (fy && fy_stride < 1))
        return T2V_ERR_ARG;
    k_path_scores<<<B, CD_NT, 0, (hipStream_t)stream_>>>(path, K, path_stride, X, nx, x_stride, Y, ny, y_stride, fx, fx_stride, fy,
                                                         fy_stride, counts, sums);
    return t2v_check_launch();
}
