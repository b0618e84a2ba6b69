// Attention alignment statistics: did the decoder read the sentence?  (Synthesizer.evaluate(alignment=True),
// Synthesizer.alignment, t2v_hip.alignment_stats.)
//
// Measure (row b: A[b, t < n, j < L], nothing else is read; p[t] = the lowest j < L that maximises A[b, t, j]):
//   path[t] = p[t];  mass[j] = sum_{t<n} A[b, t, j];  focus = (1/n) sum_t A[b, t, p[t]];
//   stats = furthest (max_t p[t]), p_last (p[n-1]), n_back (#{t >= 1: p[t] < p[t-1]}), n_jump (#{t >= 1: p[t] - p[t-1] >
//   max_jump}), longest_stall (longest run of equal consecutive p, in frames), n_uncovered (#{j < L: mass_j < cover_min}),
//   longest_gap (longest run of consecutive uncovered j), 0.
//
// k_align_scan: B x ceil(N / 16) workgroups of 256 threads, the one pass over A.  A workgroup owns AL_F = 16 consecutive
// frames of one row; thread i owns the columns i, i + 256, ...: per column it loads the 16 frames' values (a wave reads 256
// contiguous bytes of each frame), adds them in ascending t into the column's block partial and keeps, per frame, the largest
// value seen and its column (strictly larger only: the lowest column wins).  The per-frame (max, argmax) of the 256 threads
// is a shuffle butterfly in each wave (larger value, then lower column) and a four-way pick through LDS; the path is stored,
// and the frames' maxima are added in ascending t into the block's focus partial.
// k_align_finish: one workgroup per row.  mass_j = the block partials of column j in ascending block order, focus = the focus
// partials in ascending block order over n: no floating-point atomics, and the order of every sum depends on (t, j) alone,
// so a row gives the same bits alone, in any batch, at any stride and with any padding.  The run lengths are the longest run
// of ones in the flags (p[t] == p[t-1]) and (mass_j < cover_min): thread i summarises a contiguous piece as (length, leading
// run, trailing run, longest run), pieces are joined in order by a shuffle tree in each wave and by thread 0 across the four
// waves; the joins are integer, so their grouping does not matter.  Plain vector stores write everything.
#include "t2v_common.h"
#include "t2v_kernels.h"

#define AL_F T2V_ALIGN_FRAMES                     // frames per workgroup
#define AL_NT 256
#define AL_NW (AL_NT / 64)
#define AL_NONE 0x7fffffff                        // argmax of a thread that owns no column

// the longest run of ones of a piece of a 0/1 sequence
struct al_run {
    int len, pre, suf, best;                      // elements; leading, trailing and longest run of ones
};

__device__ __forceinline__ al_run al_join(const al_run a, const al_run b) {      // a, then b
    al_run r;
    r.len = a.len + b.len;
    r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
    r.suf = b.suf == b.len ? b.len + a.suf : b.suf;
    r.best = max(max(a.best, b.best), a.suf + b.pre);
    return r;
}

__device__ __forceinline__ void al_push(al_run& r, bool one) {
    const al_run e = {1, one ? 1 : 0, one ? 1 : 0, one ? 1 : 0};
    r = al_join(r, e);
}

// lane 0 receives the join of the wave's 64 pieces in lane order
__device__ __forceinline__ al_run al_wave_join(al_run r, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        al_run s;
        s.len = __shfl_down(r.len, o, 64);
        s.pre = __shfl_down(r.pre, o, 64);
        s.suf = __shfl_down(r.suf, o, 64);
        s.best = __shfl_down(r.best, o, 64);
        if (lane + o < 64) r = al_join(r, s);
    }
    return r;
}

__global__ __launch_bounds__(AL_NT) void k_align_scan(const float* __restrict__ A, long long a_stride_b, long long a_stride_t,
                                                      const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_text,
                                                      int N, int T_in, int nblk, int32_t* __restrict__ path, int path_stride,
                                                      float* __restrict__ colpart, float* __restrict__ fpart) {
    __shared__ float RV[AL_F][AL_NW];             // per frame and wave: the largest value
    __shared__ int RA[AL_F][AL_NW];               // and its column
    __shared__ float MX[AL_F];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk, t0 = blk * AL_F, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int n = min(max(n_frames[b], 0), N), L = min(max(n_text[b], 0), T_in);   // no length addresses outside the tensor
    const int nf = min(n - t0, AL_F);                                              // frames of this workgroup that exist
    if (nf <= 0 || L <= 0) return;

    float best[AL_F];
    int arg[AL_F];
#pragma unroll
    for (int f = 0; f < AL_F; ++f) {
        best[f] = -INFINITY;
        arg[f] = AL_NONE;
    }
    const float* a0 = A + (size_t)b * a_stride_b + (size_t)t0 * a_stride_t;
    float* cp = colpart + ((size_t)b * nblk + blk) * T_in;
    for (int j = tid; j < L; j += AL_NT) {
        float v[AL_F];
#pragma unroll
        for (int f = 0; f < AL_F; ++f) v[f] = f < nf ? a0[(size_t)f * a_stride_t + j] : 0.f;
        float col = v[0];
#pragma unroll
        for (int f = 1; f < AL_F; ++f) col += v[f];                                // ascending t; + 0 past the row's frames
        cp[j] = col;
#pragma unroll
        for (int f = 0; f < AL_F; ++f)
            if (v[f] > best[f] || j == tid) {                                      // a thread's first column always counts
                best[f] = v[f];
                arg[f] = j;
            }
    }
#pragma unroll
    for (int f = 0; f < AL_F; ++f) {
        float bv = best[f];
        int ba = arg[f];
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oa = __shfl_xor(ba, o, 64);
            if (ov > bv || (ov == bv && oa < ba)) {
                bv = ov;
                ba = oa;
            }
        }
        if (lane == 0) {
            RV[f][wave] = bv;
            RA[f][wave] = ba;
        }
    }
    __syncthreads();
    if (tid < nf) {
        float bv = RV[tid][0];
        int ba = RA[tid][0];
#pragma unroll
        for (int w = 1; w < AL_NW; ++w) {
            const float ov = RV[tid][w];
            const int oa = RA[tid][w];
            if (ov > bv || (ov == bv && oa < ba)) {
                bv = ov;
                ba = oa;
            }
        }
        path[(size_t)b * path_stride + t0 + tid] = ba;
        MX[tid] = bv;
    }
    __syncthreads();
    if (tid == 0) {
        float s = MX[0];
        for (int f = 1; f < nf; ++f) s += MX[f];                                   // ascending t
        fpart[(size_t)b * nblk + blk] = s;
    }
}

__global__ __launch_bounds__(AL_NT) void k_align_finish(const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_text,
                                                        int N, int T_in, int nblk, int max_jump, float cover_min,
                                                        const float* __restrict__ colpart, const float* __restrict__ fpart,
                                                        int32_t* __restrict__ path, int path_stride, float* __restrict__ mass,
                                                        int mass_stride, float* __restrict__ focus, int32_t* __restrict__ stats) {
    __shared__ float FP[AL_NT];
    __shared__ al_run RUN[2][AL_NW];
    __shared__ int CNT[4][AL_NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = min(max(n_frames[b], 0), N), L = min(max(n_text[b], 0), T_in);
    if (n == 0 || L == 0) n = L = 0;              // an empty row: path -1, mass 0, focus 0, stats 0
    int32_t* p = path + (size_t)b * path_stride;
    float* m = mass + (size_t)b * mass_stride;
    for (int t = n + tid; t < path_stride; t += AL_NT) p[t] = -1;
    for (int j = L + tid; j < mass_stride; j += AL_NT) m[j] = 0.f;
    if (n == 0) {
        if (tid < 8) stats[(size_t)b * 8 + tid] = 0;
        if (tid == 0) focus[b] = 0.f;
        return;
    }
    const int nb = (n + AL_F - 1) / AL_F;

    // the columns: thread i owns the piece [i c, (i + 1) c) of 0..L
    al_run gap = {0, 0, 0, 0};
    int n_unc = 0;
    {
        const int c = (L + AL_NT - 1) / AL_NT;
        const int j1 = min(L, (tid + 1) * c);
        for (int j = tid * c; j < j1; ++j) {
            const float* cp = colpart + (size_t)b * nblk * T_in + j;
            float s = cp[0];
            int k = 1;
            for (; k + 8 <= nb; k += 8) {                                          // 8 loads in flight, added in block order
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = cp[(size_t)(k + q) * T_in];
#pragma unroll
                for (int q = 0; q < 8; ++q) s += v[q];
            }
            for (; k < nb; ++k) s += cp[(size_t)k * T_in];
            m[j] = s;
            const bool unc = s < cover_min;
            n_unc += unc ? 1 : 0;
            al_push(gap, unc);
        }
    }
    // the transitions t = 1..n-1: thread i owns the piece [1 + i c, 1 + (i + 1) c)
    al_run same = {0, 0, 0, 0};
    int n_back = 0, n_jump = 0, furthest = tid == 0 ? p[0] : 0;
    {
        const int c = (n - 1 + AL_NT - 1) / AL_NT;
        const int t1 = min(n, 1 + (tid + 1) * c);
        int t = 1 + tid * c;
        if (t < t1) {
            int prev = p[t - 1];
            for (; t < t1; ++t) {
                const int cur = p[t];
                n_back += cur < prev ? 1 : 0;
                n_jump += cur - prev > max_jump ? 1 : 0;
                furthest = max(furthest, cur);
                al_push(same, cur == prev);
                prev = cur;
            }
        }
    }
    gap = al_wave_join(gap, lane);
    same = al_wave_join(same, lane);
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        n_unc += __shfl_xor(n_unc, o, 64);
        n_back += __shfl_xor(n_back, o, 64);
        n_jump += __shfl_xor(n_jump, o, 64);
        furthest = max(furthest, __shfl_xor(furthest, o, 64));
    }
    if (lane == 0) {
        RUN[0][wave] = gap;
        RUN[1][wave] = same;
        CNT[0][wave] = n_unc;
        CNT[1][wave] = n_back;
        CNT[2][wave] = n_jump;
        CNT[3][wave] = furthest;
    }
    // focus: the block partials in ascending order, 256 at a time through LDS
    float fsum = 0.f;
    for (int k0 = 0; k0 < nb; k0 += AL_NT) {
        __syncthreads();
        if (k0 + tid < nb) FP[tid] = fpart[(size_t)b * nblk + k0 + tid];
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(AL_NT, nb - k0);
            for (int k = 0; k < cnt; ++k) fsum = k0 + k == 0 ? FP[0] : fsum + FP[k];
        }
    }
    if (tid == 0) {                               // RUN and CNT were written before the barriers above (nb >= 1)
        al_run g = RUN[0][0], s = RUN[1][0];
        int c0 = CNT[0][0], c1 = CNT[1][0], c2 = CNT[2][0], c3 = CNT[3][0];
        for (int w = 1; w < AL_NW; ++w) {
            g = al_join(g, RUN[0][w]);
            s = al_join(s, RUN[1][w]);
            c0 += CNT[0][w];
            c1 += CNT[1][w];
            c2 += CNT[2][w];
            c3 = max(c3, CNT[3][w]);
        }
        int32_t* st = stats + (size_t)b * 8;
        st[0] = c3;
        st[1] = p[n - 1];
        st[2] = c1;
        st[3] = c2;
        st[4] = 1 + s.best;
        st[5] = c0;
        st[6] = g.best;
        st[7] = 0;
        focus[b] = fsum / (float)n;
    }
}

static int al_blocks(int N) { return (N + AL_F - 1) / AL_F; }

extern "C" size_t t2v_alignment_scratch_bytes(int B, int N, int T_in) {
    if (B < 1 || N < 1 || T_in < 1) return 0;
    return sizeof(float) * (size_t)B * al_blocks(N) * ((size_t)T_in + 1);
}

extern "C" int t2v_alignment_stats(const float* A, long long a_stride_b, long long a_stride_t, const int32_t* n_frames,
                                   const int32_t* n_text, int B, int N, int T_in, int max_jump, float cover_min, int32_t* path,
                                   int path_stride, float* mass, int mass_stride, float* focus, int32_t* stats, void* scratch,
                                   void* stream_) {
    if (!A || !n_frames || !n_text || !path || !mass || !focus || !stats || !scratch) return T2V_ERR_ARG;
    if (B < 1 || N < 1 || T_in < 1) return T2V_ERR_ARG;
    if (a_stride_t < T_in || a_stride_b < (long long)(N - 1) * a_stride_t + T_in || path_stride < N || mass_stride < T_in)
        return T2V_ERR_ARG;
    if (max_jump < 0 || !(cover_min > 0.f)) return T2V_ERR_DIMS;
    const int nblk = al_blocks(N);
    if ((long long)B * nblk > 0x7fffffffLL) return T2V_ERR_ARG;
    float* colpart = (float*)scratch;
    float* fpart = colpart + (size_t)B * nblk * T_in;
    hipStream_t stream = (hipStream_t)stream_;
    k_align_scan<<<B * nblk, AL_NT, 0, stream>>>(A, a_stride_b, a_stride_t, n_frames, n_text, N, T_in, nblk, path, path_stride,
                                                 colpart, fpart);
    int rc = t2v_check_launch();
    if (rc) return rc;
    k_align_finish<<<B, AL_NT, 0, stream>>>(n_frames, n_text, N, T_in, nblk, max_jump, cover_min, colpart, fpart, path,
                                            path_stride, mass, mass_stride, focus, stats);
    return t2v_check_launch();
}
