// Scores of the latent space: for every query vector all distances to N labelled reference vectors, reduced per query to
// its k nearest references, the per-class sums of distances and the rank of one chosen reference.  kNN accuracy, silhouette
// and the style round trip of evaluate.py --style are host arithmetic on these (latent_scores.py).
//
// k_latent_pairs<DP>: lane t of workgroup (bx, by) owns query i = LAT_NT bx + t and visits the references of slice by, a whole
//   number of tiles of LAT_TILE rows.  The query row sits in DP registers (D rounded up to 8 / 16 / 32 / 64, zero padded: a pad
//   term adds fma(0, 0, acc) = acc).  A tile of reference rows is staged in LDS, padded the same way, and every lane reads
//   row r at the same address (a broadcast, 16 bytes per read).  Per pair: d2 = sum_c (q_c - r_c)^2 from the differences in
//   ascending c, one sqrt, the class sums (a select per class: the label is the same for the whole wave), the rank count and
//   a guarded insertion into the lane's k-list.  The list lives in LDS as [slot][lane] (conflict free), sorted by (d2, index);
//   its worst d2 is cached in a register, so a pair that does not enter costs one compare.  References arrive in ascending
//   index, so "strictly smaller d2 moves ahead" is the (d2, index) order.
//   The class sums are closed per tile and stored per (tile, class, query): their order depends on the tile grid, i.e. on N
//   alone, not on the slices.  Lists and rank counts go out per (slice, query).
// k_latent_merge: lane per query.  Inserts the slice lists in slice order into one list (same rule: later slices hold higher
//   indices), adds the tile sums in ascending tile order and the rank counts, and derives class_cnt from the label histogram
//   minus the excluded reference's label.  nn_dist = sqrt(d2), correctly rounded.
// No floating-point atomics; every sum has a fixed order that depends on N alone, so equal inputs give equal bits whatever
// the slice length.
#include <cstdint>

#include "t2v_common.h"
#include "t2v_kernels.h"

#define LAT_NT 128                  // lanes (queries) per workgroup
#define LAT_TILE T2V_LATENT_TILE    // reference rows per LDS tile = rows per class-sum block
#define LAT_MAX_D 64
#define LAT_MAX_C T2V_LATENT_MAX_CLASSES
#define LAT_MAX_K T2V_LATENT_MAX_K
#define LAT_TARGET_WGS 1024         // 4 workgroups of 2 waves per CU

namespace {

struct LatGeom {
    int qblocks, tiles, slice_tiles, slices;
};

// the grid: a function of (N, M) alone (or of the caller's slice_rows), never of the device
LatGeom lat_geom(int N, int M, int slice_rows) {
    LatGeom g;
    g.qblocks = (M + LAT_NT - 1) / LAT_NT;
    g.tiles = (N + LAT_TILE - 1) / LAT_TILE;
    if (slice_rows > 0) {
        g.slice_tiles = slice_rows / LAT_TILE;
    } else {
        const int want = (LAT_TARGET_WGS + g.qblocks - 1) / g.qblocks;
        g.slice_tiles = (g.tiles + want - 1) / want;
    }
    if (g.slice_tiles < 1) g.slice_tiles = 1;
    g.slices = (g.tiles + g.slice_tiles - 1) / g.slice_tiles;
    return g;
}

// scratch, 4-byte words: [tiles * C * M] tile class sums | [slices * k * M] list d2 | [slices * k * M] list index |
// [slices * M] rank counts
struct LatScratch {
    float* part;
    float* ld;
    int32_t* li;
    int32_t* rk;
};
size_t lat_scratch_words(int M, int C, int k, const LatGeom& g) {
    return (size_t)g.tiles * C * M + 2 * (size_t)g.slices * k * M + (size_t)g.slices * M;
}
LatScratch lat_carve(void* scratch, int M, int C, int k, const LatGeom& g) {
    LatScratch s;
    float* p = (float*)scratch;
    s.part = p;
    p += (size_t)g.tiles * C * M;
    s.ld = p;
    p += (size_t)g.slices * k * M;
    s.li = (int32_t*)p;
    p += (size_t)g.slices * k * M;
    s.rk = (int32_t*)p;
    return s;
}

// the lane's sorted list in LDS, [slot][lane]; `worst` mirrors slot k - 1.  Entries arrive in ascending index among equal d2.
__device__ __forceinline__ void lat_insert(float* ld, int32_t* li, int k, int t, float key, int32_t j, float& worst) {
    int e = k - 1;
    while (e > 0 && ld[(e - 1) * LAT_NT + t] > key) {
        ld[e * LAT_NT + t] = ld[(e - 1) * LAT_NT + t];
        li[e * LAT_NT + t] = li[(e - 1) * LAT_NT + t];
        --e;
    }
    ld[e * LAT_NT + t] = key;
    li[e * LAT_NT + t] = j;
    worst = ld[(k - 1) * LAT_NT + t];
}

}  // namespace

template <int DP>
__global__ __launch_bounds__(LAT_NT) void k_latent_pairs(const float* __restrict__ R, const int32_t* __restrict__ labels, int N,
                                                         int D, int C, const float* __restrict__ Q, int M,
                                                         const int32_t* __restrict__ exclude, int self_exclude,
                                                         const int32_t* __restrict__ target, int k, int slice_tiles, int vec4,
                                                         float* __restrict__ part, float* __restrict__ out_d,
                                                         int32_t* __restrict__ out_i, int32_t* __restrict__ out_rank) {
    __shared__ __attribute__((aligned(16))) float tile[LAT_TILE * DP];
    __shared__ int32_t tlab[LAT_TILE];
    extern __shared__ __attribute__((aligned(16))) float lat_list[];        // [k][LAT_NT] d2 | [k][LAT_NT] index
    float* ld = lat_list;
    int32_t* li = (int32_t*)(lat_list + k * LAT_NT);
    const int t = threadIdx.x, i = blockIdx.x * LAT_NT + t;
    const bool live = i < M;
    const float inf = __builtin_inff();

    float q[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) q[c] = live && c < D ? Q[(size_t)i * D + c] : 0.f;
    const int ex = !live ? -1 : exclude ? exclude[i] : self_exclude ? i : -1;
    const int tg = live && target ? target[i] : -1;
    // the target's own squared distance, by the arithmetic of the pair loop; -1 (below every d2) without a target
    float dt = -1.f;
    if (tg >= 0 && tg < N) {
        const float* row = R + (size_t)tg * D;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < DP; ++c) {
            const float df = q[c] - (c < D ? row[c] : 0.f);
            acc = fmaf(df, df, acc);
        }
        dt = acc;
    }
    for (int e = 0; e < k; ++e) {
        ld[e * LAT_NT + t] = inf;
        li[e * LAT_NT + t] = -1;
    }
    float worst = inf;
    int rank = 0;

    const int tile0 = blockIdx.y * slice_tiles;
    const int tile1 = min(tile0 + slice_tiles, (N + LAT_TILE - 1) / LAT_TILE);
    constexpr int V = DP / 4;
    for (int tl = tile0; tl < tile1; ++tl) {
        const int j0 = tl * LAT_TILE, n = min(LAT_TILE, N - j0);
        __syncthreads();
        for (int x = t; x < n * V; x += LAT_NT) {
            const int r = x / V, c = (x % V) * 4;
            const float* src = R + (size_t)(j0 + r) * D + c;
            float4 v;
            if (vec4 && c + 4 <= D) {
                v = *(const float4*)src;
            } else {
                v.x = c + 0 < D ? src[0] : 0.f;
                v.y = c + 1 < D ? src[1] : 0.f;
                v.z = c + 2 < D ? src[2] : 0.f;
                v.w = c + 3 < D ? src[3] : 0.f;
            }
            *(float4*)(tile + r * DP + c) = v;
        }
        for (int r = t; r < n; r += LAT_NT) tlab[r] = labels[j0 + r];
        __syncthreads();
        float cs[LAT_MAX_C];
#pragma unroll
        for (int c = 0; c < LAT_MAX_C; ++c) cs[c] = 0.f;
        for (int r = 0; r < n; ++r) {
            const float4* row = (const float4*)(tile + r * DP);
            float acc = 0.f;
#pragma unroll
            for (int c4 = 0; c4 < V; ++c4) {
                const float4 v = row[c4];
                float df = q[4 * c4 + 0] - v.x;
                acc = fmaf(df, df, acc);
                df = q[4 * c4 + 1] - v.y;
                acc = fmaf(df, df, acc);
                df = q[4 * c4 + 2] - v.z;
                acc = fmaf(df, df, acc);
                df = q[4 * c4 + 3] - v.w;
                acc = fmaf(df, df, acc);
            }
            const int j = j0 + r;
            const int lab = tlab[r];
            const bool skip = j == ex;
            const float d = skip ? 0.f : sqrtf(acc);
#pragma unroll
            for (int c = 0; c < LAT_MAX_C; ++c) cs[c] += lab == c ? d : 0.f;
            rank += (acc < dt || (acc == dt && j < tg)) ? 1 : 0;
            const float key = skip ? inf : acc;
            if (key < worst) lat_insert(ld, li, k, t, key, j, worst);
        }
        if (live) {
#pragma unroll
            for (int c = 0; c < LAT_MAX_C; ++c)
                if (c < C) part[((size_t)tl * C + c) * M + i] = cs[c];
        }
    }
    if (live) {
        const size_t base = (size_t)blockIdx.y * k * M + i;
        for (int e = 0; e < k; ++e) {
            out_d[base + (size_t)e * M] = ld[e * LAT_NT + t];
            out_i[base + (size_t)e * M] = li[e * LAT_NT + t];
        }
        out_rank[(size_t)blockIdx.y * M + i] = rank;
    }
}

__global__ __launch_bounds__(LAT_NT) void k_latent_merge(const int32_t* __restrict__ labels, int N, int C, int M,
                                                         const int32_t* __restrict__ exclude, int self_exclude,
                                                         const int32_t* __restrict__ target, int k, int tiles, int slices,
                                                         const float* __restrict__ part, const float* __restrict__ in_d,
                                                         const int32_t* __restrict__ in_i, const int32_t* __restrict__ in_rank,
                                                         int32_t* __restrict__ nn_idx, float* __restrict__ nn_dist,
                                                         float* __restrict__ class_sum, int32_t* __restrict__ class_cnt,
                                                         int32_t* __restrict__ rank_out) {
    __shared__ int hist[LAT_MAX_C];
    extern __shared__ __attribute__((aligned(16))) float lat_list[];
    float* ld = lat_list;
    int32_t* li = (int32_t*)(lat_list + k * LAT_NT);
    const int t = threadIdx.x, i = blockIdx.x * LAT_NT + t;
    if (t < LAT_MAX_C) hist[t] = 0;
    __syncthreads();
    for (int j = t; j < N; j += LAT_NT) {
        const int lab = labels[j];
        if (lab >= 0 && lab < C) atomicAdd(&hist[lab], 1);      // integer counts: any order gives the same value
    }
    __syncthreads();
    if (i >= M) return;
    const float inf = __builtin_inff();
    for (int e = 0; e < k; ++e) {
        ld[e * LAT_NT + t] = inf;
        li[e * LAT_NT + t] = -1;
    }
    float worst = inf;
    int rank = 0;
    for (int s = 0; s < slices; ++s) {
        const size_t base = (size_t)s * k * M + i;
        for (int e = 0; e < k; ++e) {
            const float key = in_d[base + (size_t)e * M];
            if (key < worst) lat_insert(ld, li, k, t, key, in_i[base + (size_t)e * M], worst);
        }
        rank += in_rank[(size_t)s * M + i];
    }
    for (int e = 0; e < k; ++e) {
        nn_idx[(size_t)i * k + e] = li[e * LAT_NT + t];
        nn_dist[(size_t)i * k + e] = sqrtf(ld[e * LAT_NT + t]);
    }
    const int ex = exclude ? exclude[i] : self_exclude ? i : -1;
    const int exlab = ex >= 0 && ex < N ? labels[ex] : -1;
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
        for (int tl = 0; tl < tiles; ++tl) acc += part[((size_t)tl * C + c) * M + i];
        class_sum[(size_t)i * C + c] = acc;
        class_cnt[(size_t)i * C + c] = hist[c] - (exlab == c ? 1 : 0);
    }
    if (rank_out) rank_out[i] = target && target[i] >= 0 ? rank : -1;
}

namespace {

int lat_dims_ok(int N, int M, int D, int C, int k) {
    return N >= 2 && N <= T2V_LATENT_MAX_POINTS && M >= 2 && M <= T2V_LATENT_MAX_POINTS && D >= 2 && D <= LAT_MAX_D && C >= 1 &&
           C <= LAT_MAX_C && k >= 1 && k <= LAT_MAX_K;
}

int lat_slice_ok(int slice_rows) { return slice_rows == 0 || (slice_rows > 0 && slice_rows % LAT_TILE == 0); }

template <int DP>
int lat_launch(const float* R, const int32_t* labels, int N, int D, int C, const float* Q, int M, const int32_t* exclude,
               int self_exclude, const int32_t* target, int k, const LatGeom& g, const LatScratch& s, hipStream_t stream) {
    const size_t list_bytes = (size_t)2 * k * LAT_NT * 4;
    static bool raised = false;     // static + dynamic LDS passes 64 KB at DP = 64 with k = 32
    if (!raised) {
        if (hipFuncSetAttribute((const void*)k_latent_pairs<DP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                2 * LAT_MAX_K * LAT_NT * 4) != hipSuccess) {
            const int rc = t2v_check_launch();
            return rc ? rc : T2V_ERR_LAUNCH;
        }
        raised = true;
    }
    const int vec4 = D % 4 == 0 && ((uintptr_t)R & 15) == 0;
    k_latent_pairs<DP><<<dim3(g.qblocks, g.slices), LAT_NT, list_bytes, stream>>>(
        R, labels, N, D, C, Q, M, exclude, self_exclude, target, k, g.slice_tiles, vec4, s.part, s.ld, s.li, s.rk);
    return T2V_OK;
}

}  // namespace

extern "C" size_t t2v_latent_scratch_bytes(int N, int M, int C, int k, int slice_rows) {
    if (!lat_dims_ok(N, M, 2, C, k) || !lat_slice_ok(slice_rows)) return 0;
    return 4 * lat_scratch_words(M, C, k, lat_geom(N, M, slice_rows));
}

extern "C" int t2v_latent_neighbours(const float* R, const int32_t* labels, int N, int D, int C, const float* Q, int M,
                                     const int32_t* exclude, const int32_t* target, int k, int slice_rows, int32_t* nn_idx,
                                     float* nn_dist, float* class_sum, int32_t* class_cnt, int32_t* rank, void* scratch,
                                     void* stream_) {
    const int self_exclude = !Q && !exclude;
    if (!Q) {
        Q = R;
        M = N;
    }
    if (!lat_dims_ok(N, M, D, C, k)) return T2V_ERR_DIMS;
    if (!R || !labels || !nn_idx || !nn_dist || !class_sum || !class_cnt || !scratch || (target && !rank)) return T2V_ERR_ARG;
    if (!lat_slice_ok(slice_rows)) return T2V_ERR_ARG;
    if (k > N - (exclude || self_exclude ? 1 : 0)) return T2V_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    const LatGeom g = lat_geom(N, M, slice_rows);
    const LatScratch s = lat_carve(scratch, M, C, k, g);
    int rc;
    if (D <= 8)
        rc = lat_launch<8>(R, labels, N, D, C, Q, M, exclude, self_exclude, target, k, g, s, stream);
    else if (D <= 16)
        rc = lat_launch<16>(R, labels, N, D, C, Q, M, exclude, self_exclude, target, k, g, s, stream);
    else if (D <= 32)
        rc = lat_launch<32>(R, labels, N, D, C, Q, M, exclude, self_exclude, target, k, g, s, stream);
    else
        rc = lat_launch<64>(R, labels, N, D, C, Q, M, exclude, self_exclude, target, k, g, s, stream);
    if (rc != T2V_OK) return rc;
    k_latent_merge<<<g.qblocks, LAT_NT, (size_t)2 * k * LAT_NT * 4, stream>>>(labels, N, C, M, exclude, self_exclude, target, k,
                                                                             g.tiles, g.slices, s.part, s.ld, s.li, s.rk, nn_idx,
                                                                             nn_dist, class_sum, class_cnt, rank);
    return t2v_check_launch();
}
