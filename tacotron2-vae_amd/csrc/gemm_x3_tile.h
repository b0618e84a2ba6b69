// The plane GEMM's building blocks (gemm.hip: k_x3_split, k_gemm_x3p), as device functions so that a second translation unit can run
// them inside a kernel of its own: the decoder_rnn role of k_achain_bwd (decoder_train_bwd_persist.hip) turns into a worker of the
// LSTM weight-gradient product once its time loop has ended, and has to produce the very bits the grouped launch would.
//   gx_split_block  one 64-row x 32-k block of an operand -> its planes (the body of k_x3_split)
//   gx_tile         one 128 x 128 tile of a product on the planes (the body of k_gemm_x3p), on 256 threads and 48 KB of LDS
#pragma once
#include "t2v_common.h"
#include "t2v_x3.h"
#include "t2v_xchg.h"

#define GX_BM 128
#define GX_BN 128
#define GX_SK 16                    // k per stage (two k-groups of 8)
// planes of an operand with `rows` rows and K columns: Rp = rows rounded up to 128, G = k-groups rounded up to 4 (32 k);
// plane p, k-group g, row r -> 16-byte slot (p * G + g) * Rp + r.  Rows >= rows and k >= K are zero.
__host__ __device__ static inline long gx_rp(int rows) { return ((long)rows + 127) / 128 * 128; }
// np = 3: the x3 planes of an fp32 product (stages of 16 k); np = 1: ONE plane, the bf16-rounded operand of a bf16_run product (stages of 64 k)
__host__ __device__ static inline long gx_groups(int K, int np = 3) { return np == 3 ? ((long)K + 31) / 32 * 4 : ((long)K + 63) / 64 * 8; }      // (multiples of 4 / 8 k-groups)
__host__ __device__ static inline long gx_plane_slots(int rows, int K, int np = 3) { return np * gx_groups(K, np) * gx_rp(rows); }

// Block (bx, by) of the split pass: 64 rows x 32 k of `src` on 256 threads (tid), through sm.  KC: the operand is contiguous along k
// (two float4 per row and k-group when aligned), else along its rows (or neither: scalar loads either way).  Every word crosses LDS once
// so that the plane stores run along the rows (1 KB contiguous per wave) whichever way the loads ran.  on = false: the barrier only (a
// caller that loops over blocks with a workgroup whose halves hold different block counts).
template <bool KC, int NP>
__device__ __forceinline__ void gx_split_block(const float* __restrict__ src, long s_row, long s_k, int rows, int K, uint4* __restrict__ dst,
                                               long Rp, long G, int bx, int by, int tid, uint4 (*sm)[4][64], bool on = true) {
    const int row0 = bx * 64, g0 = by * 4;
    const int r = KC ? tid >> 2 : tid & 63, g = KC ? tid & 3 : tid >> 6;
    const int row = row0 + r, k0 = 8 * (g0 + g);
    if (on) {
        float v[8];
        const bool rin = row < rows;
        const float* base = src + (long)min(row, rows - 1) * s_row;
        if (KC && s_k == 1 && !(s_row & 3) && !((uintptr_t)src & 15) && k0 + 8 <= K) {
            const float4 lo = *(const float4*)(base + k0), hi = *(const float4*)(base + k0 + 4);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = rin ? v[u] : 0.f;
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float x = base[(long)min(k0 + u, K - 1) * s_k];
                v[u] = (rin && k0 + u < K) ? x : 0.f;
            }
        }
        if (NP == 3) {
            uint4 p0, p1, p2;
            t2v_split8(v, p0, p1, p2);
            sm[0][g][r] = p0; sm[NP > 1 ? 1 : 0][g][r] = p1; sm[NP > 2 ? 2 : 0][g][r] = p2;
        } else {        // bf16_run: the operand rounded to bf16 (RNE), nothing else
            sm[0][g][r] = make_uint4(t2v_pack_bf16x2(v[0], v[1]), t2v_pack_bf16x2(v[2], v[3]), t2v_pack_bf16x2(v[4], v[5]), t2v_pack_bf16x2(v[6], v[7]));
        }
    }
    __syncthreads();
    const int g2 = tid >> 6, r2 = tid & 63;
    if (on && row0 + r2 < Rp && g0 + g2 < G) {
#pragma unroll
        for (int p = 0; p < NP; ++p) dst[(p * G + g0 + g2) * Rp + row0 + r2] = sm[p][g2][r2];
    }
}

// One launch may cover up to two products that share M and K (t2v_gemm_f32_grouped: the decoder's LSTM weight gradients, DGA^T·[x...]
// and DGD^T·[x...]): the tiles of product 1 follow those of product 0 in the linear tile order.  The columns of a product's result go
// to up to three destinations (the [prenet | h | ctx] column blocks of one gate-gradient product are the gradients of different tensors).
struct GemmX3Prod {
    const uint4* Ap; const uint4* Bp;      // planes (gx_plane_slots)
    long RpA, RpB;
    int N, tiles_x, tile0, nseg;           // columns, column tiles, first linear tile, destinations
    int seg_col[3]; float* segC[3]; int seg_ldc[3];     // destination s takes columns [seg_col[s], seg_col[s + 1]) (multiples of 128)
};
struct GemmX3Args {
    GemmX3Prod pr[2];
    int nprod, ntiles;
    long G;
    const float* bias;
    int M, relu, accumulate;
    float p_drop; uint64_t seed; uint32_t rng_stream, rng_t;
    const t2v_step_params* step;
    int st_chunk;           // split-K: stages per blockIdx.z (0 = all)
    float* part; unsigned* tile_ctr;
    // hand-over (t2v_gemm_f32_grouped_handed): the first min(*done_ctr, done_cap) tiles of product done_prod exist already — an earlier
    // kernel took them from that counter and computed them with gx_tile on the same planes; their workgroups return at once
    const unsigned* done_ctr; int done_prod; unsigned done_cap;
};
#ifndef GX_NB
#define GX_NB 2                     // stage buffers: the planes of stage i + GX_NB - 1 are requested during stage i.  Two (48 KB, three
                                    // workgroups per CU) and three (72 KB, two per CU) measure the same alone and in the step (10.82 .. 10.95 ms):
                                    // what bounds the kernel is what a CU can pull in, ~13 B/clk (24 KB per stage against 768 MFMA cycles per SIMD
                                    // = the measured 0.41 MFMA-busy), not the depth of the prefetch
#endif
#ifndef GX_LDS_PAD
#define GX_LDS_PAD 0                // unused 16-byte slots on top (measurement: how many workgroups / how much free LDS a CU keeps)
#endif
#ifndef GX_NG1
#define GX_NG1 4                   // k-groups per stage of the one-plane (bf16_run) form (2 / 4 / 8 measured: 432 / 453 / 423 TFLOP/s on 4096 x 2560 x 6400)
#endif
// 16-byte slots of LDS a tile needs: [buffer][A | B][plane][k-group][row]
#define GX_TILE_SLOTS(NP, NG) (GX_NB * 2 * (NP) * (NG) * GX_BM + GX_LDS_PAD)

// Tile `lin` (linear order over the products of `a`) of product P on 256 threads: tid in [0, 256), lds_ = GX_TILE_SLOTS 16-byte slots.
// NP planes per operand, NG k-groups (of 8) per stage: <3, 2> = the x3 form of an fp32 product (six MFMAs per k-block of 16, 24 per
// wave and stage); <1, GX_NG1> = a bf16_run product on pre-rounded operands (one MFMA per k-block of 16).
// SPLITK: the launch may be cut over k (a.part; zi of nz).  store = false: everything but the stores of the result (a caller whose
// workgroup runs two tiles side by side and has an odd one left keeps the barriers of both halves in step).
// Every thread of the workgroup passes the same number of barriers whatever its tile.
template <int NP, int NG, bool SPLITK>
__device__ __forceinline__ void gx_tile(const GemmX3Args& a, const GemmX3Prod& P, const int lin, const int tid, uint4* lds_, const int zi,
                                        const int nz, const bool store = true) {
    uint4 (*Ls)[2][NP][NG][GX_BM] = (uint4 (*)[2][NP][NG][GX_BM])lds_;
    // (wave-uniform, in an SGPR for t2v_dma16 — also where the caller derived lds_ from its thread index)
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(__attribute__((address_space(3))) void*)lds_);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int by_ = (lin - P.tile0) / P.tiles_x, bx_ = (lin - P.tile0) - by_ * P.tiles_x;
    const int i0 = by_ * GX_BM, j0 = bx_ * GX_BN;
    const int nst_all = (int)(a.G / NG);
    const int st0 = a.st_chunk ? zi * a.st_chunk : 0, st1 = a.st_chunk ? min(nst_all, st0 + a.st_chunk) : nst_all;
    // DMA plan of a stage: 4 NP NG pieces of 1 KB = {A, B} x NP planes x NG k-groups x 2 row halves; wave w issues pieces w, w + 4, ...
    // A request past the end re-reads the last stage into a buffer nobody reads any more: NP NG requests per wave and stage, always —
    // what the counted wait below relies on
    constexpr int NPIECE = NP * NG;         // per wave
    auto stage_dma = [&](int st, int buf) {
        st = min(st, st1 - 1);
#pragma unroll
        for (int i = 0; i < NPIECE; ++i) {
            const int q = wave + 4 * i;
            const int op = q / (2 * NP * NG), rem = q - (2 * NP * NG) * op, p = rem / (2 * NG), g = (rem >> 1) % NG, half = rem & 1;
            const uint4* src = op ? P.Bp + (p * a.G + NG * st + g) * P.RpB + j0 + 64 * half + lane
                                  : P.Ap + (p * a.G + NG * st + g) * P.RpA + i0 + 64 * half + lane;
            t2v_dma16(src, lds0 + 16u * (unsigned)(((((buf * 2 + op) * NP + p) * NG + g) * GX_BM) + 64 * half));
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
    const int am = 64 * wm + (lane & 31), bn = 64 * wn + (lane & 31), kq = lane >> 5;
#define GX_MFMA(A_, B_, C_) C_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const t2v_bf16x8*)&(A_), *(const t2v_bf16x8*)&(B_), C_, 0, 0, 0)
#pragma unroll
    for (int d = 0; d < GX_NB - 1; ++d) stage_dma(st0 + d, d);
    t2v_wait_vmcnt<NPIECE * (GX_NB - 2)>();          // the first stage has landed, the later ones may still be on their way
    __syncthreads();
    int buf = 0;
    for (int st = st0; st < st1; ++st) {
        // the stage GX_NB - 1 ahead goes into the buffer everybody left at the last barrier
        const int nb2 = buf == 0 ? GX_NB - 1 : buf - 1;     // (buf + GX_NB - 1) % GX_NB
        stage_dma(st + GX_NB - 1, nb2);
#define GX_ALL(PA, PB)                                      \
        GX_MFMA(av[PA][0], bv[PB][0], acc[0][0]); GX_MFMA(av[PA][0], bv[PB][1], acc[0][1]); \
        GX_MFMA(av[PA][1], bv[PB][0], acc[1][0]); GX_MFMA(av[PA][1], bv[PB][1], acc[1][1])
#pragma unroll
        for (int ks = 0; ks < NG / 2; ++ks) {           // k-blocks of 16 of this stage
            uint4 av[NP][2], bv[NP][2];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                av[p][0] = Ls[buf][0][p][2 * ks + kq][am];
                av[p][1] = Ls[buf][0][p][2 * ks + kq][am + 32];
                bv[p][0] = Ls[buf][1][p][2 * ks + kq][bn];
                bv[p][1] = Ls[buf][1][p][2 * ks + kq][bn + 32];
            }
            if constexpr (NP == 3) {
                // small terms first; product-major, so that consecutive MFMAs go to different accumulators
                GX_ALL(2, 0); GX_ALL(0, 2); GX_ALL(1, 1); GX_ALL(1, 0); GX_ALL(0, 1); GX_ALL(0, 0);
            } else {
                GX_ALL(0, 0);
            }
        }
#undef GX_ALL
        // stage st + 1 must have landed before anybody passes the barrier: requests come back in order, so it has once only the
        // requests of the GX_NB - 2 stages behind it (six per wave and stage) are outstanding
        t2v_wait_vmcnt<NPIECE * (GX_NB - 2)>();
        __syncthreads();        // ... and this stage's LDS reads are done
        buf = buf == GX_NB - 1 ? 0 : buf + 1;
    }
#undef GX_MFMA
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the surplus requests of the last stages
    if constexpr (SPLITK) {
        if (a.part) {
            // split-K exactly as in k_gemm_bf16_big_rr: raw accumulators to scratch in accumulator order (write-through), the workgroup
            // that arrives last at its tile's counter adds the partials in the fixed order z = 0, 1, ... and runs the epilogue
            const size_t tiles = (size_t)a.ntiles, tile = (size_t)lin;
            {
                __amdgpu_buffer_rsrc_t rs = t2v_rsrc(a.part + (zi * tiles + tile) * (GX_BM * GX_BN));
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            u32x4 v;
                            v.x = __float_as_uint(acc[x][y][4 * q]); v.y = __float_as_uint(acc[x][y][4 * q + 1]);
                            v.z = __float_as_uint(acc[x][y][4 * q + 2]); v.w = __float_as_uint(acc[x][y][4 * q + 3]);
                            __builtin_amdgcn_raw_buffer_store_b128(v, rs, ((((x * 2 + y) * 4 + q) * 256) + tid) * 16, 0, 16);
                        }
            }
            __shared__ unsigned last_;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            unsigned* ctr = a.tile_ctr + tile;
            if (tid == 0) last_ = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nz - 1 ? 1u : 0u;
            __syncthreads();
            if (!last_) return;
            if (tid == 0) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
            for (int z0 = 0; z0 < nz; z0 += 2) {
                u32x4 v[2][16];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int z = min(z0 + u, nz - 1);
                    __amdgpu_buffer_rsrc_t rs = t2v_rsrc(a.part + (z * tiles + tile) * (GX_BM * GX_BN));
#pragma unroll
                    for (int g = 0; g < 16; ++g) v[u][g] = __builtin_amdgcn_raw_buffer_load_b128(rs, (g * 256 + tid) * 16, 0, 16);
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (z0 + u < nz) {
#pragma unroll
                        for (int g = 0; g < 16; ++g) {
                            acc[g >> 3][(g >> 2) & 1][4 * (g & 3)] += __uint_as_float(v[u][g].x);
                            acc[g >> 3][(g >> 2) & 1][4 * (g & 3) + 1] += __uint_as_float(v[u][g].y);
                            acc[g >> 3][(g >> 2) & 1][4 * (g & 3) + 2] += __uint_as_float(v[u][g].z);
                            acc[g >> 3][(g >> 2) & 1][4 * (g & 3) + 3] += __uint_as_float(v[u][g].w);
                        }
                    }
            }
        }
    }
    if (!store) return;
    const uint64_t seed = t2v_step_seed(a.seed, a.step);
    // destination of this tile's columns (a tile never straddles two: their boundaries are multiples of 128)
    int sg = 0;
    if (P.nseg > 1 && j0 >= P.seg_col[1]) sg = 1;
    if (P.nseg > 2 && j0 >= P.seg_col[2]) sg = 2;
    float* const Cd = P.segC[sg];
    const int ldc = P.seg_ldc[sg], jc0 = j0 - P.seg_col[sg];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int jl = 64 * wn + 32 * y + (lane & 31), j = j0 + jl;
            if (j < P.N) {
                const float bvs = a.bias ? a.bias[j] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = i0 + 64 * wm + 32 * x + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (i < a.M) {
                        const size_t idx = (size_t)i * ldc + jc0 + jl;
                        float v = acc[x][y][r] + bvs;
                        if (a.accumulate) v += Cd[idx];
                        if (a.relu) v = fmaxf(v, 0.f);
                        if (a.p_drop > 0.f) v *= t2v_drop_scale(seed, a.rng_stream, a.rng_t, (uint32_t)idx, a.p_drop);
                        Cd[idx] = v;
                    }
                }
            }
        }
}
