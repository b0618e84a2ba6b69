// Free-running decode as ONE persistent launch (reference Decoder.inference model.py:428-464 / the loop at
// synthesizer.py:139-154): 256 workgroups x 512 threads stay resident for the whole utterance, every weight of the
// loop lives in registers / LDS, and the five dependent stages of a frame
//     attention_rnn -> attention -> decoder_rnn -> projection (+ folded Prenet layer 0) -> Prenet layer 1
// hand their small result vectors (1024 / 512 / 256 values per item) from CU to CU as plain 4-byte values in a FRESH,
// sentinel-filled exchange row per frame (write-through sc1 stores, sc1 loads; a word that is no longer T2V_SENT IS the
// data — no tags, no counters, no fences, no grid barrier).  Round 3: half the bytes of the former 8-byte {value, tag}
// granules — what a gather costs is its bytes (a CU pulls ~11 B/cycle from beyond its L2) — and an adaptive nap
// in front of every poll, so that the first round of a gather is not the one that is bound to fail.  Nothing is streamed from HBM per frame: the 71 MB of LSTM weights that the launch-per-stage
// loop (decoder_infer.hip) re-reads every frame are read once.
//
// Roles (every workgroup runs the frame loop, phases in the same order, so the waits cannot form a cycle):
//   all 256 workgroups : 4 hidden units of both LSTM cells (16 gate rows each): rows x K/8 per wave in VGPRs
//                        (136 per lane), VALU dot products against the LDS copy of the state vectors
//   wg 0 .. 8B-1       : attention slice (item b = wg/8, 16 attention dims + 64 context columns): W_q slice, memory /
//                        processed-memory slices and the alignment window stay in LDS for all frames
//   wg 64 .. 106       : 8 of the 337 projection rows each (80 mel + gate + 256 folded Prenet-0 rows), rows in LDS
//   wg 128 .. 159      : 8 Prenet layer-1 rows each
// The gate row decides the stop (model.py:453) and publishes it as a granule every workgroup reads at the top of the
// next frame: nothing is computed after the stop frame.
// Limits of this path: B <= 4, T_in <= 224 (LDS residency of the attention operands); the launch-per-stage loop serves
// everything else (and the stepwise decode() API).
#include "t2v_common.h"
#include "t2v_kernels.h"
#include "t2v_xchg.h"
#include <limits.h>

#define PD_THREADS 512
#define PD_MAXB 4
#define PD_MAXT 224
#ifndef PD_CTXW
#define PD_CTXW 4          // positions per round of the context sum (t2v_ctx_partial); the attention workgroups have few registers to spare
#endif
#define PD_SPIN 3000000u
#define PD_XW 2816                 // LDS state row: [h_att 1024 | ctx 512 | pre1 256 | h_dec 1024]
#define PD_X_HA 0
#define PD_X_CX 1024
#define PD_X_P1 1536
#define PD_X_HD 1792
#define PD_KATT 1792               // attention_rnn K: [h_att | ctx | pre1]   (contiguous in the LDS row)
#define PD_KDEC 2560               // decoder_rnn   K: [h_att | ctx | h_dec]  (h_dec sits 256 further)
#define PD_NROW 337
#define PD_WG_PROJ 64
#define PD_WG_PRE1 128

struct PersistArgs {
    const float* w_ih_att; const float* w_hh_att; const float* w_ih_dec; const float* w_hh_dec;   // nn.LSTMCell tensors
    const float* bias_att; const float* bias_dec;     // (4096) b_ih + b_hh
    const float* wq;          // (128,1024) query_layer weight
    const float* wcomb;       // fused location filter, forward copy F[d][g][st]
    const float* v;           // (128)
    const float* proj_w;      // (337,1536) [linear_projection; gate_layer; W0·linear_projection]
    const float* proj_b;      // (337)
    const float* w1;          // (256,256) Prenet layer 1
    const float* memory;      // (B,T_in,512)
    const float* pm;          // (B,T_in,128)
    const int32_t* lengths;   // (B) or NULL
    const float* pre_first;   // (B,256) Prenet(go frame)
    float* MEL; float* GATE; float* AL;      // (Tmax,B,80) (Tmax,B) (Tmax+1,B,T_in): AL[t+1] = weights of frame t
    int* stop_flag;
    float* xg;                // exchange rows, one per frame: t_end x pd_row(B) floats, sentinel-filled by the launcher
    unsigned* err;
    int B, T_in, t_end;
    float gate_logit_thr, p_prenet;
    uint64_t seed;
    unsigned long long* prof;   // optional: stamps of frame 100 (workgroup 0 slots 0..9, workgroup 64 slots 10..13, workgroup 128 slots 14..16)
};
// per-workgroup time line of frame 100 on the chip-wide 100 MHz counter: prof[64 + workgroup * 16 + slot] (tools/dbg_persist.py)
#define PD_RT(SLOT) do { if (a.prof && t == 100 && tid == 0) a.prof[64 + wg * 16 + (SLOT)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define PD_STAMP(WG, I) do { if (a.prof && t == 100 && wg == (WG) && tid == 0) a.prof[(I)] = __builtin_readcyclecounter(); } while (0)

// exchange row of one frame (floats)
__host__ __device__ static inline unsigned pd_hatt(int B) { (void)B; return 0u; }
__host__ __device__ static inline unsigned pd_hdec(int B) { return (unsigned)B * 1024u; }
__host__ __device__ static inline unsigned pd_ctx(int B) { return (unsigned)B * 2048u; }
__host__ __device__ static inline unsigned pd_pre0(int B) { return (unsigned)B * 2560u; }
__host__ __device__ static inline unsigned pd_pre1(int B) { return (unsigned)B * 2816u; }
__host__ __device__ static inline unsigned pd_ex(int B) { return (unsigned)B * 3072u; }          // [b][8][256]
__host__ __device__ static inline unsigned pd_stop(int B) { return (unsigned)B * 5120u; }
__host__ __device__ static inline unsigned pd_row(int B) { return (unsigned)B * 5120u + 32u; }

#ifndef PD_POLL2
#define PD_POLL2 0
#endif
// 4-byte publish at a float offset.  Kept as a function: with the offset arithmetic written out at the call sites the
// compiler schedules the kernel differently.
__device__ __forceinline__ void pd_put(__amdgpu_buffer_rsrc_t r, unsigned off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)(off * 4u), 0, T2V_SC1);
}

// Poll the n (<= 2 * 512, even) values at `off` until none is the sentinel, then copy them to LDS: thread = two adjacent
// values (one 8-byte load).  Naps `nap` first (adapted by the caller from the returned number of failed rounds).  On a
// timeout the error word is set and *flag cleared (an LDS int, 1 on entry) — the caller syncs before reading dst.
__device__ __forceinline__ int pd_gather(float* dst, __amdgpu_buffer_rsrc_t r, unsigned off, int n, int nap, unsigned* err, int* flag) {
    const int tid = threadIdx.x;
    for (int i = 0; i < nap; i += 4) __builtin_amdgcn_s_sleep(4);
    const bool on = 2 * tid < n;
    u32x2 x = {0u, 0u};
    unsigned spins = 0;
#if PD_POLL2
    // (measurement variant, -DPD_POLL2=1: two polls in flight, half a round trip apart.  Same-box A/B: 14.68 vs 14.39 us per
    // frame — twice the requests on lines that 256 workgroups already poll cost more than the quarter round trip they save)
    u32x2 x0 = {T2V_SENT, T2V_SENT}, x1 = {T2V_SENT, T2V_SENT};
    if (on) x0 = t2v_ld_b64(r, (off + 2u * (unsigned)tid) * 4u);
    __builtin_amdgcn_s_sleep(4);
    if (on) x1 = t2v_ld_b64(r, (off + 2u * (unsigned)tid) * 4u);
    for (;;) {
        if (__all(!on || (x0[0] != T2V_SENT && x0[1] != T2V_SENT))) { x = x0; break; }
        if (on) x0 = t2v_ld_b64(r, (off + 2u * (unsigned)tid) * 4u);
        if (__all(!on || (x1[0] != T2V_SENT && x1[1] != T2V_SENT))) { x = x1; break; }
        if (on) x1 = t2v_ld_b64(r, (off + 2u * (unsigned)tid) * 4u);
        if (t2v_give_up(spins, PD_SPIN, err, flag)) break;
    }
#else
    for (;;) {
        if (on) x = t2v_ld_b64(r, (off + 2u * (unsigned)tid) * 4u);
        if (__all(x[0] != T2V_SENT && x[1] != T2V_SENT)) break;
        __builtin_amdgcn_s_sleep(1);
        if (t2v_give_up(spins, PD_SPIN, err, flag)) break;
    }
#endif
    if (on) *(float2*)(dst + 2 * tid) = make_float2(__uint_as_float(x[0]), __uint_as_float(x[1]));
    return (int)spins;
}
// The same row of ALL items of the batch (item b at dst + b * PD_XW, row offset off + b * stride) in ONE polling pass: the loads of
// the (up to four) items are in flight together.  Item by item — pd_gather in a loop — every item pays its own memory round
// trip on the frame's chain: 15.5 us per frame at B = 2 against 12.6 at B = 1 (round 6).  Items past B re-read item B - 1.
__device__ __forceinline__ int pd_gather_items(float* dst, __amdgpu_buffer_rsrc_t r, unsigned off, unsigned stride, int n, int B, int nap,
                                               unsigned* err, int* flag) {
    if (B == 1) return pd_gather(dst, r, off, n, nap, err, flag);
    const int tid = threadIdx.x;
    for (int i = 0; i < nap; i += 4) __builtin_amdgcn_s_sleep(4);
    const bool on = 2 * tid < n;
    u32x2 x[PD_MAXB];
#pragma unroll
    for (int b = 0; b < PD_MAXB; ++b) x[b] = u32x2{0u, 0u};
    unsigned spins = 0;
    for (;;) {
        bool ok = true;
        if (on) {
#pragma unroll
            for (int b = 0; b < PD_MAXB; ++b) x[b] = t2v_ld_b64(r, (off + (unsigned)min(b, B - 1) * stride + 2u * (unsigned)tid) * 4u);
#pragma unroll
            for (int b = 0; b < PD_MAXB; ++b) ok = ok && x[b][0] != T2V_SENT && x[b][1] != T2V_SENT;
        }
        if (__all(ok)) break;
        __builtin_amdgcn_s_sleep(1);
        if (t2v_give_up(spins, PD_SPIN, err, flag)) break;
    }
    if (on) {
#pragma unroll
        for (int b = 0; b < PD_MAXB; ++b)
            if (b < B) *(float2*)(dst + (size_t)b * PD_XW + 2 * tid) = make_float2(__uint_as_float(x[b][0]), __uint_as_float(x[b][1]));
    }
    return (int)spins;
}
// a copy of v the compiler cannot see through: what is derived from it is recomputed where it is used (two or three VALU
// instructions) instead of being hoisted out of the frame loop and kept — spilled — across it
__device__ __forceinline__ int pd_opaque(int v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ int pd_adapt(int nap, int rounds) {       // units of 64 cycles; first round should just succeed
    if (rounds > 1) return min(48, nap + 4 * min(rounds - 1, 3));
    if (rounds == 0) return (3 * nap) >> 2;
    return nap;
}

// LSTM gate rows of this workgroup for one cell: lane = (row r = lane>>2 (unit r>>2, gate r&3), kq = lane&3); weights in
// registers, VALU dot products against the LDS copy of the state vectors, partial dot products -> red[wave][r][b].
// Round 4: the two LSTM GEMVs of a frame are cut by WHEN their inputs exist, so that only the columns of the value that has
// just arrived are left on the frame's dependency chain:
//   attention_rnn(t+1) = [h_att(t) | ctx(t)] (1536 columns, known when ctx(t) has been gathered: evaluated in the shadow of
//                        the projection / Prenet stages of frame t)  +  Prenet output (256 columns: the chain)
//   decoder_rnn(t)     = h_dec(t-1) (1024 columns, known since the previous frame)  +  h_att(t) (1024, evaluated while the
//                        attention workgroups work)  +  ctx(t) (512 columns: the chain)
// Every wave owns an eighth of EACH part, so a late part is spread over all 8 waves of the workgroup.  Weight register j of a
// lane (wave w, k quarter kq) <-> logical column:
//   attention_rnn  j < 48: 192 w + 4 j + kq                      j >= 48: 1536 + 32 w + 4 (j - 48) + kq        [h_att|ctx] , [pre1]
//   decoder_rnn    j < 32: 128 w + 4 j + kq (h_att)   j < 64: 1536 + 128 w + 4 (j - 32) + kq (h_dec)   else: 1024 + 64 w + 4 (j - 64) + kq (ctx)
__device__ __forceinline__ int pd_ka(int wave, int j, int kq) { return j < 48 ? 192 * wave + 4 * j + kq : 1536 + 32 * wave + 4 * (j - 48) + kq; }
__device__ __forceinline__ int pd_kd(int wave, int j, int kq) {
    return j < 32 ? 128 * wave + 4 * j + kq : (j < 64 ? 1536 + 128 * wave + 4 * (j - 32) + kq : 1024 + 64 * wave + 4 * (j - 64) + kq);
}
// acc[b] += sum_{j in [J0, J1)} wreg[j] * x_b[column of j]   (DEC: decoder_rnn mapping; its h_dec columns sit 256 further in the LDS row)
template <int NJ, int J0, int J1, bool DEC>
__device__ __forceinline__ void pd_gemv_part(const float (&wreg)[NJ], const float* X, int B, float (&acc)[PD_MAXB]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane & 3;
#pragma unroll
    for (int b = 0; b < PD_MAXB; ++b) {
        if (b < B) {
            const float* xb = X + (size_t)b * PD_XW;
            float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
            for (int j = J0; j < J1; j += 2) {
                const int k0 = DEC ? pd_kd(wave, j, kq) : pd_ka(wave, j, kq), k1 = DEC ? pd_kd(wave, j + 1, kq) : pd_ka(wave, j + 1, kq);
                acc0 = fmaf(wreg[j], xb[k0 + ((DEC && j >= 32 && j < 64) ? 256 : 0)], acc0);
                acc1 = fmaf(wreg[j + 1], xb[k1 + ((DEC && j + 1 >= 32 && j + 1 < 64) ? 256 : 0)], acc1);
            }
            acc[b] += acc0 + acc1;
        }
    }
}
// quad sum of the lanes of a gate row -> red[wave][r][b]; the accumulators start the next frame at zero
__device__ __forceinline__ void pd_gemv_finish(float (&acc)[PD_MAXB], int B, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane & 3, r = lane >> 2;
#pragma unroll
    for (int b = 0; b < PD_MAXB; ++b) {
        if (b < B) {
            float v = acc[b];
            v = T2V_DPP_ADD(v, 0xB1);
            v = T2V_DPP_ADD(v, 0x4E);
            if (kq == 0) red[(wave * 16 + r) * PD_MAXB + b] = v;
        }
        acc[b] = 0.f;
    }
}

// Per-item outputs / inputs of a batched synthesis (t2v_decoder_infer_persistent_items, decoder_persist_kernel.inc)
struct PersistItems {
    int* stop_item;                 // (B), preset INT_MAX by the caller
    const uint64_t* item_seeds;     // (B)
};

// Attention window (include/t2vae.h t2v_dec_window), clamped by the launcher so that p - back and p + ahead cannot overflow
struct PersistWindow {
    int back, ahead;
};
// The planned decode (include/t2vae.h t2v_decoder_infer_persistent_plan): the window and the plan its centre is read from
struct PersistPlan {
    int back, ahead;
    const int32_t* plan;            // (B, plan_stride)
    const int32_t* n_plan;          // (B)
    int plan_stride;
};
// (value, index) of the larger value, the lower index on a tie, over the 64 lanes of a wave; every lane ends with the result
__device__ __forceinline__ void pd_argmax_wave(float& v, int& j) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(v, m, 64);
        const int oj = __shfl_xor(j, m, 64);
        if (ov > v || (ov == v && oj < j)) { v = ov; j = oj; }
    }
}

#define PD_WINDOW 0
#define PD_ITEMS 0
#include "decoder_persist_kernel.inc"
#undef PD_ITEMS
#define PD_ITEMS 1
#include "decoder_persist_kernel.inc"
#undef PD_ITEMS
#undef PD_WINDOW
#define PD_WINDOW 1
#define PD_ITEMS 0
#include "decoder_persist_kernel.inc"
#undef PD_ITEMS
#define PD_ITEMS 1
#include "decoder_persist_kernel.inc"
#undef PD_ITEMS
#undef PD_WINDOW
#define PD_WINDOW 2
#define PD_ITEMS 0
#include "decoder_persist_kernel.inc"
#undef PD_ITEMS
#define PD_ITEMS 1
#include "decoder_persist_kernel.inc"
#undef PD_ITEMS
#undef PD_WINDOW

static size_t pd_lds_bytes(int B, int T_in) {
    const size_t Tcap = (size_t)((T_in + 15) / 16) * 16;
    size_t f = (size_t)B * PD_XW + 8 * 16 * PD_MAXB + PD_MAXB * 16 + 2 * PD_MAXB * 4 + 4;
    const size_t attn = 16 * 1028 + Tcap * 64 + Tcap * 16 + 2 * (Tcap + 32) + Tcap + T2V_CTX_PAD + 16 + 8 * 64 + 64 + 16 * 64;
    const size_t proj = 8 * 1536;
    f += attn > proj ? attn : proj;
    return f * sizeof(float);
}

// exchange scratch: one sentinel-filled row per frame
extern "C" long t2v_decoder_persist_scratch_floats(int B, int t_end) {
    return (B < 1 || B > PD_MAXB || t_end < 1) ? 0 : (long)((size_t)t_end * pd_row(B));
}
// The workgroups of this kernel spin on each other's granules, so ALL 256 must be resident at once: one per CU on a
// device with >= 256 CUs whose occupancy query admits this launch configuration (512 threads, the run-time LDS carve).
// A device that is shared with other work can still fail to co-schedule them — the bounded spins then set the error word
// and Decoder.inference re-runs the utterance on the launch-per-stage loop.
static int pd_supported(const void* kernel, int B, int T_in) {
    if (!(B >= 1 && B <= PD_MAXB && T_in >= 1 && T_in <= PD_MAXT && pd_lds_bytes(B, T_in) <= T2V_LDS_MAX)) return 0;
    static bool raised = false;
    return t2v_persist_resident(kernel, PD_THREADS, pd_lds_bytes(B, T_in),
                                {(const void*)k_decode_persist, (const void*)k_decode_persist_items,
                                 (const void*)k_decode_persist_win, (const void*)k_decode_persist_items_win,
                                 (const void*)k_decode_persist_plan, (const void*)k_decode_persist_items_plan}, raised);
}
extern "C" int t2v_decoder_persist_supported(int B, int T_in) {
    return pd_supported((const void*)k_decode_persist, B, T_in);
}

static int pd_launch(const t2v_dec_persist_weights* w, const t2v_dec_persist_bufs* s, int B, int T_in, int t_end,
                     float gate_threshold, float p_prenet, uint64_t seed, const t2v_dec_items* items, const t2v_dec_window* window,
                     const PersistPlan* plan, hipStream_t stream) {
    if (plan && (!window || !plan->plan || !plan->n_plan || plan->plan_stride < 1)) return T2V_ERR_ARG;
    const void* kernel = plan ? (items ? (const void*)k_decode_persist_items_plan : (const void*)k_decode_persist_plan) : window ? (items ? (const void*)k_decode_persist_items_win : (const void*)k_decode_persist_win)
                                : (items ? (const void*)k_decode_persist_items : (const void*)k_decode_persist);
    if (!w || !s || !pd_supported(kernel, B, T_in) || t_end < 1) return T2V_ERR_ARG;
    if (!w->w_ih_att || !w->w_hh_att || !w->w_ih_dec || !w->w_hh_dec || !w->bias_att || !w->bias_dec || !w->wq || !w->wcomb ||
        !w->v || !w->proj_w || !w->proj_b || !w->prenet_w1 || !s->memory || !s->pm || !s->pre_first || !s->MEL || !s->GATE ||
        !s->AL || !s->stop_flag || !s->exchange || !s->err_word)
        return T2V_ERR_ARG;
    if (items && (!items->stop_item || !items->item_seeds)) return T2V_ERR_ARG;
    if (window && (window->back < 0 || window->ahead < 0)) return T2V_ERR_ARG;
    if (((uintptr_t)s->exchange & 15) || (size_t)t_end * pd_row(B) * 4 >= 0x7fffffffull) return T2V_ERR_ARG;      // 31-bit buffer offsets
    const size_t lds = pd_lds_bytes(B, T_in);     // (pd_supported raised the dynamic-LDS limit)
    t2v_fill_sentinel(s->exchange, (size_t)t_end * pd_row(B) / 4, 1024, stream);
    (void)hipMemsetAsync(s->err_word, 0, sizeof(unsigned), stream);
    PersistArgs a;
    a.w_ih_att = w->w_ih_att; a.w_hh_att = w->w_hh_att; a.w_ih_dec = w->w_ih_dec; a.w_hh_dec = w->w_hh_dec;
    a.bias_att = w->bias_att; a.bias_dec = w->bias_dec; a.wq = w->wq; a.wcomb = w->wcomb; a.v = w->v;
    a.proj_w = w->proj_w; a.proj_b = w->proj_b; a.w1 = w->prenet_w1;
    a.memory = s->memory; a.pm = s->pm; a.lengths = s->lengths; a.pre_first = s->pre_first;
    a.MEL = s->MEL; a.GATE = s->GATE; a.AL = s->AL; a.stop_flag = s->stop_flag;
    a.xg = (float*)s->exchange; a.err = s->err_word;
    a.B = B; a.T_in = T_in; a.t_end = t_end;
    a.gate_logit_thr = gate_threshold <= 0.f ? -INFINITY : (gate_threshold >= 1.f ? INFINITY : logf(gate_threshold / (1.f - gate_threshold)));
    a.p_prenet = p_prenet; a.seed = seed;
    a.prof = g_t2v_prof;
    // (a window wider than the text covers it whatever p is: clamped, so that the kernel's p - back / p + ahead stay small)
    const PersistWindow wn = {window ? (window->back < T_in ? window->back : T_in) : 0, window ? (window->ahead < T_in ? window->ahead : T_in) : 0};
    if (plan) {
        const PersistPlan pl = {wn.back, wn.ahead, plan->plan, plan->n_plan, plan->plan_stride};
        if (items) k_decode_persist_items_plan<<<T2V_NWG, PD_THREADS, lds, stream>>>(a, PersistItems{items->stop_item, items->item_seeds}, pl);
        else k_decode_persist_plan<<<T2V_NWG, PD_THREADS, lds, stream>>>(a, pl);
    } else if (window && items) k_decode_persist_items_win<<<T2V_NWG, PD_THREADS, lds, stream>>>(a, PersistItems{items->stop_item, items->item_seeds}, wn);
    else if (window) k_decode_persist_win<<<T2V_NWG, PD_THREADS, lds, stream>>>(a, wn);
    else if (items) k_decode_persist_items<<<T2V_NWG, PD_THREADS, lds, stream>>>(a, PersistItems{items->stop_item, items->item_seeds});
    else k_decode_persist<<<T2V_NWG, PD_THREADS, lds, stream>>>(a);
    return t2v_check_launch();
}

extern "C" int t2v_decoder_infer_persistent(const t2v_dec_persist_weights* w, const t2v_dec_persist_bufs* s, int B, int T_in,
                                            int t_end, float gate_threshold, float p_prenet, uint64_t seed, void* stream_) {
    return pd_launch(w, s, B, T_in, t_end, gate_threshold, p_prenet, seed, nullptr, nullptr, nullptr, (hipStream_t)stream_);
}

// the same with per-item stop frames and dropout seeds (batched synthesis); seed is unused when items->item_seeds is set
extern "C" int t2v_decoder_infer_persistent_items(const t2v_dec_persist_weights* w, const t2v_dec_persist_bufs* s, int B, int T_in,
                                                  int t_end, float gate_threshold, float p_prenet, uint64_t seed,
                                                  const t2v_dec_items* items, void* stream_) {
    if (!items) return T2V_ERR_ARG;
    return pd_launch(w, s, B, T_in, t_end, gate_threshold, p_prenet, seed, items, nullptr, nullptr, (hipStream_t)stream_);
}

// the same with the attention window of t2v_dec_window; items may be NULL (one seed, the global stop rule alone)
extern "C" int t2v_decoder_infer_persistent_window(const t2v_dec_persist_weights* w, const t2v_dec_persist_bufs* s, int B, int T_in,
                                                   int t_end, float gate_threshold, float p_prenet, uint64_t seed,
                                                   const t2v_dec_items* items, const t2v_dec_window* window, void* stream_) {
    if (!window) return T2V_ERR_ARG;
    return pd_launch(w, s, B, T_in, t_end, gate_threshold, p_prenet, seed, items, window, nullptr, (hipStream_t)stream_);
}

// the planned decode: the window around plan[b, min(t, n_plan[b] - 1)]; items may be NULL
extern "C" int t2v_decoder_infer_persistent_plan(const t2v_dec_persist_weights* w, const t2v_dec_persist_bufs* s, int B, int T_in,
                                                 int t_end, float gate_threshold, float p_prenet, uint64_t seed,
                                                 const t2v_dec_items* items, const t2v_dec_window* window, const int32_t* plan,
                                                 int plan_stride, const int32_t* n_plan, void* stream_) {
    if (!window) return T2V_ERR_ARG;
    const PersistPlan pl = {0, 0, plan, n_plan, plan_stride};
    return pd_launch(w, s, B, T_in, t_end, gate_threshold, p_prenet, seed, items, window, &pl, (hipStream_t)stream_);
}
