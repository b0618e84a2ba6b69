/* libt2vae_hip — C ABI of the MI355X-native Tacotron2-VAE hot path.
 *
 * The reference (jinhan/tacotron2-vae) has no FFI of its own: its hot path sits behind Python
 * module names.  This header is the boundary our host-side mirror
 * (the Python modules under tacotron2-vae_amd/) binds with ctypes; each entry point cites the reference code it
 * replaces.  All pointers are DEVICE pointers owned by the caller (PyTorch's allocator in our
 * host code); the library allocates nothing, launches asynchronously on `stream`
 * (a hipStream_t passed as void*), and returns 0 or a negative t2v error code.
 * Layouts are row-major fp32 unless stated; LSTM gates are stacked i,f,g,o (PyTorch order).
 */
#ifndef T2VAE_H
#define T2VAE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define T2V_OK 0
#define T2V_ERR_DIMS -1     /* geometry differs from the compiled default hparams */
#define T2V_ERR_ARG -2      /* null pointer / bad size */
#define T2V_ERR_LAUNCH -3   /* hipGetLastError() != hipSuccess after a launch */

const char* t2v_version(void);
/* last HIP error string recorded by a failing call (thread-local) */
const char* t2v_last_error(void);

/* Tracing aid: device buffer of 32 uint64 that the attention kernels fill with s_memtime stamps at
 * their phase boundaries (forward slots 0..7, backward 16..23); NULL (default) disables it. */
void t2v_set_phase_profile(unsigned long long* dev_buf32);
/* Measurement aid: a one-thread launch on `stream` that writes the chip-wide 100 MHz wall clock into dev_buf[slot]
 * (phase time line of an undisturbed graph replay: tools/stamps.py). */
int t2v_stamp(unsigned long long* dev_buf, int slot, void* stream);
/* Test aid: `wgs` workgroups (256 threads each) that occupy CUs for `microseconds` doing nothing — a stand-in for a
 * neighbour (another process, a communication kernel) while the persistent kernels start. */
int t2v_debug_spin(int wgs, int microseconds, void* stream);

/* Per-step parameters in DEVICE memory (optional).  Kernel arguments are frozen when a training step is captured
 * into a HIP graph; this 32-byte record is read by the kernels at run time instead, so every replay gets fresh
 * dropout masks (epoch is mixed into every dropout seed: seed + epoch * 0x9E3779B97F4A7C15), the right Adam bias
 * corrections / learning rate and KL weight.  NULL (default): the by-value arguments of each call are used. */
typedef struct t2v_step_params {
    uint64_t epoch;      /* training iteration */
    float lr;            /* Adam step size (train.py:209-210 sets it every iteration) */
    float bc1;           /* 1 - beta1^t */
    float bc2s;          /* sqrt(1 - beta2^t) */
    float kl_weight;     /* loss_function.py:15-24 */
    float pad[2];
} t2v_step_params;
void t2v_set_step_params(const t2v_step_params* dev);
/* Per-stream binding (one training engine = one rank = one stream, SURVEY.md 8(b) "thread-safe per ctx"): launches on
 * `stream` read THIS record; launches on a stream without a binding read the process default above.  dev = NULL removes
 * the binding.  Two engines in one process therefore never share a step record as long as each runs on its own stream. */
int t2v_set_step_params_stream(void* stream, const t2v_step_params* dev);

/* ------------------------------------------------------------------ weight packing
 * Re-lays the two decoder LSTM cells' weights into MFMA-fragment order for the per-step
 * weight-streaming kernels.  Replaces nothing in the reference (cuDNN/cuBLAS choose their own
 * layouts); inputs are the nn.LSTMCell tensors themselves (model.py:224-235), read in place:
 *   w_ih_att (4096,768) [prenet | ctx], w_hh_att (4096,1024), w_ih_dec (4096,1536) [h_att | ctx], w_hh_dec (4096,1024)
 *   logical Wcat_att (4096,k_att) = [w_hh_att | w_ih_att[:,256:768] (| w_ih_att[:,0:256])]
 *              k_att = 1536 (training; prenet term hoisted) or 1792 (inference)
 *   logical Wcat_dec (4096,2560)  = [w_ih_dec | w_hh_dec]
 *   packF_*  : forward tiles,  4096*k_att and 4096*2560 floats
 *   packB_*  : transposed tiles for the backward data-gradient GEMV, 4096*1536 and 4096*2560 floats (may be NULL)
 *   packF_att and packF_dec may BOTH be NULL when only the transposed tiles are wanted (forward on the persistent kernel) */
int t2v_pack_lstm_weights(const float* w_ih_att, const float* w_hh_att, const float* w_ih_dec,
                          const float* w_hh_dec, int k_att, float* packF_att, float* packF_dec,
                          float* packB_att, float* packB_dec, void* stream);
/* bf16_run: the same tiles with every weight rounded to bf16 (RNE), laid out in 32-column blocks (16 bytes = 8 values per
 * lane and block: lane l of a 16-row tile holds columns 32 kb + 8 (l >> 4) .. + 8): the two per-step LSTM kernels then
 * stream 33.5 MB instead of 67 MB with HALF the weight-load instructions and multiply bf16-rounded states on
 * v_mfma_f32_16x16x32_bf16 (fp32 accumulation, fp32 cell state, fp32 saved activations).  Same buffer sizes or half. */
int t2v_pack_lstm_weights_bf16(const float* w_ih_att, const float* w_hh_att, const float* w_ih_dec,
                               const float* w_hh_dec, int k_att, void* packF_att, void* packF_dec,
                               void* packB_att, void* packB_dec, void* stream);

/* LocationLayer (model.py:12-28) is a bias-free conv followed by a bias-free linear layer, i.e. ONE linear map of the
 * 2 x 31 alignment window: W_comb[d][32c + k] = sum_f loc_dense[d][f] * loc_conv[f][c][k] (128 x 64; k < 31, columns
 * 31 and 63 are zero).  The attention kernels evaluate the layer (and its backward) through this fused filter bank.
 * wcomb: 2*128*64 floats, W_comb stored twice in the order the consuming lanes read it as float4 runs:
 *   [0, 8192)      F[d][g][st]  = W_comb[d][4st + g]     (g < 4, st < 16)   forward
 *   [8192, 16384)  R[kk][g][st] = W_comb[4st + g][kk]    (g < 4, st < 32)   backward
 * Call once per pass after the weights changed. */
int t2v_fuse_location_weights(const float* loc_conv, const float* loc_dense, float* wcomb, void* stream);

typedef struct t2v_dec_weights {
    const float* packF_att;   /* from t2v_pack_lstm_weights */
    const float* packF_dec;
    const float* packB_att;   /* NULL for inference */
    const float* packB_dec;
    const float* bias_att;    /* (4096) bias_ih+bias_hh; used only when gpre == NULL */
    const float* bias_dec;    /* (4096) bias_ih+bias_hh */
    const float* wqT;         /* (1024,128) query_layer weight, transposed (model.py:35) */
    const float* wcomb;       /* (2,128,64) fused location filter bank (t2v_fuse_location_weights; model.py:17-22) */
    const float* v;           /* (128)      attention v (model.py:39) */
    int32_t packs_bf16;       /* != 0: the four packs came from t2v_pack_lstm_weights_bf16 (hparams bf16_run) */
} t2v_dec_weights;

/* Saved-activation arena of one teacher-forced decoder pass (caller allocates; t2v_decoder_train_fwd clears the rows
 * marked "row 0 = 0" — the zero initial states of model.py:280-296 — together with its sync words in one launch). */
typedef struct t2v_dec_train_bufs {
    const float* gpre;      /* (T,B,4096)  prenet(x_t)·W_ih[:, :256]^T + b_ih + b_hh */
    const float* memory;    /* (B,T_in,512) encoder outputs + style */
    const float* pm;        /* (B,T_in,128) memory_layer(memory) (model.py:290) */
    const int32_t* lengths; /* (B) valid encoder positions; NULL = no mask */
    float* XS;    /* (T+2,B,2560) XS[t+1] = [h_att_t | ctx_t | h_dec_{t-1}]; row 0 = 0 (rows 0..1 are cleared) */
    float* CA;    /* (T+1,B,1024) pre-dropout cell of attention_rnn; row 0 = 0 */
    float* CD;    /* (T+1,B,1024) pre-dropout cell of decoder_rnn;   row 0 = 0 */
    float* GA;    /* (T,B,4096) gate activations i,f,g,o of attention_rnn; NULL (with GD, S) = forward only */
    float* GD;    /* (T,B,4096) gate activations of decoder_rnn */
    float* QP;    /* (t2v_decoder_qp_floats(B, T_in)) scratch: per-workgroup partial queries, sync / error words, the
                     decode loop's exchange area, then the attention kernel's energy-exchange granules */
    float* AL;    /* (T+1,B,T_in) AL[t+1] = attention weights of step t; row 0 = 0 */
    float* ACUM;  /* (T+1,B,T_in) cumulative weights; row 0 = 0 */
    float* S;     /* (T,B,T_in,128) tanh(...) of the energies; overwritten with dpre by bwd; NULL = forward only */
} t2v_dec_train_bufs;

/* floats the QP scratch needs for (B, T_in): B*256*128 + 4160 + 2*B*8*ceil16(T_in) */
long t2v_decoder_qp_floats(int B, int T_in);

/* Decoder.forward's time loop (model.py:415-421 → Decoder.decode 346-389 → Attention.forward
 * 67-88), teacher forced, both LSTM cells + location-sensitive attention.  The 80-mel/gate
 * projection (model.py:385-388) is hoisted out of the loop: it reads [h_dec_t | ctx_t] from XS.
 * Dropout on the LSTM states (model.py:361-364,378-381) uses a counter-based RNG keyed by
 * (seed, stream, t, b, unit); p = 0 disables it.  B <= 16 per call (callers split larger batches: items are
 * independent inside the loop); 1 <= T_in <= 4096 (the reference is unbounded; koemo reaches 555 symbols). */
int t2v_decoder_train_fwd(const t2v_dec_weights* w, const t2v_dec_train_bufs* s,
                          int B, int T_in, int T_out, float p_att, float p_dec,
                          uint64_t seed, void* stream);
/* The same forward loop as ONE persistent launch (csrc/decoder_train_persist.hip): 256 workgroups stay resident for all
 * T_out steps, the LSTM weights of both cells live in registers (read once per pass from the nn.LSTMCell tensors — no
 * packs), attention_rnn -> attention -> attention_rnn is the only per-step dependency chain (teacher forcing: decoder_rnn
 * trails one step behind on the same workgroups), and the recurrent state travels between CUs THROUGH a sentinel-filled
 * copy of the saved activations (`scratch`): a word that is no longer 0xFFFFFFFF has been produced — no tags, no flags,
 * no grid barrier.  Writes the same arena as t2v_decoder_train_fwd (XS, CA, CD, GA, GD, AL, ACUM, S; QP only supplies
 * the error word), so t2v_decoder_train_bwd runs on it unchanged; dropout masks are the same counter-based ones, i.e.
 * the two paths agree to fp32 summation order.  Supported when t2v_decoder_train_persist_supported(B, T_in) != 0:
 * B <= 6, T_in <= 560 (round 6; up to 224 symbols the attention workgroups keep their W_q / processed-memory slices in LDS,
 * beyond in registers), a device with >= 256 CUs that can hold one 512-thread workgroup with this LDS carve per CU.
 * scratch: t2v_decoder_train_persist_scratch_floats(B, T_in, T_out) floats, 16-byte aligned (filled by the call). */
typedef struct t2v_dec_train_persist_weights {
    const float* w_ih_att; const float* w_hh_att;   /* attention_rnn (4096,768) [prenet | ctx], (4096,1024) */
    const float* w_ih_dec; const float* w_hh_dec;   /* decoder_rnn   (4096,1536) [h_att | ctx], (4096,1024) */
    const float* bias_dec;  /* (4096) bias_ih + bias_hh of decoder_rnn (attention_rnn's biases are inside gpre) */
    const float* wq;        /* (128,1024) query_layer weight (model.py:35), NOT transposed */
    const float* wcomb;     /* t2v_fuse_location_weights output */
    const float* v;         /* (128) */
} t2v_dec_train_persist_weights;
int t2v_decoder_train_persist_supported(int B, int T_in);
long t2v_decoder_train_persist_scratch_floats(int B, int T_in, int T_out);
int t2v_decoder_train_fwd_persistent(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s, float* scratch,
                                     int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed, void* stream);

/* The same pass for hparams.bf16_run (BASELINE configs[4]: B = 16 per GPU; replaces reference fp16_optimizer.py:51-382 /
 * train.py:22-28 on the decoder loop model.py:415-421, 346-389): B <= 16, T_in <= 560.  The LSTM weights are rounded to bf16
 * (RNE, as t2v_pack_lstm_weights_bf16) into MFMA tiles that stay in registers for the whole pass — a workgroup owns 8 hidden
 * units of both cells, the batch is the N dimension of v_mfma_f32_16x16x32_bf16 — the recurrent state travels between the
 * workgroups as bf16 rows laid out as the MFMA's B operand; fp32 accumulation, cell state, attention and saved activations,
 * i.e. the arithmetic of t2v_decoder_train_fwd with bf16 packs (packs_bf16 = 1).  Same arena, same dropout masks.
 * scratch: t2v_decoder_train_persist16_scratch_floats(B, T_in, T_out) floats, 16-byte aligned (filled by the call). */
int t2v_decoder_train_persist16_supported(int B, int T_in);
long t2v_decoder_train_persist16_scratch_floats(int B, int T_in, int T_out);
int t2v_decoder_train_fwd_persistent16(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s, float* scratch,
                                       int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed, void* stream);

/* Measurement aid for bench.py: re-issues only the selected kernels of a finished forward pass on
 * its saved arena (bit0 = k_lstm_fwd256 (both LSTM cells), bit1 = k_attn_fwd),
 * so their average launch duration can be bracketed with events on `stream`.  Results are
 * bit-identical to the first pass (the kernels are pure functions of the arena). */
int t2v_decoder_replay_fwd_kernels(const t2v_dec_weights* w, const t2v_dec_train_bufs* s,
                                   int B, int T_in, int T_out, float p_att, float p_dec,
                                   uint64_t seed, int kernel_mask, void* stream);

typedef struct t2v_dec_bwd_bufs {
    const float* dHC;  /* (T,B,1536) grad wrt [h_dec_t | ctx_t] coming from the projection */
    float* DGA;   /* (T,B,4096) out: grad wrt attention_rnn pre-activations (== grad of gpre) */
    float* DGD;   /* (T,B,4096) out: grad wrt decoder_rnn pre-activations */
    float* DQ;    /* (T,B,S,128,2) out: per-position-slice partials of the grad wrt the processed query as 8-byte
                     {value, tag} granules ([...,0] = value; sum over dim 2), S = t2v_attn_bwd_slices(T_in) */
    float* DCTX;  /* (T,B,512)  out: grad wrt attention context */
    float* YD;    /* (B,2560) scratch, zeroed by the call */
    float* YA;    /* (B,1536) scratch, zeroed by the call */
    float* DCA;   /* (B,1024) scratch */
    float* DCD;   /* (B,1024) scratch */
    float* GPREV; /* (2,B,S,2,64) scratch: per-slice partial alignment-window gradients, parity double-buffered */
    float* GCUM;  /* (B*S*ceil16(T_in) + 64) scratch: per-workgroup copies of the cumulative-weights gradient, then
                     sync words ([1] != 0 afterwards: a bounded spin timed out) */
    float* DV;    /* (B,S,128) out: per-item, per-slice grad of attention v (sum over dims 0,1 = dv) */
} t2v_dec_bwd_bufs;

/* position slices per item of the attention backward: ceil(T_in / 16) for T_in <= 128, else ceil(T_in / 32) */
int t2v_attn_bwd_slices(int T_in);

/* Hand-written BPTT of the loop above (what autograd does for the reference at train.py:225).
 * On return S holds dpre = grad wrt (q + loc + pm) per (t,b,j,d). */
int t2v_decoder_train_bwd(const t2v_dec_weights* w, const t2v_dec_train_bufs* s,
                          const t2v_dec_bwd_bufs* g, int B, int T_in, int T_out,
                          float p_att, float p_dec, uint64_t seed, void* stream);

/* Measurement aid like t2v_decoder_replay_fwd_kernels for the reverse pass (bit0 = k_lstm_bwd256, bit1 = k_attn_cell_bwd) on the
 * buffers of a finished backward.  Timing only: S already holds dpre, so the replayed attention backward is not a
 * second valid gradient (the launch shapes, operand sizes and hand-offs are those of the real pass). */
int t2v_decoder_replay_bwd_kernels(const t2v_dec_weights* w, const t2v_dec_train_bufs* s,
                                   const t2v_dec_bwd_bufs* g, int B, int T_in, int T_out,
                                   float p_att, float p_dec, uint64_t seed, int kernel_mask, void* stream);

/* Deferred weight gradients of the location layer (model.py:24-28) reduced over the whole decoder pass in one
 * streaming kernel + a fixed-order partial sum (what autograd accumulates step by step at train.py:225), through
 * the fused filter bank:  dW_comb[d][c,k] = sum_{t,b,j} dpre[t,b,j,d] * a_c[t,b,j+k-15], then
 *   d_loc_dense (128,32)  = dW_comb · loc_conv^T,   d_loc_conv (32,2,31) = loc_dense^T · dW_comb.
 * dpre = S after t2v_decoder_train_bwd, al/acum = rows 0..T-1 of AL/ACUM (a_0 / a_1).
 * part_scratch: t2v_attn_wgrad_scratch_floats() floats. */
int t2v_attn_wgrad_scratch_floats(void);
int t2v_attn_wgrad(const float* dpre, const float* al, const float* acum, const float* loc_conv,
                   const float* loc_dense, float* part_scratch, float* d_loc_dense, float* d_loc_conv,
                   int B, int T_in, int T, void* stream);


/* ------------------------------------------------------------------ persistent BPTT (csrc/decoder_train_bwd_persist.hip)
 * The reverse recurrence of the decoder loop as one persistent launch for the shapes of the persistent forward
 * (t2v_decoder_bwd_persist_supported: B <= 6, T_in <= 576 — 96-position attention slices beyond 224 symbols —, >= 256 CUs).
 * err_word (1 x uint32, zeroed by the call): != 0 afterwards = a bounded spin timed out. */
int t2v_decoder_bwd_persist_supported(int B, int T_in);
/* The WHOLE reverse pass as ONE persistent launch (k_achain_bwd): attention_rnn + attention form the per-step dependency
 * chain (all-gather dga(t+1) -> Wcat_att^T columns -> d ctx(t) -> attention(t) backward on position-split workgroups ->
 * dq(t) -> W_q^T, cell backward -> dga(t)); decoder_rnn's chain (cell backward, all-gather of dgd, Wcat_dec^T columns)
 * runs one step ahead on the same workgroups in the shadow of the attention workgroups.  All transposed LSTM weight
 * columns live in registers (read once per pass from the nn.LSTMCell tensors).  Same outputs as t2v_decoder_train_bwd:
 *   DGA, DGD (T,B,4096), DCTX (T,B,512), S overwritten with dpre, DV (B,S,128) per-slice partial dv (sum dims 0,1),
 *   DQP (T,B,S,128) per-slice partial dq rows (sum over dim 2 = dq of a step), S = t2v_attn_bwd_slices(T_in).
 * w: the struct of the persistent forward (bias_dec unused); s: the forward pass's arena (gpre, QP unused);
 * scratch: t2v_decoder_bwd_achain_scratch_floats(B, T_in, T_out) floats, 16-byte aligned; DQP 16-byte aligned. */
long t2v_decoder_bwd_achain_scratch_floats(int B, int T_in, int T_out);
/* position slices per item of the ONE-LAUNCH reverse pass (second-to-last dimension of its DQP (T,B,S,128) and DV (B,S,128)):
 * t2v_attn_bwd_slices(T_in) up to 224 symbols, ceil(T_in / 96) beyond */
int t2v_decoder_bwd_persist_slices(int T_in);
/* Weight-gradient epilogue of the pass (dw, may be NULL = none): the decoder_rnn workgroups finish their chain well before the
 * attention_rnn chain ends; with dw they then work on [d_w_ih_dec | d_w_hh_dec] (+)= DGD^T · x_cur, the second group of the grouped
 * product t2v_gemm_f32_grouped {(DGA^T, ...), (DGD^T, [x_cur[:, :1536], x_cur[:, 1536:]])} with M = 4096, K = T_out * B: they write that
 * group's operand planes to `planes` (= grouped scratch + t2v_gemm_f32_grouped_group_offset(.., 1)) and take 128 x 128 tiles from the
 * counter at scratch + t2v_decoder_bwd_achain_dw_offset() until the attention_rnn chain is about to end or tile_cap (< 0: none)
 * is reached.  t2v_gemm_f32_grouped_handed(.., handed = 1, that counter, tile_cap) must follow on the same buffers: it computes the
 * rest.  A tile has the same bits whichever kernel computes it.  x3 mode only (t2v_gemm_f32_set_mode), T_out * B >= 32. */
typedef struct t2v_achain_dw {
    float* planes;
    float* d_w_ih; int ld_ih;       /* (4096, 1536), row stride in floats */
    float* d_w_hh; int ld_hh;       /* (4096, 1024) */
    int accumulate;                 /* add to d_w_* instead of overwriting them */
    int tile_cap;                   /* tests: at most this many tiles in the pass (< 0: no cap; 0: planes only) */
} t2v_achain_dw;
long t2v_decoder_bwd_achain_dw_offset(int B, int T_in, int T_out);
int t2v_decoder_bwd_achain(const t2v_dec_train_persist_weights* w, const t2v_achain_dw* dw, const t2v_dec_train_bufs* s,
                           const float* dHC, float* DGA, float* DGD, float* DCTX, float* DV, float* DQP, float* scratch,
                           uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed,
                           void* stream);
/* The reverse pass for hparams.bf16_run, B <= 16 (BASELINE configs[4]; the bf16 counterpart of t2v_decoder_bwd_achain: same
 * arithmetic as t2v_decoder_train_bwd with bf16 packs — transposed LSTM weights and gate gradients rounded to bf16 in front of
 * every product, fp32 accumulation, fp32 cell / attention backward).  ONE persistent launch: Wcat^T lives in registers as bf16
 * MFMA tiles, cut into 128-column x 1024-row blocks (48 + 80 workgroups publish partial column sums), 16 + 16 workgroups run
 * the cells of 64 hidden units each, B * S workgroups the attention backward (S = t2v_decoder_bwd_persist16_slices(T_in):
 * slices of 16 positions up to 96 symbols, 32 up to 192, 96 beyond).  Supported when B <= 16, T_in <= 560 (B * S <= 96 always holds).
 * DV (B,S,128), DQP (T_out,B,S,128), scratch: t2v_decoder_bwd_persist16_scratch_floats() floats, 16-byte aligned (filled by
 * the call); dq(t) summed over the slices lies at float offset t2v_decoder_bwd_persist16_dq_offset() of scratch as
 * (T_out, 16, 128).  err_word: set to 1 when a bounded spin gave up (results invalid). */
int t2v_decoder_bwd_persist16_supported(int B, int T_in);
int t2v_decoder_bwd_persist16_slices(int T_in);
/* ... and at this T_out: 1 when every exchange array stays below the 2^31-byte reach of the kernel's buffer offsets (the widest
 * one reaches it at T_out = 3 277) — what a caller asks before its FORWARD pass commits to this reverse pass. */
int t2v_decoder_bwd_persist16_fits(int B, int T_in, int T_out);
long t2v_decoder_bwd_persist16_scratch_floats(int B, int T_in, int T_out);
long t2v_decoder_bwd_persist16_dq_offset(int B, int T_in, int T_out);
int t2v_decoder_bwd_persistent16(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s, const float* dHC,
                                 float* DGA, float* DGD, float* DCTX, float* DV, float* DQP, float* scratch,
                                 uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed,
                                 void* stream);
/* Its preparation (error word, sentinel fills of scratch and DQP: functions of nothing but the buffers, so a training step
 * issues it on a side stream right behind the decoder forward) as a call of its own, and the pass without it. */
int t2v_decoder_bwd_persistent16_prepare(float* DQP, float* scratch, uint32_t* err_word, int B, int T_in, int T_out, void* stream);
int t2v_decoder_bwd_persistent16_prepared(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s, const float* dHC,
                                          float* DGA, float* DGD, float* DCTX, float* DV, float* DQP, float* scratch,
                                          uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed,
                                          void* stream);

/* float offset inside `scratch` of dq(t) summed over the position slices, (T_out,B,128) floats, valid when the pass has ended
 * (-1: shape outside the persistent range) */
long t2v_decoder_bwd_achain_dq_offset(int B, int T_in, int T_out);
/* The preparation of t2v_decoder_bwd_achain as a call of its own (error word, sentinel fills, the factor arrays of both cells — functions
 * of the forward pass's saved activations alone, so a training step issues it right after the decoder forward, on a side
 * stream, next to the Postnet), and the pass without it.  scratch / DQP / err_word: the same buffers in both calls. */
int t2v_decoder_bwd_achain_prepare(const t2v_dec_train_bufs* s, float* DQP, float* scratch, uint32_t* err_word, int B, int T_in,
                                   int T_out, float p_att, float p_dec, uint64_t seed, void* stream);
int t2v_decoder_bwd_achain_prepared(const t2v_dec_train_persist_weights* w, const t2v_achain_dw* dw, const t2v_dec_train_bufs* s,
                           const float* dHC, float* DGA, float* DGD, float* DCTX, float* DV, float* DQP, float* scratch,
                           uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed,
                           void* stream);

/* ------------------------------------------------------------------ reverse passes with an alignment gradient
 * The five reverse passes above for a loss that reads the attention itself (t2v_guided_attention): the same calls with one more
 * operand, dAL — the upstream gradient of the alignments, contiguous (T_out, B, T_in) floats, dAL[t] belonging to the alignment of
 * decoder step t (arena row AL[t + 1]).  Inside the softmax backward of step t it is one more addend of the gradient with respect
 * to alpha(t).  dAL == NULL: no such gradient — the pass is then the kernel of the call above, bit for bit (the calls above are
 * these with NULL). */
int t2v_decoder_train_bwd_align(const t2v_dec_weights* w, const t2v_dec_train_bufs* s,
                                const t2v_dec_bwd_bufs* g, const float* dAL, int B, int T_in, int T_out,
                                float p_att, float p_dec, uint64_t seed, void* stream);
int t2v_decoder_bwd_achain_align(const t2v_dec_train_persist_weights* w, const t2v_achain_dw* dw, const t2v_dec_train_bufs* s,
                                 const float* dHC, const float* dAL, float* DGA, float* DGD, float* DCTX, float* DV, float* DQP,
                                 float* scratch, uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec,
                                 uint64_t seed, void* stream);
int t2v_decoder_bwd_achain_prepared_align(const t2v_dec_train_persist_weights* w, const t2v_achain_dw* dw,
                                          const t2v_dec_train_bufs* s, const float* dHC, const float* dAL, float* DGA, float* DGD,
                                          float* DCTX, float* DV, float* DQP, float* scratch, uint32_t* err_word, int B, int T_in,
                                          int T_out, float p_att, float p_dec, uint64_t seed, void* stream);
int t2v_decoder_bwd_persistent16_align(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s, const float* dHC,
                                       const float* dAL, float* DGA, float* DGD, float* DCTX, float* DV, float* DQP, float* scratch,
                                       uint32_t* err_word, int B, int T_in, int T_out, float p_att, float p_dec, uint64_t seed,
                                       void* stream);
int t2v_decoder_bwd_persistent16_prepared_align(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s,
                                                const float* dHC, const float* dAL, float* DGA, float* DGD, float* DCTX, float* DV,
                                                float* DQP, float* scratch, uint32_t* err_word, int B, int T_in, int T_out,
                                                float p_att, float p_dec, uint64_t seed, void* stream);

/* ------------------------------------------------------------------ guided attention loss (csrc/guided_attention.hip)
 * The penalty on attention weight far from the diagonal (Tachibana et al., DCTTS; ESPnet's GuidedAttentionLoss), value and gradient:
 *   W[b][t][j] = 1 - exp(-(j / N_b - t / T_b)^2 / (2 sigma^2))  for t < T_b and j < N_b, else 0      (N_b = in_len[b], T_b = out_len[b])
 *   D = sum_b T_b N_b,   L = sum A W / D,   G = W / D.
 * A: alignments (B, T, T_in) with element strides sb, st, sj (whatever layout the decoder returned them in).  loss: one float.
 * G: contiguous (T, B, T_in) — the dAL operand of the passes above.  part: t2v_guided_attention_part_doubles(B, T) doubles of
 * scratch.  Products in fp32, summed in fp64 in an order fixed by the shapes: the same bits from run to run.  D is computed on the
 * device; nothing is read back, and the call can be captured in a graph.  Lengths are clamped to [0, T] / [0, T_in]. */
long t2v_guided_attention_part_doubles(int B, int T);
int t2v_guided_attention(const float* A, long sb, long st, long sj, const int64_t* in_len, const int64_t* out_len,
                         float* loss, float* G, double* part, int B, int T, int T_in, float sigma, void* stream);

/* ------------------------------------------------------------------ free-running decode
 * Decoder.inference (model.py:428-464) == the synthesizer loop (synthesizer.py:139-154): steps
 * t_begin..t_end-1, each = attention_rnn → attention → decoder_rnn → 80-mel/gate projection → Prenet of
 * the new frame (dropout p_prenet stays on at inference, model.py:101).  The caller runs chunks and reads
 * `stop_flag` (first t with sigmoid(gate) > gate_threshold for every item, INT_MAX if none) between
 * them.  external_prenet != 0: PRE[t] is supplied by the caller for every step (the per-step
 * `decoder.prenet(x)` + `decoder.decode(x)` call sequence) and no Prenet is evaluated here.
 * Arena rows as in t2v_dec_train_bufs (XS (Tmax+2,B,2560) rows 0,1 zeroed; CA/CD/AL/ACUM row 0 zeroed);
 * PRE[0] = Prenet(go frame) is written by the caller.  B <= 8, T_in <= 4096; QP as in t2v_dec_train_bufs. */
typedef struct t2v_dec_infer_bufs {
    const float* memory;     /* (B,T_in,512) */
    const float* pm;         /* (B,T_in,128) */
    const int32_t* lengths;  /* NULL at inference (mask=None, model.py:441) */
    float* XS; float* CA; float* CD; float* QP; float* AL; float* ACUM;
    float* PRE;              /* (Tmax+1,B,256) prenet outputs */
    float* MEL;              /* (Tmax,B,80) out */
    float* GATE;             /* (Tmax,B)    out */
    int32_t* stop_flag;      /* (1) */
    const float* prenet_w1;  /* (256,256) Prenet layer 1 */
    const float* proj_w;     /* (337,1536) rows 0..79 = linear_projection, row 80 = gate_layer, rows 81..336 = W0·linear_projection
                                (Prenet layer 0 is bias-free and linear in the mel frame: folded so it need not wait for it) */
    const float* proj_b;     /* (337) linear_projection / gate_layer biases, then W0·b_projection */
} t2v_dec_infer_bufs;

int t2v_decoder_infer_steps(const t2v_dec_weights* w, const t2v_dec_infer_bufs* s, int B, int T_in,
                            int t_begin, int t_end, float gate_threshold, float p_prenet,
                            int external_prenet, uint64_t seed, void* stream);

/* The same loop as ONE persistent launch (csrc/decoder_persist.hip): 256 workgroups stay resident for the whole
 * utterance, all weights in registers / LDS, the per-frame state vectors travel between CUs as 4-byte values in a sentinel-filled row per frame,
 * the loop ends on the frame the gate fires (nothing is computed after it).  Runs frames 0..t_end-1 from the zero state;
 * pre_first = Prenet(go frame).  Supported when t2v_decoder_persist_supported(B, T_in) != 0 (B <= 4 and the attention
 * operands of T_in positions fit the 160 KB LDS: T_in <= 224 at B = 1, 192 at B = 2, 160 at B = 3, 128 at B = 4); everything else
 * takes t2v_decoder_infer_steps.
 * Weights are the nn.LSTMCell / LinearNorm tensors themselves (no packing). */
typedef struct t2v_dec_persist_weights {
    const float* w_ih_att; const float* w_hh_att;   /* (4096,768) [prenet | ctx], (4096,1024) */
    const float* w_ih_dec; const float* w_hh_dec;   /* (4096,1536) [h_att | ctx], (4096,1024) */
    const float* bias_att; const float* bias_dec;   /* (4096) b_ih + b_hh */
    const float* wq;        /* (128,1024) query_layer weight */
    const float* wcomb;     /* t2v_fuse_location_weights output */
    const float* v;         /* (128) */
    const float* proj_w;    /* (337,1536) as in t2v_dec_infer_bufs */
    const float* proj_b;    /* (337) */
    const float* prenet_w1; /* (256,256) */
} t2v_dec_persist_weights;
typedef struct t2v_dec_persist_bufs {
    const float* memory;     /* (B,T_in,512) */
    const float* pm;         /* (B,T_in,128) */
    const int32_t* lengths;  /* NULL at inference */
    const float* pre_first;  /* (B,256) */
    float* MEL;              /* (t_end,B,80) out */
    float* GATE;             /* (t_end,B) out */
    float* AL;               /* (t_end+1,B,T_in) out: row t+1 = attention weights of frame t */
    int32_t* stop_flag;      /* (1): first frame on which every item's gate fired (caller presets INT_MAX) */
    void* exchange;          /* t2v_decoder_persist_scratch_floats(B, t_end) floats of exchange rows, 16-byte aligned (filled by the call) */
    uint32_t* err_word;      /* (1): != 0 afterwards: a bounded spin timed out */
} t2v_dec_persist_bufs;
long t2v_decoder_persist_scratch_floats(int B, int t_end);
int t2v_decoder_persist_supported(int B, int T_in);
int t2v_decoder_infer_persistent(const t2v_dec_persist_weights* w, const t2v_dec_persist_bufs* s, int B, int T_in,
                                 int t_end, float gate_threshold, float p_prenet, uint64_t seed, void* stream);

/* Per-item variants of both decode loops, for a batch of texts decoded together (model.py Decoder.inference_batch).
 * The global stop rule is unchanged (every item fired); in addition
 *   stop_item[b]  receives the first frame on which item b's gate fired (atomicMin; the caller presets INT_MAX);
 *   item_seeds[b] replaces `seed` for item b, and its Prenet-0/1 dropout masks use the element index of item 0: exactly the
 *                 mask stream of a B = 1 decode with seed item_seeds[b].
 * Both pointers are device arrays of B entries and must be set.  The entries without `_items` are unchanged. */
typedef struct t2v_dec_items {
    int32_t* stop_item;          /* (B) */
    const uint64_t* item_seeds;  /* (B) */
} t2v_dec_items;
int t2v_decoder_infer_steps_items(const t2v_dec_weights* w, const t2v_dec_infer_bufs* s, int B, int T_in,
                                  int t_begin, int t_end, float gate_threshold, float p_prenet,
                                  int external_prenet, uint64_t seed, const t2v_dec_items* items, void* stream);
int t2v_decoder_infer_persistent_items(const t2v_dec_persist_weights* w, const t2v_dec_persist_bufs* s, int B, int T_in,
                                       int t_end, float gate_threshold, float p_prenet, uint64_t seed,
                                       const t2v_dec_items* items, void* stream);

/* Attention window of the free-running decode (an attention constraint; Decoder.attention_window = (back, ahead), two
 * integers >= 0).  For item b at frame t:
 *   - p is the index of the largest weight of the item's alignment of frame t-1.  Ties go to the lowest index.  Frame 0 sees
 *     the all-zero initial weights, so p = 0.
 *   - The energies of all positions outside p - back <= j <= p + ahead are treated as -inf.  So are all positions
 *     j >= len_b (lengths[b]; T_in without lengths).
 *   - Softmax, context, cumulative weights and everything downstream are unchanged.
 * Weights outside the window are exactly 0.0.  The window always contains p, so it is never empty.  The cumulative weights
 * keep accumulating the windowed weights, so the location features see what the constrained decoder did.
 * Free-running decode only: the teacher-forced pass and training have no window.
 * The two entries below take the arguments of the `_items` entries plus the window (a host struct, read during the call;
 * back, ahead >= 0, values above T_in mean T_in).  `items` may be NULL here: one seed and the global stop rule, as the entries
 * without `_items`.  A call of t2v_decoder_infer_steps_window with t_begin > 0 continues a decode begun with the same window.
 * t2v_decoder_infer_persistent_window runs where t2v_decoder_persist_supported(B, T_in) != 0, as the other two. */
typedef struct t2v_dec_window {
    int32_t back;    /* positions kept behind p */
    int32_t ahead;   /* positions kept in front of p */
} t2v_dec_window;
int t2v_decoder_infer_steps_window(const t2v_dec_weights* w, const t2v_dec_infer_bufs* s, int B, int T_in,
                                   int t_begin, int t_end, float gate_threshold, float p_prenet,
                                   int external_prenet, uint64_t seed, const t2v_dec_items* items,
                                   const t2v_dec_window* window, void* stream);
int t2v_decoder_infer_persistent_window(const t2v_dec_persist_weights* w, const t2v_dec_persist_bufs* s, int B, int T_in,
                                        int t_end, float gate_threshold, float p_prenet, uint64_t seed,
                                        const t2v_dec_items* items, const t2v_dec_window* window, void* stream);

/* Duration plan of the free-running decode (rhythm control; Decoder.inference(plan=, n_plan=)).  The window centre p of the
 * attention window above no longer comes from the previous frame's weights but from a plan, device data that names one symbol
 * per frame.  For item b at frame t:
 *   - q = plan[b * plan_stride + min(t, n_plan[b] - 1)];
 *   - p = min(max(q, 0), len_b - 1)  (len_b = lengths[b]; T_in without lengths);
 *   - everything else is the window's: the energies of all positions outside p - back <= j <= p + ahead, and of all positions
 *     j >= len_b, are treated as -inf.  Weights outside the window are exactly 0.0.  The cumulative weights keep accumulating
 *     the constrained weights, so the location features see what the constrained decoder did.  The window contains p, so it
 *     is never empty.
 * t is the absolute frame index: a call of t2v_decoder_infer_steps_plan with t_begin > 0 continues a plan.  Behind its end
 * (t >= n_plan[b]) the plan holds its last symbol.  Free-running decode only: the teacher-forced pass and training have no
 * plan.
 * The two entries below take the arguments of the `_window` entries plus plan (B rows of plan_stride int32), plan_stride and
 * n_plan (B int32), device pointers.  `window` is required; (0, 0) is the hard, one-hot form.  1 <= n_plan[b] <= plan_stride
 * is the caller's to check on the host; the kernels clamp the index to 0 .. plan_stride - 1, so no n_plan addresses outside
 * the plan.  A null plan or n_plan, or plan_stride < 1, is T2V_ERR_ARG.
 * t2v_duration_plan below makes a plan from symbol durations. */
int t2v_decoder_infer_steps_plan(const t2v_dec_weights* w, const t2v_dec_infer_bufs* s, int B, int T_in,
                                 int t_begin, int t_end, float gate_threshold, float p_prenet,
                                 int external_prenet, uint64_t seed, const t2v_dec_items* items,
                                 const t2v_dec_window* window, const int32_t* plan, int plan_stride, const int32_t* n_plan,
                                 void* stream);
int t2v_decoder_infer_persistent_plan(const t2v_dec_persist_weights* w, const t2v_dec_persist_bufs* s, int B, int T_in,
                                      int t_end, float gate_threshold, float p_prenet, uint64_t seed,
                                      const t2v_dec_items* items, const t2v_dec_window* window, const int32_t* plan,
                                      int plan_stride, const int32_t* n_plan, void* stream);

/* Length regulator (csrc/plan.hip): symbol durations -> the plan above.  dur (B, dur_stride) fp32, frames per symbol,
 * fractions allowed; n_ids (B) int32, the symbols of row b; rate: NULL (1), or fp32 factors multiplied in, element (b, j) at
 * rate[b rate_stride_b + j rate_stride_j] (a scalar on the device: both strides 0).  All in integers, so that a row's result
 * depends neither on its batch nor on the order of a scan (the fixed-point choice of t2v_tsm):
 *   q_j = llrint((double)dur_j * (double)rate_j * 65536.0) for j < n_ids[b]  (round to nearest, ties to even);
 *   C_j = q_0 + ... + q_j in int64;  E_j = (C_j + 32768) >> 16,  E_{-1} = 0;
 *   symbol j owns the frames E_{j-1} <= t < E_j; a symbol with an empty range is skipped;
 *   n_plan[b] = min(E_last, T_max);  plan[b, t] = j for t < n_plan[b];
 *   plan[b, t] for n_plan[b] <= t < T_max is the last value, or 0 for an empty plan.
 * A row with a negative or non-finite dur_j * rate_j, or with dur_j * rate_j > 2^20, gets n_plan[b] = -1 and a plan of zeros;
 * the other rows are not affected.  n_ids is clamped to 0 .. S.
 * One workgroup per row, one launch.  1 <= S <= T2V_PLAN_MAX_SYMBOLS, else T2V_ERR_DIMS.  A null dur, n_ids, plan or n_plan,
 * B or T_max < 1, dur_stride < S, plan_stride < T_max or a negative rate stride is T2V_ERR_ARG. */
#define T2V_PLAN_MAX_SYMBOLS 4096   /* the frame ends E_j of a row in LDS: 4096 int32 (T2V_MAX_T_IN symbols) */
int t2v_duration_plan(const float* dur, int dur_stride, const int32_t* n_ids, const float* rate, int rate_stride_b,
                      int rate_stride_j, int B, int S, int T_max, int32_t* plan, int plan_stride, int32_t* n_plan,
                      void* stream);

/* ------------------------------------------------------------------ Conv1d + BatchNorm1d + activation
 * The encoder conv bank (model.py:159-177) and the Postnet (model.py:110-148): stride-1 "same" Conv1d as
 * an implicit GEMM on fp32 MFMA, BatchNorm1d (train: biased batch statistics over B*T incl. padded frames;
 * eval: running statistics), tanh / ReLU / none, dropout.  All activations are (B, C, T) fp32.
 *   t2v_conv1d_fwd : Y = conv(X, W) + bias; stat_part ((t2v_conv1d_stat_blocks(B,T,Cin,Cout,KS), Cout, 2) or NULL)
 *                    receives per-column-block partial [sum, sum of squares] per channel.
 *   t2v_bn_act_fwd : out = dropout(act(BN(y)));  act 0 none / 1 tanh / 2 relu.  training != 0 finalises
 *                    the statistics from stat_part, writes mean/rstd for the backward and updates the
 *                    running buffers (momentum, unbiased variance).
 *   t2v_bn_act_bwd : dy (grad wrt the conv output), dgamma, dbeta from dout.  dconv_bias ((M) or NULL) receives the
 *                    gradient of the bias of the convolution that feeds this training-mode BatchNorm, which is
 *                    identically zero (dy has zero mean per channel): written here so the caller launches no fill.
 *   t2v_conv1d_bwd : dX (may be NULL; needs Wt_scratch of W's size) and dW (may be NULL).  W == NULL with dX: Wt_scratch
 *                    already holds the flipped, transposed weight (t2v_conv1d_flip_weights ran earlier in the step); W is not
 *                    read when only dW is asked for.
 *   t2v_conv1d_flip_weights : Wt[i] (Cin, Cout, KS) = W[i] (Cout, Cin, KS) transposed with the taps reversed — the operand
 *                    of the data-gradient convolution — for n <= 16 layers in ONE launch (host arrays of n pointers / dims). */
int t2v_conv1d_stat_blocks(int B, int T, int Cin, int Cout, int KS);
/* the same for t2v_conv1d_fwd_bf16 (bf16_run keeps the tiles of its own kernels) */
int t2v_conv1d_stat_blocks_bf16(int B, int T, int Cin, int Cout, int KS);
/* launches of t2v_conv1d_fwd / t2v_conv1d_bwd (data gradient) so far in this process that took the LDS-DMA kernel of the fp32-MFMA
 * route (k_conv5_fwd_dma); those with T2V_CONV_STAGING=0 or with weights that are not 16-byte aligned take k_conv5_fwd and do not count */
long long t2v_conv1d_staged_launches(void);
int t2v_conv1d_fwd(const float* W, const float* X, const float* bias, float* Y, float* stat_part,
                   int B, int Cin, int T, int Cout, int KS, void* stream);
int t2v_conv1d_dw_scratch_floats(int B, int Cin, int T, int Cout, int KS);   /* 0 -> dw_scratch may be NULL */
int t2v_conv1d_bwd(const float* W, const float* X, const float* dY, float* dX, float* dW, float* Wt_scratch,
                   float* dw_scratch,
                   int B, int Cin, int T, int Cout, int KS, void* stream);
int t2v_conv1d_flip_weights(const float* const* W, float* const* Wt, const int* Cout, const int* Cin, int KS, int n,
                            void* stream);
/* bf16_run variants (BASELINE configs[4]; replace the reference's fp16 path, fp16_optimizer.py / loss_scaler.py):
 * fp32 tensors in and out, operands rounded to bf16 on the way into LDS, fp32 accumulation on bf16 MFMA.
 * Wp_scratch: W's element count x 2 bytes.  Round 5: the weight gradient as well (dY and X rounded to bf16 while staged,
 * v_mfma_f32_16x16x16_bf16; W and Wp_scratch are not needed for a dW-only call, dw_scratch as t2v_conv1d_dw_scratch_floats);
 * T2V_ERR_DIMS unless KS == 5 and the reduction channel count is a multiple of 16. */
int t2v_conv1d_fwd_bf16(const float* W, const float* X, const float* bias, float* Y, float* stat_part,
                        void* Wp_scratch, int B, int Cin, int T, int Cout, int KS, void* stream);
int t2v_conv1d_bwd_bf16(const float* W, const float* X, const float* dY, float* dX, float* dW,
                        void* Wp_scratch, float* dw_scratch, int B, int Cin, int T, int Cout, int KS, void* stream);

int t2v_bn_act_fwd(const float* y, const float* stat_part, int nblk, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float* mean_out, float* rstd_out, float* out,
                   int B, int M, int T, int act, int training, float p_drop, float momentum, float eps,
                   uint64_t seed, uint32_t rng_stream, uint32_t rng_t, void* stream);
/* eval-mode forward over a ragged batch: out = act(BN(y)) with the running statistics at t < lengths[b] and 0 at every
 * t >= lengths[b] (lengths: (B) int32 on the device), so that the next convolution of the stack reads each item's tail as
 * the zero padding of that item convolved alone.  No dropout (eval), one launch like t2v_bn_act_fwd. */
int t2v_bn_act_fwd_len(const float* y, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float* out, const int32_t* lengths, int B, int M, int T, int act, float eps,
                       void* stream);
int t2v_bn_act_bwd(const float* y, const float* dout, const float* mean, const float* rstd,
                   const float* gamma, const float* beta, float* dy, float* dgamma, float* dbeta,
                   float* dconv_bias, int B, int M, int T, int act, float p_drop, uint64_t seed,
                   uint32_t rng_stream, uint32_t rng_t, void* stream);
/* the same for eval-mode BatchNorm (running statistics are constants: no batch-statistic terms in dy, dconv_bias =
 * gamma rstd sum(dz) instead of zeros); mean = running_mean, rstd = 1 / sqrt(running_var + eps) */
int t2v_bn_act_bwd_eval(const float* y, const float* dout, const float* mean, const float* rstd,
                   const float* gamma, const float* beta, float* dy, float* dgamma, float* dbeta,
                   float* dconv_bias, int B, int M, int T, int act, float p_drop, uint64_t seed,
                   uint32_t rng_stream, uint32_t rng_t, void* stream);
/* gridDim.y that t2v_bn_act_fwd (backward = 0) / t2v_bn_act_bwd[_eval] (backward != 0) plans for these dimensions: 1 = one
 * workgroup per channel, > 1 = every channel cut into that many slices of B*T (few wide channels: M <= 128 and B*T >= 16384
 * forward, >= 8192 backward; at most 64 slices and about 1024 / M).  The forward cuts only in training and without partials
 * (training, has_partials: what the call passes; the backward ignores both, it cuts in eval mode too).  It answers the PLAN, from
 * the code the launches read: a sliced launch takes its partials from a ring of the library, and if the ring has no room the
 * launch runs unsliced all the same.  T2V_ERR_ARG for a dimension below 1. */
int t2v_bn_act_slices(int backward, int B, int M, int T, int training, int has_partials);

/* ------------------------------------------------------------------ symbol embedding
 * nn.Embedding(n_symbols, C) of the text encoder (model.py:474-482) as used at model.py:528
 * (`transcript_embedding(text).transpose(1, 2)`): ids (B,T) int64 -> out (B,C,T) channel-major, the layout the first
 * encoder Conv1d reads.  Backward: dW (n_symbols,C) = per-symbol sum of dy (B,C,T) over the positions holding that
 * symbol, ascending position order (deterministic). */
int t2v_embedding_fwd(const long long* ids, const float* W, float* out_bct, int B, int T, int C, int n_symbols, void* stream);
int t2v_embedding_bwd(const long long* ids, const float* dy_bct, float* dW, int B, int T, int C, int n_symbols, void* stream);

/* backward of the GEMM's relu / dropout epilogue (Prenet, model.py:96-99): out = dy * [y != 0] * scale, where y is the
 * forward output (already relu'd and scaled by 1/(1-p)) and scale = 1/(1-p); n contiguous floats, 16-byte aligned. */
int t2v_gemm_epilogue_bwd(const float* dy, const float* y, float* out, size_t n, float scale, void* stream);

/* ------------------------------------------------------------------ column sums (bias gradients)
 * out[j] = sum_i A[i*lda + j] for a row-major (M,N) matrix: what autograd computes as `grad.sum(0)` for the bias of
 * every nn.Linear / LSTM cell on the path (model.py:171-190, 200-236) and for the sum over decoder steps of the
 * processed-memory gradient (model.py:60-64).  Fixed slice boundaries and summation order (bit-reproducible).
 * scratch: t2v_colsum_scratch_floats(M,N) floats (may be 0 -> NULL). */
long t2v_colsum_scratch_floats(long M, long N);
int t2v_colsum(const float* A, long lda, long M, long N, float* scratch, float* out, void* stream);

/* ------------------------------------------------------------------ fused epilogues (round 4, csrc/glue.hip)
 * t2v_mask_outputs: Tacotron2.parse_output (model.py:509-520) in one launch — mel (B,C,T) and mel_post (B,C,T) := 0,
 * gate (B,T) := gate_fill (1e3) at frames t >= lengths[b]; in place (the reference fills `.data`).
 * t2v_reparam_fwd / _bwd: VAE_GST.reparameterize (modules.py:74-81): z = eps * exp(0.5 logvar) + mu over n floats, and
 * dlogvar = dz * eps * exp(0.5 logvar) * 0.5 (dmu = dz needs no launch).
 * t2v_gather_words: *dst[i] = *src[i] for n four-byte device words (16 per launch): the asynchronous error ledger of the
 * host mirror collects the error words of a step's cooperative kernels with it. */
int t2v_mask_outputs(float* mel, float* mel_post, float* gate, const int* lengths, int B, int C, int T, float gate_fill,
                     void* stream);
/* t2v_mask_time: out (B,C,T) = x at t < lengths[b], 0 at t >= lengths[b] (out may be x): the input of a length-masked
 * conv stack (Encoder.inference / Postnet.forward with lengths). */
int t2v_mask_time(const float* x, float* out, const int32_t* lengths, int B, int C, int T, void* stream);
int t2v_reparam_fwd(const float* eps, const float* mu, const float* logvar, float* z, long n, void* stream);
int t2v_reparam_bwd(const float* dz, const float* eps, const float* logvar, float* dlogvar, long n, void* stream);
int t2v_gather_words(const void* const* src, void* const* dst, int n, void* stream);
/* out[r] = [a[r][0..na) | b[r][0..nb)], rows of float4-aligned widths / strides (lda, ldb in floats): the (h_dec, context) input
 * rows of linear_projection + gate_layer (model.py:385-388) gathered from the decoder arena in one launch */
int t2v_concat2_rows(const float* a, long lda, int na, const float* b, long ldb, int nb, float* out, long rows, void* stream);

/* ------------------------------------------------------------------ encoder BiLSTM recurrence
 * nn.LSTM(512, 256, bidirectional) on a packed sequence (model.py:171-173, 183-190), recurrent part only:
 * gx (2,B,T,1024) = X·W_ih^T + b_ih + b_hh per direction (time-batched GEMM done by the caller), whh
 * (2,1024,256).  Persistent cooperative kernels (16 workgroups, W_hh register-resident for all T steps).
 * y (B,T,512) and dg (2,B,T,1024) are cleared by the calls themselves (padded positions stay zero);
 * hx_scratch (2*2*16*256 8-byte granules = 2*2*2*16*256 floats) / dgx_scratch (2*2*16*16*256 granules = 2*2*2*16*16*256
 * floats: per direction and step parity, the 256 partial recurrent gradients x 16 items of each of 16 producers) are exchange
 * buffers of {value, step tag} granules (zeroed by the call); sync3 = 3 uint32 (zeroed by the call; sync3[2] != 0
 * afterwards means a bounded spin timed out).  gates/cells (saved
 * activations) may be NULL for inference.  B <= 16. */
int t2v_bilstm_fwd(const float* gx, const float* whh, const int32_t* lengths, float* y, float* gates,
                   float* cells, float* hx_scratch, uint32_t* sync3, int B, int T, void* stream);
int t2v_bilstm_bwd(const float* whh, const int32_t* lengths, const float* dy, const float* gates,
                   const float* cells, float* dg, float* dgx_scratch, uint32_t* sync3, int B, int T,
                   void* stream);

/* ------------------------------------------------------------------ dense layers (time-batched)
 * C[i][j] (+)= sum_k A[i*sAi + k*sAk] * B[j*sBj + k*sBk] (+ bias[j]), optional ReLU and dropout epilogue
 * (dropout mask = counter RNG keyed by (seed, rng_stream, rng_t, i*ldc+j)).  Hand-written fp32 MFMA tile
 * for Prenet (model.py:91-102), memory_layer (model.py:290), the hoisted attention_rnn input term and the
 * fused linear_projection+gate_layer (model.py:385-388) — forward (NT) and both gradients (NN / TN). */
int t2v_gemm_f32(const float* A, long sAi, long sAk, const float* B, long sBj, long sBk, const float* bias,
                 float* C, int ldc, int M, int N, int K, int relu, int accumulate, float p_drop,
                 uint64_t seed, uint32_t rng_stream, uint32_t rng_t, void* stream);
/* Same product with split-K for skinny deep-K shapes (weight gradients of small layers with K = T*B): when
 * t2v_gemm_splitk_scratch_floats(M,N,K) > 0 and `splitk_scratch` holds that many floats, the k range is cut over
 * gridDim.z and the partial tiles are summed in a fixed order together with the epilogue (deterministic); otherwise
 * identical to t2v_gemm_f32. */
long t2v_gemm_splitk_scratch_floats(int M, int N, int K);
int t2v_gemm_f32_splitk(const float* A, long sAi, long sAk, const float* B, long sBj, long sBk, const float* bias,
                        float* C, int ldc, int M, int N, int K, int relu, int accumulate, float p_drop,
                        uint64_t seed, uint32_t rng_stream, uint32_t rng_t, float* splitk_scratch, void* stream);

/* Round 6: how the LARGE fp32 products (>= 64 tiles of 128x128, 16-byte-aligned operand runs) are computed.
 * mode 1 (default; T2V_F32_GEMM=native selects 0): "x3" — every fp32 operand is cut exactly into three bf16 values
 * (a = a0 + a1 + a2) and the product is accumulated in fp32 from six v_mfma_f32_32x32x16_bf16 per k-block; the omitted
 * cross terms are <= 2^-25 |a b|, below the rounding of one fp32 product: fp32-class results (same error bound against fp64
 * as the fp32-MFMA kernel, tests/test_gemm_gpu.py) at up to 2.7x the fp32 matrix peak of gfx950 (which has no TF32 path).
 * mode 0: v_mfma_f32_32x32x2_f32 for every product.  Pass -1 to query.  Returns the previous mode.  Process-wide. */
int t2v_gemm_f32_set_mode(int x3);

/* Grouped form of the large fp32 products (round 6): for every group g and part p   C[g][p] (+)= A_g · B_{g,p}^T   with all A_g
 * (M x K) and B_{g,p} (N[p] x K), element strides as in t2v_gemm_f32.  The decoder's four nn.LSTMCell weight gradients
 * (reference model.py:221-226 under autograd) are two groups — A = the gate gradients of a cell, parts = the column blocks
 * [prenet | h_att | ctx] / [h_att + ctx | h_dec] of its input: in x3 mode (t2v_gemm_f32_set_mode) every operand is split ONCE and
 * all tiles run as ONE launch (1 024 tiles = two full rounds of the chip, no k-split); otherwise, or when an N[p] is not a
 * multiple of 128, the products run one by one on t2v_gemm_f32.  ngroups <= 2, nb <= 3.  scratch:
 * t2v_gemm_f32_grouped_scratch_floats() floats, 16-byte aligned. */
typedef struct t2v_gemm_group {
    const float* A;
    long sAi;
    long sAk;
    int nb;
    const float* B[3];
    long sBj[3];
    long sBk[3];
    int N[3];
    float* C[3];
    int ldc[3];
} t2v_gemm_group;
long t2v_gemm_f32_grouped_scratch_floats(const t2v_gemm_group* groups, int ngroups, int M, int K);
int t2v_gemm_f32_grouped(const t2v_gemm_group* groups, int ngroups, int M, int K, int accumulate, float* scratch, void* stream);
/* The grouped product behind a kernel that has worked on group `handed` already (t2v_achain_dw): the group's planes exist at float
 * offset t2v_gemm_f32_grouped_group_offset(groups, ngroups, M, K, handed) of `scratch` (-1: these shapes have no plane form), and the
 * first min(*done_ctr, done_cap) tiles of the group (row-major over 128 x 128 tiles of A_g x [B_g0 | B_g1 | ..]) are done; *done_ctr
 * is read on the device.  No split launches for that group; everything else as t2v_gemm_f32_grouped. */
long t2v_gemm_f32_grouped_group_offset(const t2v_gemm_group* groups, int ngroups, int M, int K, int g);
int t2v_gemm_f32_grouped_handed(const t2v_gemm_group* groups, int ngroups, int M, int K, int accumulate, float* scratch, int handed,
                                const uint32_t* done_ctr, int done_cap, void* stream);
/* bf16_run form: the same grouping on ONE bf16 plane per operand (operands rounded to bf16, RNE, once by the split pass; fp32
 * accumulation — the arithmetic of t2v_gemm_bf16). */
long t2v_gemm_bf16_grouped_scratch_floats(const t2v_gemm_group* groups, int ngroups, int M, int K);
int t2v_gemm_bf16_grouped(const t2v_gemm_group* groups, int ngroups, int M, int K, int accumulate, float* scratch, void* stream);

/* ... and the fp32 k = 5 Conv1d forward / data gradient (t2v_conv1d_fwd / t2v_conv1d_bwd) on the same six-product scheme
 * (csrc/conv_x3.hip).  mode 0: never; 1: every eligible shape (KS = 5, Cin % 16 == 0, Cin, Cout >= 64); 2 (default; T2V_CONV_X3
 * presets it): launches of >= 192 tiles of 128 x 128 only — at the B = 6 step's shapes its fixed costs (split passes, channel-split
 * tiles) outweigh the faster loop, at B = 16 it runs a Postnet layer in 152 us against 212.  Only effective while
 * t2v_gemm_f32_set_mode is 1.  t2v_conv1d_stat_blocks answers for the current mode.  Pass -1 to query.  Returns the previous mode. */
int t2v_conv1d_x3_set_mode(int mode);
/* 1 when the k = 5 convolution Cin -> Cout of t2v_conv1d_fwd (bf16 = 0) / t2v_conv1d_fwd_bf16 (bf16 = 1) takes the plane kernels of
 * conv_x3.hip in the current mode, 0 when it runs on the tiled kernels (mode, tile count, and whether the call's scratch fits) */
int t2v_conv1d_takes_x3(int B, int Cin, int T, int Cout, int KS, int bf16);
/* Which kernel a Conv1d call runs: the answer of the one function (conv_route of csrc/conv_gemm.hip) that t2v_conv1d_fwd / _bwd /
 * _fwd_bf16 / _bwd_bf16 are dispatched by, so it follows t2v_conv1d_x3_set_mode, t2v_gemm_f32_set_mode and the T2V_CONV_* switches
 * of the process.  op: T2V_CONV_OP_FWD, _DX (the data gradient: the convolution Cout -> Cin of dY with the flipped, transposed
 * weights) or _DW; B, Cin, T, Cout, KS: the LAYER's dimensions as the entry points take them; bf16: the bf16_run entries;
 * w_mod16: the address modulo 16 of the weights the kernel reads (W forward, Wt_scratch for the data gradient; the bf16 entries and
 * the weight gradient ignore it).  Returns a T2V_CONV_ROUTE_* value, T2V_ERR_ARG for a dimension below 1 or an even KS,
 * T2V_ERR_DIMS with bf16 where this launch has no bf16 kernel (the bf16 entries then return it).  Every output pointer may be NULL:
 *   *fallback           the tiled family that runs instead when T2V_CONV_ROUTE_PLANE1 as a data gradient finds no slice of the
 *                       library's ring for the flipped weights (equal to the return value everywhere else);
 *   *tile               forward / data gradient on the tiled kernels: output positions per workgroup / 16 (2 .. 6; under the plane
 *                       kernels: of *fallback); tiled weight gradient: positions per k-tile, 80 or 96; k_conv_gemm: 0;
 *   *ksplit             2 = the input channels are cut in halves (gridDim.z of k_conv5_fwd[_dma]), else 1;
 *   *dw_splits          weight gradient: k-splits, empty trailing ones included (1 = none);
 *   *stat_blocks        forward: rows of stat_part the launch writes (t2v_conv1d_stat_blocks[_bf16]);
 *   *dw_scratch_floats  weight gradient: floats of dw_scratch THIS launch writes (t2v_conv1d_dw_scratch_floats is the bf16 answer,
 *                       which is never smaller);
 *   *plane_splits, *plane_chunk   plane kernels: gridDim.z over the input channels and the stages (16 channels on T2V_CONV_ROUTE_X3,
 *                       32 on _PLANE1) per split, the last split holding what is left; 0, 0 on every other family.
 * It answers the PLAN, like t2v_bn_act_slices: a ksplit = 2 launch takes its raw tiles from a ring of the library, and if the ring
 * has no slice the same kernel runs uncut (same tiles, same partial blocks).  Host only: nothing is launched. */
#define T2V_CONV_OP_FWD 0
#define T2V_CONV_OP_DX 1
#define T2V_CONV_OP_DW 2
#define T2V_CONV_ROUTE_GEMM 0            /* k_conv_gemm: any Cin, KS = 3 or 5 */
#define T2V_CONV_ROUTE_FWD 1             /* k_conv5_fwd: register-staged */
#define T2V_CONV_ROUTE_FWD_DMA 2         /* k_conv5_fwd_dma: staged by LDS-DMA */
#define T2V_CONV_ROUTE_X3 3              /* k_conv5_x3<3, 2>: three bf16 planes per operand */
#define T2V_CONV_ROUTE_BF16 4            /* k_conv5_fwd_bf16: 16 channels per k-tile */
#define T2V_CONV_ROUTE_BF16K32 5         /* k_conv5_fwd_bf16k32: 32 channels per k-tile */
#define T2V_CONV_ROUTE_PLANE1 6          /* k_conv5_x3<1, 4>: one pre-rounded bf16 plane per operand */
#define T2V_CONV_ROUTE_DW 7              /* k_conv5_dw */
#define T2V_CONV_ROUTE_DW_BF16 8         /* k_conv5_dw_bf16 */
#define T2V_CONV_ROUTES 9
int t2v_conv1d_route(int op, int B, int Cin, int T, int Cout, int KS, int bf16, int w_mod16, int* fallback, int* tile, int* ksplit,
                     int* dw_splits, int* stat_blocks, int* dw_scratch_floats, int* plane_splits, int* plane_chunk);
const char* t2v_conv1d_route_name(int route);

/* nbatch independent products C_z = A_z · B_z^T (z-th operands at A + z*sAb, B + z*sBb, C + z*sCb; element strides as in
 * t2v_gemm_f32, no bias / epilogue) in one launch.  Replaces the per-item loop that autograd's bmm backward of
 * `attention_context = torch.bmm(attention_weights.unsqueeze(1), memory)` (model.py:84-85) amounts to for d_memory. */
int t2v_gemm_f32_batched(const float* A, long sAb, long sAi, long sAk, const float* B, long sBb, long sBj, long sBk,
                         float* C, long sCb, int ldc, int nbatch, int M, int N, int K, void* stream);
/* same contract, bf16 operands / fp32 accumulate (bf16_run) */
int t2v_gemm_bf16(const float* A, long sAi, long sAk, const float* B, long sBj, long sBk, const float* bias,
                  float* C, int ldc, int M, int N, int K, int relu, int accumulate, float p_drop,
                  uint64_t seed, uint32_t rng_stream, uint32_t rng_t, void* stream);
/* bf16 product with split-K for the 128x128-tile kernel (the deferred LSTM weight gradients of the decoder, model.py:221-226
 * under autograd: 64 .. 384 tiles with K = T*B): when t2v_gemm_bf16_splitk_scratch_floats(M,N,K) > 0 and `splitk_scratch` holds
 * that many floats, the k range is cut over gridDim.z, the partial accumulators are summed in a fixed order (deterministic)
 * with the epilogue; otherwise identical to t2v_gemm_bf16. */
long t2v_gemm_bf16_splitk_scratch_floats(int M, int N, int K);
int t2v_gemm_bf16_splitk(const float* A, long sAi, long sAk, const float* B, long sBj, long sBk, const float* bias,
                         float* C, int ldc, int M, int N, int K, int relu, int accumulate, float p_drop,
                         uint64_t seed, uint32_t rng_stream, uint32_t rng_t, float* splitk_scratch, void* stream);

/* Which kernel t2v_gemm_f32[_splitk] (bf16 = 0) / t2v_gemm_bf16[_splitk] (bf16 = 1) run for a product: the answer of the very
 * function the launches are dispatched by, so it follows t2v_gemm_f32_set_mode and the T2V_GEMM_* / T2V_X3_* / T2V_BF16_GEMM_PLANES
 * switches of the process.  a_mod16 / b_mod16 / scratch_mod16: the base addresses modulo 16; has_scratch: a split-K scratch is
 * passed (the plain entry points pass none).  Returns a T2V_GEMM_ROUTE_* value (T2V_ERR_ARG for an empty product);
 * *form (may be NULL): bit 0 = the kernel stages A along k, bit 1 = B along k (otherwise along the rows);
 * *splits (may be NULL): k-splits launched, empty trailing ones included (1 = none); *k_per_split (may be NULL): split z sums
 * k in [z * k_per_split, (z + 1) * k_per_split) (K when there is no split).  Host only: nothing is launched. */
#define T2V_GEMM_ROUTE_F32_64 0          /* k_gemm_f32: 64x64 tile, fp32 MFMA */
#define T2V_GEMM_ROUTE_F32_64_SPLITK 1   /* ... cut over k, the last workgroup of a tile sums the partials */
#define T2V_GEMM_ROUTE_F32_BIG_128 2     /* k_gemm_f32_big: 128x128 tile */
#define T2V_GEMM_ROUTE_F32_BIG_64 3      /* k_gemm_f32_big: 128x64 tile */
#define T2V_GEMM_ROUTE_F32_X3 4          /* k_x3_split + k_gemm_x3p<3,2>: three bf16 planes per operand */
#define T2V_GEMM_ROUTE_BF16_64 5         /* k_gemm_bf16: 64x64 tile */
#define T2V_GEMM_ROUTE_BF16_64_SPLITK 6
#define T2V_GEMM_ROUTE_BF16_BIG 7        /* k_gemm_bf16_big_rr: 128x128 tile */
#define T2V_GEMM_ROUTE_BF16_BIG_SPLITK 8
#define T2V_GEMM_ROUTE_BF16_PLANES 9     /* k_x3_split + k_gemm_x3p<1,4>: one pre-rounded bf16 plane per operand */
#define T2V_GEMM_ROUTE_BF16_TO_F32_BIG 10 /* a bf16 call that k_gemm_f32_big takes (fp32 operands, nothing rounded) */
#define T2V_GEMM_ROUTES 11
int t2v_gemm_route(int M, int N, int K, long sAi, long sAk, long sBj, long sBk, int a_mod16, int b_mod16, int scratch_mod16,
                   int has_scratch, int relu, float p_drop, int bf16, int* form, int* splits, int* k_per_split);
const char* t2v_gemm_route_name(int route);


/* ------------------------------------------------------------------ reference encoder / VAE / loss
 * t2v_conv2d_s2_* : Conv2d 3x3 stride 2 pad 1 of ReferenceEncoder (modules.py:45-57); coord != 0 appends the
 *                   CoordConv channels xx, yy, rr (CoordConv.py:37-74) to x on the fly (w then has Cx+3 inputs).
 *                   BatchNorm2d+ReLU = t2v_bn_act_* on the (B, C, H*W) view with stat_part = NULL.
 * t2v_gru_*       : nn.GRU(256,256) recurrence (modules.py:60-62,78); gi = x·W_ih^T + b_ih outside; hs
 *                   (B,T+1,256) all hidden states (hs[:,0] = 0), gsave (B,T,4,256); dgi/dgh (B,T,768) gradients
 *                   wrt the input-side / hidden-side gate pre-activations.
 * t2v_loss_fwd_bwd: Tacotron2Loss_VAE (loss_function.py:27-44) value + gradients of the total in one launch;
 *                   out4 = [total, recon, kl, kl_weight]; part192 = 192 floats scratch, ticket = zeroed uint32. */
int t2v_conv2d_s2_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Cx, int H, int W,
                      int Cout, int coord, void* stream);
/* dw_scratch: t2v_conv2d_s2_dw_scratch_floats(...) floats (0 -> may be NULL): position-chunk partials of dW */
int t2v_conv2d_s2_dw_scratch_floats(int B, int Cx, int H, int W, int Cout, int coord);
int t2v_conv2d_s2_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* dw_scratch,
                      int B, int Cx, int H, int W, int Cout, int coord, void* stream);

/* The same convolution (forward / weight + data gradients) as batched GEMMs on the MFMA GEMM kernel (round 3; the reference
 * encoder's late layers have <= 39 output positions per item — far too few for a thread-per-output kernel).  `scratch` holds
 * t2v_conv2d_s2_gemm_scratch_floats(...) floats: the forward leaves the im2col matrix col[b][pos][c*9 + kh*3 + kw] there,
 * the backward needs it (same buffer, untouched in between) and overwrites it. */
long t2v_conv2d_s2_gemm_scratch_floats(int B, int Cx, int H, int W, int Cout, int coord);
int t2v_conv2d_s2_fwd_gemm(const float* x, const float* w, const float* bias, float* y, float* scratch, int B, int Cx, int H, int W,
                           int Cout, int coord, void* stream);
int t2v_conv2d_s2_bwd_gemm(const float* x, const float* w, const float* dy, float* dx, float* dw, float* scratch, int B, int Cx, int H,
                           int W, int Cout, int coord, void* stream);
/* xchg: 2*16*256 floats (forward) / 2*16*768 floats (backward) exchange buffer of the 8 cooperating workgroups;
 * sync2: 2 uint32 (zeroed by the call; sync2[1] != 0 afterwards means a bounded spin timed out). */
int t2v_gru_fwd(const float* gi, const float* whh, const float* bhh, float* hs, float* gsave, float* xchg,
                uint32_t* sync2, int B, int T, void* stream);
int t2v_gru_bwd(const float* whh, const float* hs, const float* gsave, const float* dh_last, float* dgi,
                float* dgh, float* xchg, uint32_t* sync2, int B, int T, void* stream);

/* Ragged inference instances (eval only, no backward): item b of a padded batch comes out as if run alone.
 * hlen (B, int32, device): item b's input height; H = the padded height (>= every hlen[b]).  Rows h >= hlen[b] are item b's
 * zero padding and are never read; with coord the xx channel is normalised by hlen[b] - 1.  x_tstride == 0: x is (B, Cx, H, W).
 * x_tstride > 0 (layer 0, Cx == 1, x_tstride >= H): x is the padded mel (B, W, x_tstride) and item b's (hlen[b], W) image is the
 * reinterpretation of its own contiguous (W, hlen[b]) block (modules.py:67), gathered in place: element (h, w) is
 * x[b][f / hlen[b]][f % hlen[b]], f = h*W + w.  Output rows past (hlen[b] - 1) / 2 + 1 are left with values nobody should read.
 * T2V_ERR_ARG for a null pointer (hlen included), bad sizes, or x_tstride with Cx != 1 or x_tstride < H.  The per-item
 * heights are the caller's to check on the host (2 <= hlen[b] <= H with coord); the kernels clamp them to H, so no length
 * addresses outside x.  The GEMM form's scratch: t2v_conv2d_s2_gemm_ragged_scratch_floats(...) floats (the im2col matrix). */
int t2v_conv2d_s2_fwd_ragged(const float* x, const float* w, const float* bias, float* y, const int32_t* hlen, int B, int Cx,
                             int H, int W, int Cout, int coord, int x_tstride, void* stream);
long t2v_conv2d_s2_gemm_ragged_scratch_floats(int B, int Cx, int H, int W, int Cout, int coord);
int t2v_conv2d_s2_fwd_gemm_ragged(const float* x, const float* w, const float* bias, float* y, float* scratch,
                                  const int32_t* hlen, int B, int Cx, int H, int W, int Cout, int coord, int x_tstride,
                                  void* stream);
/* t2v_gru_fwd plus h_last (B,256): h_last[b] = hs[b, steps[b]], written inside the recurrence.  steps (B, int32, device),
 * each in 1..T (checked by the caller; an item outside that range gets no h_last row).  gsave may be NULL. */
int t2v_gru_fwd_len(const float* gi, const float* whh, const float* bhh, float* hs, float* gsave, float* xchg,
                    uint32_t* sync2, const int32_t* steps, float* h_last, int B, int T, void* stream);
int t2v_loss_fwd_bwd(const float* mel, const float* post, const float* mel_t, const float* gate,
                     const float* gate_t, const float* mu, const float* logvar, float* dmel, float* dpost,
                     float* dgate, float* dmu, float* dlogvar, float* part192, float* out4, uint32_t* ticket,
                     uint64_t n_mel, int n_gate, int n_lat, float kl_weight, void* stream);
/* KL control (csrc/kl_control.hip): t2v_loss_fwd_bwd with free bits and a KL capacity target, still one launch.  mu, logvar (B, D),
 * 1 <= D <= 256.  k[d] = the batch mean of kl[:, d];  K' = B * sum_d max(k[d], free_bits), a dimension with k[d] <= free_bits is
 * floored: it adds B * free_bits and its dmu / dlogvar are exactly 0 (free_bits == 0: off, K' = KL).  capacity >= 0:
 * T = |K' - B * capacity| and the latent gradients carry s = sign(K' - B * capacity), 0 at equality; capacity < 0: off, T = K',
 * s = 1.  total = recon + w * T, w from the device step record when one is installed, else kl_weight.
 * out8 = [total, recon, KL (raw, as t2v_loss_fwd_bwd), w, K', T, number of floored dimensions, s]; part128 = 128 floats scratch,
 * ticket = zeroed uint32.  monitor: NULL, or 3 * D + 2 doubles the launch updates: [0] rows seen, [1] launches seen, then per
 * dimension the running mean of mu[:, d], its M2 (sum of squared deviations, merged batch by batch) and sum kl[:, d]; zero it
 * to start a window.  Deterministic: the same bits from run to run, issued eagerly or replayed from a graph.
 * T2V_ERR_ARG for a null pointer (monitor excepted), B < 1, D outside 1..256, free_bits < 0 or a NaN. */
int t2v_loss_fwd_bwd_klc(const float* mel, const float* post, const float* mel_t, const float* gate,
                         const float* gate_t, const float* mu, const float* logvar, float* dmel, float* dpost,
                         float* dgate, float* dmu, float* dlogvar, float* part128, float* out8, uint32_t* ticket,
                         double* monitor, uint64_t n_mel, int n_gate, int B, int D, float kl_weight, float free_bits,
                         float capacity, void* stream);

/* ------------------------------------------------------------------ optimiser
 * clip_grad_norm_(params, max_norm) + Adam.step() of the reference loop (train.py:226-229,
 * Adam built at train.py:171-172) fused over one flat fp32 arena.  `grads` holds the SUM over
 * ranks after the all-reduce; inv_world = 1/world_size applies the averaging of
 * distributed.py:162.  partials: (1024) scratch; norm_out[0] receives the pre-clip global
 * L2 norm (the value the reference logs as grad.norm).  All four arenas 16-byte aligned.
 * bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (the caller computes them in double like torch.optim.Adam); with
 * t2v_set_step_params installed, lr / bc1 / sqrt(bc2) come from the device record instead. */
int t2v_clip_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, uint64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay,
                       float max_norm, float inv_world, float bc1, float bc2, float* partials,
                       float* norm_out, void* stream);
/* The same step, guarded (round 4): guard[0..guard_n) are error words of the step's cooperative / persistent kernels
 * (device memory).  If any of them is non-zero when the step runs, NOTHING is updated (parameters and both moment arenas keep
 * their values) and norm_out[0] reads NaN: the host finds the error at its next sync, switches the persistent kernels off
 * and runs the iteration again.  guard_n == 0: the plain step. */
int t2v_clip_adam_step_guarded(float* params, float* grads, float* exp_avg, float* exp_avg_sq, uint64_t n,
                               float lr, float beta1, float beta2, float eps, float weight_decay,
                               float max_norm, float inv_world, float bc1, float bc2, float* partials,
                               float* norm_out, const uint32_t* guard, int guard_n, void* stream);
/* The guarded step with a weight average folded in: `ema` (n floats, 16-byte aligned like the other arenas) holds an
 * exponential moving average of the parameters and is updated in the same launch, right behind each parameter:
 *     ema = fmaf(rate_t, p_new - ema, ema)        p_new: the fp32 value this step stores to params
 *     rate_t = ema_warmup ? max(ema_rate, 9 / (10 + t)) : ema_rate       (TensorFlow's min(decay, (1 + t) / (10 + t)) as a rate)
 * ema_rate = 1 - decay, formed by the caller in double and rounded once (the fp32 neighbour of 1e-4 for decay 0.9999, not
 * 1 - (float)0.9999, which is 1.7e-4 relative off); it must lie in (0, 1].  t counts the updates made so far: `epoch` of the
 * device step record when one is bound to `stream` (so that a replayed graph sees the rate of ITS step, like lr and bc1),
 * else the by-value ema_t.  A skipped step (non-zero guard word) leaves `ema` untouched like the other arenas; a NULL or
 * misaligned `ema` or an ema_rate outside (0, 1] is T2V_ERR_ARG before anything is launched.  36 instead of 28 bytes of
 * traffic per element; params, both moments and norm_out get the very bits of t2v_clip_adam_step_guarded. */
int t2v_clip_adam_ema_step_guarded(float* params, float* grads, float* exp_avg, float* exp_avg_sq, uint64_t n,
                                   float lr, float beta1, float beta2, float eps, float weight_decay,
                                   float max_norm, float inv_world, float bc1, float bc2, float* partials,
                                   float* norm_out, const uint32_t* guard, int guard_n, float* ema, float ema_rate,
                                   int ema_warmup, uint64_t ema_t, void* stream);

/* ------------------------------------------------------------------ STFT -> mel front end
 * TacotronSTFT.mel_spectrogram (layers.py:75-92): reflect pad n_fft/2, periodic-Hann STFT
 * (stft.py:77-105), magnitude, mel filterbank, log(clamp(.,1e-5)) — batched, per-utterance lengths,
 * zero fill past T_b = n_samples[b]/hop + 1 (the collate pad value, data_utils.py:126).
 * Only n_fft = 1024, hop = 256, n_mel = 80 (T2V_ERR_DIMS otherwise).  Exactly one of wav_f32 /
 * wav_i16 is non-NULL; `scale` multiplies the samples (1/max_wav_value for int16 PCM).
 * Tables are built by the host mirror (layers.TacotronSTFT): window (1024), tw512 = exp(-2πik/512)
 * as (512,2), tw1024 = exp(-2πik/1024) as (513,2), mel filter rows in CSR form. */
int t2v_mel_frontend(const float* wav_f32, const int16_t* wav_i16, const int64_t* n_samples, int B,
                     int n_stride, float scale, int n_fft, int hop, int n_mel, const float* window,
                     const float* tw512, const float* tw1024, const int32_t* mel_start,
                     const int32_t* mel_len, const float* mel_w, int maxw, float* mel_out,
                     int t_stride, void* stream);

/* ------------------------------------------------------------------ STFT / inverse STFT / Griffin-Lim vocoder
 * stft.STFT and audio_processing.griffin_lim (reference stft.py:77-140, audio_processing.py:52-68) for n_fft = win = 1024,
 * hop = 256, periodic Hann (T2V_ERR_DIMS otherwise), fp32.  Tables as for t2v_mel_frontend: window (1024), tw512 (512,2),
 * tw1024 (513,2).  Spectra are (B, 513, t_stride); n_frames[b] (int32, <= t_stride) is utterance b's frame count T_b and
 * its signal has (T_b - 1) * 256 samples.  Everything past an utterance's length is written as zero.
 *
 * t2v_stft_polar: STFT.transform — reflect pad 512, window, |X| and atan2(Im, Re) (0 where X = 0); T_b = n_samples[b]/256 + 1;
 *   the host refuses n_samples <= 512 as the reference's reflect pad does. */
int t2v_stft_polar(const float* wav, const int64_t* n_samples, int B, int n_stride, int n_fft, int hop,
                   const float* window, const float* tw512, const float* tw1024, float* mag, float* phase,
                   int t_stride, void* stream);
/* t2v_istft: STFT.inverse — the reference's pinv basis is the inverse real FFT (imaginary parts of bins 0 and 512 ignored);
 * frames windowed, overlap-added, divided by window_sumsquare where it is > FLT_MIN, 512 samples trimmed at each end.
 * out: (B, out_stride).  scratch: t2v_istft_scratch_bytes(B, t_stride) bytes of device memory. */
size_t t2v_istft_scratch_bytes(int B, int t_stride);
int t2v_istft(const float* mag, const float* phase, const int32_t* n_frames, int B, int t_stride, int n_fft, int hop,
              const float* window, const float* tw512, const float* tw1024, void* scratch, float* out, int out_stride,
              void* stream);
/* t2v_griffin_lim: audio_processing.griffin_lim from the initial `angles` (B, 513, t_stride): one inverse, n_iters fused
 * iterations (one launch each, no host synchronisation), a final overlap-add.  scratch: t2v_griffin_lim_scratch_bytes. */
size_t t2v_griffin_lim_scratch_bytes(int B, int t_stride);
int t2v_griffin_lim(const float* mag, const float* angles, const int32_t* n_frames, int B, int t_stride, int n_fft,
                    int hop, int n_iters, const float* window, const float* tw512, const float* tw1024, void* scratch,
                    float* out, int out_stride, void* stream);
/* t2v_mel_to_magnitude: linear magnitude from a log mel, M = max(P exp(mel), 0) with P = pinv(mel_basis) (513, n_mel)
 * row-major; mel (B, n_mel, t_stride) -> mag (B, 513, t_stride).  n_mel = 80 only. */
int t2v_mel_to_magnitude(const float* mel, const float* pinv_basis, const int32_t* n_frames, int B, int t_stride,
                         int n_mel, float* mag, void* stream);
/* t2v_griffin_lim_fast: fast Griffin-Lim (Perraudin, Balazs, Soendergaard 2013, in librosa's form).  With
 * alpha = momentum / (1 + momentum) and tprev = 0 at the start, every iteration takes rebuilt = STFT(ISTFT(M phase)),
 * a = rebuilt - alpha tprev, tprev <- rebuilt, and the new phase a / |a| (0 where |a| = 0).  One launch per iteration as
 * t2v_griffin_lim; tprev is one complex spectrum per frame in scratch, read and written by that frame's workgroup alone.
 * momentum = 0 is t2v_griffin_lim itself (the same launches); momentum outside [0, 1) is T2V_ERR_ARG.
 * scratch: t2v_griffin_lim_fast_scratch_bytes. */
size_t t2v_griffin_lim_fast_scratch_bytes(int B, int t_stride);
int t2v_griffin_lim_fast(const float* mag, const float* angles, const int32_t* n_frames, int B, int t_stride, int n_fft,
                         int hop, int n_iters, float momentum, const float* window, const float* tw512,
                         const float* tw1024, void* scratch, float* out, int out_stride, void* stream);
/* t2v_mel_to_magnitude_nnls: the non-negative least-squares inverse of the filterbank B (n_mel, 513) by projected gradient.
 * Per frame, m = exp(mel) and M = max(P m, 0) as t2v_mel_to_magnitude; then n_iters times r = B M - m and
 * M <- max(M - B^T r / lipschitz, 0), lipschitz = ||B||_2^2, which makes ||B M - m|| non-increasing.  No convergence test;
 * n_iters = 0 gives t2v_mel_to_magnitude's bits.  B comes in two-tap form (device arrays): bin k lies in the filters
 * tap_lo[k] and tap_lo[k] + 1 only (0 <= tap_lo <= n_mel - 2) with the weights tap_w0[k] and tap_w1[k], and filter f covers
 * the bins filt_start[f] .. filt_start[f] + filt_len[f] - 1; the caller checks that this reproduces B exactly, the kernel
 * clamps the indices so that none addresses outside its tables.  One launch, a workgroup per 16 frames with M and r in LDS
 * for all iterations; no atomics, and the order of every sum depends on the filter or the bin alone, so a frame gives the
 * same bits in any batch, at any stride and with any padding.  Frames past n_frames[b] are written 0 and their mel is not
 * read.  n_mel = 80 only (T2V_ERR_DIMS); a null pointer, B < 1, t_stride < 1, n_iters < 0 or lipschitz <= 0: T2V_ERR_ARG. */
int t2v_mel_to_magnitude_nnls(const float* mel, const float* pinv_basis, const int32_t* tap_lo, const float* tap_w0,
                              const float* tap_w1, const int32_t* filt_start, const int32_t* filt_len, float lipschitz,
                              int n_iters, const int32_t* n_frames, int B, int t_stride, int n_mel, float* mag,
                              void* stream);

/* ------------------------------------------------------------------ mel-spectral distortion with dynamic time warping
 * The distance between two log-mels of different lengths (csrc/dtw.hip), for scoring free-running synthesis against its
 * ground truth.  X is (B, n_mel, x_stride) and Y (B, n_mel, y_stride), fp32; pair b uses the first nx[b] / ny[b] frames and
 * nothing past them is read.  Local cost d(i, j) = ||x_i - y_j||_2 computed from the differences; recurrence Sakoe-Chiba
 * "symmetric2" without a band: D(1,1) = 2 d(1,1), D(i,j) = min(D(i-1,j) + d, D(i,j-1) + d, D(i-1,j-1) + 2 d);
 * dist[b] = D(nx[b], ny[b]) / (nx[b] + ny[b]), which is exact for this step pattern (every path has weight nx + ny).
 * One launch, one workgroup per pair; a pair's result does not depend on B or on its place in the batch.
 * n_mel = 80 only (T2V_ERR_DIMS).  A null pointer, B < 1 or a stride < 1 is T2V_ERR_ARG.  The lengths are device data and
 * the caller's to check on the host: 1 <= nx[b] <= min(x_stride, T2V_DTW_MAX_FRAMES), the same for ny.  A pair that
 * breaks this is refused by the kernel before it addresses anything, and its dist[b] is NaN.
 * scratch: t2v_mel_dtw_scratch_bytes(B, x_stride, y_stride) bytes (one row of D per pair, handed from one strip of 512
 * X-frames to the next); call it with the strides, or with any tx_max / ty_max not below them. */
#define T2V_DTW_MAX_FRAMES 2048     /* per side: the longest pair the tests check against an fp64 recurrence */
size_t t2v_mel_dtw_scratch_bytes(int B, int tx_max, int ty_max);
int t2v_mel_dtw(const float* X, const int32_t* nx, int x_stride, const float* Y, const int32_t* ny, int y_stride,
                int B, int n_mel, float* dist, void* scratch, void* stream);

/* ------------------------------------------------------------------ exact t-SNE of the latents to 2 dimensions
 * The map of the reference README's "Visualization" section (csrc/tsne.hip): X (N, D) fp32 -> Y (N, 2), all pairs, no
 * approximation.  4 <= N <= T2V_TSNE_MAX_POINTS and 2 <= D <= 64, else T2V_ERR_DIMS; a null pointer, a perplexity outside
 * (0, N/3), n_iter < 1 or a non-positive exaggeration / learning rate is T2V_ERR_ARG.  Nothing past row N of any array is
 * read.  No floating-point atomics: the order of every sum depends on N alone, so equal inputs give equal bits.
 * scratch: t2v_tsne_scratch_bytes(N, D) bytes serve all three calls (0 for sizes that are refused).
 * t2v_tsne_affinities: P (N, N) dense fp32, P_ij = (p_j|i + p_i|j) / (2N) with p_j|i the Gaussian conditional whose precision
 *   a 100-step binary search fits to `perplexity` (entropy tolerance 1e-5, p_i|i = 0).  P is symmetric to the bit, and
 *   t2v_tsne_gradient / t2v_tsne_run rely on that: they read P_ij as P[j][i].
 * t2v_tsne_gradient: one pass over all pairs at the map Y: grad (N, 2) = 4 [ex sum_j P_ij w_ij (y_i - y_j) -
 *   (1/Z) sum_j w_ij^2 (y_i - y_j)], w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{k != l} w_kl; *kl_or_null, when given, receives
 *   sum_{i != j} P' log(max(P', 2^-52) / Q) with P' = ex P, Q = w / Z (zero entries of P add nothing).
 * t2v_tsne_run: n_iter iterations from Y_inout on `stream`, no host synchronisation: T2V_TSNE_EXAG_ITERS iterations at
 *   exaggeration 12 and momentum 0.5, then exaggeration 1 and momentum 0.8; per coordinate gains += 0.2 where update and
 *   gradient differ in sign, *= 0.8 elsewhere, floor 0.01; update = momentum * update - learning_rate * gains * grad.
 *   kl_trace: ceil(n_iter / 50) floats; slot k is the objective (with the exaggeration of that iteration) at the map after
 *   min(50 (k + 1), n_iter) updates. */
#define T2V_TSNE_MAX_POINTS 16384   /* dense fp32 P: 1 GiB */
#define T2V_TSNE_EXAG_ITERS 250
size_t t2v_tsne_scratch_bytes(int N, int D);
int t2v_tsne_affinities(const float* X, int N, int D, float perplexity, float* P, void* scratch, void* stream);
int t2v_tsne_gradient(const float* P, const float* Y, int N, float exaggeration, float* grad, float* kl_or_null,
                      void* scratch, void* stream);
int t2v_tsne_run(const float* P, float* Y_inout, int N, int n_iter, float learning_rate, float* kl_trace, void* scratch,
                 void* stream);

/* ------------------------------------------------------------------ YIN pitch tracker
 * F0 tracks of B waveforms (csrc/f0.hip) on the mel front end's grid: 16 kHz, hop 256, integration window 1024, so frame t
 * and mel frame t are the same instant.  y is (B, y_stride) fp32; row b has n[b] samples and n[b] / 256 + 1 frames; every
 * sample index outside [0, n[b]) counts as 0 and nothing outside is read.  Per frame, with s = 256 t - 512:
 *   d(tau) = sum_{j<1024} (x[s+j] - x[s+j+tau])^2 for tau = 1..tau_max, from the differences;
 *   d'(tau) = d(tau) tau / sum_{k<=tau} d(k), 1 where that sum is 0;
 *   tau* = the smallest tau in [tau_min, tau_max] with d' < threshold, moved to tau + 1 while d'(tau + 1) < d'(tau);
 *   no such tau: the frame is unvoiced (no fall-back to the global minimum);
 *   f0 = 16000 / (tau* + delta), delta = clamp((a - c) / (2 (a - 2b + c)), -1, 1) for a, b, c = d'(tau* - 1 .. tau* + 1) when
 *   both neighbours lie in 1..tau_max and a - 2b + c > 0, else 0.
 * f0 (B, out_stride): Hz, 0 where unvoiced; aperiodicity (B, out_stride): d'(tau*), 1 where unvoiced.  Columns from a row's
 * frame count up to y_stride / 256 + 1 are written as 0 / 1; columns past that are not written.
 * The order of every sum depends on (t, tau) alone: a row gives the same bits alone, in any batch and at any stride.
 * A null pointer, B < 1, a stride < 1 or out_stride < y_stride / 256 + 1 is T2V_ERR_ARG; tau outside
 * 1 <= tau_min < tau_max <= T2V_F0_MAX_LAG is T2V_ERR_DIMS.  The lengths are device data and the caller's to check on the
 * host (1 <= n[b] <= y_stride); the kernel clamps a length to 0..y_stride, so none addresses outside the tensor. */
#define T2V_F0_MAX_LAG 400          /* 40 Hz at 16 kHz */
int t2v_f0_yin(const float* y, const int32_t* n, int y_stride, int B, int tau_min, int tau_max, float threshold, float* f0,
               float* aperiodicity, int out_stride, void* stream);

/* ------------------------------------------------------------------ attention alignment statistics
 * Did the decoder read the sentence?  Per-row numbers of B alignment matrices (csrc/align.hip).  A is fp32 with element
 * (b, t, j) at A[b a_stride_b + t a_stride_t + j] (B rows of N frames by T_in text positions); row b has n_frames[b] valid
 * frames and n_text[b] valid text positions (device int32).  Only A[b, t < n, j < L] is read: padding may hold anything, and
 * A is never written.  With p[t] = the lowest j < L that maximises A[b, t, j]:
 *   path  (B, path_stride) int32: p[t] for t < n, -1 from n to the stride;
 *   mass  (B, mass_stride) fp32:  sum_{t<n} A[b, t, j] for j < L, 0 from L to the stride;
 *   focus (B) fp32:               (1/n) sum_t A[b, t, p[t]];
 *   stats (B, 8) int32:           furthest = max_t p[t];  p_last = p[n-1];  n_back = #{t >= 1: p[t] < p[t-1]};
 *                                 n_jump = #{t >= 1: p[t] - p[t-1] > max_jump};  longest_stall = the longest run of equal
 *                                 consecutive p, in frames (>= 1);  n_uncovered = #{j < L: mass_j < cover_min};
 *                                 longest_gap = the longest run of consecutive uncovered positions;  one reserved word, 0.
 * One pass over A: a workgroup owns T2V_ALIGN_FRAMES consecutive frames of one row and leaves their argmax and its block's
 * column sums; a second kernel adds the block partials in ascending block order.  No floating-point atomics: the order of
 * every sum depends on (t, j) alone, so a row gives the same bits alone, in any batch, at any stride and with any padding.
 * Any B, N, T_in >= 1.  The lengths are device data and the caller's to check on the host (1 <= n <= N, 1 <= L <= T_in); the
 * kernels clamp them to 0..N and 0..T_in, so none addresses outside the tensor, and a row with n = 0 or L = 0 gets focus 0,
 * all stats 0, path -1 and mass 0.
 * A null pointer, B, N or T_in < 1, a_stride_t < T_in, a_stride_b < (N - 1) a_stride_t + T_in, path_stride < N or
 * mass_stride < T_in is T2V_ERR_ARG; max_jump < 0 or cover_min <= 0 is T2V_ERR_DIMS.
 * scratch: t2v_alignment_scratch_bytes(B, N, T_in) bytes of device memory, the caller's (0 for sizes that are refused). */
#define T2V_ALIGN_FRAMES 16         /* frames per workgroup: the block of the column partial sums */
size_t t2v_alignment_scratch_bytes(int B, int N, int T_in);
int t2v_alignment_stats(const float* A, long long a_stride_b, long long a_stride_t, const int32_t* n_frames,
                        const int32_t* n_text, int B, int N, int T_in, int max_jump, float cover_min, int32_t* path,
                        int path_stride, float* mass, int mass_stride, float* focus, int32_t* stats, void* scratch,
                        void* stream);

/* ------------------------------------------------------------------ wavs at any rate: resample, trim, crop
 * The stage in front of the mel front end (csrc/resample.hip).
 *
 * t2v_resample: polyphase resampling of B rows by the rational ratio up / down (lowest terms).  x is (B, x_stride), fp32 or,
 * with x_is_pcm16, int16 PCM multiplied by `scale` (1 / 32768) as it is loaded (scale is ignored for fp32); row b has n[b]
 * samples (device int32), every sample index outside [0, n[b]) counts as 0 and nothing outside is read.  taps: the device
 * table t[0 .. 2 half] the caller made (fp32).  With n_out[b] = ceil(n[b] up / down):
 *   y[b][m] = sum_i t[m down - i up + half] x[b][i]   over 0 <= i < n[b] and tap index in 0 .. 2 half,   m < n_out[b],
 * y (B, out_stride) fp32 is 0 from n_out[b] to out_stride.
 * The order of every sum depends on m alone: a row gives the same bits alone, in any batch and at any stride.
 * up == down launches nothing and writes nothing.  A null pointer, B < 1, a stride < 1 or above 2^30, up or down < 1, half < 1
 * or out_stride < ceil(x_stride up / down) is T2V_ERR_ARG; a table of more than T2V_RESAMPLE_MAX_TAPS entries (2 half + 1), or
 * up > 2 half, is T2V_ERR_DIMS.  The lengths are the caller's to check on the host; the kernel clamps a length to 0..x_stride.
 *
 * t2v_trim_bounds: energy trim on the front end's grid.  Frame t of row b covers the samples [256 t - 512, 256 t + 512) (0
 * outside [0, n)), ms[t] is its mean square, a row has n / 256 + 1 frames, ref = max_t ms[t].  A frame sounds when ref > 0 and
 * ms[t] > ref 10^(-top_db / 10).  With first / last the outermost sounding frames: bounds[b] = (256 max(0, first - pad_frames),
 * min(n, 256 (last + 1 + pad_frames))); a row with no sounding frame keeps (0, n).  bounds is (B, 2) int32; ms is
 * (B, ms_stride) fp32 scratch of the caller's that holds the frames' mean squares afterwards (0 past a row's frame count).
 * A frame's sum has a fixed order.  A null pointer, B < 1, y_stride < 1 or ms_stride < y_stride / 256 + 1 is T2V_ERR_ARG;
 * top_db <= 0 or pad_frames outside 0..2^20 is T2V_ERR_DIMS.
 *
 * t2v_crop_rows: out[b][c] = y[b][start + c] for c < end - start, 0 up to out_stride, (start, end) = bounds[b] clamped to
 * 0 <= start <= end <= y_stride; out of place.  out is fp32, or with out_is_pcm16 int16: y 32768 rounded to nearest-even and
 * clamped to [-32768, 32767].  stats (int16 form only, may be null) is (B, 2) int32: the count of samples of [start, end) that
 * were clamped, and the bit pattern of the fp32 max |y| over them.  Columns past out_stride are not written but are counted.
 * A null pointer, B < 1, a stride < 1 or stats with fp32 output is T2V_ERR_ARG. */
#define T2V_RESAMPLE_MAX_TAPS 32768
int t2v_resample(const void* x, int x_is_pcm16, float scale, const int32_t* n, int x_stride, int B, const float* taps, int up,
                 int down, int half, float* y, int out_stride, void* stream);
int t2v_trim_bounds(const float* y, const int32_t* n, int y_stride, int B, float top_db, int pad_frames, float* ms, int ms_stride,
                    int32_t* bounds, void* stream);
int t2v_crop_rows(const float* y, int y_stride, const int32_t* bounds, int B, void* out, int out_is_pcm16, int out_stride,
                  int32_t* stats, void* stream);

/* ------------------------------------------------------------------ scores of the latent space: neighbours and class sums
 * All distances from M query vectors to N labelled reference vectors (csrc/latent.hip), reduced per query.  R (N, D) fp32,
 * labels (N) int32 in 0..C-1, Q (M, D) fp32; Q null means Q = R and M = N (the M argument is then ignored).
 * exclude (M) int32 or null: reference exclude[i] is skipped for query i in every output but rank; -1 skips nothing.  With Q
 * null and exclude null the meaning is leave-one-out, exclude[i] = i.  Exclusion is by index, never by distance: an exact
 * duplicate of the query at another index stays a neighbour.  target (M) int32 or null; -1 means no target.
 * d2(i, j) = sum_c (q_c - r_c)^2 from the differences, accumulated in ascending c (fused multiply-add); not the
 * |q|^2 + |r|^2 - 2 q.r expansion, so small-integer inputs give exact distances and exact ties.  References are ordered by
 * (d2, index) ascending: ties go to the lower index.  Per query i:
 *   nn_idx (M, k) int32, nn_dist (M, k) fp32: the k first non-excluded references in that order, nn_dist = sqrt(d2);
 *   class_sum (M, C) fp32:  the sum of sqrt(d2) over the non-excluded references of each class;
 *   class_cnt (M, C) int32: their counts;
 *   rank (M) int32: with target[i] >= 0 the number of references (excluded or not) that sort strictly before reference
 *     target[i]; -1 where target[i] is -1 or target is null.  rank may be null when target is.
 * N or M outside 2..T2V_LATENT_MAX_POINTS, D outside 2..64, C outside 1..T2V_LATENT_MAX_CLASSES or k outside
 * 1..T2V_LATENT_MAX_K is T2V_ERR_DIMS.  A null required pointer (scratch included), a target without rank, k above the
 * smallest number of non-excluded references a query can have (N - 1 when exclude is given or implied, else N), or a
 * slice_rows that is neither 0 nor a positive multiple of T2V_LATENT_TILE is T2V_ERR_ARG.  labels, exclude and target are
 * device data and the caller's to check on the host (labels in 0..C-1, the others in -1..N-1), and the vectors must be
 * finite.  An index outside its range addresses nothing: it is treated as -1, and such a label is counted in no class.
 * Nothing past row N or M of any array is read or written.
 * Lane per query; the references are cut into slices of slice_rows rows over the workgroups (0: a length chosen from (N, M)
 * alone) and a second kernel merges the slices in order.  The class sums are closed per T2V_LATENT_TILE references and
 * added in ascending tile order, so no output bit depends on slice_rows.  No floating-point atomics: the order of every sum
 * depends on N alone, and equal inputs give equal bits.
 * scratch: t2v_latent_scratch_bytes(N, M, C, k, slice_rows) bytes of device memory (0 for sizes that are refused). */
#define T2V_LATENT_MAX_POINTS 16384
#define T2V_LATENT_MAX_CLASSES 8
#define T2V_LATENT_MAX_K 32
#define T2V_LATENT_TILE 128         /* reference rows per LDS tile and per block of the class sums */
size_t t2v_latent_scratch_bytes(int N, int M, int C, int k, int slice_rows);
int t2v_latent_neighbours(const float* R, const int32_t* labels, int N, int D, int C, const float* Q, int M,
                          const int32_t* exclude, const int32_t* target, int k, int slice_rows, int32_t* nn_idx,
                          float* nn_dist, float* class_sum, int32_t* class_cnt, int32_t* rank, void* scratch, void* stream);

/* ------------------------------------------------------------------ frame-aligned scores: MCD and F0 errors on a DTW path
 * What the prosody-transfer papers report (MCD-13 with DTW, gross pitch error, voicing decision error, F0 frame error), taken
 * along the warping path between a synthesised and a recorded utterance (csrc/aligned.hip).
 *
 * Cepstrum.  M is the project's log-mel (natural log, (B, 80, m_stride) fp32, row b of n[b] frames; nothing past them is read):
 *   c_k(t) = sqrt(2 / 80) sum_{n<80} M[n, t] cos(pi k (n + 1/2) / 80),   k = 1 .. T2V_NCEP;   c_0 is left out.
 * This is the mel-cepstral distortion "from an 80-band log-mel" of the prosody-transfer papers, not the one of a vocoder's
 * mel-generalised cepstrum.  table is the caller's device array (T2V_NCEP, 80) fp32, row k - 1 holding
 * sqrt(2 / 80) cos(pi k (n + 1/2) / 80) computed in fp64 and rounded once; the kernel adds the 80 terms in index order (fused
 * multiply-add).  out is (B, T2V_NCEP, out_stride) fp32, coefficient k at row k - 1, 0 from n[b] to out_stride.
 *
 * Path.  X is (B, n_cep, x_stride) and Y (B, n_cep, y_stride), fp32 cepstra; pair b uses the first nx[b] / ny[b] frames.
 * Local cost d(i, j) = ||x_i - y_j||_2 from the differences; the recurrence is t2v_mel_dtw's (symmetric2, no band):
 *   D(0, 0) = 2 d(0, 0),   D(i, j) = min(D(i-1, j-1) + 2 d, D(i-1, j) + d, D(i, j-1) + d);   dist[b] = D(Tx-1, Ty-1) / (Tx + Ty).
 * Ties go to the diagonal, then to (i-1, j), then to (i, j-1).  The path is walked back from (Tx-1, Ty-1) to (0, 0) through
 * the stored decisions and written start to end: path (B, path_stride, 2) int32 holds (i_p, j_p) for p < K[b], and is not
 * written past K[b]; max(Tx, Ty) <= K <= Tx + Ty - 1.
 * Lengths are 1 .. min(stride, T2V_DTW_MAX_FRAMES) per side and path_stride >= Tx + Ty - 1; they are device data and the
 * caller's to check on the host.  A pair that breaks this is refused by the kernels before they address anything and before
 * their first barrier: its dist[b] is NaN and its K[b] is 0.
 * scratch: t2v_cep_dtw_scratch_bytes(B, x_stride, y_stride) bytes: one 2-bit decision per cell, 16 bits per thread and step,
 * (ty + (tx - 1) / 8) * 512 bytes per pair (1.18 MB at the maximum).  t2v_cep_dtw_path is t2v_cep_dtw_forward (dist and the
 * table) followed by t2v_cep_dtw_walk (K and path from the table); the halves are exported for timing them apart.
 *
 * Scores.  t2v_path_scores takes any path (points are clamped into the pair's lengths), the cepstra it indexes and two F0
 * tracks fx (B, fx_stride), fy (B, fy_stride) in Hz per frame, 0 (or anything not > 0) meaning unvoiced; a null track is
 * unvoiced everywhere.  Over the points p = (i_p, j_p), p < K[b]:
 *   counts (B, T2V_ALIGNED_COUNTS) int32:  K;  n_both = #{both voiced};  n_vde = #{exactly one voiced};
 *                                          n_gpe = #{both voiced and |fx - fy| > 0.2 fy}.
 *   sums (B, T2V_ALIGNED_SUMS) fp32:  sum d_p;  sum e and sum e^2 with e = 1200 log2(fx / fy) cents over the both-voiced points;
 *                                     S_xx, S_yy, S_xy: the second moments of (log2 fx, log2 fy) over the both-voiced points,
 *                                     centred on their means (two passes: the means, then the centred sums);
 *                                     sum |i_p / max(Tx-1, 1) - j_p / max(Ty-1, 1)|;  one reserved word, 0.
 * The division into means is the caller's, in fp64: mcd_db = (10 / ln 10) sqrt(2) sum d / K, vde = n_vde / K,
 * gpe = n_gpe / n_both, ffe = (n_vde + n_gpe) / K, lf0_rmse = sqrt(sum e^2 / n_both), lf0_corr = S_xy / sqrt(S_xx S_yy),
 * warp_dev = the last sum / K (0 for a linear stretch).  A pair with bad lengths, K[b] outside 1..path_stride or a length above
 * its track's stride gets counts 0 and sums NaN.
 * Every sum is a fixed-order tree (thread t adds the points t, t + 256, ... in order, then a tree over the 256 threads): no
 * floating-point atomics, nothing depends on B or a stride, so a pair gives the same bits alone and in any batch.
 * n_mel = 80 and n_cep = T2V_NCEP only (T2V_ERR_DIMS); a null required pointer, B < 1 or a stride < 1 is T2V_ERR_ARG. */
#define T2V_NCEP 13
#define T2V_ALIGNED_COUNTS 4
#define T2V_ALIGNED_SUMS 8
int t2v_mel_cepstrum(const float* M, const int32_t* n, int m_stride, int B, int n_mel, int n_cep, const float* table, float* out,
                     int out_stride, void* stream);
size_t t2v_cep_dtw_scratch_bytes(int B, int tx_max, int ty_max);
int t2v_cep_dtw_forward(const float* X, const int32_t* nx, int x_stride, const float* Y, const int32_t* ny, int y_stride, int B,
                        int n_cep, float* dist, void* scratch, void* stream);
int t2v_cep_dtw_walk(const int32_t* nx, int x_stride, const int32_t* ny, int y_stride, int B, const void* scratch, int32_t* K,
                     int32_t* path, int path_stride, void* stream);
int t2v_cep_dtw_path(const float* X, const int32_t* nx, int x_stride, const float* Y, const int32_t* ny, int y_stride, int B,
                     int n_cep, float* dist, int32_t* K, int32_t* path, int path_stride, void* scratch, void* stream);
int t2v_path_scores(const int32_t* path, const int32_t* K, int path_stride, const float* X, const int32_t* nx, int x_stride,
                    const float* Y, const int32_t* ny, int y_stride, const float* fx, int fx_stride, const float* fy, int fy_stride,
                    int B, int n_cep, int32_t* counts, float* sums, void* stream);

/* ------------------------------------------------------------------ loudness and energy: a BS.1770 meter
 * The K-weighted, gated loudness of ITU-R BS.1770-4 / EBU R 128 (mono) and the K-weighted level per frame of the front end's
 * grid, over a ragged batch (csrc/loudness.hip).  y is (B, y_stride) fp32, row b has n[b] samples (device int32); nothing at or
 * past n[b] is read.  hop is the rate / 10 (100 ms in samples, 800 .. 4800: 8 to 48 kHz; else T2V_ERR_DIMS).
 *
 * table: the caller's device array of 8 + 16 * 65 fp64.  [0 .. 7) the K-weighting b0 b1 b2 a1 a2 (high shelf) d1 d2 (high
 * pass, whose numerator is 1 -2 1) for the rate, each rounded to fp32 and held as fp64, [7] unused, then the 4 x 4 matrices
 * M^0 .. M^64, row-major, M = A^T2V_LOUDNESS_CHUNK, A the zero-input step of the cascade in transposed direct form II on the
 * state (s1, s2, t1, t2):
 *   A = [-a1 1 0 0; -a2 0 0 0; -2 - d1 0 -d1 1; 1 - d2 0 -d2 0],
 * computed in fp64 from those coefficients.  The filter state is fp64 (the high pass's poles lie 0.005 to 0.015 from z = 1: an
 * fp32 state leaves a noise floor near -85 dBFS behind a loud passage); samples and sums of squares are fp32.  z is the weighted
 * signal from a zero state, 0 outside [0, n).
 * Building the table from C: round the seven coefficients to float, widen them to double, fill A as above, square A six times
 * for M = A^64, then table[8 + 16 p + 4 i + j] = (M^p)[i][j] for p = 0 (the identity), 1, ..., 64 by repeated multiplication,
 * all in double; upload the 1 048 doubles once per rate.  The entry cannot check that the powers belong to the coefficients: a
 * table built otherwise gives a wrong state at every chunk boundary, not an error (t2v_hip.loudness_table is the model).
 *
 * frame_ms (B, ms_stride): ms[t] = mean of z^2 over [256 t - 512, 256 t + 512) for the n / 256 + 1 frames, +0 behind them.
 * block_pw (B, blk_stride): the mean of z^2 over the complete 400 ms blocks [j hop, j hop + 4 hop), nb = (n - 4 hop) / hop + 1
 *   of them (0 when n < 4 hop), +0 behind them.
 * rows (B, 8) int32: [0] the bits of the fp32 sum of block_pw over the gated blocks (l_j = -0.691 + 10 log10 block_pw[j] above
 *   -70 and above the relative gate, 10 below -0.691 + 10 log10 of the mean over the blocks above -70), [1] the bits of the
 *   ungated mean square over [0, n), [2] the bits of the largest block power, [3] the count of gated blocks, [4] nb, the rest 0.
 *   The gates compare powers in fp32.  Integrated loudness = -0.691 + 10 log10(sum / count) is the caller's, in fp64.
 * Every sum has an order that depends on the position in the row alone, without floating-point atomics: a row gives the same
 * bits alone, in any batch and at any stride.
 * A null pointer, B < 1, y_stride < 1 or above 2^30, ms_stride < y_stride / 256 + 1, blk_stride < 1 or below the blocks of
 * y_stride samples is T2V_ERR_ARG.  The lengths are the caller's to check on the host; the kernels clamp them to 0..y_stride.
 * scratch: t2v_loudness_scratch_bytes(B, y_stride, hop) bytes of device memory (0 for sizes that are refused).
 *
 * t2v_scale_rows: y[b][c] *= gains[b] for c < n[b], in place; columns from n[b] on are not touched.  gains is device fp32 (B). */
#define T2V_LOUDNESS_CHUNK 64       /* samples per lane of the filter kernel */
#define T2V_LOUDNESS_TILE 16384     /* samples per workgroup tile: 256 chunks, between which the filter state is scanned */
size_t t2v_loudness_scratch_bytes(int B, int y_stride, int hop);
int t2v_loudness(const float* y, const int32_t* n, int y_stride, int B, const double* table, int hop, float* frame_ms,
                 int ms_stride, float* block_pw, int blk_stride, int32_t* rows, void* scratch, void* stream);
int t2v_scale_rows(float* y, const int32_t* n, int y_stride, int B, const float* gains, void* stream);

/* ------------------------------------------------------------------ tempo and pitch: a phase vocoder
 * Time-scale modification of a ragged batch of polar spectrograms (csrc/tsm.hip).  mag and phase are (B, 513, t_stride) fp32
 * as t2v_stft_polar writes them (hop = a quarter window), row b has n_frames[b] frames (device int32, clamped to 0..T; T <=
 * t_stride is the most any row has); nothing at or past frame n_frames[b] is read.  The rate is num / den, each in
 * 1..T2V_TSM_MAX_RATIO (else T2V_ERR_DIMS): above 1 is faster.  Row b gets n_out[b] = ceil(n_frames[b] den / num) frames of
 * mag_out and phase_out (B, 513, out_stride); both are +0 from n_out[b] to out_stride.  For output frame j, with
 * i = (j num) / den and a = ((j num) % den) / den in integers:
 *   mag_out[j, k]   = (1 - a) mag[i, k] + a mag[i + 1, k], frame i + 1 == n_frames[b] counting as magnitude 0;
 *   phase_out[j, k] = phase[0, k] + sum over j' < j of d[j', k], d = wrap(phase[i' + 1, k] - phase[i', k] - pi k / 2) + pi k / 2
 *                     (past the end: pi k / 2 alone), given modulo 2 pi, in [-pi, pi).
 * The sum is a prefix sum of 32-bit fixed-point fractions of a turn (round(p 2^32 / 2 pi) of each fp32 phase): integer
 * addition, so a row gives the same bits alone, in any batch, at any stride, and output j is off by at most 2 (j + 1) 2^-33
 * turns plus its one rounding to fp32.
 * phase_lock != 0: identity phase locking.  The peaks of analysis frame i (mag[i, k] greater than mag[i, k +-1] and
 * mag[i, k +-2]; neighbours outside 0..512 are not compared) keep their sums; every other bin takes its nearest peak's
 * (a tie: the lower peak's) plus phase[i, k] - phase[i, kp]; a frame without a peak stays as it is.  The sums themselves are
 * never locked.  It needs scratch: t2v_phase_vocoder_scratch_bytes(B, out_stride, phase_lock) bytes of device memory (0
 * without locking), and B <= 65535.
 * phase == phase_out == NULL: magnitudes only (no scratch, phase_lock ignored).
 * A null required pointer, one of phase / phase_out alone, B < 1, T outside 1..T2V_TSM_MAX_FRAMES, t_stride < T or
 * out_stride < ceil(T den / num) is T2V_ERR_ARG. */
#define T2V_TSM_BINS 513
#define T2V_TSM_MAX_RATIO 1023
#define T2V_TSM_MAX_FRAMES (1 << 20)
size_t t2v_phase_vocoder_scratch_bytes(int B, int out_stride, int phase_lock);
int t2v_phase_vocoder(const float* mag, const float* phase, const int32_t* n_frames, int B, int T, int t_stride, int num, int den,
                      int phase_lock, float* mag_out, float* phase_out, int out_stride, void* scratch, void* stream);

/* ------------------------------------------------------------------ a phase from magnitudes alone
 * Single-pass spectrogram inversion (Beauregard, Harish and Wyse 2015) of a ragged batch (csrc/phase_init.hip): the start that
 * Griffin-Lim otherwise draws at random.  mag and phase_out are (B, 513, t_stride) fp32 as t2v_stft_polar writes them (n_fft
 * 1024, hop 256: a quarter turn per bin and frame), row b has n_frames[b] frames (device int32, clamped to 0..T; T <= t_stride
 * is the most any row has); nothing at or past frame n_frames[b] is read, and phase_out is +0 from there to t_stride.
 * Turns are 32-bit fixed-point fractions of a turn, uint32, wrapping.  In frame m:
 *   a peak is a bin k in 1..511 with mag[k] > mag[k - 1] and mag[k] > mag[k + 1] in fp32 (a plateau has none);
 *   p = (0.5 (a - c)) / ((a - 2 b) + c) in fp64, uncontracted, from a, b, c = mag[k - 1], mag[k], mag[k + 1];
 *   adv(k, m) = ((k & 3) << 30) + rint(p 2^30) at a peak and 0 elsewhere;  acc(k, m) = sum of adv(k, m') over m' <= m;
 *   bin k takes its nearest peak kp (a tie: the lower one): turns = acc(kp, m) - ((k - kp) << 31) + rint(p(kp, m) 2^31),
 *   phase_out = (float)((double)(int32_t)turns 2 pi / 2^32), in [-pi, pi);  a frame without a peak is +0 in every bin.
 * The sums are integer sums: a row gives the same bits alone, in any batch and at any stride.
 * scratch: t2v_spsi_scratch_bytes(B, t_stride) bytes of device memory (the accumulators); the library allocates nothing.
 * B < 1, T outside 1..T2V_TSM_MAX_FRAMES, t_stride < T or above 2^30, or more than 2^31 - 1 workgroups is T2V_ERR_DIMS; a null
 * pointer is T2V_ERR_ARG. */
size_t t2v_spsi_scratch_bytes(int B, int t_stride);
int t2v_spsi(const float* mag, const int32_t* n_frames, int B, int T, int t_stride, float* phase_out, void* scratch, void* stream);

/* ------------------------------------------------------------------ spectral envelope: pitch and timbre as two knobs
 * The true-envelope estimate of a ragged batch of STFT magnitudes, and the spectrum with its envelope moved along frequency
 * (csrc/envelope.hip, one launch).  mag is (B, 513, t_stride) fp32 as t2v_stft_polar writes it, row b has n_frames[b] frames
 * (device int32, clamped to 0..T; T <= t_stride is the most any row has); nothing at or past frame n_frames[b] is read.
 * Per frame, m[k] its 513 magnitudes:
 *   floor = max(1e-7f * max_k m[k], 1e-10f) (the max is exact in fp32),  L[k] = log(max(m[k], floor)).
 *   lifter(x), order 1..T2V_ENV_MAX_ORDER: x[0..512] is even-extended to 1024 points (x[1024 - k] = x[k]); its DFT / 1024 is
 *     the real cepstrum c[n]; c[n] is kept for n <= order and n >= 1024 - order and zeroed elsewhere; the DFT of that, real
 *     part of bins 0..512, is the result.  Both are the same forward real 1024-point FFT of a real even sequence; imaginary
 *     parts are dropped.
 *   True envelope (Roebel and Rodet), a fixed count iters in 0..T2V_ENV_MAX_ITERS: A = L; iters + 1 times E = lifter(A),
 *     A = max(L, E).  The result is the last E, a natural-log envelope; iters = 0 is the plain cepstral envelope.  There is
 *     no convergence test: a frame's bits depend on that frame alone, whatever the batch and the strides.
 *   Warp by p / q, each in 1..T2V_TSM_MAX_RATIO, positions in integers: pos = k p, i = pos / q, a = (pos % q) / q,
 *     Ew[k] = (1 - a) E[i] + a E[i + 1], and Ew[k] = E[512] for i >= 512;  mag_out[k] = m[k] exp(Ew[k] - E[k]): the envelope
 *     read at k p / q, so it moves along frequency by q / p, and the fine structure stays.  p == q gives m[k], bit for bit.
 * log_env_out and mag_out are (B, 513, out_stride), either may be NULL; both are +0 from n_frames[b] to out_stride.  The
 * library keeps no scratch and reads no table.
 * order, iters, p or q out of range, B < 1, T outside 1..T2V_TSM_MAX_FRAMES or more than 2^31 - 1 workgroups is T2V_ERR_DIMS;
 * a null mag or n_frames, both outputs NULL, or a stride below T (or above 2^30) is T2V_ERR_ARG. */
#define T2V_ENV_BINS 513
#define T2V_ENV_MAX_ORDER 256
#define T2V_ENV_MAX_ITERS 32
int t2v_spectral_envelope(const float* mag, const int32_t* n_frames, int B, int T, int t_stride, int order, int iters, int p, int q,
                          float* log_env_out, float* mag_out, int out_stride, void* stream);

/* ------------------------------------------------------------------ voice quality: spectral balance and cepstral peak prominence
 * The spectral-balance descriptors of eGeMAPS (Eyben et al. 2016) and the cepstral peak prominence of Hillenbrand et al. (1994)
 * of a ragged batch of 16 kHz waveforms (csrc/voice.hip, one launch), on the grid of t2v_f0_yin, t2v_loudness and
 * t2v_trim_bounds: y is (B, y_stride) fp32, row b has n[b] samples (device int32, clamped to 0..y_stride) and n[b] / 256 + 1
 * frames (none for n[b] = 0); frame t covers the samples [256 t - 512, 256 t + 512), every sample index outside [0, n[b])
 * counts as 0 and nothing outside is read.  Per frame, with x its 1024 samples, w the front end's periodic Hann window
 * (0.5 - 0.5 cos(2 pi i / 1024) in fp64, rounded once), P[k] = |DFT1024(x w)[k]|^2 for k = 0..512 (a bin is 15.625 Hz),
 * fl = max(1e-9 max_k P, the smallest normal fp32) and dB(v) = 10 log10 v, the T2V_VOICE_FEATS planes of out,
 * (B, T2V_VOICE_FEATS, t_stride) fp32 with time contiguous, are
 *   0 level_db       dB(max(sum_{k=4..319} P, fl)): the 50 Hz - 5 kHz band; the host gates on it;
 *   1 alpha_db       dB(max(sum_{k=64..319} P, fl) / max(sum_{k=4..63} P, fl)): 1 - 5 kHz over 50 Hz - 1 kHz;
 *   2 hammarberg_db  dB(max(max_{k=0..127} P, fl) / max(max_{k=128..319} P, fl)): the peak below 2 kHz over the peak in 2 - 5 kHz;
 *   3 slope_db_khz   the least-squares slope of L[k] = dB(max(P[k], fl)) on 15.625 k / 1000 over k = 32..96 (500 - 1500 Hz),
 *                    from centred abscissae: sum (k - 64) L[k] / 357.5;
 *   4 cpp_db         c[q] = Re DFT1024(even extension of L)[q] / 1024 for q = 0..512 (L[1024 - k] = L[k]; the transform of the
 *                    spectral envelope's lifter), C[q] = 20 log10 max(|c[q]|, 1e-3 max_{q=16..266} |c[q]|, 1e-4), q* the lowest q
 *                    in 32..266 (the 60 - 500 Hz lags of the tracker) with the largest C[q]; cpp_db = C[q*] less the value at q*
 *                    of the least-squares line of C on q over q = 16..266.  A difference of dB values: the scale of L drops out;
 *   5 cpp_lag        (float)q*.
 * The floor fl holds for every band sum and band maximum, so a band without energy in a frame that is not silent reads 90 dB
 * under the frame's largest bin and no ratio divides by 0.  The absolute floor 1e-4 (dB: c has L's unit) is some four decades
 * under the cepstral peak of a voice and far above the rounding of a flat L (a single impulse): such a frame has all C equal,
 * cpp_db 0 to rounding and cpp_lag 32, whatever the rounding was.
 * The transform of x w runs in fp64 and each P[k] is rounded to fp32 once (an fp32 transform is off by a fraction of an ulp
 * of the largest bin in every bin, and the planes read bins 50 to 90 dB under it); everything from L on is fp32.
 * A frame with sum_k P = 0 is silent: level_db = T2V_VOICE_SILENT_DB and +0 on the other five.  Frames at and past a row's
 * count are +0 on all planes, up to t_stride.
 * A workgroup owns T2V_VOICE_FRAMES consecutive frames of one row, a wave each.  Every sum and maximum is a wave reduction in
 * a fixed order, ties go to the lower index, and there is no floating-point atomic: a frame's bits depend on that frame alone,
 * so a row gives the same bits alone, in any batch and at any stride.  The call takes no table and no scratch.
 * A null pointer, B < 1, y_stride < 1 or above 2^30, or t_stride < y_stride / 256 + 1 is T2V_ERR_ARG; more than 2^31 - 1
 * workgroups (B ceil(t_stride / T2V_VOICE_FRAMES)) is T2V_ERR_DIMS. */
#define T2V_VOICE_FEATS 6
#define T2V_VOICE_FRAMES 8          /* frames per workgroup */
#define T2V_VOICE_SILENT_DB -200
int t2v_voice_quality(const float* y, const int32_t* n, int y_stride, int B, float* out, int t_stride, void* stream);

/* ------------------------------------------------------------------ batch collate from the resident corpus (csrc/collate.hip)
 * The training set lives on the device as flat stores (corpus.ResidentCorpus): utterance u has its log-mel (80, n_frames[u])
 * fp32, row-major with its OWN row stride n_frames[u], at mel_store + mel_off[u], and its n_ids[u] symbol ids (int32) at
 * id_store + id_off[u]; speaker[u] and emotion[u] are class indices.  All of these and idx are device memory.
 *
 * One launch writes the reference's collated batch (data_utils.py:88-137) for the B utterances idx[0 .. B), row b from
 * utterance idx[b] (the caller has sorted the rows), with T_b = n_frames[idx[b]] and L_b = n_ids[idx[b]]:
 *   text_padded (B, T_in) int64       the ids, then 0;
 *   mel_padded (B, 80, T_out) fp32    the stored frames, then 0.0;
 *   gate_padded (B, T_out) fp32       1.0 from frame T_b - 1 on, 0.0 before;
 *   output_lengths (B) int64          T_b;
 *   speakers (B, n_speakers), emotions (B, n_emotions) int64   one-hot rows (all 0 for a class index outside the width).
 * Every output element is written exactly once, pads included, so the outputs may be uninitialised memory; no atomics: equal
 * inputs give equal bits.  The indices and the two widths are the caller's to check on the host (0 <= idx[b] < n_utts,
 * L_b <= T_in, T_b <= T_out); the kernel clamps an index to 0..n_utts-1 and the counts to T_in / T_out, so nothing outside a
 * store is read and nothing outside an output is written, whatever idx holds.
 * A null pointer, B < 1, n_utts < 1, T_in < 1, T_out < 1, n_speakers < 1 or n_emotions < 1 is T2V_ERR_ARG. */
int t2v_collate_batch(const float* mel_store, const int64_t* mel_off, const int32_t* n_frames, const int32_t* id_store,
                      const int64_t* id_off, const int32_t* n_ids, const int32_t* speaker, const int32_t* emotion,
                      const int32_t* idx, int B, int n_utts, int T_in, int T_out, int n_speakers, int n_emotions,
                      int64_t* text_padded, float* mel_padded, float* gate_padded, int64_t* output_lengths,
                      int64_t* speakers, int64_t* emotions, void* stream);

/* ------------------------------------------------------------------ forced alignment: symbol durations by monotonic search
 * The best monotonic path through B alignment matrices (csrc/durations.hip), with the strides and lengths of
 * t2v_alignment_stats: A fp32 with element (b, t, j) at A[b a_stride_b + t a_stride_t + j]; row b has n = n_frames[b] valid
 * frames and L = n_ids[b] valid symbols (device int32).  Only A[b, t < n, j < L] is read and A is never written.  Measure:
 *   a(t, j) = max(A[b, t, j], T2V_MAS_FLOOR); a NaN counts as the floor;
 *   a path p has p_0 = 0, p_{n-1} = L - 1 and p_t - p_{t-1} in {0, ..., max_step};
 *   Q(0, 0) = ln a(0, 0);  Q(t, j) = ln a(t, j) + max_{s = 0..max_step} Q(t-1, j-s), one fp32 add per cell (logf, then +);
 *   on equal Q the smallest step wins (staying beats advancing);
 *   cells outside the reachable band (j <= t S and L - 1 - j <= (n - 1 - t) S, S = max_step) are -inf and never chosen.
 * Outputs, by a walk back from (n - 1, L - 1) along the kept decisions:
 *   path      (B, path_stride) int32: p_t for t < n, -1 from n to the stride;
 *   durations (B, sym_stride) int32:  the number of frames t with p_t = j for j < L, 0 from L to the stride;
 *   starts    (B, sym_stride) int32:  the first frame of symbol j, or, where its duration is 0 (a skipped symbol, max_step >=
 *                                     2), the frame where it would start: the prefix sums of durations.  0 from L on;
 *   score     (B) fp32:               Q(n-1, L-1) / n, the mean over frames of ln a(t, p_t).
 * A row with no feasible path (L - 1 > (n - 1) max_step, or a length clamped to 0) gets score NaN, path -1, durations 0 and
 * starts 0 over the whole strides; the other rows of the batch are not affected.
 * One workgroup per row; a row gives the same bits alone, in any batch, at any stride and with any padding.  No atomics.
 * Any B, N >= 1; 1 <= T_in <= T2V_MAS_MAX_SYMBOLS and 1 <= max_step <= 3, else T2V_ERR_DIMS.  A null pointer, B, N or
 * T_in < 1, a_stride_t < T_in, a_stride_b < (N - 1) a_stride_t + T_in, path_stride < N or sym_stride < T_in is T2V_ERR_ARG.
 * The lengths are the caller's to check on the host (1 <= n <= N, 1 <= L <= T_in); the kernel clamps them to 0..N and 0..T_in,
 * so none addresses outside the tensor.
 * scratch: t2v_mas_scratch_bytes(B, N, T_in) bytes of device memory, the caller's: one decision byte per cell (0 for sizes
 * that are refused).
 *
 * t2v_segment_means: sums of a frame track over the segments of such a path.  v (B, v_stride) fp32; counted (B, v_stride)
 * bytes, non-zero where a frame counts, or NULL (every frame counts); starts / durations (B, seg_stride) int32.  For symbol
 * j < T_in of row b, with the segment [starts, starts + durations) clamped to 0..v_stride:
 *   sums (B, out_stride) fp32:    0.f + the v of its counted frames, added in ascending frame order;
 *   counts (B, out_stride) int32: the number of those frames.
 * One thread per symbol: the order of every sum depends on the row alone.  A segment of duration 0 gives 0 and 0.  Columns
 * from T_in to out_stride are not written.  A null pointer other than counted, B, T_in or v_stride < 1, seg_stride < T_in or
 * out_stride < T_in is T2V_ERR_ARG. */
#define T2V_MAS_MAX_SYMBOLS 2048    /* the two live rows of Q in LDS: 2 x 2048 fp32 */
#define T2V_MAS_FLOOR 1e-8f         /* below fp32's epsilon next to a row sum of 1; |ln| = 18.42 bounds a cell's penalty */
size_t t2v_mas_scratch_bytes(int B, int N, int T_in);
int t2v_mas(const float* A, long long a_stride_b, long long a_stride_t, const int32_t* n_frames, const int32_t* n_ids, int B,
            int N, int T_in, int max_step, int32_t* path, int path_stride, int32_t* durations, int32_t* starts, int sym_stride,
            float* score, void* scratch, void* stream);
int t2v_segment_means(const float* v, const void* counted, int v_stride, const int32_t* starts, const int32_t* durations,
                      int seg_stride, int B, int T_in, float* sums, int32_t* counts, int out_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
