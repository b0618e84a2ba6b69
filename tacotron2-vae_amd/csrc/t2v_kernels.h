// Internal kernel-argument structs shared by the decoder translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include "../../include/t2vae.h"
#include "t2v_common.h"

enum { T2V_RNG_ATT_H = 1, T2V_RNG_ATT_C = 2, T2V_RNG_DEC_H = 3, T2V_RNG_DEC_C = 4,
       T2V_RNG_PRENET0 = 5, T2V_RNG_PRENET1 = 6 };

int t2v_check_launch();
// gemm.hip: `n` zeroed arrival counters for a launch whose workgroups find out which of them finishes last (split-K tiles,
// column-sum slices); the launch leaves them at zero
unsigned* t2v_arrival_counters(int n);
extern unsigned long long* g_t2v_prof;   // device buffer of 32 u64 or NULL (t2v_set_phase_profile)                 // records hipGetLastError() for t2v_last_error()
const t2v_step_params* t2v_step_for(hipStream_t stream);   // device-side per-step parameters bound to this stream, else the process default, else NULL

// several device regions (byte counts: multiples of 4) zeroed by ONE launch (t2v_runtime.hip)
struct T2VZeroRegions {
    void* p[10];
    size_t bytes[10];
    int n = 0;
    void add(void* ptr, size_t nbytes) { p[n] = ptr; bytes[n] = nbytes; ++n; }
};
void t2v_zero_regions(T2VZeroRegions& z, hipStream_t stream);

// persistent decoder kernels (t2v_xchg.h, t2v_runtime.hip):
// n16 16-byte words at p set to the exchange sentinel by `grid` workgroups of 256 threads
__global__ void k_sentinel_fill(uint4* p, size_t n16);
void t2v_fill_sentinel(void* p, size_t n16, int grid, hipStream_t stream);
// the device has >= T2V_NWG CUs (one resident workgroup each)
bool t2v_persist_cus_ok();
// dynamic-LDS limit of `kernels` raised to T2V_LDS_MAX once (`raised`: the launcher's flag); false leaves the runtime error pending
bool t2v_persist_raise_lds(std::initializer_list<const void*> kernels, bool& raised);
// 1 when T2V_NWG workgroups of `kernel` (`threads` threads, `lds` bytes of dynamic LDS) can all be resident: enough CUs, the
// limit raised (as above), occupancy >= 1 per CU; a runtime error on the way is cleared
int t2v_persist_resident(const void* kernel, int threads, size_t lds, std::initializer_list<const void*> kernels, bool& raised);
struct LstmFwdArgs;
struct AttnFwdArgs;

// ---- layout of the QP scratch buffer (t2v_dec_train_bufs.QP / t2v_dec_infer_bufs.QP), in floats:
//   [0, B*256*128)            per-workgroup partial queries of the current step
//   + [0, 64)                 uint32 sync / error words (attention error word = [31]; decode loop: counter [32], error [47])
//   + [64, 64 + 4096)         exchange area of the decode loop's projection/Prenet kernel
//   + [4160, 4160 + 2*B*8*Tcap)  8-byte {partial energy, epoch tag} granules of the attention forward exchange,
//                             Tcap = T_in rounded up to 16  (t2v_decoder_qp_floats() in t2vae.h returns the total)
typedef unsigned long long t2v_u64;
static inline size_t t2v_tcap(int T_in) { return (size_t)((T_in + 15) / 16) * 16; }
static inline size_t t2v_qp_sync_off(int B) { return (size_t)B * 256 * 128; }
static inline size_t t2v_qp_xchg_off(int B) { return t2v_qp_sync_off(B) + 64; }
static inline size_t t2v_qp_ex_off(int B) { return t2v_qp_sync_off(B) + 64 + 4096; }
#define T2V_MAX_T_IN 4096
static inline size_t t2v_qp_floats(int B, int T_in) { return t2v_qp_ex_off(B) + 2 * (size_t)B * 8 * t2v_tcap(T_in); }
// attention-backward slicing: positions per workgroup and slices per item
static inline int t2v_attn_bwd_js(int T_in) { return T_in <= 128 ? 16 : 32; }
static inline int t2v_attn_bwd_slices_(int T_in) { const int js = t2v_attn_bwd_js(T_in); return (T_in + js - 1) / js; }
void t2v_launch_lstm_fwd(int mode, const LstmFwdArgs& a, hipStream_t stream);
void t2v_launch_attn_fwd(const AttnFwdArgs& f, int B, int T_in, hipStream_t stream);
void t2v_launch_attn_fwd_window(const AttnFwdArgs& f, int B, int T_in, int back, int ahead, hipStream_t stream);   // free-running decode: t2v_dec_window
void t2v_launch_attn_fwd_plan(const AttnFwdArgs& f, int B, int T_in, int back, int ahead, const int32_t* plan, int plan_stride,
                              const int32_t* n_plan, int t, hipStream_t stream);                                   // the planned decode
// The two persistent forward launchers (fp32 / bf16), after their shape and offset checks: the checks of the remaining
// arguments, then the per-pass resets — the sync / error words, the zero initial states of the arena (as
// t2v_decoder_train_fwd).  Returns the sync words, or NULL (nothing issued) on a bad argument.
static inline unsigned* t2v_persist_fwd_begin(const t2v_dec_train_persist_weights* w, const t2v_dec_train_bufs* s, const float* scratch,
                                              int B, int T_in, hipStream_t stream) {
    if (!w->w_ih_att || !w->w_hh_att || !w->w_ih_dec || !w->w_hh_dec || !w->bias_dec || !w->wq || !w->wcomb || !w->v || !s->gpre ||
        !s->memory || !s->pm || !s->XS || !s->CA || !s->CD || !s->QP || !s->AL || !s->ACUM)
        return nullptr;
    if ((uintptr_t)scratch & 15) return nullptr;
    unsigned* sync = (unsigned*)(s->QP + t2v_qp_sync_off(B));
    T2VZeroRegions z;
    z.add(sync, 64 * sizeof(uint32_t));
    z.add(s->XS, sizeof(float) * 2 * B * T2V_XW);
    z.add(s->CA, sizeof(float) * B * T2V_H);
    z.add(s->CD, sizeof(float) * B * T2V_H);
    z.add(s->AL, sizeof(float) * B * T_in);
    z.add(s->ACUM, sizeof(float) * B * T_in);
    t2v_zero_regions(z, stream);
    return sync;
}

// What the two persistent forward kernels share with their attention role (t2v_attn_role_fwd.inc)
#define T2V_AF_THREADS 512           // workgroup size of both kernels
#define T2V_AF_SPIN 1500000u         // bound of their waits
#define T2V_AF_MAXT 224              // LDS-resident W_q / processed-memory slices up to here
#define T2V_AF_MAXT_LONG 560         // register-resident ones beyond (the LONG instantiations)
#define T2V_AF_NTI_LONG 5            // 16-position tiles per wave of the long form: 8 waves x 5 x 16 = 640 >= 560
// floats of the role's LDS carve; `tail`: what the kernel keeps between rss and flag (AF_TAIL)
static inline size_t t2v_attn_fwd_lds_floats(int T_in, size_t tail) {
    const size_t Tcap = t2v_tcap(T_in);
    const bool lng = T_in > T2V_AF_MAXT;                 // W_q / processed memory in registers
    return (lng ? 0 : 16 * 1028) + Tcap * 64 + (lng ? 0 : Tcap * 16) + 2 * (Tcap + 32) + Tcap + (lng ? T2V_CTX_PAD : 0) + T2V_H + 16 +
           32 * 16 + 8 * 64 + 32 + 32 + tail + 4;
}

struct LstmFwdArgs {
    const float4* packA;
    const float4* packD;
    int k_att;
    const float* xs_prev;   // XS[t]   (B,2560) = [h_att_{t-1} | ctx_{t-1} | h_dec_{t-2}]
    float* xs_next;         // XS[t+1]
    const float* gpre_t;    // (B,4096) hoisted prenet term + biases (training) or NULL
    const float* pre_t;     // (B,256) prenet output (inference) or NULL
    const float* bias_att;
    const float* bias_dec;
    const float* ca_prev;   // CA[t]
    float* ca_cur;          // CA[t+1]
    const float* cd_prev;   // CD[t-1]
    float* cd_cur;          // CD[t]
    float* ga_t;            // GA[t]   or NULL
    float* gd_t;            // GD[t-1] or NULL
    const float* wqT;
    float* qp;
    int shared_x;           // fp32 packs: one load of the [h_att | ctx] state columns serves both cells (lstm256_stream_shared)
    int B, t, do_att, do_dec;
    float p_att, p_dec;
    uint64_t seed;
    const t2v_step_params* step;
};

struct AttnFwdArgs {
    const float* qp;
    const float* al_prev;
    const float* acum_prev;
    float* al_cur;
    float* acum_cur;
    const float* memory;
    const float* pm;
    const int32_t* lengths;
    const float* wcomb;         // (128,64) fused location filter bank (t2v_fuse_location_weights)
    const float* v;
    float* xs_next;
    float* s_save;
    int T_in;
    unsigned long long* prof;   // optional phase stamps (s_memtime) from workgroup (0,0) thread 0
    t2v_u64* ex;                // (B,8,Tcap) granules {partial energy, tag}: exchange between the 8 workgroups of an item
    unsigned* err;              // error word (bounded-spin timeout)
    unsigned epoch;             // 1-based launch index within the pass = the granule tag of this step
};

struct LstmBwdArgs {
    const float4* packBD;   // 160 tiles (uint2 per lane and k-block when the packs are bf16)
    const float4* packBA;   // 96 tiles
    const float* dgd_t;     // DGD[t]   (B,4096)
    const float* dga_n;     // DGA[t+1] (B,4096) or NULL
    float* YD;              // (B,2560)
    float* YA;              // (B,1536)
    int B;
    int flip;               // walk the k-blocks backwards (alternates per launch for L2 reuse)
};

struct AttnBwdArgs {
    const float* dHC_t;     // (B,1536)
    const float* YD;
    const float* YA;
    const float* al_cur;    // AL[t+1]
    const float* memory;
    const float* wcomb;     // (128,64) fused location filter bank
    const float* v;
    float* S_t;             // (B,T_in,128) in: tanh outputs, out: dpre
    t2v_u64* DQ_t;          // (B,S,128) granules {partial dq, tag 1}
    float* DCTX_t;          // (B,512)
    const float* ctx_t;     // XS[t+1] + 1024: attention context of step t (row stride 2560)
    const float* GP_in;     // (B,S,2,64) per-slice partial dcat rows written by reverse step t+1
    float* GP_out;          // (B,S,2,64) ... written by this step (other parity)
    float* GC;              // (B,S,Tcap) per-workgroup running copies of the cumulative-weights gradient
    float* DV;              // (B,S,128) per-slice accumulators
    int T_in;
    unsigned long long* prof;
    // last, so that every field above sits where it sat before the operand existed
    const float* dal_t;     // (B,T_in) upstream gradient of the alignment of step t (k_attn_cell_bwd<.., true>; nullptr in the others)
};

struct CellBwdArgs {
    const float* YD;
    const float* YA;
    const t2v_u64* DQ_t;    // (B,S,128) granules of step t
    int S;                  // slices per item
    const float* wqT;       // (1024,128)
    const float* dHC_prev;  // dHC[t-1] (B,1536)
    const float* GA_t;      // GA[t]
    const float* CA_cur;    // CA[t+1] (c~_t)
    const float* CA_prev;   // CA[t]   (c~_{t-1})
    const float* GD_p;      // GD[t-1]
    const float* CD_cur;    // CD[t]   (c~_{t-1} of decoder_rnn)
    const float* CD_prev;   // CD[t-1]
    float* DGA_t;           // DGA[t]
    float* DGD_p;           // DGD[t-1]
    float* DCA;
    float* DCD;
    int B, t, do_att, do_dec;
    float p_att, p_dec;
    uint64_t seed;
    const t2v_step_params* step;
    unsigned* err;          // error word (bounded-spin timeout)
    unsigned long long* prof;   // optional phase stamps of cell workgroup 0 (t2v_set_phase_profile slots 24..28)
};
