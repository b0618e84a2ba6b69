// The forward kernels of the reference encoder, included twice by refenc.hip: REFENC_RAGGED 0 defines the training
// path's k_conv2d_s2_fwd / k_im2col_s2 / k_gru_fwd, REFENC_RAGGED 1 the ragged inference instances k_conv2d_s2_fwd_ragged /
// k_im2col_s2_ragged (input rows bounded at each item's own height, refenc_in_ragged) and k_gru_fwd_len (each item's state
// after its own step count -> h_last).  Two preprocessor instances rather than a template: the REFENC_RAGGED 0 text is the
// kernels as they were, so their instructions stay the same (DESIGN 7d).
#if REFENC_RAGGED
#define REFENC_IN(b, c, h, w) refenc_in_ragged(a, rg, b, c, h, w)
#else
#define REFENC_IN(b, c, h, w) refenc_in(a, b, c, h, w)
#endif

// grid = (tiles of Ho*Wo, B*Cout): the filter of this output channel sits in LDS (broadcast reads)
#if REFENC_RAGGED
__global__ __launch_bounds__(256) void k_conv2d_s2_fwd_ragged(Conv2dArgs a, RaggedSrc rg) {
#else
__global__ __launch_bounds__(256) void k_conv2d_s2_fwd(Conv2dArgs a) {
#endif
    __shared__ float wsh[131 * 9];
    const int Cin = a.Cx + (a.coord ? 3 : 0);
    const int b = blockIdx.y / a.Cout, co = blockIdx.y % a.Cout;
    for (int i = threadIdx.x; i < Cin * 9; i += 256) wsh[i] = a.w[(size_t)co * Cin * 9 + i];
    __syncthreads();
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.Ho * a.Wo) return;
    const int ho = r / a.Wo, wo = r - ho * a.Wo;
    float acc = a.bias ? a.bias[co] : 0.f;
    for (int c = 0; c < Cin; ++c)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
                acc = fmaf(wsh[c * 9 + kh * 3 + kw], REFENC_IN(b, c, 2 * ho - 1 + kh, 2 * wo - 1 + kw), acc);
    a.y[((size_t)b * a.Cout + co) * a.Ho * a.Wo + r] = acc;
}

#if REFENC_RAGGED
__global__ __launch_bounds__(256) void k_im2col_s2_ragged(Conv2dArgs a, RaggedSrc rg, float* __restrict__ col) {
#else
__global__ __launch_bounds__(256) void k_im2col_s2(Conv2dArgs a, float* __restrict__ col) {
#endif
    const int Cin = a.Cx + (a.coord ? 3 : 0), K = Cin * 9, P = a.Ho * a.Wo;
    const size_t n = (size_t)a.B * P * K;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int k = (int)(e % K);
        const size_t bp = e / K;
        const int pos = (int)(bp % P), b = (int)(bp / P);
        const int c = k / 9, t9 = k - c * 9, kh = t9 / 3, kw = t9 - kh * 3;
        const int ho = pos / a.Wo, wo = pos - ho * a.Wo;
        col[e] = REFENC_IN(b, c, 2 * ho - 1 + kh, 2 * wo - 1 + kw);
    }
}

// REFENC_RAGGED 1: item b's answer is its state after its own steps[b] steps, written to h_last[b] in the step that makes it;
// the item keeps stepping over its padded rows after that, and nothing reads those states.
#if REFENC_RAGGED
__global__ __launch_bounds__(256) void k_gru_fwd_len(GruArgs a, const int* steps, float* h_last) {
#else
__global__ __launch_bounds__(256) void k_gru_fwd(GruArgs a) {
#endif
    const int j = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = lane & 15, g = lane >> 4;
    const bool bvalid = b < a.B;
#if REFENC_RAGGED
    const int stepb = bvalid ? steps[b] : 0;
#endif
    __shared__ float hbuf[16][GRU_H + 4];
    // A fragments of this wave's two tiles: row i = lane&15 -> (unit i>>2, gate slot i&3), k = 4s + g
    float wreg[2][64];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const int unit = j * GRU_UNITS + (2 * wave + tt) * 4 + ((lane & 15) >> 2);
        const int slot = lane & 3;
#pragma unroll
        for (int s = 0; s < 64; ++s)
            wreg[tt][s] = slot < 3 ? a.whh[(size_t)(slot * GRU_H + unit) * GRU_H + 4 * s + g] : 0.f;
    }
    float bh[2][3];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const int U = j * GRU_UNITS + (2 * wave + tt) * 4 + g;
#pragma unroll
        for (int r = 0; r < 3; ++r) bh[tt][r] = a.bhh[r * GRU_H + U];
        if (bvalid) a.hs[((size_t)b * (a.T + 1)) * GRU_H + U] = 0.f;
    }
    for (int i = tid; i < 16 * (GRU_H + 4); i += 256) (&hbuf[0][0])[i] = 0.f;
    __syncthreads();

    for (int t = 0; t < a.T; ++t) {
        float giv[2][3];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int U = j * GRU_UNITS + (2 * wave + tt) * 4 + g;
#pragma unroll
            for (int r = 0; r < 3; ++r) giv[tt][r] = bvalid ? a.gi[((size_t)b * a.T + t) * GRU_G + r * GRU_H + U] : 0.f;
        }
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const float* hrow = &hbuf[b][g];
#pragma unroll
        for (int s = 0; s < 64; ++s) {
            const float hv = hrow[4 * s];
            acc0 = mfma16x4(wreg[0][s], hv, acc0);
            acc1 = mfma16x4(wreg[1][s], hv, acc1);
        }
        float* hx_w = a.xchg + (size_t)(t & 1) * 16 * GRU_H;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const f32x4 acc = tt == 0 ? acc0 : acc1;
            const int U = j * GRU_UNITS + (2 * wave + tt) * 4 + g;
            if (bvalid) {
                const float r = sigmoidf_(giv[tt][0] + acc[0] + bh[tt][0]);
                const float z = sigmoidf_(giv[tt][1] + acc[1] + bh[tt][1]);
                const float hn = acc[2] + bh[tt][2];
                const float n = tanhf_(giv[tt][2] + r * hn);
                const float hnew = (1.f - z) * n + z * hbuf[b][U];
                if (a.gsave) {
                    float* sv = a.gsave + (((size_t)b * a.T + t) * 4) * GRU_H + U;
                    sv[0] = r; sv[GRU_H] = z; sv[2 * GRU_H] = n; sv[3 * GRU_H] = hn;
                }
                a.hs[((size_t)b * (a.T + 1) + t + 1) * GRU_H + U] = hnew;
#if REFENC_RAGGED
                if (t + 1 == stepb) h_last[(size_t)b * GRU_H + U] = hnew;
#endif
                st_sc1(hx_w + (size_t)b * GRU_H + U, hnew);
            }
        }
        if (t + 1 == a.T) break;
        if (!group_barrier(a.sync, (unsigned)(GRU_NW * (t + 1)), a.sync + 1)) return;
        {   // the new hidden state of every item: all loads of a thread in flight at once (round 6 — as a plain loop over the items
            // every iteration waited for its own load: one memory round trip per item and step; rows past B re-read row B - 1)
            float hv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) hv[u] = ld_sc1(hx_w + (size_t)min(u, a.B - 1) * GRU_H + tid);
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (u < a.B) hbuf[u][tid] = hv[u];
        }
        __syncthreads();
    }
}

#undef REFENC_IN
