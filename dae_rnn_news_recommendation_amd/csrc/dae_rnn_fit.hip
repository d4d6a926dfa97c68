// dae_rnn_fit.hip -- the training steps of the LSTM and plain-RNN user models (dae_lstm_pair_loss, dae_rnn_pair_loss): one mini-batch
// of click histories forward and backward through time, the pairwise ranking loss of dae_user_pair_loss on the states of
// dae_lstm_user_states / dae_rnn_user_states, and the gradients of the four weight arrays.  E is fixed and gets no gradient.
// Definition: include/dae_hip.h.  The form is that of dae_gru_fit.hip, whose head explains the steps, the time-major stash and the
// weight-gradient route; what follows is what differs.  G = 4 gate blocks (LSTM, torch's order i, f, g, o) or 1 (RNN).
//
// Stash.  Row-major images [R x Hp], R = base[S], padding rows and columns >= H exact zeros:
//     HP   the input state of every step: slab 0 zeros, slab s + 1 rows < n_(s+1) = the outputs of step s
//     HG   the output state of every step; gru_loss_kernel (dae_fit_kernels.h) replaces each row by G
//     LSTM: SI SF SG SO   the gates; the backward step replaces them IN PLACE by da_i, da_f, da_g, da_o (the lane that reads an
//                         element is the one that writes it)
//           SC            c', the cell after every step.  The cell BEFORE step s is slab s - 1 of SC at the same sorted position (the
//                         users of a step are a prefix of those of the step before); at step 0 it is slab 0 of HP, which is zeros
//     RNN:  SH            a second copy of h', which survives the loss kernel's overwrite of HG; the backward step replaces it IN
//                         PLACE by da = dh (1 - h'^2)
// and transposed, K-contiguous images made once after the last backward step: DT [G Hp x R] (the da blocks in torch's gate order),
// HPT [Hp x R] and XT [Hp x R].  For these cells dgi = dgh, so the one DT serves both weight-gradient contractions.  13 arrays of
// R x Hp floats for the LSTM, 6 for the RNN.
//
// Forward: lstm_step_kernel<SKIP_K, LstmTrainParams> / rnn_step_kernel<SKIP_K, RnnTrainParams> (dae_rnn_step.h) -- the inference
// kernels' K loops and gate arithmetic; the epilogues store every gate as it is first complete.  The LSTM training form reads the
// cell from SC's previous slab and writes the next one instead of updating one buffer in place.
//
// Backward, LSTM: lstm_back_kernel, one launch per step from S - 1 down to 0, grid pad128(n_s) / 128 x Hp / 128.  One K loop of
// length 4 Hp over four segments -- A = slab s + 1 of da_i, da_f, da_g, da_o, Bt = the gate blocks of the image of W_hh^T
// [Hp x 4 Hp] -- gives the carry of dh through the recurrent weights; rows >= n_(s+1) do not take it and tiles wholly beyond skip
// the loop.  Epilogue, tc = tanhf(c') recomputed from the stored c' (the forward's own value):
//     dh = G + carry_h      dc = dh o (1 - tc^2) + carry_c (rows < n_(s+1))      da_o = dh tc o (1 - o)
//     da_i = dc g i (1 - i)      da_g = dc i (1 - g^2)      da_f = dc c_prev f (1 - f)      carry_c <- dc f
// carry_c is one [pad128(M) x Hp] buffer, every element owned by one lane of one tile; it is read only where the step after wrote
// it.  The LSTM has no direct h carry.  Two workgroups per CU (one accumulator set, nothing kept across passes).
// Backward, RNN: rnn_back_kernel, one K segment (A = slab s + 1 of da, Bt = W_hh^T), epilogue da = (G + carry) (1 - h'^2); no carry
// buffer; two workgroups per CU.
//
// Weight gradients: dW_ih = DT . XT^T and dW_hh = DT . HPT^T by the exact-fp32 NT GEMM of dae_gemm.hip, split over K into slabs
// that rnn_dw_fold_kernel adds in slab order; db_ih = db_hh = the row sums of DT (fp64, fixed order).
//
// Everything is a fixed-order sum, no atomics: bit-identical run to run.  The margins and the pair count are per-row quantities of
// states that do not depend on the other users (dae_rnn.hip); the gradients sum over rows in stash order and agree under a
// permutation of the users to rounding only.
#include "dae_fit_kernels.h"    // gru_loss_kernel, gru_loss_fold_kernel, gru_transpose_kernel
#include "dae_rnn_step.h"

#include <vector>

namespace dae {

// WhT[j][g Hp + k] = W_hh[g H + k][j]: the Bt operand of the backward step, zero outside H x H of every gate block
__global__ __launch_bounds__(256) void rnn_wht_kernel(const float* __restrict__ W_hh, int64_t ldwh, int H, int Hp, int G, float* __restrict__ WhT) {
    const int j = blockIdx.x;
    for (int q = threadIdx.x; q < G * Hp; q += 256) {
        const int g = q / Hp, k = q - g * Hp;
        WhT[(int64_t)j * G * Hp + q] = (j < H && k < H) ? W_hh[((int64_t)g * H + k) * ldwh + j] : 0.f;
    }
}

struct LstmBackParams {
    GemmParams g;                 // four K segments: A = slab s + 1 of da_i, da_f, da_g, da_o; Bt = the gate blocks of the W_hh^T image
    float *i, *f, *gg, *o;        // slab s: read, then overwritten with da_i, da_f, da_g, da_o
    const float* c;               // slab s of SC: c'
    const float* cprev;           // slab s - 1 of SC (slab 0 of HP, zeros, at step 0)
    const float* G;               // slab s of HG
    float* carry;                 // [pad128(M) x Hp]: in dc f of step s + 1 (rows < next), out that of step s (rows < rows)
    int H, Hp, rows, next;        // rows = n_s, next = n_(s+1) (0 at the last step)
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void lstm_back_kernel(LstmBackParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int tiles_n = p.Hp / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
    f32x16 acc[2][2];
    // a tile wholly beyond the users of the step after has no carry: no K tiles, the accumulators stay zero
    gemm_mainloop<float, 2>(p.g, tm, tn, 0, tm * BM < p.next ? p.g.ktiles_total : 0, lds, acc);
    const int Hp = p.Hp;
    const int col0 = tn * BN + wn * 64 + c;
    const int rbase = wm * 64 + 4 * g;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int i = tm * BM + rbase + acc_row(mt, rr, 0);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int col = col0 + nt * 32;
                const int64_t at = (int64_t)i * Hp + col;
                float da_i = 0.f, da_f = 0.f, da_g = 0.f, da_o = 0.f;
                if (i < p.rows && col < p.H) {
                    float dh = p.G[at];
                    if (i < p.next) dh += acc[mt][nt][rr];
                    const float gi = p.i[at], gf = p.f[at], gc = p.gg[at], go = p.o[at];
                    const float tc = tanhf(p.c[at]);
                    float dc = dh * go * (1.0f - tc * tc);
                    if (i < p.next) dc += p.carry[at];
                    da_o = dh * tc * go * (1.0f - go);
                    da_i = dc * gc * gi * (1.0f - gi);
                    da_g = dc * gi * (1.0f - gc * gc);
                    da_f = dc * p.cprev[at] * gf * (1.0f - gf);
                    p.carry[at] = dc * gf;
                }
                p.i[at] = da_i; p.f[at] = da_f; p.gg[at] = da_g; p.o[at] = da_o;
            }
        }
}

struct RnnBackParams {
    GemmParams g;                 // one K segment: A = slab s + 1 of da; Bt = the W_hh^T image
    float* h;                     // slab s of SH: h' read, then overwritten with da
    const float* G;               // slab s of HG
    int H, Hp, rows, next;        // rows = n_s, next = n_(s+1) (0 at the last step)
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void rnn_back_kernel(RnnBackParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int tiles_n = p.Hp / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
    f32x16 acc[2][2];
    gemm_mainloop<float, 2>(p.g, tm, tn, 0, tm * BM < p.next ? p.g.ktiles_total : 0, lds, acc);
    const int Hp = p.Hp;
    const int col0 = tn * BN + wn * 64 + c;
    const int rbase = wm * 64 + 4 * g;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int i = tm * BM + rbase + acc_row(mt, rr, 0);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int col = col0 + nt * 32;
                const int64_t at = (int64_t)i * Hp + col;
                float da = 0.f;
                if (i < p.rows && col < p.H) {
                    float dh = p.G[at];
                    if (i < p.next) dh += acc[mt][nt][rr];
                    const float h = p.h[at];
                    da = dh * (1.0f - h * h);
                }
                p.h[at] = da;
            }
        }
}

// dW[(g H + k) ld + j] = the sum over the slabs, in slab order, of S[(g Hp + k) Hp + j]; block = one row g H + k (torch's gate order
// is the order of the DT blocks)
__global__ __launch_bounds__(256) void rnn_dw_fold_kernel(const float* __restrict__ slabs, int splits, int64_t slab_stride, int H, int Hp,
                                                          float* __restrict__ dW, int64_t ld) {
    const int row = blockIdx.x, g = row / H, k = row - g * H;
    const float* s = slabs + ((int64_t)g * Hp + k) * Hp;
    for (int j = threadIdx.x; j < H; j += 256) {
        float v = 0.f;
        for (int sl = 0; sl < splits; ++sl) v += s[(int64_t)sl * slab_stride + j];
        dW[(int64_t)row * ld + j] = v;
    }
}

// the bias gradients: db_ih = db_hh = the row sums of DT [G Hp x R], one wave per row, fp64, lane sums in column order and then a
// fixed butterfly
__global__ __launch_bounds__(256) void rnn_db_kernel(const float* __restrict__ DT, int64_t R, int H, int Hp, int G, float* __restrict__ db_ih,
                                                     float* __restrict__ db_hh) {
    const int lane = threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (row >= G * Hp) return;
    const int b = row / Hp, j = row - b * Hp;
    if (j >= H) return;
    double s = 0.0;
    for (int64_t k = lane; k < R; k += 64) s += (double)DT[(int64_t)row * R + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        const float v = (float)s;
        db_ih[b * H + j] = v;
        db_hh[b * H + j] = v;
    }
}

// G gate blocks.  E, W_ih, W_hh, W_hh^T images, P; the stash images (13: LSTM, 6: RNN); the LSTM's cell carry; row_event, rowloss,
// rowpairs; split-K slabs
static uint64_t rf_workspace(int64_t G, int64_t Nap, int64_t Hp, int64_t Mp, int64_t Rb) {
    return al256(Nap * Hp * 4) + 3 * al256(G * Hp * Hp * 4) + al256(Nap * G * Hp * 4) + (G == 4 ? 13 : 6) * al256(Rb * Hp * 4) +
           (G == 4 ? al256(Mp * Hp * 4) : 0) + 2 * al256(Rb * 8) + al256(Rb * 4) + al256((uint64_t)GF_MAX_SPLITS * G * Hp * Hp * 4);
}

}  // namespace dae

using namespace dae;

// the body of both exports: G = 4 (LSTM) or 1 (RNN).  `fn` prefixes every message.
template <int G>
static int rnn_pair_loss(const char* fn, const float* E, int64_t lde, int32_t Na, int32_t H, const float* W_ih, int64_t ldwi, const float* W_hh,
                         int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr, const int32_t* items, const int32_t* order,
                         int64_t M, int64_t nnz, int32_t T, const int64_t* active_host, const int32_t* negatives, int32_t n_neg, double* loss,
                         int64_t* n_pairs, float* dW_ih, int64_t ld_dwi, float* dW_hh, int64_t ld_dwh, float* db_ih, float* db_hh, float* margin,
                         void* workspace, uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(M >= 0 && nnz >= 0 && T >= 0, "%s: negative count (M = %lld, nnz = %lld, T = %d)", fn, (long long)M, (long long)nnz, T);
    DAE_CHECK_ARG(Na > 0 && H > 0, "%s: Na and H must be positive (got %d, %d)", fn, Na, H);
    DAE_CHECK_ARG(n_neg >= 1 && n_neg <= GF_MAX_NEG, "%s: n_neg must be in 1..%d (got %d)", fn, GF_MAX_NEG, n_neg);
    DAE_CHECK_ARG(E && indptr, "%s: E / indptr are NULL", fn);
    DAE_CHECK_ARG(W_ih && W_hh && b_ih && b_hh, "%s: W_ih / W_hh / b_ih / b_hh are NULL", fn);
    DAE_CHECK_ARG((items && negatives) || nnz == 0, "%s: items / negatives are NULL", fn);
    DAE_CHECK_ARG(order || M == 0, "%s: order is NULL", fn);
    DAE_CHECK_ARG(active_host || T == 0, "%s: active_host is NULL", fn);
    DAE_CHECK_ARG(loss && n_pairs, "%s: loss / n_pairs are NULL", fn);
    DAE_CHECK_ARG(dW_ih && dW_hh && db_ih && db_hh, "%s: dW_ih / dW_hh / db_ih / db_hh are NULL", fn);
    DAE_CHECK_ARG(lde >= H && ldwi >= H, "%s: lde (%lld) and ldwi (%lld) must be >= H (%d): the state is scored against E, so D = H", fn,
                  (long long)lde, (long long)ldwi, H);
    DAE_CHECK_ARG(ldwh >= H && ld_dwi >= H && ld_dwh >= H, "%s: ldwh (%lld), ld_dwi (%lld) and ld_dwh (%lld) must be >= H (%d)", fn,
                  (long long)ldwh, (long long)ld_dwi, (long long)ld_dwh, H);
    int64_t events = 0;
    for (int t = 0; t < T; ++t) {
        DAE_CHECK_ARG(active_host[t] >= 0 && active_host[t] <= (t ? active_host[t - 1] : M),
                      "%s: active_host must be non-increasing and at most M (active_host[%d] = %lld)", fn, t, (long long)active_host[t]);
        events += active_host[t];
    }
    DAE_CHECK_ARG(events <= nnz, "%s: the schedule's T = %d steps hold %lld events, more than nnz = %lld", fn, T, (long long)events,
                  (long long)nnz);
    const int64_t Nap = pad128(Na), Hp = pad128(H), Mp = pad128(M), Rb = gf_rows_bound(nnz, T);
    DAE_CHECK_ARG(Nap * G * Hp * 4 < (1ll << 32) && G * Hp * Hp * 4 < (1ll << 32) && Mp * Hp * 4 < (1ll << 32) && G * Hp * Rb * 4 < (1ll << 32),
                  "%s: an operand image exceeds 4 GiB (Na = %d, H = %d, M = %lld, nnz = %lld: split the users into smaller calls)", fn, Na, H,
                  (long long)M, (long long)nnz);
    DAE_CHECK_ARG(M < (1ll << 31) && nnz < (1ll << 31), "%s: M = %lld / nnz = %lld exceed the grid", fn, (long long)M, (long long)nnz);
    hipStream_t st = (hipStream_t)stream;
    // the training steps: step s runs the users that have an event s + 1
    std::vector<int64_t> base;                                  // base[s] for s = 0 .. S
    base.push_back(0);
    for (int t = 1; t < T && active_host[t] > 0; ++t) base.push_back(base.back() + pad128(active_host[t]));
    const int S = (int)base.size() - 1;
    const int64_t R = base[S];
    auto rows_of = [&](int s) -> int64_t { return s < S ? active_host[s + 1] : 0; };
    if (S > 0) {                                                // (before any HIP call: every argument error comes first)
        const uint64_t need = rf_workspace(G, Nap, Hp, Mp, Rb);
        DAE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%llu < %llu bytes)", fn,
                      (unsigned long long)(workspace ? workspace_bytes : 0), (unsigned long long)need);
        DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "%s: workspace must be 256-byte aligned", fn);
    }
    if (margin && nnz > 0) DAE_CHECK_HIP(hipMemsetAsync(margin, 0, (size_t)nnz * n_neg * 4, st));
    if (S == 0) {                                               // nothing to predict: zero loss, zero pairs, zero gradients
        DAE_LAUNCH(gru_loss_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)nullptr, (const int32_t*)nullptr, (int64_t)0, loss, n_pairs);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(rnn_dw_fold_kernel, dim3(G * H), dim3(256), 0, st, (const float*)nullptr, 0, (int64_t)0, (int)H, (int)Hp, dW_ih, ld_dwi);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(rnn_dw_fold_kernel, dim3(G * H), dim3(256), 0, st, (const float*)nullptr, 0, (int64_t)0, (int)H, (int)Hp, dW_hh, ld_dwh);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(rnn_db_kernel, dim3((unsigned)(G * Hp / 4)), dim3(256), 0, st, (const float*)nullptr, (int64_t)0, (int)H, (int)Hp, G, db_ih, db_hh);
        DAE_CHECK_LAUNCH();
        return 0;
    }
    char* w = (char*)workspace;
    auto carve = [&](uint64_t bytes) { char* q = w; w += al256(bytes); return q; };
    float* Ei = (float*)carve(Nap * Hp * 4);
    float* Wi = (float*)carve(G * Hp * Hp * 4);
    float* Wh = (float*)carve(G * Hp * Hp * 4);
    float* WhT = (float*)carve(G * Hp * Hp * 4);
    float* P = (float*)carve(Nap * G * Hp * 4);
    float* HP = (float*)carve(Rb * Hp * 4);
    float* HG = (float*)carve(Rb * Hp * 4);
    float* SG[4] = {nullptr, nullptr, nullptr, nullptr};        // LSTM: SI, SF, SG, SO (torch's order); RNN: SH
    for (int b = 0; b < G; ++b) SG[b] = (float*)carve(Rb * Hp * 4);
    float* SC = G == 4 ? (float*)carve(Rb * Hp * 4) : nullptr;
    float* DT = (float*)carve(G * Rb * Hp * 4);
    float* HPT = (float*)carve(Rb * Hp * 4);
    float* XT = (float*)carve(Rb * Hp * 4);
    float* carry = G == 4 ? (float*)carve(Mp * Hp * 4) : nullptr;
    int64_t* row_event = (int64_t*)carve(Rb * 8);
    double* rowloss = (double*)carve(Rb * 8);
    int32_t* rowpairs = (int32_t*)carve(Rb * 4);
    float* slabs = (float*)carve((uint64_t)GF_MAX_SPLITS * G * Hp * Hp * 4);
    // ---- 1. operand images and the input projection of every article (as dae_lstm_user_states / dae_rnn_user_states) ----
    if (int rc = launch_row_normalize(E, lde, Na, H, 0, 0, Ei, Hp, (int)Hp, (int)Nap, st)) return rc;
    for (int g = 0; g < G; ++g) {
        if (int rc = launch_row_normalize(W_ih + (int64_t)g * H * ldwi, ldwi, H, H, 0, 0, Wi + (int64_t)g * Hp * Hp, Hp, (int)Hp, (int)Hp, st)) return rc;
        if (int rc = launch_row_normalize(W_hh + (int64_t)g * H * ldwh, ldwh, H, H, 0, 0, Wh + (int64_t)g * Hp * Hp, Hp, (int)Hp, (int)Hp, st)) return rc;
    }
    DAE_LAUNCH(rnn_wht_kernel, dim3((unsigned)Hp), dim3(256), 0, st, W_hh, ldwh, (int)H, (int)Hp, G, WhT);
    DAE_CHECK_LAUNCH();
    if (int rc = launch_gemm_f32out(DAE_F32, (int)Nap, (int)(G * Hp), Ei, Hp, Wi, Hp, (int)Hp, nullptr, 0, nullptr, 0, 0, P, G * Hp, 1, 0, st,
                                    GEMM_ROLE_GENERIC))
        return rc;
    DAE_LAUNCH(rnn_bias_kernel, dim3((unsigned)Na), dim3(256), 0, st, P, (int)H, (int)Hp, G, b_ih, b_hh);
    DAE_CHECK_LAUNCH();
    DAE_CHECK_HIP(hipMemsetAsync(HP, 0, (size_t)(base[1] * Hp * 4), st));       // slab 0: h = 0 (and the LSTM's c = 0)
    // ---- 2. forward, one launch per step ----
    {
        using TP = std::conditional_t<G == 4, LstmTrainParams, RnnTrainParams>;
        TP p;
        memset(&p, 0, sizeof(p));
        p.g.seg[0].lda_b = p.g.seg[0].ldb_b = Hp * 4;
        p.g.seg[0].Bt = (const char*)Wh;
        p.g.seg[0].ktiles = p.g.ktiles_total = (int)(Hp * 4 / BKB);
        p.g.nseg = 1; p.g.splits = 1; p.g.out_scale = 1.f;
        p.P = P; p.indptr = indptr; p.items = items; p.order = order;
        p.nnz = nnz; p.Na = Na; p.H = H; p.Hp = (int)Hp; p.all_states = 1;      // the U row of a tile's user = the row's event (row_event)
        for (int s = 0; s < S; ++s) {
            const int64_t o = base[s] * Hp;
            p.g.seg[0].A = (const char*)(HP + o);
            p.hprev = HP + o; p.hnext = HP + (s + 1 < S ? base[s + 1] * Hp : 0);      // the last step has no successor and writes none
            p.hout = HG + o; p.row_event = row_event + base[s];
            p.t = s; p.active = (int)rows_of(s); p.next = (int)rows_of(s + 1);
            const bool skip_k = s == 0;                         // h = 0: every product is an exact zero
            const int64_t grid = (base[s + 1] - base[s]) / BM * (Hp / BN);
            int rc;
            if constexpr (G == 4) {
                p.si = SG[0] + o; p.sf = SG[1] + o; p.sg = SG[2] + o; p.so = SG[3] + o; p.sc = SC + o;
                p.cprev = s == 0 ? HP : SC + base[s - 1] * Hp;
                rc = skip_k ? sweep_launch<lstm_step_kernel<true, LstmTrainParams>>(grid, LSTM_LDS, LSTM_LDS, st, p)
                            : sweep_launch<lstm_step_kernel<false, LstmTrainParams>>(grid, LSTM_LDS, LSTM_LDS, st, p);
            } else {
                p.sh = SG[0] + o;
                rc = skip_k ? sweep_launch<rnn_step_kernel<true, RnnTrainParams>>(grid, RNN_LDS, RNN_LDS, st, p)
                            : sweep_launch<rnn_step_kernel<false, RnnTrainParams>>(grid, RNN_LDS, RNN_LDS, st, p);
            }
            if (rc) return rc;
        }
    }
    // ---- 3. loss, margins and G ----
    {
        GruLossParams p;
        p.E = E; p.lde = lde; p.Na = Na; p.H = H; p.Hp = (int)Hp; p.items = items; p.negatives = negatives; p.n_neg = n_neg; p.nnz = nnz;
        p.hg = HG; p.row_event = row_event; p.R = R; p.rowloss = rowloss; p.rowpairs = rowpairs; p.margin = margin;
        DAE_LAUNCH(gru_loss_kernel, dim3((unsigned)(R / 4)), dim3(256), 0, st, p);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(gru_loss_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)rowloss, (const int32_t*)rowpairs, R, loss, n_pairs);
        DAE_CHECK_LAUNCH();
    }
    // ---- 4. backward, one launch per step ----
    {
        std::conditional_t<G == 4, LstmBackParams, RnnBackParams> p;
        memset(&p, 0, sizeof(p));
        for (int k = 0; k < G; ++k) {
            p.g.seg[k].lda_b = Hp * 4; p.g.seg[k].ldb_b = G * Hp * 4;
            p.g.seg[k].Bt = (const char*)(WhT + (int64_t)k * Hp);
            p.g.seg[k].ktiles = (int)(Hp * 4 / BKB);
        }
        p.g.nseg = G; p.g.ktiles_total = G * (int)(Hp * 4 / BKB); p.g.splits = 1; p.g.out_scale = 1.f;
        p.H = H; p.Hp = (int)Hp;
        for (int s = S - 1; s >= 0; --s) {
            const int64_t o = base[s] * Hp, on = (s + 1 < S ? base[s + 1] : 0) * Hp;
            for (int k = 0; k < G; ++k) p.g.seg[k].A = (const char*)(SG[k] + on);
            p.G = HG + o;
            p.rows = (int)rows_of(s); p.next = (int)rows_of(s + 1);
            const int64_t grid = (base[s + 1] - base[s]) / BM * (Hp / BN);
            int rc;
            if constexpr (G == 4) {
                p.i = SG[0] + o; p.f = SG[1] + o; p.gg = SG[2] + o; p.o = SG[3] + o; p.c = SC + o;
                p.cprev = s == 0 ? HP : SC + base[s - 1] * Hp;
                p.carry = carry;
                rc = sweep_launch<lstm_back_kernel>(grid, GRU_RING, GRU_RING, st, p);
            } else {
                p.h = SG[0] + o;
                rc = sweep_launch<rnn_back_kernel>(grid, GRU_RING, GRU_RING, st, p);
            }
            if (rc) return rc;
        }
    }
    // ---- 5. the weight gradients: K-contiguous images, two split-K GEMMs, fixed-order folds ----
    {
        const dim3 tg((unsigned)(R / 64), (unsigned)(Hp / 64));
        for (int b = 0; b < G; ++b) {
            DAE_LAUNCH(gru_transpose_kernel<false>, tg, dim3(256), 0, st, (const float*)SG[b], Hp, (const int64_t*)nullptr, (const int32_t*)nullptr, 0, 0,
                       DT + (int64_t)b * Hp * R, R);
            DAE_CHECK_LAUNCH();
        }
        DAE_LAUNCH(gru_transpose_kernel<false>, tg, dim3(256), 0, st, (const float*)HP, Hp, (const int64_t*)nullptr, (const int32_t*)nullptr, 0, 0, HPT, R);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(gru_transpose_kernel<true>, tg, dim3(256), 0, st, E, lde, (const int64_t*)row_event, items, (int)Na, (int)H, XT, R);
        DAE_CHECK_LAUNCH();
        const int64_t tiles = (G * Hp / BM) * (Hp / BN), ktiles = R * 4 / BKB;
        const int splits = (int)std::max<int64_t>(1, std::min<int64_t>(GF_MAX_SPLITS, std::min<int64_t>(ktiles / 4, 1024 / tiles)));
        const int64_t slab = G * Hp * Hp;
        if (int rc = launch_gemm_f32out(DAE_F32, (int)(G * Hp), (int)Hp, DT, R, XT, R, (int)R, nullptr, 0, nullptr, 0, 0, slabs, Hp, splits, slab, st,
                                        GEMM_ROLE_GENERIC))
            return rc;
        DAE_LAUNCH(rnn_dw_fold_kernel, dim3(G * H), dim3(256), 0, st, (const float*)slabs, splits, slab, (int)H, (int)Hp, dW_ih, ld_dwi);
        DAE_CHECK_LAUNCH();
        if (int rc = launch_gemm_f32out(DAE_F32, (int)(G * Hp), (int)Hp, DT, R, HPT, R, (int)R, nullptr, 0, nullptr, 0, 0, slabs, Hp, splits, slab, st,
                                        GEMM_ROLE_GENERIC))
            return rc;
        DAE_LAUNCH(rnn_dw_fold_kernel, dim3(G * H), dim3(256), 0, st, (const float*)slabs, splits, slab, (int)H, (int)Hp, dW_hh, ld_dwh);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(rnn_db_kernel, dim3((unsigned)(G * Hp / 4)), dim3(256), 0, st, (const float*)DT, R, (int)H, (int)Hp, G, db_ih, db_hh);
        DAE_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" uint64_t dae_lstm_pair_loss_workspace(int32_t Na, int32_t H, int64_t M, int64_t nnz, int32_t T, int32_t n_neg) {
    if (Na <= 0 || H <= 0 || M < 0 || nnz < 0 || T < 0 || n_neg < 1 || n_neg > GF_MAX_NEG) return 0;
    return rf_workspace(4, pad128(Na), pad128(H), pad128(M), gf_rows_bound(nnz, T));
}

extern "C" uint64_t dae_rnn_pair_loss_workspace(int32_t Na, int32_t H, int64_t M, int64_t nnz, int32_t T, int32_t n_neg) {
    if (Na <= 0 || H <= 0 || M < 0 || nnz < 0 || T < 0 || n_neg < 1 || n_neg > GF_MAX_NEG) return 0;
    return rf_workspace(1, pad128(Na), pad128(H), pad128(M), gf_rows_bound(nnz, T));
}

extern "C" int dae_lstm_pair_loss(const float* E, int64_t lde, int32_t Na, int32_t H, const float* W_ih, int64_t ldwi, const float* W_hh,
                                  int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr, const int32_t* items,
                                  const int32_t* order, int64_t M, int64_t nnz, int32_t T, const int64_t* active_host,
                                  const int32_t* negatives, int32_t n_neg, double* loss, int64_t* n_pairs, float* dW_ih, int64_t ld_dwi,
                                  float* dW_hh, int64_t ld_dwh, float* db_ih, float* db_hh, float* margin, void* workspace,
                                  uint64_t workspace_bytes, void* stream) {
    return rnn_pair_loss<4>("lstm_pair_loss", E, lde, Na, H, W_ih, ldwi, W_hh, ldwh, b_ih, b_hh, indptr, items, order, M, nnz, T, active_host,
                            negatives, n_neg, loss, n_pairs, dW_ih, ld_dwi, dW_hh, ld_dwh, db_ih, db_hh, margin, workspace, workspace_bytes, stream);
}

extern "C" int dae_rnn_pair_loss(const float* E, int64_t lde, int32_t Na, int32_t H, const float* W_ih, int64_t ldwi, const float* W_hh,
                                 int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr, const int32_t* items,
                                 const int32_t* order, int64_t M, int64_t nnz, int32_t T, const int64_t* active_host,
                                 const int32_t* negatives, int32_t n_neg, double* loss, int64_t* n_pairs, float* dW_ih, int64_t ld_dwi,
                                 float* dW_hh, int64_t ld_dwh, float* db_ih, float* db_hh, float* margin, void* workspace,
                                 uint64_t workspace_bytes, void* stream) {
    return rnn_pair_loss<1>("rnn_pair_loss", E, lde, Na, H, W_ih, ldwi, W_hh, ldwh, b_ih, b_hh, indptr, items, order, M, nnz, T, active_host,
                            negatives, n_neg, loss, n_pairs, dW_ih, ld_dwi, dW_hh, ld_dwh, db_ih, db_hh, margin, workspace, workspace_bytes, stream);
}
