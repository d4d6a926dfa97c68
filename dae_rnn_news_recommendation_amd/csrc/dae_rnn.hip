// dae_rnn.hip -- user states from browsing histories by an LSTM (dae_lstm_user_states) and by a plain tanh RNN (dae_rnn_user_states):
// the other two recurrent user models of "Embedding-based News Recommendation for Millions of Users" (KDD'17), inference (their training: dae_rnn_fit.hip), weights
// in the layout of torch.nn.LSTM and torch.nn.RNN(nonlinearity='tanh').  The GRU is dae_gru.hip; this file follows its form.
//
// Per user, events oldest first, x = E[items[e]] (D floats), h and c (H floats, zero or the caller's rows at the start):
//   LSTM (row blocks i, f, g, o):  i, f, o = sigmoid(W_i. x + b_i. + W_h. h + b_h.)   g = tanh(W_ig x + b_ig + W_hg h + b_hg)
//                                  c' = f * c + i * g      h' = o * tanh(c')
//   RNN  (one row block):          h' = tanh(W_ih x + b_ih + W_hh h + b_hh)
//
// Layout: time-major, as the GRU (head of dae_gru.hip): the users sorted by history length, step t ONE launch over the active[t]
// users with more than t events, grid = ceil(active[t] / 128) x Hp / 128, 256 threads, a workgroup owns 128 users (sorted positions)
// and 128 hidden columns; h ping-pongs between two [pad128(M) x Hp] buffers whose columns >= H stay exact zeros.  Everything that does
// not depend on h is computed once per call and per ARTICLE:
//   P[a][g Hp + j] = W_ih[g H + j] . E[a] + b_ih[g H + j] + b_hh[g H + j]        [pad128(Na) x G Hp] fp32, G = 4 (LSTM) or 1 (RNN)
// by the exact-fp32 NT GEMM of dae_gemm.hip on zero-padded images of E and W_ih (every gate block padded to Hp rows), then
// rnn_bias_kernel.  No bias is multiplied by a gate here, so there is no separate image of a recurrent bias.
//
// lstm_step_kernel (dae_rnn_step.h, shared with the trainer) runs the K loop of gemm_mainloop<float, 2> four times, A = the previous state buffer, Bt = the i, g, f, o row
// blocks of the W_hh image [4 Hp x Hp], in that order, with one f32x16[2][2] carry (64 registers per lane) beside the accumulators:
// the i pass leaves sigmoid(.) in the carry, the g pass multiplies tanh(.) into it, the f pass reads the row's c, forms
// c' = f * c + carry, writes c' back and keeps it in the carry, the o pass writes h' = o * tanh(c') to the next state buffer and to U
// (all_states: row = event; else at the user's last step: row = user).  ONE cell buffer [pad128(M) x Hp], updated in place: the
// element of c that a lane reads in the f pass is the element that lane writes, no other lane or workgroup touches it during the
// launch, and the launches of a stream run in order.  C (the cell state after every user's last event) is written by the f pass of
// the user's last step.  The live set is the GRU's (64 accumulator + 64 carry registers): __launch_bounds__(256, 1), no scratch.
// rnn_step_kernel is one K loop with the epilogue tanh(P + acc) and no carry: __launch_bounds__(256, 2).
// The 128 (item, U row) pairs of the tile's users sit in 1.5 KiB of LDS behind the staging ring; the LSTM step adds the 128 C rows (1 KiB).
//
// First step without stored h (t == 0, h0 == NULL): the accumulators are zeroed instead of running the K loop (every product
// would be an exact zero) and the same epilogue runs, with c read from the buffer the init kernel wrote (c0 or zeros): by
// construction the bits of a call with zero h0.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 is an exact fmaf chain over k in ascending order, one chain per output element, which
// depends on its own A row and Bt row alone; expf (gru_sigmoid) / tanhf and IEEE division in the gates; no atomics.  So a user's
// states are bit-identical run to run and do not depend on the other users of the call, their order, the tile or the launch a row
// falls into, on all_states or on the caller's chunking; continuing from stored (h, c) runs the instructions the unsplit history runs.
#include "dae_rnn_step.h"       // RnnStepParams, lstm_step_kernel, rnn_step_kernel; gru_sigmoid, gemm_mainloop, sweep_launch, al256

namespace dae {

// S0[i] = h0[order[i]] or zero and (LSTM) C0[i] = c0[order[i]] or zero, zero in the columns >= H; a user without events gets its
// row of U (last-state mode) and of C
__global__ __launch_bounds__(256) void rnn_init_kernel(float* __restrict__ S0, float* __restrict__ C0, int Hp, int H,
                                                       const int32_t* __restrict__ order, const int64_t* __restrict__ indptr,
                                                       const float* __restrict__ h0, int64_t ldh0, const float* __restrict__ c0, int64_t ldc0,
                                                       int all_states, float* __restrict__ U, int64_t ldu, float* __restrict__ C, int64_t ldc) {
    const int64_t i = blockIdx.x;
    const int64_t u = order[i];
    const bool empty = indptr[u + 1] == indptr[u];
    for (int j = threadIdx.x; j < Hp; j += 256) {
        const float v = (h0 && j < H) ? h0[u * ldh0 + j] : 0.f;
        S0[i * Hp + j] = v;
        if (empty && !all_states && j < H) U[u * ldu + j] = v;
        if (C0) {
            const float w = (c0 && j < H) ? c0[u * ldc0 + j] : 0.f;
            C0[i * Hp + j] = w;
            if (empty && C && j < H) C[u * ldc + j] = w;
        }
    }
}

}  // namespace dae

using namespace dae;

// G gate blocks: E image, W_ih image, W_hh image, P, two state buffers and, for the LSTM (G == 4), the cell buffer
static uint64_t rnn_workspace(int64_t G, int64_t Nap, int64_t Dp, int64_t Hp, int64_t Mp) {
    return al256(Nap * Dp * 4) + al256(G * Hp * Dp * 4) + al256(G * Hp * Hp * 4) + al256(Nap * G * Hp * 4) + (G == 4 ? 3 : 2) * al256(Mp * Hp * 4);
}

// the body of both exports: G = 4 with c0 / C (LSTM), G = 1 without (RNN).  `fn` prefixes every message.
template <int G>
static int rnn_user_states(const char* fn, const float* E, int64_t lde, int32_t Na, int32_t D, int32_t H, const float* W_ih, int64_t ldwi,
                           const float* W_hh, int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr, const int32_t* items,
                           const int32_t* order, int64_t M, int64_t nnz, int32_t T, const int64_t* active_host, const float* h0, int64_t ldh0,
                           const float* c0, int64_t ldc0, int32_t all_states, float* U, int64_t ldu, float* C, int64_t ldc, void* workspace,
                           uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(M >= 0 && nnz >= 0 && T >= 0, "%s: negative count (M = %lld, nnz = %lld, T = %d)", fn, (long long)M, (long long)nnz, T);
    DAE_CHECK_ARG(Na > 0 && D > 0 && H > 0, "%s: Na, D and H must be positive (got %d, %d, %d)", fn, Na, D, H);
    DAE_CHECK_ARG(E && indptr, "%s: E / indptr are NULL", fn);
    DAE_CHECK_ARG(W_ih && W_hh && b_ih && b_hh, "%s: W_ih / W_hh / b_ih / b_hh are NULL", fn);
    DAE_CHECK_ARG(items || nnz == 0, "%s: items is NULL", fn);
    DAE_CHECK_ARG(order || M == 0, "%s: order is NULL", fn);
    DAE_CHECK_ARG(active_host || T == 0, "%s: active_host is NULL", fn);
    DAE_CHECK_ARG(U || (all_states ? nnz : M) == 0, "%s: U is NULL", fn);
    DAE_CHECK_ARG(lde >= D && ldwi >= D, "%s: lde (%lld) and ldwi (%lld) must be >= D (%d)", fn, (long long)lde, (long long)ldwi, D);
    DAE_CHECK_ARG(ldwh >= H && ldu >= H && (!h0 || ldh0 >= H), "%s: ldwh (%lld), ldu (%lld) and ldh0 (%lld) must be >= H (%d)", fn,
                  (long long)ldwh, (long long)ldu, (long long)ldh0, H);
    DAE_CHECK_ARG((!c0 || ldc0 >= H) && (!C || ldc >= H), "%s: ldc0 (%lld) and ldc (%lld) must be >= H (%d)", fn, (long long)ldc0,
                  (long long)ldc, H);
    int64_t events = 0;
    for (int t = 0; t < T; ++t) {
        DAE_CHECK_ARG(active_host[t] >= 0 && active_host[t] <= (t ? active_host[t - 1] : M),
                      "%s: active_host must be non-increasing and at most M (active_host[%d] = %lld)", fn, t, (long long)active_host[t]);
        events += active_host[t];
    }
    DAE_CHECK_ARG(events <= nnz, "%s: the schedule's T = %d steps hold %lld events, more than nnz = %lld", fn, T, (long long)events,
                  (long long)nnz);
    const int64_t Nap = pad128(Na), Dp = pad128(D), Hp = pad128(H), Mp = pad128(M);
    DAE_CHECK_ARG(Nap * Dp * 4 < (1ll << 32) && G * Hp * Dp * 4 < (1ll << 32) && G * Hp * Hp * 4 < (1ll << 32) && Nap * G * Hp * 4 < (1ll << 32) &&
                      Mp * Hp * 4 < (1ll << 32),
                  "%s: an operand image exceeds 4 GiB (split the users into smaller calls)", fn);
    if (M == 0) return 0;
    const uint64_t need = rnn_workspace(G, Nap, Dp, Hp, Mp);
    DAE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%llu < %llu bytes)", fn,
                  (unsigned long long)(workspace ? workspace_bytes : 0), (unsigned long long)need);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "%s: workspace must be 256-byte aligned", fn);
    DAE_CHECK_ARG(M < (1ll << 31), "%s: M = %lld exceeds the grid", fn, (long long)M);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    float* Ei = (float*)w;   w += al256(Nap * Dp * 4);
    float* Wi = (float*)w;   w += al256(G * Hp * Dp * 4);
    float* Wh = (float*)w;   w += al256(G * Hp * Hp * 4);
    float* P = (float*)w;    w += al256(Nap * G * Hp * 4);
    float* S[2];
    S[0] = (float*)w;        w += al256(Mp * Hp * 4);
    S[1] = (float*)w;        w += al256(Mp * Hp * 4);
    float* cell = G == 4 ? (float*)w : nullptr;
    // ---- 1. operand images ----
    if (int rc = launch_row_normalize(E, lde, Na, D, 0, 0, Ei, Dp, (int)Dp, (int)Nap, st)) return rc;
    for (int g = 0; g < G; ++g) {
        if (int rc = launch_row_normalize(W_ih + (int64_t)g * H * ldwi, ldwi, H, D, 0, 0, Wi + (int64_t)g * Hp * Dp, Dp, (int)Dp, (int)Hp, st)) return rc;
        if (int rc = launch_row_normalize(W_hh + (int64_t)g * H * ldwh, ldwh, H, H, 0, 0, Wh + (int64_t)g * Hp * Hp, Hp, (int)Hp, (int)Hp, st)) return rc;
    }
    // ---- 2. the input projection of every article ----
    if (int rc = launch_gemm_f32out(DAE_F32, (int)Nap, (int)(G * Hp), Ei, Dp, Wi, Dp, (int)Dp, nullptr, 0, nullptr, 0, 0, P, G * Hp, 1, 0, st,
                                    GEMM_ROLE_GENERIC))
        return rc;
    DAE_LAUNCH(rnn_bias_kernel, dim3((unsigned)Na), dim3(256), 0, st, P, (int)H, (int)Hp, (int)G, b_ih, b_hh);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(rnn_init_kernel, dim3((unsigned)M), dim3(256), 0, st, S[0], cell, (int)Hp, (int)H, order, indptr, h0, ldh0, c0, ldc0,
               all_states ? 1 : 0, U, ldu, C, ldc);
    DAE_CHECK_LAUNCH();
    // ---- 3. one launch per step ----
    RnnStepParams p;
    memset(&p, 0, sizeof(p));
    p.g.seg[0].lda_b = p.g.seg[0].ldb_b = Hp * 4;
    p.g.seg[0].Bt = (const char*)Wh;
    p.g.seg[0].ktiles = p.g.ktiles_total = (int)(Hp * 4 / BKB);
    p.g.nseg = 1; p.g.splits = 1; p.g.out_scale = 1.f;
    p.P = P; p.cell = cell; p.indptr = indptr; p.items = items; p.order = order; p.U = U; p.ldu = ldu; p.C = C; p.ldc = ldc;
    p.nnz = nnz; p.Na = Na; p.H = H; p.Hp = (int)Hp; p.all_states = all_states ? 1 : 0;
    for (int t = 0; t < T && active_host[t] > 0; ++t) {
        p.g.seg[0].A = (const char*)S[t & 1];
        p.hprev = S[t & 1]; p.hnext = S[(t & 1) ^ 1];
        p.t = t; p.active = (int)active_host[t];
        const bool skip_k = t == 0 && !h0;                      // h = 0: every product is an exact zero
        const int64_t grid = (active_host[t] + BM - 1) / BM * (Hp / BN);
        int rc;
        if constexpr (G == 4)
            rc = skip_k ? sweep_launch<lstm_step_kernel<true>>(grid, LSTM_LDS, LSTM_LDS, st, p)
                        : sweep_launch<lstm_step_kernel<false>>(grid, LSTM_LDS, LSTM_LDS, st, p);
        else
            rc = skip_k ? sweep_launch<rnn_step_kernel<true>>(grid, RNN_LDS, RNN_LDS, st, p)
                        : sweep_launch<rnn_step_kernel<false>>(grid, RNN_LDS, RNN_LDS, st, p);
        if (rc) return rc;
    }
    return 0;
}

extern "C" uint64_t dae_lstm_user_states_workspace(int32_t Na, int32_t D, int32_t H, int64_t M) {
    if (Na <= 0 || D <= 0 || H <= 0 || M < 0) return 0;
    return rnn_workspace(4, pad128(Na), pad128(D), pad128(H), pad128(M));
}

extern "C" uint64_t dae_rnn_user_states_workspace(int32_t Na, int32_t D, int32_t H, int64_t M) {
    if (Na <= 0 || D <= 0 || H <= 0 || M < 0) return 0;
    return rnn_workspace(1, pad128(Na), pad128(D), pad128(H), pad128(M));
}

extern "C" int dae_lstm_user_states(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t H, const float* W_ih, int64_t ldwi,
                                    const float* W_hh, int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr,
                                    const int32_t* items, const int32_t* order, int64_t M, int64_t nnz, int32_t T,
                                    const int64_t* active_host, const float* h0, int64_t ldh0, const float* c0, int64_t ldc0,
                                    int32_t all_states, float* U, int64_t ldu, float* C, int64_t ldc, void* workspace,
                                    uint64_t workspace_bytes, void* stream) {
    return rnn_user_states<4>("lstm_user_states", E, lde, Na, D, H, W_ih, ldwi, W_hh, ldwh, b_ih, b_hh, indptr, items, order, M, nnz, T,
                              active_host, h0, ldh0, c0, ldc0, all_states, U, ldu, C, ldc, workspace, workspace_bytes, stream);
}

extern "C" int dae_rnn_user_states(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t H, const float* W_ih, int64_t ldwi,
                                   const float* W_hh, int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr,
                                   const int32_t* items, const int32_t* order, int64_t M, int64_t nnz, int32_t T,
                                   const int64_t* active_host, const float* h0, int64_t ldh0, int32_t all_states, float* U, int64_t ldu,
                                   void* workspace, uint64_t workspace_bytes, void* stream) {
    return rnn_user_states<1>("rnn_user_states", E, lde, Na, D, H, W_ih, ldwi, W_hh, ldwh, b_ih, b_hh, indptr, items, order, M, nnz, T,
                              active_host, h0, ldh0, nullptr, 0, all_states, U, ldu, nullptr, 0, workspace, workspace_bytes, stream);
}
