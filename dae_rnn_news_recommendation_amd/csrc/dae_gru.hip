// dae_gru.hip -- user states from browsing histories by a GRU (dae_gru_user_states): the recurrent user model of "Embedding-based
// News Recommendation for Millions of Users" (KDD'17), inference only, weights in the layout of torch.nn.GRU.
//
// Per user, events oldest first, x = E[items[e]] (D floats), h (H floats, zero or the caller's row at the start):
//   gi = W_ih x + b_ih     gh = W_hh h + b_hh                      (row blocks r, z, n)
//   r = sigmoid(gi_r + gh_r)   z = sigmoid(gi_z + gh_z)   n = tanh(gi_n + r * gh_n)   h' = (1 - z) * n + z * h
//
// Layout: time-major.  At H = 500 the recurrent weights are 3 MB, so a wave per user (dae_user.hip) would stream them per event;
// instead the users are sorted by history length (`order`, `active_host`: the caller's schedule) and step t is ONE launch over
// the active[t] users that have more than t events -- a 128 x 128-tile exact-fp32 GEMM h W_hh^T with the gate arithmetic in its
// epilogue.  Everything that does not depend on h is computed once per call, per ARTICLE and not per event:
//   P[a][g Hp + j] = W_ih[g H + j] . E[a] + b_ih[g H + j] (+ b_hh[g H + j] for g = r, z)        [pad128(Na) x 3 Hp] fp32
// by the exact-fp32 NT GEMM of dae_gemm.hip on zero-padded images of E and W_ih, then gru_bias_kernel.
//
// gru_step_kernel: grid = ceil(active[t] / 128) x Hp / 128, 256 threads (4 waves), a workgroup owns 128 active users (sorted
// positions) and 128 hidden columns.  It runs the K loop of gemm_mainloop<float, 2> three times, A = the previous state buffer
// [pad128(M) x Hp], Bt = the r, n, z row blocks of the W_hh image [3 Hp x Hp] (every gate block padded to Hp rows, so that a
// gate is a tile-row offset): r is finished first and kept in registers (64 per lane), the n pass overwrites it with n, the z
// pass produces h'.  The epilogue gathers the three P values of the row's item, reads h from the previous buffer, writes h' to
// the other of the two ping-pong state buffers and -- all_states: to U[event]; else at the user's last step: to U[user].
// Rows >= active[t] and columns >= H never reach U; the state buffers keep exact zeros in the columns >= H.
// The 128 (item, U row) pairs of the tile's users sit in 1.5 KiB of LDS behind the staging ring (65.5 KiB).  r / n stay in
// registers because neither home in LDS exists -- the ring is live during the next K loop and a second 64 KiB tile would leave
// one workgroup per CU as well -- and with them the kernel needs 256 VGPRs + 64 AGPRs: __launch_bounds__(256, 1), no scratch (at
// two workgroups per CU it spilled; parking r / n in global memory instead reached two per CU and was not faster: DESIGN 5).
//
// Arithmetic: v_mfma_f32_32x32x2_f32 is an exact fmaf chain over k in ascending order, one chain per output element, and an
// output element depends on its own A row and Bt row alone; expf / tanhf and IEEE division in the gates; no atomics.  So a
// user's states are bit-identical run to run and do not depend on the other users of the call, their order, the tile or the
// launch a row falls into, or on all_states.  Continuing from a stored state (h0) runs the instructions the unsplit history runs.
#include "dae_gru_step.h"       // gru_step_kernel, gru_bias_kernel, gru_sigmoid: shared with the training step (dae_gru_fit.hip)

namespace dae {

// S0[i] = h0[order[i]] or zero, zero in the columns >= H; a user without events gets its row of U (last-state mode)
__global__ __launch_bounds__(256) void gru_init_kernel(float* __restrict__ S0, int Hp, int H, const int32_t* __restrict__ order,
                                                       const int64_t* __restrict__ indptr, const float* __restrict__ h0, int64_t ldh0,
                                                       int all_states, float* __restrict__ U, int64_t ldu) {
    const int64_t i = blockIdx.x;
    const int64_t u = order[i];
    const bool empty = indptr[u + 1] == indptr[u];
    for (int j = threadIdx.x; j < Hp; j += 256) {
        const float v = (h0 && j < H) ? h0[u * ldh0 + j] : 0.f;
        S0[i * Hp + j] = v;
        if (empty && !all_states && j < H) U[u * ldu + j] = v;
    }
}

}  // namespace dae

using namespace dae;

static uint64_t gru_workspace(int64_t Nap, int64_t Dp, int64_t Hp, int64_t Mp) {
    // E image, W_ih image, W_hh image, P, b_hn image, two state buffers
    return al256(Nap * Dp * 4) + al256(3 * Hp * Dp * 4) + al256(3 * Hp * Hp * 4) + al256(Nap * 3 * Hp * 4) + al256(Hp * 4) + 2 * al256(Mp * Hp * 4);
}

extern "C" uint64_t dae_gru_user_states_workspace(int32_t Na, int32_t D, int32_t H, int64_t M) {
    if (Na <= 0 || D <= 0 || H <= 0 || M < 0) return 0;
    return gru_workspace(pad128(Na), pad128(D), pad128(H), pad128(M));
}

extern "C" int dae_gru_user_states(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t H, const float* W_ih, int64_t ldwi,
                                   const float* W_hh, int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr,
                                   const int32_t* items, const int32_t* order, int64_t M, int64_t nnz, int32_t T,
                                   const int64_t* active_host, const float* h0, int64_t ldh0, int32_t all_states, float* U, int64_t ldu,
                                   void* workspace, uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(M >= 0 && nnz >= 0 && T >= 0, "gru_user_states: negative count (M = %lld, nnz = %lld, T = %d)", (long long)M, (long long)nnz, T);
    DAE_CHECK_ARG(Na > 0 && D > 0 && H > 0, "gru_user_states: Na, D and H must be positive (got %d, %d, %d)", Na, D, H);
    DAE_CHECK_ARG(E && indptr, "gru_user_states: E / indptr are NULL");
    DAE_CHECK_ARG(W_ih && W_hh && b_ih && b_hh, "gru_user_states: W_ih / W_hh / b_ih / b_hh are NULL");
    DAE_CHECK_ARG(items || nnz == 0, "gru_user_states: items is NULL");
    DAE_CHECK_ARG(order || M == 0, "gru_user_states: order is NULL");
    DAE_CHECK_ARG(active_host || T == 0, "gru_user_states: active_host is NULL");
    DAE_CHECK_ARG(U || (all_states ? nnz : M) == 0, "gru_user_states: U is NULL");
    DAE_CHECK_ARG(lde >= D && ldwi >= D, "gru_user_states: lde (%lld) and ldwi (%lld) must be >= D (%d)", (long long)lde, (long long)ldwi, D);
    DAE_CHECK_ARG(ldwh >= H && ldu >= H && (!h0 || ldh0 >= H), "gru_user_states: ldwh (%lld), ldu (%lld) and ldh0 (%lld) must be >= H (%d)",
                  (long long)ldwh, (long long)ldu, (long long)ldh0, H);
    int64_t events = 0;
    for (int t = 0; t < T; ++t) {
        DAE_CHECK_ARG(active_host[t] >= 0 && active_host[t] <= (t ? active_host[t - 1] : M),
                      "gru_user_states: active_host must be non-increasing and at most M (active_host[%d] = %lld)", t, (long long)active_host[t]);
        events += active_host[t];
    }
    DAE_CHECK_ARG(events <= nnz, "gru_user_states: the schedule's T = %d steps hold %lld events, more than nnz = %lld", T, (long long)events,
                  (long long)nnz);
    const int64_t Nap = pad128(Na), Dp = pad128(D), Hp = pad128(H), Mp = pad128(M);
    DAE_CHECK_ARG(Nap * Dp * 4 < (1ll << 32) && 3 * Hp * Dp * 4 < (1ll << 32) && 3 * Hp * Hp * 4 < (1ll << 32) && Mp * Hp * 4 < (1ll << 32),
                  "gru_user_states: an operand image exceeds 4 GiB (split the users into smaller calls)");
    if (M == 0) return 0;
    const uint64_t need = gru_workspace(Nap, Dp, Hp, Mp);
    DAE_CHECK_ARG(workspace && workspace_bytes >= need, "gru_user_states: workspace too small (%llu < %llu bytes)",
                  (unsigned long long)(workspace ? workspace_bytes : 0), (unsigned long long)need);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "gru_user_states: workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    float* Ei = (float*)w;   w += al256(Nap * Dp * 4);
    float* Wi = (float*)w;   w += al256(3 * Hp * Dp * 4);
    float* Wh = (float*)w;   w += al256(3 * Hp * Hp * 4);
    float* P = (float*)w;    w += al256(Nap * 3 * Hp * 4);
    float* bhn = (float*)w;  w += al256(Hp * 4);
    float* S[2];
    S[0] = (float*)w;        w += al256(Mp * Hp * 4);
    S[1] = (float*)w;
    // ---- 1. operand images ----
    if (int rc = launch_row_normalize(E, lde, Na, D, 0, 0, Ei, Dp, (int)Dp, (int)Nap, st)) return rc;
    for (int g = 0; g < 3; ++g) {
        if (int rc = launch_row_normalize(W_ih + (int64_t)g * H * ldwi, ldwi, H, D, 0, 0, Wi + (int64_t)g * Hp * Dp, Dp, (int)Dp, (int)Hp, st)) return rc;
        if (int rc = launch_row_normalize(W_hh + (int64_t)g * H * ldwh, ldwh, H, H, 0, 0, Wh + (int64_t)g * Hp * Hp, Hp, (int)Hp, (int)Hp, st)) return rc;
    }
    // ---- 2. the input projection of every article ----
    if (int rc = launch_gemm_f32out(DAE_F32, (int)Nap, (int)(3 * Hp), Ei, Dp, Wi, Dp, (int)Dp, nullptr, 0, nullptr, 0, 0, P, 3 * Hp, 1, 0, st,
                                    GEMM_ROLE_GENERIC))
        return rc;
    DAE_LAUNCH(gru_bias_kernel, dim3((unsigned)Na + 1), dim3(256), 0, st, P, (int)Na, (int)H, (int)Hp, b_ih, b_hh, bhn);
    DAE_CHECK_LAUNCH();
    DAE_CHECK_ARG(M < (1ll << 31), "gru_user_states: M = %lld exceeds the grid", (long long)M);
    DAE_LAUNCH(gru_init_kernel, dim3((unsigned)M), dim3(256), 0, st, S[0], (int)Hp, (int)H, order, indptr, h0, ldh0, all_states ? 1 : 0, U, ldu);
    DAE_CHECK_LAUNCH();
    // ---- 3. one launch per step ----
    GruStepParams p;
    memset(&p, 0, sizeof(p));
    p.g.seg[0].lda_b = p.g.seg[0].ldb_b = Hp * 4;
    p.g.seg[0].Bt = (const char*)Wh;
    p.g.seg[0].ktiles = p.g.ktiles_total = (int)(Hp * 4 / BKB);
    p.g.nseg = 1; p.g.splits = 1; p.g.out_scale = 1.f;
    p.P = P; p.bhn = bhn; p.indptr = indptr; p.items = items; p.order = order; p.U = U; p.ldu = ldu;
    p.nnz = nnz; p.Na = Na; p.H = H; p.Hp = (int)Hp; p.all_states = all_states ? 1 : 0;
    for (int t = 0; t < T && active_host[t] > 0; ++t) {
        p.g.seg[0].A = (const char*)S[t & 1];
        p.hprev = S[t & 1]; p.hnext = S[(t & 1) ^ 1];
        p.t = t; p.active = (int)active_host[t];
        p.skip_k = (t == 0 && !h0) ? 1 : 0;                     // h = 0: every product is an exact zero
        const int64_t grid = (active_host[t] + BM - 1) / BM * (Hp / BN);
        if (int rc = p.skip_k ? sweep_launch<gru_step_kernel<true>>(grid, GRU_LDS, GRU_LDS, st, p)
                              : sweep_launch<gru_step_kernel<false>>(grid, GRU_LDS, GRU_LDS, st, p))
            return rc;
    }
    return 0;
}
