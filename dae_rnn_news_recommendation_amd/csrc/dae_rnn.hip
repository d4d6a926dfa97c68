// dae_rnn.hip -- user states from browsing histories by an LSTM (dae_lstm_user_states) and by a plain tanh RNN (dae_rnn_user_states):
// the other two recurrent user models of "Embedding-based News Recommendation for Millions of Users" (KDD'17), inference only, weights
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
// lstm_step_kernel runs the K loop of gemm_mainloop<float, 2> four times, A = the previous state buffer, Bt = the i, g, f, o row
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
#include "dae_gru_step.h"       // gru_sigmoid and, through dae_score_sweep.h, gemm_mainloop, sweep_launch, al256

namespace dae {

constexpr int RNN_LDS = GRU_RING + 128 * 4 + 128 * 8;                // ring, items, U rows
constexpr int LSTM_LDS = RNN_LDS + 128 * 8;                         // and C rows

// P += b_ih + b_hh (rows < Na, columns < H of each of the G gate blocks)
__global__ __launch_bounds__(256) void rnn_bias_kernel(float* __restrict__ P, int H, int Hp, int G, const float* __restrict__ b_ih,
                                                       const float* __restrict__ b_hh) {
    float* p = P + (int64_t)blockIdx.x * G * Hp;
    for (int q = threadIdx.x; q < G * Hp; q += 256) {
        const int g = q / Hp, j = q - g * Hp;
        if (j < H) p[q] += b_ih[g * H + j] + b_hh[g * H + j];
    }
}

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

struct RnnStepParams {
    GemmParams g;                 // one K segment: A = previous state buffer, Bt = W_hh image (gate q = tile rows q * Hp / 128 ...)
    const float* hprev;           // = g.seg[0].A
    float* hnext;                 // [pad128(M) x Hp]
    float* cell;                  // LSTM: [pad128(M) x Hp], updated in place
    const float* P;               // [pad128(Na) x G Hp]
    const int64_t* indptr; const int32_t* items; const int32_t* order;
    float* U; int64_t ldu;
    float* C; int64_t ldc;        // LSTM: [M x ldc] or NULL
    int64_t nnz;
    int Na, H, Hp, t, active, all_states;
};

// the tile's users: the item of this step, the row of U to write and (CELL: the LSTM) the row of C to write (-1: none)
template <bool CELL>
__device__ __forceinline__ void rnn_tile_rows(const RnnStepParams& p, int tm, int tid, int* s_item, long long* s_urow, long long* s_crow) {
    if (tid < 128) {
        const int i = tm * BM + tid;
        int it = 0;
        long long urow = -1;
        [[maybe_unused]] long long crow = -1;
        if (i < p.active) {
            const int64_t u = p.order[i];
            const int64_t e0 = p.indptr[u], e1 = p.indptr[u + 1];
            // e0 + t by the schedule's contract; a caller error (see dae_hip.h) must not become a stray read
            const int64_t e = max(min(min(e0 + p.t, e1 - 1), p.nnz - 1), (int64_t)0);
            it = min(max(p.items[e], 0), p.Na - 1);
            urow = p.all_states ? e : (e == e1 - 1 ? u : -1);
            if constexpr (CELL) crow = (p.C && e == e1 - 1) ? u : -1;
        }
        s_item[tid] = it;
        s_urow[tid] = urow;
        if constexpr (CELL) s_crow[tid] = crow;
    }
    __syncthreads();
}

template <bool SKIP_K>
__global__ __launch_bounds__(GEMM_THREADS, 1) void lstm_step_kernel(RnnStepParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int* s_item = reinterpret_cast<int*>(lds + GRU_RING);
    long long* s_urow = reinterpret_cast<long long*>(lds + GRU_RING + 128 * 4);
    long long* s_crow = reinterpret_cast<long long*>(lds + GRU_RING + 128 * 4 + 128 * 8);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int tiles_n = p.Hp / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
    rnn_tile_rows<true>(p, tm, tid, s_item, s_urow, s_crow);
    const int Hp = p.Hp;
    const int col0 = tn * BN + wn * 64 + c;                     // this lane's columns: col0, col0 + 32
    const int rbase = wm * 64 + 4 * g;                          // its rows: rbase + acc_row(mt, r, 0)
    f32x16 acc[2][2], keep[2][2];                               // keep: i, then i * g, then c'
    // ---- i = sigmoid(P_i + acc) ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* pr = p.P + (int64_t)s_item[rbase + acc_row(mt, r, 0)] * (4 * Hp) + col0;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) keep[mt][nt][r] = gru_sigmoid(pr[nt * 32] + acc[mt][nt][r]);
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four rows' P values in flight, not all 32 (VGPRs)
        }
    __syncthreads();                                            // every wave is done with the staging ring
    // ---- g = tanh(P_g + acc), carry = i * g ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, 2 * tiles_n + tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* pr = p.P + (int64_t)s_item[rbase + acc_row(mt, r, 0)] * (4 * Hp) + 2 * Hp + col0;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) keep[mt][nt][r] = keep[mt][nt][r] * tanhf(pr[nt * 32] + acc[mt][nt][r]);
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    __syncthreads();
    // ---- f = sigmoid(P_f + acc), c' = f * c + carry ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, tiles_n + tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = rbase + acc_row(mt, r, 0);
            const int i = tm * BM + lrow;
            if (i < p.active) {
                const float* pr = p.P + (int64_t)s_item[lrow] * (4 * Hp) + Hp + col0;
                float* cp = p.cell + (int64_t)i * Hp + col0;
                const long long crow = s_crow[lrow];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float f = gru_sigmoid(pr[nt * 32] + acc[mt][nt][r]);
                    const bool in = col0 + nt * 32 < p.H;
                    const float v = in ? f * cp[nt * 32] + keep[mt][nt][r] : 0.f;
                    cp[nt * 32] = v;
                    keep[mt][nt][r] = v;
                    if (crow >= 0 && in) p.C[crow * p.ldc + col0 + nt * 32] = v;
                }
            }
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    __syncthreads();
    // ---- o = sigmoid(P_o + acc), h' = o * tanh(c') ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, 3 * tiles_n + tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = rbase + acc_row(mt, r, 0);
            const int i = tm * BM + lrow;
            if (i < p.active) {
                const float* pr = p.P + (int64_t)s_item[lrow] * (4 * Hp) + 3 * Hp + col0;
                float* hn = p.hnext + (int64_t)i * Hp + col0;
                const long long urow = s_urow[lrow];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float o = gru_sigmoid(pr[nt * 32] + acc[mt][nt][r]);
                    const bool in = col0 + nt * 32 < p.H;
                    const float v = in ? o * tanhf(keep[mt][nt][r]) : 0.f;
                    hn[nt * 32] = v;
                    if (urow >= 0 && in) p.U[urow * p.ldu + col0 + nt * 32] = v;
                }
            }
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
}

template <bool SKIP_K>
__global__ __launch_bounds__(GEMM_THREADS, 2) void rnn_step_kernel(RnnStepParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int* s_item = reinterpret_cast<int*>(lds + GRU_RING);
    long long* s_urow = reinterpret_cast<long long*>(lds + GRU_RING + 128 * 4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int tiles_n = p.Hp / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
    rnn_tile_rows<false>(p, tm, tid, s_item, s_urow, nullptr);
    const int Hp = p.Hp;
    const int col0 = tn * BN + wn * 64 + c;
    const int rbase = wm * 64 + 4 * g;
    f32x16 acc[2][2];
    // ---- h' = tanh(P + acc) ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = rbase + acc_row(mt, r, 0);
            const int i = tm * BM + lrow;
            if (i < p.active) {
                const float* pr = p.P + (int64_t)s_item[lrow] * Hp + col0;
                float* hn = p.hnext + (int64_t)i * Hp + col0;
                const long long urow = s_urow[lrow];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const bool in = col0 + nt * 32 < p.H;
                    const float v = in ? tanhf(pr[nt * 32] + acc[mt][nt][r]) : 0.f;
                    hn[nt * 32] = v;
                    if (urow >= 0 && in) p.U[urow * p.ldu + col0 + nt * 32] = v;
                }
            }
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
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
