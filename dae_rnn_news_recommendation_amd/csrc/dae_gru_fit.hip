// dae_gru_fit.hip -- the training step of the GRU user model (dae_gru_pair_loss): one mini-batch of click histories forward and
// backward through time, the pairwise ranking loss of dae_user_pair_loss on the states of dae_gru_user_states, and the gradients
// of the four weight arrays.  E is fixed and gets no gradient.  Definition: include/dae_hip.h.
//
// Steps.  The state after a user's last event predicts nothing, so training runs the histories without their last event: step s
// (s = 0 .. S - 1) reads event s of the n_s = active[s + 1] users that have an event s + 1 to predict.  The schedule is sorted by
// history length, so these are the sorted positions 0 .. n_s - 1.
//
// Stash.  Everything a step leaves behind is time-major: row (s, i) lives at base[s] + i, base[s] = sum of pad128(n_s') over the
// steps before s.  A step's slab is one contiguous [pad128(n_s) x Hp] matrix, the padding rows and the columns >= H are exact
// zeros, and so every image is a GEMM operand as it stands -- row-major it is the A panel of a backward step, transposed it is
// the K extent (all steps at once) of a weight-gradient contraction.  Row-major images [R x Hp], R = base[S]:
//     HP   the input state of every step: slab 0 zeros, slab s + 1 rows < n_(s+1) = the outputs of step s
//     HG   the output state of every step; gru_loss_kernel replaces each row by G, the loss gradient with respect to it
//     SR SZ SN SQ   r, z, n and q = W_hn h + b_hn; the backward step replaces them IN PLACE by da_r, da_z, da_n, dq (the lane that
//                   reads an element is the one that writes it)
// and transposed, K-contiguous images made once after the last backward step: DT [4 Hp x R] = [da_n; da_r; da_z; dq] (rows
// 0 .. 3 Hp are dgi in the gate order n, r, z, rows Hp .. 4 Hp are dgh in the order r, z, n), HPT [Hp x R] and XT [Hp x R], the
// gathered embedding of every row's event.  12 arrays of R x Hp floats; R <= nnz + 127 (T - 1).
//
// Forward: gru_step_kernel<SKIP_K, GruTrainParams> (dae_gru_step.h) -- the inference kernel's three K loops and gate arithmetic;
// the epilogues store r, then q and n, then z and h' as each is first complete.
//
// Loss: gru_loss_kernel (in dae_fit_kernels.h, which dae_rnn_fit.hip shares, as are the fold and the transpose), one wave per
// stash row.  Lane l owns the columns l, l + 64, ...; a margin is the lanes' fmaf chains in column order added by the DPP tree of dae_common.h.  The row's partial loss (fp64) and pair count go to per-row slots that
// gru_loss_fold_kernel adds in a fixed order; no atomics.
//
// Backward: gru_back_kernel, one launch per step from S - 1 down to 0, grid pad128(n_s) / 128 x Hp / 128.  One K loop of length 3 Hp
// over three segments -- A = slab s + 1 of da_r, da_z, dq, Bt = the gate blocks of the image of W_hh^T [Hp x 3 Hp] -- gives the
// carry through the recurrent weights; rows >= n_(s+1) of it are masked and tiles wholly beyond skip the loop.  The epilogue adds G
// and the direct carry dh z of the step after (a [pad128(M) x Hp] buffer, every element owned by one lane of one tile).
// One accumulator set, nothing kept across passes: two workgroups per CU.
//
// Weight gradients: dW_ih = dgi^T X and dW_hh = dgh^T HP by the exact-fp32 NT GEMM of dae_gemm.hip on the transposed images,
// split over K into slabs that gru_dw_fold_kernel adds in slab order; db_ih / db_hh are the row sums of DT (fp64, fixed order).
// X is the gathered form (XT): the alternative, a segment sum of dgi per article followed by dP^T E, needs a sort of the rows by
// article or atomics, and the gather costs one more R x Hp image against twelve.
//
// Everything is a fixed-order sum: bit-identical run to run.  The margins and the pair count are per-row quantities of states that
// do not depend on the other users (dae_gru.hip), so they do not depend on the order of the users; the gradients sum over rows in
// stash order and agree under a permutation to rounding only.
#include "dae_fit_kernels.h"    // gru_loss_kernel, gru_loss_fold_kernel, gru_transpose_kernel; dae_gru_step.h

#include <vector>

namespace dae {

// WhT[j][g Hp + k] = W_hh[g H + k][j]: the Bt operand of the backward step, zero outside H x H of every gate block
__global__ __launch_bounds__(256) void gru_wht_kernel(const float* __restrict__ W_hh, int64_t ldwh, int H, int Hp, float* __restrict__ WhT) {
    const int j = blockIdx.x;
    for (int q = threadIdx.x; q < 3 * Hp; q += 256) {
        const int g = q / Hp, k = q - g * Hp;
        WhT[(int64_t)j * 3 * Hp + q] = (j < H && k < H) ? W_hh[((int64_t)g * H + k) * ldwh + j] : 0.f;
    }
}

struct GruBackParams {
    GemmParams g;                 // three K segments: A = slab s + 1 of da_r, da_z, dq; Bt = the gate blocks of the W_hh^T image
    float *r, *z, *n, *q;         // slab s: read, then overwritten with da_r, da_z, da_n, dq
    const float* hprev;           // slab s of HP
    const float* G;               // slab s of HG
    float* carry;                 // [pad128(M) x Hp]: in dh z of step s + 1 (rows < next), out that of step s (rows < rows)
    int H, Hp, rows, next;        // rows = n_s, next = n_(s+1) (0 at the last step)
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void gru_back_kernel(GruBackParams p) {
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
                float da_r = 0.f, da_z = 0.f, da_n = 0.f, dq = 0.f;
                if (i < p.rows && col < p.H) {
                    float dh = p.G[at];
                    if (i < p.next) dh += p.carry[at] + acc[mt][nt][rr];
                    const float r = p.r[at], z = p.z[at], n = p.n[at], q = p.q[at], h = p.hprev[at];
                    const float dn = dh * (1.0f - z), dz = dh * (h - n);
                    da_n = dn * (1.0f - n * n);
                    da_z = dz * z * (1.0f - z);
                    dq = da_n * r;
                    da_r = da_n * q * r * (1.0f - r);
                    p.carry[at] = dh * z;
                }
                p.r[at] = da_r; p.z[at] = da_z; p.n[at] = da_n; p.q[at] = dq;
            }
        }
}

// dW[(g H + k) ld + j] = the sum over the slabs, in slab order, of S[(m_g Hp + k) Hp + j]; block = one row g H + k
__global__ __launch_bounds__(256) void gru_dw_fold_kernel(const float* __restrict__ slabs, int splits, int64_t slab_stride, int H, int Hp, int m0, int m1,
                                                          int m2, float* __restrict__ dW, int64_t ld) {
    const int row = blockIdx.x, g = row / H, k = row - g * H;
    const int m = g == 0 ? m0 : g == 1 ? m1 : m2;
    const float* s = slabs + ((int64_t)m * Hp + k) * Hp;
    for (int j = threadIdx.x; j < H; j += 256) {
        float v = 0.f;
        for (int sl = 0; sl < splits; ++sl) v += s[(int64_t)sl * slab_stride + j];
        dW[(int64_t)row * ld + j] = v;
    }
}

// the bias gradients: row sums of DT [4 Hp x R] (blocks da_n, da_r, da_z, dq), one wave per row, fp64, lane sums in column order
// and then a fixed butterfly
__global__ __launch_bounds__(256) void gru_db_kernel(const float* __restrict__ DT, int64_t R, int H, int Hp, float* __restrict__ db_ih,
                                                     float* __restrict__ db_hh) {
    const int lane = threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (row >= 4 * Hp) return;
    const int b = row / Hp, j = row - b * Hp;
    if (j >= H) return;
    double s = 0.0;
    for (int64_t k = lane; k < R; k += 64) s += (double)DT[(int64_t)row * R + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        const float v = (float)s;
        if (b == 0) db_ih[2 * H + j] = v;
        else if (b == 1) { db_ih[j] = v; db_hh[j] = v; }
        else if (b == 2) { db_ih[H + j] = v; db_hh[H + j] = v; }
        else db_hh[2 * H + j] = v;
    }
}

static uint64_t gf_workspace(int64_t Nap, int64_t Hp, int64_t Mp, int64_t Rb) {
    // E, W_ih, W_hh, W_hh^T images, P, b_hn image; 12 stash images; carry; row_event, rowloss, rowpairs; split-K slabs
    return al256(Nap * Hp * 4) + 3 * al256(3 * Hp * Hp * 4) + al256(Nap * 3 * Hp * 4) + al256(Hp * 4) + 12 * al256(Rb * Hp * 4) +
           al256(Mp * Hp * 4) + 2 * al256(Rb * 8) + al256(Rb * 4) + al256((uint64_t)GF_MAX_SPLITS * 3 * Hp * Hp * 4);
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_gru_pair_loss_workspace(int32_t Na, int32_t H, int64_t M, int64_t nnz, int32_t T, int32_t n_neg) {
    if (Na <= 0 || H <= 0 || M < 0 || nnz < 0 || T < 0 || n_neg < 1 || n_neg > GF_MAX_NEG) return 0;
    return gf_workspace(pad128(Na), pad128(H), pad128(M), gf_rows_bound(nnz, T));
}

extern "C" int dae_gru_pair_loss(const float* E, int64_t lde, int32_t Na, int32_t H, const float* W_ih, int64_t ldwi, const float* W_hh,
                                 int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr, const int32_t* items,
                                 const int32_t* order, int64_t M, int64_t nnz, int32_t T, const int64_t* active_host,
                                 const int32_t* negatives, int32_t n_neg, double* loss, int64_t* n_pairs, float* dW_ih, int64_t ld_dwi,
                                 float* dW_hh, int64_t ld_dwh, float* db_ih, float* db_hh, float* margin, void* workspace,
                                 uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(M >= 0 && nnz >= 0 && T >= 0, "gru_pair_loss: negative count (M = %lld, nnz = %lld, T = %d)", (long long)M, (long long)nnz, T);
    DAE_CHECK_ARG(Na > 0 && H > 0, "gru_pair_loss: Na and H must be positive (got %d, %d)", Na, H);
    DAE_CHECK_ARG(n_neg >= 1 && n_neg <= GF_MAX_NEG, "gru_pair_loss: n_neg must be in 1..%d (got %d)", GF_MAX_NEG, n_neg);
    DAE_CHECK_ARG(E && indptr, "gru_pair_loss: E / indptr are NULL");
    DAE_CHECK_ARG(W_ih && W_hh && b_ih && b_hh, "gru_pair_loss: W_ih / W_hh / b_ih / b_hh are NULL");
    DAE_CHECK_ARG((items && negatives) || nnz == 0, "gru_pair_loss: items / negatives are NULL");
    DAE_CHECK_ARG(order || M == 0, "gru_pair_loss: order is NULL");
    DAE_CHECK_ARG(active_host || T == 0, "gru_pair_loss: active_host is NULL");
    DAE_CHECK_ARG(loss && n_pairs, "gru_pair_loss: loss / n_pairs are NULL");
    DAE_CHECK_ARG(dW_ih && dW_hh && db_ih && db_hh, "gru_pair_loss: dW_ih / dW_hh / db_ih / db_hh are NULL");
    DAE_CHECK_ARG(lde >= H && ldwi >= H, "gru_pair_loss: lde (%lld) and ldwi (%lld) must be >= H (%d): the state is scored against E, so D = H",
                  (long long)lde, (long long)ldwi, H);
    DAE_CHECK_ARG(ldwh >= H && ld_dwi >= H && ld_dwh >= H, "gru_pair_loss: ldwh (%lld), ld_dwi (%lld) and ld_dwh (%lld) must be >= H (%d)",
                  (long long)ldwh, (long long)ld_dwi, (long long)ld_dwh, H);
    int64_t events = 0;
    for (int t = 0; t < T; ++t) {
        DAE_CHECK_ARG(active_host[t] >= 0 && active_host[t] <= (t ? active_host[t - 1] : M),
                      "gru_pair_loss: active_host must be non-increasing and at most M (active_host[%d] = %lld)", t, (long long)active_host[t]);
        events += active_host[t];
    }
    DAE_CHECK_ARG(events <= nnz, "gru_pair_loss: the schedule's T = %d steps hold %lld events, more than nnz = %lld", T, (long long)events,
                  (long long)nnz);
    const int64_t Nap = pad128(Na), Hp = pad128(H), Mp = pad128(M), Rb = gf_rows_bound(nnz, T);
    DAE_CHECK_ARG(Nap * Hp * 4 < (1ll << 32) && 3 * Hp * Hp * 4 < (1ll << 32) && Mp * Hp * 4 < (1ll << 32) && 4 * Hp * Rb * 4 < (1ll << 32),
                  "gru_pair_loss: an operand image exceeds 4 GiB (Na = %d, H = %d, M = %lld, nnz = %lld: split the users into smaller calls)", Na, H,
                  (long long)M, (long long)nnz);
    DAE_CHECK_ARG(M < (1ll << 31) && nnz < (1ll << 31), "gru_pair_loss: M = %lld / nnz = %lld exceed the grid", (long long)M, (long long)nnz);
    hipStream_t st = (hipStream_t)stream;
    // the training steps: step s runs the users that have an event s + 1
    std::vector<int64_t> base;                                  // base[s] for s = 0 .. S
    base.push_back(0);
    for (int t = 1; t < T && active_host[t] > 0; ++t) base.push_back(base.back() + pad128(active_host[t]));
    const int S = (int)base.size() - 1;
    const int64_t R = base[S];
    auto rows_of = [&](int s) -> int64_t { return s < S ? active_host[s + 1] : 0; };
    if (margin && nnz > 0) DAE_CHECK_HIP(hipMemsetAsync(margin, 0, (size_t)nnz * n_neg * 4, st));
    if (S == 0) {                                               // nothing to predict: zero loss, zero pairs, zero gradients
        DAE_LAUNCH(gru_loss_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)nullptr, (const int32_t*)nullptr, (int64_t)0, loss, n_pairs);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(gru_dw_fold_kernel, dim3(3 * H), dim3(256), 0, st, (const float*)nullptr, 0, (int64_t)0, (int)H, (int)Hp, 0, 0, 0, dW_ih, ld_dwi);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(gru_dw_fold_kernel, dim3(3 * H), dim3(256), 0, st, (const float*)nullptr, 0, (int64_t)0, (int)H, (int)Hp, 0, 0, 0, dW_hh, ld_dwh);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(gru_db_kernel, dim3((unsigned)Hp), dim3(256), 0, st, (const float*)nullptr, (int64_t)0, (int)H, (int)Hp, db_ih, db_hh);
        DAE_CHECK_LAUNCH();
        return 0;
    }
    const uint64_t need = gf_workspace(Nap, Hp, Mp, Rb);
    DAE_CHECK_ARG(workspace && workspace_bytes >= need, "gru_pair_loss: workspace too small (%llu < %llu bytes)",
                  (unsigned long long)(workspace ? workspace_bytes : 0), (unsigned long long)need);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "gru_pair_loss: workspace must be 256-byte aligned");
    char* w = (char*)workspace;
    auto carve = [&](uint64_t bytes) { char* q = w; w += al256(bytes); return q; };
    float* Ei = (float*)carve(Nap * Hp * 4);
    float* Wi = (float*)carve(3 * Hp * Hp * 4);
    float* Wh = (float*)carve(3 * Hp * Hp * 4);
    float* WhT = (float*)carve(3 * Hp * Hp * 4);
    float* P = (float*)carve(Nap * 3 * Hp * 4);
    float* bhn = (float*)carve(Hp * 4);
    float* HP = (float*)carve(Rb * Hp * 4);
    float* HG = (float*)carve(Rb * Hp * 4);
    float* SR = (float*)carve(Rb * Hp * 4);
    float* SZ = (float*)carve(Rb * Hp * 4);
    float* SN = (float*)carve(Rb * Hp * 4);
    float* SQ = (float*)carve(Rb * Hp * 4);
    float* DT = (float*)carve(4 * Rb * Hp * 4);
    float* HPT = (float*)carve(Rb * Hp * 4);
    float* XT = (float*)carve(Rb * Hp * 4);
    float* carry = (float*)carve(Mp * Hp * 4);
    int64_t* row_event = (int64_t*)carve(Rb * 8);
    double* rowloss = (double*)carve(Rb * 8);
    int32_t* rowpairs = (int32_t*)carve(Rb * 4);
    float* slabs = (float*)carve((uint64_t)GF_MAX_SPLITS * 3 * Hp * Hp * 4);
    // ---- 1. operand images and the input projection of every article (as dae_gru_user_states) ----
    if (int rc = launch_row_normalize(E, lde, Na, H, 0, 0, Ei, Hp, (int)Hp, (int)Nap, st)) return rc;
    for (int g = 0; g < 3; ++g) {
        if (int rc = launch_row_normalize(W_ih + (int64_t)g * H * ldwi, ldwi, H, H, 0, 0, Wi + (int64_t)g * Hp * Hp, Hp, (int)Hp, (int)Hp, st)) return rc;
        if (int rc = launch_row_normalize(W_hh + (int64_t)g * H * ldwh, ldwh, H, H, 0, 0, Wh + (int64_t)g * Hp * Hp, Hp, (int)Hp, (int)Hp, st)) return rc;
    }
    DAE_LAUNCH(gru_wht_kernel, dim3((unsigned)Hp), dim3(256), 0, st, W_hh, ldwh, (int)H, (int)Hp, WhT);
    DAE_CHECK_LAUNCH();
    if (int rc = launch_gemm_f32out(DAE_F32, (int)Nap, (int)(3 * Hp), Ei, Hp, Wi, Hp, (int)Hp, nullptr, 0, nullptr, 0, 0, P, 3 * Hp, 1, 0, st,
                                    GEMM_ROLE_GENERIC))
        return rc;
    DAE_LAUNCH(gru_bias_kernel, dim3((unsigned)Na + 1), dim3(256), 0, st, P, (int)Na, (int)H, (int)Hp, b_ih, b_hh, bhn);
    DAE_CHECK_LAUNCH();
    DAE_CHECK_HIP(hipMemsetAsync(HP, 0, (size_t)(base[1] * Hp * 4), st));       // slab 0: h = 0
    // ---- 2. forward, one launch per step ----
    {
        GruTrainParams p;
        memset(&p, 0, sizeof(p));
        p.g.seg[0].lda_b = p.g.seg[0].ldb_b = Hp * 4;
        p.g.seg[0].Bt = (const char*)Wh;
        p.g.seg[0].ktiles = p.g.ktiles_total = (int)(Hp * 4 / BKB);
        p.g.nseg = 1; p.g.splits = 1; p.g.out_scale = 1.f;
        p.P = P; p.bhn = bhn; p.indptr = indptr; p.items = items; p.order = order; p.U = nullptr; p.ldu = 0;
        p.nnz = nnz; p.Na = Na; p.H = H; p.Hp = (int)Hp; p.all_states = 0;
        for (int s = 0; s < S; ++s) {
            const int64_t o = base[s] * Hp;
            p.g.seg[0].A = (const char*)(HP + o);
            p.hprev = HP + o; p.hnext = HP + (s + 1 < S ? base[s + 1] * Hp : 0);      // the last step has no successor and writes none
            p.sr = SR + o; p.sz = SZ + o; p.sn = SN + o; p.sq = SQ + o; p.hout = HG + o; p.row_event = row_event + base[s];
            p.t = s; p.active = (int)rows_of(s); p.next = (int)rows_of(s + 1);
            p.skip_k = s == 0 ? 1 : 0;                          // h = 0: every product is an exact zero
            const int64_t grid = (base[s + 1] - base[s]) / BM * (Hp / BN);
            if (int rc = p.skip_k ? sweep_launch<gru_step_kernel<true, GruTrainParams>>(grid, GRU_LDS, GRU_LDS, st, p)
                                  : sweep_launch<gru_step_kernel<false, GruTrainParams>>(grid, GRU_LDS, GRU_LDS, st, p))
                return rc;
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
        GruBackParams p;
        memset(&p, 0, sizeof(p));
        float* const img[3] = {SR, SZ, SQ};
        for (int k = 0; k < 3; ++k) {
            p.g.seg[k].lda_b = Hp * 4; p.g.seg[k].ldb_b = 3 * Hp * 4;
            p.g.seg[k].Bt = (const char*)(WhT + (int64_t)k * Hp);
            p.g.seg[k].ktiles = (int)(Hp * 4 / BKB);
        }
        p.g.nseg = 3; p.g.ktiles_total = 3 * (int)(Hp * 4 / BKB); p.g.splits = 1; p.g.out_scale = 1.f;
        p.carry = carry; p.H = H; p.Hp = (int)Hp;
        for (int s = S - 1; s >= 0; --s) {
            const int64_t o = base[s] * Hp, on = (s + 1 < S ? base[s + 1] : 0) * Hp;
            for (int k = 0; k < 3; ++k) p.g.seg[k].A = (const char*)(img[k] + on);
            p.r = SR + o; p.z = SZ + o; p.n = SN + o; p.q = SQ + o; p.hprev = HP + o; p.G = HG + o;
            p.rows = (int)rows_of(s); p.next = (int)rows_of(s + 1);
            const int64_t grid = (base[s + 1] - base[s]) / BM * (Hp / BN);
            if (int rc = sweep_launch<gru_back_kernel>(grid, GRU_RING, GRU_RING, st, p)) return rc;
        }
    }
    // ---- 5. the weight gradients: K-contiguous images, two split-K GEMMs, fixed-order folds ----
    {
        const dim3 tg((unsigned)(R / 64), (unsigned)(Hp / 64));
        float* const src[4] = {SN, SR, SZ, SQ};
        for (int b = 0; b < 4; ++b) {
            DAE_LAUNCH(gru_transpose_kernel<false>, tg, dim3(256), 0, st, (const float*)src[b], Hp, (const int64_t*)nullptr, (const int32_t*)nullptr, 0, 0,
                       DT + (int64_t)b * Hp * R, R);
            DAE_CHECK_LAUNCH();
        }
        DAE_LAUNCH(gru_transpose_kernel<false>, tg, dim3(256), 0, st, (const float*)HP, Hp, (const int64_t*)nullptr, (const int32_t*)nullptr, 0, 0, HPT, R);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(gru_transpose_kernel<true>, tg, dim3(256), 0, st, E, lde, (const int64_t*)row_event, items, (int)Na, (int)H, XT, R);
        DAE_CHECK_LAUNCH();
        const int64_t tiles = (3 * Hp / BM) * (Hp / BN), ktiles = R * 4 / BKB;
        const int splits = (int)std::max<int64_t>(1, std::min<int64_t>(GF_MAX_SPLITS, std::min<int64_t>(ktiles / 4, 1024 / tiles)));
        const int64_t slab = 3 * Hp * Hp;
        if (int rc = launch_gemm_f32out(DAE_F32, (int)(3 * Hp), (int)Hp, DT, R, XT, R, (int)R, nullptr, 0, nullptr, 0, 0, slabs, Hp, splits, slab, st,
                                        GEMM_ROLE_GENERIC))
            return rc;
        DAE_LAUNCH(gru_dw_fold_kernel, dim3(3 * H), dim3(256), 0, st, (const float*)slabs, splits, slab, (int)H, (int)Hp, 1, 2, 0, dW_ih, ld_dwi);
        DAE_CHECK_LAUNCH();
        if (int rc = launch_gemm_f32out(DAE_F32, (int)(3 * Hp), (int)Hp, DT + Hp * R, R, HPT, R, (int)R, nullptr, 0, nullptr, 0, 0, slabs, Hp, splits, slab,
                                        st, GEMM_ROLE_GENERIC))
            return rc;
        DAE_LAUNCH(gru_dw_fold_kernel, dim3(3 * H), dim3(256), 0, st, (const float*)slabs, splits, slab, (int)H, (int)Hp, 0, 1, 2, dW_hh, ld_dwh);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(gru_db_kernel, dim3((unsigned)Hp), dim3(256), 0, st, (const float*)DT, R, (int)H, (int)Hp, db_ih, db_hh);
        DAE_CHECK_LAUNCH();
    }
    return 0;
}
