// dae_rank.hip -- the rank of one target corpus row per query row among all corpus rows, without the Nq x Nc matrix
// (dae_rank_similarity): the full-rank twin of dae_topk_similarity_ex, for AUC, mean rank and untruncated MRR / nDCG.
//
// The scores and the order are those of dae_topk.hip: rows normalised by row_normalize_kernel into zero-padded fp32 operand
// images, products by gemm_mainloop<float, 2> over the whole K range in one pass, every (score, index) pair mapped to the
// 64-bit key pair_key (dae_score_sweep.h) = score_key(score) << 32 | ~index (score descending, then index ascending,
// -0 == +0).  What is new is an epilogue that COUNTS the keys above one key per row instead of selecting the k largest.
//
//   rank[i] = 1 + #{ j < Nc : j != t, j not in row i's exclusion list, not (exclude_self and j == i), key(S[i, j], j) > key(S[i, t], t) }
//
// 1. rank_gather_kernel copies the targets' rows of the corpus image into a third image G [Nqp x Dp] (row i = corpus row t_i).
// 2. rank_target_kernel, one workgroup per query tile: the same K loop on (query tile qt of Q, tile qt of G); the diagonal of
//    the 128 x 128 result is S[i, t_i], out of the instruction sequence that produces it in the sweep (the value of an MFMA
//    output element depends on its two operand rows and the K order alone, not on its place in the tile), so target_score and
//    the key are bit-equal to what dae_topk_similarity writes for that pair.  Writes the key (8 bytes per row), target_score
//    and rank = 1 (0 for a row without a target).
// 3. rank_tiles_kernel: grid = (query tiles) x (corpus slices), 256 threads (4 waves), as topk_tiles_kernel.  Per 128-column
//    tile the keys above the row's target key are counted straight from the accumulators: a lane holds 32 rows x 2 columns of
//    the tile; the compare's lane mask is counted per half wave on the scalar unit and lane l of a wave keeps the running
//    count of the wave's row l for the whole slice.  Columns >= Nc (zero padding: score 0, which would
//    beat every negative target) and the self pair are masked; the target itself has an equal key and is never counted.
//    Exclusion lists (RowFilter, dae_score_sweep.h) only remove competitors: the sweep counts every column, then the listed
//    ones are taken out again.  Lane l < 32 of wave w owns query row 32 w + l and a cursor into the list it reads (row_list_of); the
//    items of a list that fall into the current tile are the run behind the cursor.  Only when some row of the query tile has
//    an item in the tile is the tile written to LDS (over the dead staging ring); the owner lanes read the listed columns'
//    scores there, compare and count.  The work is one step per list item -- it does not grow with rank.
//    End of the slice: counters and corrections meet in a [128] LDS array (integer atomics) and one atomic add per row goes
//    to rank -- integers, so the result is bit-identical run to run and independent of the corpus split and the grid.
// LDS: 64 KiB ring / tile + 1 KiB keys + 0.5 KiB counts = 65.5 KiB, two workgroups per CU.
//
// Candidate windows (dae_rank_similarity_win, rank_tiles_kernel<*, true>): row i's competitors are only the columns
// win_lo[i] <= j < win_hi[i].  By window_prologue (dae_score_sweep.h) the query tile's windows, clamped to [0, Nc], go to LDS
// (+1 KiB) and the workgroups of a query tile split the tiles of the union of its non-empty windows; the two compares join the ballots of the
// count loop (bounds read from LDS per row, not kept across the K loop), a list item outside the row's window is not taken out
// again (the sweep never counted it), and a workgroup with an empty slice adds nothing.  rank_tiles_kernel<*, false> is the
// kernel as it was; rank_gather_kernel and rank_target_kernel do not know about windows.
//
// Shared stamped lists (dae_rank_similarity_seq, rank_tiles_kernel<true, *, true>): the cursor walks the list of its row's USER and an
// item is taken out again only if its stamp is at most the row's limit -- the test sits in front of the "was it counted, does it beat
// the target" step; an item stamped later stays counted.  Per owner lane that is one more pointer (the stamps beside the items) and
// the limit; nothing new lives in the count loop.  rank_tiles_kernel<*, *, false> is the kernel as it was.
#include "dae_score_sweep.h"

namespace dae {

constexpr int RANK_SLOTS = 512;            // workgroups in flight on the MI355X: 256 CUs x 2 (the slice count is sized for it)
constexpr int RANK_TILE_BYTES = BM * BN * 4;
constexpr int RANK_LDS = RANK_TILE_BYTES + 128 * 8 + 128 * 4;
constexpr int RANK_WIN_LDS = RANK_LDS + 2 * 128 * 4 + 16;   // + the query tile's windows and their union
constexpr int RANK_TARGET_LDS = lds_bytes_for(2);

__global__ __launch_bounds__(256) void rank_gather_kernel(const float* __restrict__ Ci, const int32_t* __restrict__ targets, int Nq, int Nc,
                                                          int Dp, float* __restrict__ G) {
    const int i = blockIdx.x;                                   // < Nqp
    int t = i < Nq ? targets[i] : 0;
    t = min(max(t, 0), Nc - 1);                                 // a caller error (see dae_hip.h) must not become a stray read
    const f32x4* src = reinterpret_cast<const f32x4*>(Ci + (int64_t)t * Dp);
    f32x4* dst = reinterpret_cast<f32x4*>(G + (int64_t)i * Dp);
    for (int d = threadIdx.x; d < Dp / 4; d += 256) dst[d] = src[d];
}

struct RankTargetParams {
    GemmParams g;                 // one K segment: A = query image, Bt = gathered image
    int Nq, Nc;
    const int32_t* targets;       // [Nq]
    uint64_t* tkey;               // [Nqp]
    int32_t* rank;                // [Nq]
    float* target_score;          // [Nq]
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void rank_target_kernel(RankTargetParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int qt = blockIdx.x;
    f32x16 acc[2][2];
    gemm_mainloop<float, 2>(p.g, qt, qt, 0, p.g.ktiles_total, lds, acc);
    if (wm != wn) return;                                       // the diagonal lies in the waves (0, 0) and (1, 1), blocks mt == nt
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (acc_row(0, r, g) != c) continue;                // block (mt, mt): the value of row == column
            const int gi = qt * BM + wm * 64 + acc_col(mt, c);
            if (gi >= p.Nq) continue;
            const int t = p.targets[gi];
            const float s = acc[mt][mt][r];
            if (t < 0) {
                p.tkey[gi] = ~0ull;                             // above every key: nothing is counted
                p.rank[gi] = 0;
                p.target_score[gi] = -__builtin_inff();
            } else {
                p.tkey[gi] = pair_key(s, min(t, p.Nc - 1));
                p.rank[gi] = 1;
                p.target_score[gi] = s;
            }
        }
}

struct RankParams {
    GemmParams g;                 // one K segment: A = query image, Bt = corpus image
    int Nq, Nc, splits, ctiles;
    const uint64_t* tkey;         // [Nqp] target keys (rank_target_kernel)
    int32_t* rank;                // [Nq], holds 1 (0 without a target) on entry
    RowFilter f;                  // which columns compete in a row (dae_score_sweep.h); a listed column is counted, then taken out again
};

template <bool EXCL, bool WIN, bool SEQ = false>
__global__ __launch_bounds__(GEMM_THREADS, 2) void rank_tiles_kernel(RankParams p) {
    static_assert(EXCL || !SEQ, "the shared lists are a form of the exclusion lists");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* tile = reinterpret_cast<float*>(lds);
    uint64_t* tk = reinterpret_cast<uint64_t*>(lds + RANK_TILE_BYTES);     // the query tile's target keys
    int* cnt = reinterpret_cast<int*>(tk + 128);                           // keys above the target, per row, this slice
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.x % p.splits, qt = blockIdx.x / p.splits;
    int ct0 = (int)((int64_t)p.ctiles * split / p.splits), ct1 = (int)((int64_t)p.ctiles * (split + 1) / p.splits);
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    if (tid < 128) {
        const int gi = qt * BM + tid;
        tk[tid] = gi < p.Nq ? p.tkey[gi] : ~0ull;
        cnt[tid] = 0;
    }
    int* wlo = reinterpret_cast<int*>(lds + RANK_LDS);          // the query tile's windows (WIN only; behind the counts)
    int* whi = wlo + 128;
    if constexpr (WIN) window_prologue(p.f.win_lo, p.f.win_hi, p.Nq, p.Nc, qt, split, p.splits, wlo, whi, whi + 128, ct0, ct1);
    // ---- the exclusion cursor of this lane's row (lanes 0..31 of every wave) ----
    const int xrow = wave * 32 + lane, xgi = qt * BM + xrow;
    RowList xl = {nullptr, nullptr, 0, 0};
    int xpos = 0, xnext = INT32_MAX, xsub = 0;
    uint64_t xkey = ~0ull;
    if constexpr (EXCL) {
        if (lane < 32 && xgi < p.Nq) {
            xkey = p.tkey[xgi];
            xl = row_list_of<SEQ>(p.f, xgi);
            if (xkey == ~0ull) xl.n = 0;                        // no target: nothing to count
            xpos = lower_bound_i32(xl.X, xl.n, ct0 * BN);       // first item of the slice
            if (xpos < xl.n) xnext = xl.X[xpos];
        }
    }
    int n = 0;                                                  // lane l: keys above the target of row wm * 64 + l in this wave's 64 columns
    __syncthreads();
    for (int ct = ct0; ct < ct1; ++ct) {
        f32x16 acc[2][2];
        gemm_mainloop<float, 2>(p.g, qt, ct, 0, p.g.ktiles_total, lds, acc);
        // ---- count from the accumulators (tk lies behind the ring).  A register of the tile holds two rows, one per half wave:
        //      the compare's lane mask is the ballot, its two halves are counted on the scalar unit and added to the rows' lanes ----
        const int j0 = ct * BN + wn * 64 + c, j1 = j0 + 32;
        const bool ok0 = j0 < p.Nc, ok1 = j1 < p.Nc;
        int ln = lane;
        asm volatile("" : "+v"(ln));                           // per tile: keeps the rows' lane masks and LDS addresses out of the registers that live across the K loop
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = acc_row(mt, r, 0);                         // the row of lanes 0..31 (g = 0); lanes 32..63 hold lrow + 4
                const int row = wm * 64 + lrow + 4 * (ln >> 5);
                const uint64_t t = tk[row];
                const int self = p.f.exclude_self ? qt * BM + row : -1;
                uint64_t b0, b1;
                if constexpr (WIN) {                            // the row's bounds come from LDS here: nothing lives across the K loop
                    const int wl = wlo[row], wh = whi[row];
                    b0 = __ballot(ok0 && j0 != self && j0 >= wl && j0 < wh && pair_key(acc[mt][0][r], j0) > t);
                    b1 = __ballot(ok1 && j1 != self && j1 >= wl && j1 < wh && pair_key(acc[mt][1][r], j1) > t);
                } else {
                    b0 = __ballot(ok0 && j0 != self && pair_key(acc[mt][0][r], j0) > t);
                    b1 = __ballot(ok1 && j1 != self && pair_key(acc[mt][1][r], j1) > t);
                }
                const int lo = __popc((uint32_t)b0) + __popc((uint32_t)b1), hi = __popc((uint32_t)(b0 >> 32)) + __popc((uint32_t)(b1 >> 32));
                n += (ln == lrow ? lo : 0) + (ln == lrow + 4 ? hi : 0);
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four rows' keys in flight, not all 32 (VGPRs)
            }
        if constexpr (!EXCL) __syncthreads();                   // every wave is done with the staging ring
        if constexpr (EXCL) {
            const int tile_end = (ct + 1) * BN;
            // the barrier also says that every wave is done with the staging ring
            if (__syncthreads_or(xnext < tile_end)) {
                acc_to_tile(acc, tile, wm, wn, g, c);
                __syncthreads();
                int last = -1;
                while (xnext < tile_end) {                      // the run of this row's list inside the tile
                    const int x = xnext;
                    bool inw = true;                            // outside the row's window the sweep did not count it
                    if constexpr (WIN) inw = x >= wlo[xrow] && x < whi[xrow];
                    if constexpr (SEQ) inw = inw && xl.S[xpos] <= xl.lim;      // stamped later than this row: not barred, stays counted
                    if (x >= ct * BN && x != last && x < p.Nc && !(p.f.exclude_self && x == xgi) && inw)
                        xsub += (int)(pair_key(tile[xrow * BN + (x - ct * BN)], x) > xkey);
                    last = x;
                    ++xpos;
                    xnext = xpos < xl.n ? xl.X[xpos] : INT32_MAX;
                }
                __syncthreads();                                // the tile is the next K loop's staging ring
            }
        }
    }
    // ---- the slice's counts: lanes -> LDS -> one atomic per row ----
    if (n) atomicAdd(&cnt[wm * 64 + lane], n);
    if constexpr (EXCL)
        if (xsub) atomicSub(&cnt[xrow], xsub);
    __syncthreads();
    if (tid < 128 && qt * BM + tid < p.Nq && cnt[tid] != 0) atomicAdd(&p.rank[qt * BM + tid], cnt[tid]);
}

static int rank_splits(int Nq, int Nc) { return sweep_splits(Nq, Nc, RANK_SLOTS, RANK_SLOTS); }      // no cap of its own

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_rank_similarity_workspace(int32_t Nq, int32_t Nc, int32_t D) {
    if (Nq <= 0 || Nc <= 0 || D <= 0) return 0;
    const uint64_t Nqp = pad128(Nq), Dp = pad128(D);
    // query image, corpus image, gathered target image, one key per query row
    return sweep_images_bytes(Nq, Nc, D) + al256(Nqp * Dp * 4) + al256(Nqp * 8);
}

extern "C" uint64_t dae_rank_similarity_win_workspace(int32_t Nq, int32_t Nc, int32_t D) {
    return dae_rank_similarity_workspace(Nq, Nc, D);            // the windows are read in place
}

extern "C" uint64_t dae_rank_similarity_seq_workspace(int32_t Nq, int32_t Nc, int32_t D) {
    return dae_rank_similarity_workspace(Nq, Nc, D);            // the shared lists are read in place
}

// dae_rank_similarity_win and dae_rank_similarity_seq (seq: the entry takes the shared stamped lists)
static int rank_run(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D, int32_t norm,
                    int32_t metric, RowFilter f, bool seq, const int32_t* targets, int32_t* rank, float* target_score, void* workspace,
                    uint64_t workspace_bytes, void* stream) {
    if (int rc = sweep_filter_check("rank_similarity", f, seq)) return rc;
    DAE_CHECK_ARG(Q && workspace && Nq > 0 && D > 0 && ldq >= D, "rank_similarity: bad input");
    DAE_CHECK_ARG(targets && rank && target_score, "rank_similarity: targets / rank / target_score are NULL");
    DAE_CHECK_ARG(!f.exclude_self || !C, "rank_similarity: exclude_self needs C == NULL (the corpus is Q itself)");
    hipStream_t st = (hipStream_t)stream;
    SweepOperands o;
    if (int rc = sweep_prepare("rank_similarity", Q, ldq, Nq, C, ldc, Nc, D, norm, metric, workspace, workspace_bytes,
                               dae_rank_similarity_workspace(Nq, Nc, D), st, o))
        return rc;
    const int splits = rank_splits(Nq, Nc);
    float* Gi = (float*)o.rest;
    uint64_t* tkey = (uint64_t*)(o.rest + al256(o.Nqp * o.Dp * 4));
    DAE_LAUNCH(rank_gather_kernel, dim3((unsigned)o.Nqp), dim3(256), 0, st, o.Ci, targets, (int)Nq, (int)Nc, (int)o.Dp, Gi);
    DAE_CHECK_LAUNCH();
    RankTargetParams tp;
    memset(&tp, 0, sizeof(tp));
    tp.g = o.g;
    tp.g.seg[0].Bt = (const char*)Gi;
    tp.Nq = Nq; tp.Nc = Nc; tp.targets = targets; tp.tkey = tkey; tp.rank = rank; tp.target_score = target_score;
    if (int rc = sweep_launch<rank_target_kernel>(o.Nqp / BM, RANK_TARGET_LDS, RANK_TARGET_LDS, st, tp)) return rc;
    RankParams p;
    memset(&p, 0, sizeof(p));
    p.g = o.g;
    p.Nq = Nq; p.Nc = Nc; p.splits = splits; p.ctiles = (int)(o.Ncp / BN);
    p.tkey = tkey; p.rank = rank; p.f = f;
    return DAE_SWEEP_LAUNCH_FILTERED(rank_tiles_kernel, f, RANK_LDS, RANK_WIN_LDS, o.Nqp / BM * splits, st, p);
}

extern "C" int dae_rank_similarity_win(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                                       int32_t norm, int32_t metric, int32_t exclude_self, const int64_t* excl_indptr,
                                       const int32_t* excl_items, const int32_t* win_lo, const int32_t* win_hi, const int32_t* targets,
                                       int32_t* rank, float* target_score, void* workspace, uint64_t workspace_bytes, void* stream) {
    const RowFilter f = {exclude_self, excl_indptr, excl_items, win_lo, win_hi, nullptr, nullptr, nullptr, 0};
    return rank_run(Q, ldq, Nq, C, ldc, Nc, D, norm, metric, f, false, targets, rank, target_score, workspace, workspace_bytes, stream);
}

extern "C" int dae_rank_similarity_seq(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                                       int32_t norm, int32_t metric, int32_t exclude_self, const int64_t* list_indptr,
                                       const int32_t* list_items, const int32_t* list_stamps, int32_t n_lists, const int32_t* row_list,
                                       const int32_t* row_limit, const int32_t* win_lo, const int32_t* win_hi, const int32_t* targets,
                                       int32_t* rank, float* target_score, void* workspace, uint64_t workspace_bytes, void* stream) {
    const RowFilter f = {exclude_self, list_indptr, list_items, win_lo, win_hi, list_stamps, row_list, row_limit, n_lists};
    return rank_run(Q, ldq, Nq, C, ldc, Nc, D, norm, metric, f, true, targets, rank, target_score, workspace, workspace_bytes, stream);
}

extern "C" int dae_rank_similarity(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                                   int32_t norm, int32_t metric, int32_t exclude_self, const int64_t* excl_indptr,
                                   const int32_t* excl_items, const int32_t* targets, int32_t* rank, float* target_score,
                                   void* workspace, uint64_t workspace_bytes, void* stream) {
    return dae_rank_similarity_win(Q, ldq, Nq, C, ldc, Nc, D, norm, metric, exclude_self, excl_indptr, excl_items, nullptr, nullptr,
                                   targets, rank, target_score, workspace, workspace_bytes, stream);
}
