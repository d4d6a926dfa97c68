// dae_topk.hip -- the k most similar corpus rows of every query row, without the N x N matrix (dae_topk_similarity).
//
// The scores are those of dae_pairwise_similarity: rows normalised by row_normalize_kernel (dae_similarity.hip) into
// zero-padded fp32 operand images, products on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) of dae_gemm_tile.h.  What is
// new is the epilogue: the 128 x 128 score tile never leaves the CU, only the candidates that enter a row's running top-k.
//
// Order.  Every (score, index) pair maps to one 64-bit key, score_key(score) << 32 | ~index: a larger key is a better pair,
// i.e. score descending, then index ascending -- a total order, so the result does not depend on tiling, on the corpus
// split or on the grid, and is bit-identical run to run.  Key 0 (below every finite score) marks an empty slot.
//
// Phase A, topk_tiles_kernel: grid = (query tiles) x (corpus slices), 256 threads (4 waves).  A workgroup walks the
// 128-column corpus tiles of its slice; per tile
//   1. gemm_mainloop<float, 2>: the 128 x 128 fp32 score tile in the accumulators (LDS: the 2 x 32 KiB staging ring);
//   2. the accumulators go to LDS as a [128][128] fp32 tile, over the dead staging ring (64 KiB);
//   3. wave w owns query rows 32w .. 32w+31.  Per row the 64 lanes hold 2 columns each and compare their keys with the
//      row's threshold (the key of its current k-th entry, LDS); a ballot finds the few that beat it, and only then is
//      the row's sorted list (k keys in the global partial buffer, L2-resident) merged with them: every old entry moves
//      down by the number of candidates above it, every candidate lands at (old entries above it: binary search) +
//      (candidates above it), positions >= k drop out.
//      With exclusion lists (dae_topk_similarity_ex / _seq; RowFilter, dae_score_sweep.h) the lanes whose key beat the threshold
//      look their column up in the list their row reads (row_list_of, list_has: a binary search) and the ballot is taken again:
//      the test runs only on the few candidates that would enter a merge, and an excluded candidate never takes one of the k
//      slots.  topk_tiles_kernel<false> is the kernel without lists, unchanged.
//      Step 3's code is topk_tile_epilogue in dae_score_sweep.h: dae_words.hip runs it on score tiles of its own.
// LDS: 64 KiB tile / staging + 1 KiB thresholds + 0.5 KiB list lengths + 4 x 2 KiB merge scratch = 73.5 KiB, two
// workgroups per CU.  Phase B, topk_merge_kernel: one workgroup per query row merges the `splits` sorted lists the same
// way (each entry's rank = its position + the entries above it in the other lists) and writes idx / score.
//
// Candidate windows (dae_topk_similarity_win, topk_tiles_kernel<*, true>): row i admits only the columns win_lo[i] <= j <
// win_hi[i].  The query tile's 128 (lo, hi) pairs, clamped to [0, Nc], go to LDS (+1 KiB: 74.5 KiB, still two workgroups per
// CU); the workgroups of a query tile split the tiles of the UNION of its non-empty windows among them instead of [0, ctiles),
// a row whose window misses the current tile is passed over, and the two compares join ok0 / ok1, so a column outside the
// window never reaches the ballot, the exclusion search or the merge.  A workgroup with an empty slice writes part_n = 0.
// topk_tiles_kernel<*, false> is the kernel as it was.
//
// Shared stamped lists (dae_topk_similarity_seq, topk_tiles_kernel<true, *, true>): the same lookup in the list the row shares with
// the other states of its user, an item counting up to its stamp.  Neighbouring rows read the same list addresses; nothing is
// staged in LDS, the budget is unchanged.  topk_tiles_kernel<*, *, false> is the kernel as it was.
//
// Corpus chunks (dae_topk_images): the two operand images are built by the caller (dae_sweep_image.hip) and hold rows
// row0 .. row0 + Nq of the queries and col0 .. col0 + Nc of the corpus; the keys, the self test and the exclusion lookup use
// those global ids (TopkParams::row0 / col0; zero in every other entry).  Each row's sorted keys are carried from one corpus
// chunk to the next: phase A seeds a row's threshold with the k-th key of a full carry, so a candidate that cannot enter the
// final list loses at the first compare and the partial lists hold only keys above it; phase B merges the carry as one more
// list (33 x 128 keys of LDS), writes the merged row back to the carry and idx / score from it.  The order is total, so after
// the last chunk the row is the one the one-shot sweep returns, bit for bit.  All of it sits behind the template flags CHUNK
// (topk_tiles_kernel) and CARRY (topk_merge_kernel): the instantiations of the other entries are the kernels as they were.
#include "dae_score_sweep.h"

namespace dae {

struct TopkParams {
    GemmParams g;                 // one K segment: A = query image, Bt = corpus image
    int Nq, Nc, Nqp, k, splits, ctiles;
    uint64_t* part;               // [splits][Nqp][k] sorted keys
    int* part_n;                  // [splits][Nqp] valid keys per list
    RowFilter f;                  // which columns may compete in a row (dae_score_sweep.h)
    // dae_topk_images (topk_tiles_kernel<*, *, *, true> only): image row i is query row0 + i, image column j is candidate col0 + j --
    // the ids in the keys, in the self test and in the exclusion items (excl_indptr is already offset to the image's first row)
    int row0, col0;
    uint64_t* carry;              // [Nqp][k] each row's sorted keys over the corpus chunks before this one, or NULL
    int* carry_n;                 // [Nqp] valid keys per row
};

template <bool EXCL, bool WIN, bool SEQ = false, bool CHUNK = false>
__global__ __launch_bounds__(GEMM_THREADS, 2) void topk_tiles_kernel(TopkParams p) {
    static_assert(EXCL || !SEQ, "the shared lists are a form of the exclusion lists");
    static_assert(!CHUNK || (!WIN && !SEQ), "dae_topk_images takes neither windows nor shared lists");
    const int row0 = CHUNK ? p.row0 : 0, col0 = CHUNK ? p.col0 : 0;     // <*, *, *, false>: the kernel as it was
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* tile = reinterpret_cast<float*>(lds);
    uint64_t* th = reinterpret_cast<uint64_t*>(lds + TOPK_TILE_BYTES);
    int* len = reinterpret_cast<int*>(th + 128);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t* Ls = reinterpret_cast<uint64_t*>(len + 128) + wave * 2 * TOPK_MAX;     // this wave's copy of the list being merged
    uint64_t* Cs = Ls + TOPK_MAX;                                                    // and its candidates
    const int split = blockIdx.x % p.splits, qt = blockIdx.x / p.splits;
    int ct0 = (int)((int64_t)p.ctiles * split / p.splits), ct1 = (int)((int64_t)p.ctiles * (split + 1) / p.splits);
    const int k = p.k;
    if (tid < 128) { th[tid] = 0; len[tid] = 0; }
    if constexpr (CHUNK) {
        // a full carry: its k-th key is the threshold from the first tile on, so a candidate needs one compare to lose
        const int gi = qt * BM + tid;
        if (tid < 128 && gi < p.Nq && p.carry_n[gi] == k) th[tid] = p.carry[(int64_t)gi * k + k - 1];
    }
    int* wlo = reinterpret_cast<int*>(lds + TOPK_LDS);          // the query tile's windows (WIN only; behind the merge scratch)
    int* whi = wlo + 128;
    if constexpr (WIN) window_prologue(p.f.win_lo, p.f.win_hi, p.Nq, p.Nc, qt, split, p.splits, wlo, whi, whi + 128, ct0, ct1);
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int ct = ct0; ct < ct1; ++ct) {
        f32x16 acc[2][2];
        gemm_mainloop<float, 2>(p.g, qt, ct, 0, p.g.ktiles_total, lds, acc);
        __syncthreads();                                        // every wave is done with the staging ring
        acc_to_tile(acc, tile, wm, wn, g, c);
        __syncthreads();
        topk_tile_epilogue<EXCL, WIN, SEQ, CHUNK>(p, tile, th, len, Ls, Cs, wlo, whi, qt, ct, split, row0, col0, k, lane, wave, below);
        __syncthreads();                                        // the tile is the next K loop's staging ring
    }
    if (tid < 128 && qt * BM + tid < p.Nq) p.part_n[(int64_t)split * p.Nqp + qt * BM + tid] = len[tid];
}

template <bool CARRY>
__global__ __launch_bounds__(256) void topk_merge_kernel(const uint64_t* __restrict__ part, const int* __restrict__ part_n, int Nqp,
                                                         int splits, int k, int32_t* __restrict__ idx, float* __restrict__ score,
                                                         int64_t ldk, uint64_t* carry, int* carry_n) {
    // CARRY (dae_topk_images): the carry is one more list, list `splits`, and the merged row is written back to it
    __shared__ uint64_t keys[(TOPK_MAX_SPLITS + (CARRY ? 1 : 0)) * TOPK_MAX];
    __shared__ int off[TOPK_MAX_SPLITS + 2];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lists = splits + (CARRY ? 1 : 0);
    if (tid == 0) {
        off[0] = 0;
        for (int s = 0; s < splits; ++s) off[s + 1] = off[s] + part_n[(int64_t)s * Nqp + row];
        if constexpr (CARRY) off[lists] = off[splits] + min(max(carry_n[row], 0), k);
    }
    __syncthreads();
    const int total = off[lists];
    for (int s = 0; s < lists; ++s) {
        const uint64_t* L = !CARRY || s < splits ? part + ((int64_t)s * Nqp + row) * k : carry + (int64_t)row * k;
        for (int p = tid; p < off[s + 1] - off[s]; p += 256) keys[off[s] + p] = L[p];
    }
    __syncthreads();                                            // the carry is in LDS: its row may be overwritten
    int32_t* oi = idx + (int64_t)row * ldk;
    float* os = score + (int64_t)row * ldk;
    for (int e = tid; e < total; e += 256) {
        int s = 0;
        while (e >= off[s + 1]) ++s;
        const uint64_t x = keys[e];
        int rank = e - off[s];
        for (int t = 0; t < lists; ++t)
            if (t != s) rank += keys_above(keys + off[t], off[t + 1] - off[t], x);
        if (rank < k) {
            oi[rank] = pair_key_index(x);
            os[rank] = pair_key_score(x);
            if constexpr (CARRY) carry[(int64_t)row * k + rank] = x;
        }
    }
    for (int r = total + tid; r < k; r += 256) { oi[r] = -1; os[r] = -__builtin_inff(); }
    if (CARRY && tid == 0) carry_n[row] = min(total, k);
}

int topk_merge_launch(const uint64_t* part, const int* part_n, int Nq, int Nqp, int splits, int k, int32_t* idx, float* score, int64_t ldk,
                      hipStream_t st) {
    DAE_LAUNCH(topk_merge_kernel<false>, dim3(Nq), dim3(256), 0, st, part, part_n, Nqp, splits, k, idx, score, ldk, (uint64_t*)nullptr,
               (int*)nullptr);
    DAE_CHECK_LAUNCH();
    return 0;
}

static int topk_splits(int Nq, int Nc) { return sweep_splits(Nq, Nc, TOPK_SLOTS, TOPK_MAX_SPLITS); }

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_topk_similarity_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t k) {
    if (Nq <= 0 || Nc <= 0 || D <= 0 || k <= 0) return 0;
    const uint64_t Nqp = pad128(Nq), s = topk_splits(Nq, Nc);
    return sweep_images_bytes(Nq, Nc, D) + al256(s * Nqp * (uint64_t)k * 8) + al256(s * Nqp * 4);
}

extern "C" uint64_t dae_topk_similarity_ex_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t k) {
    return dae_topk_similarity_workspace(Nq, Nc, D, k);         // the exclusion lists are read in place
}

extern "C" uint64_t dae_topk_similarity_win_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t k) {
    return dae_topk_similarity_workspace(Nq, Nc, D, k);         // the windows are read in place
}

extern "C" uint64_t dae_topk_similarity_seq_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t k) {
    return dae_topk_similarity_workspace(Nq, Nc, D, k);         // the shared lists are read in place
}

// dae_topk_similarity_win and dae_topk_similarity_seq (seq: the entry takes the shared stamped lists)
static int topk_run(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D, int32_t norm,
                    int32_t metric, int32_t k, RowFilter f, bool seq, int32_t* idx, float* score, int64_t ldk, void* workspace,
                    uint64_t workspace_bytes, void* stream) {
    if (int rc = sweep_filter_check("topk_similarity", f, seq)) return rc;
    DAE_CHECK_ARG(Q && idx && score && workspace && Nq > 0 && D > 0 && ldq >= D, "topk_similarity: bad input");
    DAE_CHECK_ARG(k >= 1 && k <= TOPK_MAX, "topk_similarity: k must be in 1..%d (got %d)", TOPK_MAX, k);
    DAE_CHECK_ARG(!f.exclude_self || !C, "topk_similarity: exclude_self needs C == NULL (the corpus is Q itself)");
    DAE_CHECK_ARG(ldk >= k, "topk_similarity: ldk (%lld) must be >= k (%d)", (long long)ldk, k);
    hipStream_t st = (hipStream_t)stream;
    SweepOperands o;
    if (int rc = sweep_prepare("topk_similarity", Q, ldq, Nq, C, ldc, Nc, D, norm, metric, workspace, workspace_bytes,
                               dae_topk_similarity_workspace(Nq, Nc, D, k), st, o))
        return rc;
    const int splits = topk_splits(Nq, Nc);
    TopkParams p;
    memset(&p, 0, sizeof(p));
    p.g = o.g;
    p.Nq = Nq; p.Nc = Nc; p.Nqp = (int)o.Nqp; p.k = k; p.splits = splits;
    p.ctiles = (int)(o.Ncp / BN);
    p.part = (uint64_t*)o.rest; p.part_n = (int*)(o.rest + al256((uint64_t)splits * o.Nqp * k * 8));
    p.f = f;
    if (int rc = DAE_SWEEP_LAUNCH_FILTERED(topk_tiles_kernel, f, TOPK_LDS, TOPK_WIN_LDS, o.Nqp / BM * splits, st, p)) return rc;
    return topk_merge_launch(p.part, p.part_n, Nq, p.Nqp, splits, k, idx, score, ldk, st);
}

extern "C" uint64_t dae_topk_carry_bytes(int32_t Nq, int32_t k) {
    if (Nq <= 0 || k <= 0) return 0;
    return al256((uint64_t)pad128(Nq) * (uint64_t)k * 8) + al256((uint64_t)pad128(Nq) * 4);
}

extern "C" uint64_t dae_topk_images_workspace(int32_t Nq, int32_t Nc, int32_t k) {
    if (Nq <= 0 || Nc <= 0 || k <= 0) return 0;
    const uint64_t Nqp = pad128(Nq), s = topk_splits(Nq, Nc);
    return al256(s * Nqp * (uint64_t)k * 8) + al256(s * Nqp * 4);
}

extern "C" int dae_topk_images(const float* Qi, int32_t Nq, int32_t row0, const float* Ci, int32_t Nc, int32_t col0, int32_t D, int32_t k,
                               int32_t exclude_self, const int64_t* excl_indptr, const int32_t* excl_items, void* carry, int32_t* idx,
                               float* score, int64_t ldk, void* workspace, uint64_t workspace_bytes, void* stream) {
    RowFilter f = {exclude_self, excl_indptr, excl_items, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    if (int rc = sweep_filter_check("topk_images", f, false)) return rc;
    DAE_CHECK_ARG(idx && score && carry, "topk_images: idx / score / carry are NULL");
    DAE_CHECK_ARG(k >= 1 && k <= TOPK_MAX, "topk_images: k must be in 1..%d (got %d)", TOPK_MAX, k);
    DAE_CHECK_ARG(ldk >= k, "topk_images: ldk (%lld) must be >= k (%d)", (long long)ldk, k);
    DAE_CHECK_ARG(row0 >= 0 && col0 >= 0 && (int64_t)row0 + Nq <= INT32_MAX && (int64_t)col0 + Nc <= INT32_MAX,
                  "topk_images: row0 / col0 must not be negative, and the global ids must fit 31 bits");
    DAE_CHECK_ARG(((uintptr_t)carry % 256) == 0, "topk_images: carry must be 256-byte aligned");
    SweepOperands o;
    if (int rc = sweep_prepare_images("topk_images", Qi, Nq, Ci, Nc, D, workspace, workspace_bytes, dae_topk_images_workspace(Nq, Nc, k), o))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const int splits = topk_splits(Nq, Nc);
    TopkParams p;
    memset(&p, 0, sizeof(p));
    p.g = o.g;
    p.Nq = Nq; p.Nc = Nc; p.Nqp = (int)o.Nqp; p.k = k; p.splits = splits;
    p.ctiles = (int)(o.Ncp / BN);
    p.part = (uint64_t*)o.rest; p.part_n = (int*)(o.rest + al256((uint64_t)splits * o.Nqp * k * 8));
    p.f = f;
    p.row0 = row0; p.col0 = col0;
    p.carry = (uint64_t*)carry; p.carry_n = (int*)((char*)carry + al256((uint64_t)o.Nqp * k * 8));
    if (int rc = f.excl_indptr ? sweep_launch<topk_tiles_kernel<true, false, false, true>>(o.Nqp / BM * splits, TOPK_LDS, TOPK_LDS, st, p)
                               : sweep_launch<topk_tiles_kernel<false, false, false, true>>(o.Nqp / BM * splits, TOPK_LDS, TOPK_LDS, st, p))
        return rc;
    DAE_LAUNCH(topk_merge_kernel<true>, dim3(Nq), dim3(256), 0, st, p.part, p.part_n, p.Nqp, splits, k, idx, score, ldk, p.carry, p.carry_n);
    DAE_CHECK_LAUNCH();
    return 0;
}

extern "C" int dae_topk_similarity_win(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                                       int32_t norm, int32_t metric, int32_t k, int32_t exclude_self, const int64_t* excl_indptr,
                                       const int32_t* excl_items, const int32_t* win_lo, const int32_t* win_hi, int32_t* idx,
                                       float* score, int64_t ldk, void* workspace, uint64_t workspace_bytes, void* stream) {
    const RowFilter f = {exclude_self, excl_indptr, excl_items, win_lo, win_hi, nullptr, nullptr, nullptr, 0};
    return topk_run(Q, ldq, Nq, C, ldc, Nc, D, norm, metric, k, f, false, idx, score, ldk, workspace, workspace_bytes, stream);
}

extern "C" int dae_topk_similarity_seq(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                                       int32_t norm, int32_t metric, int32_t k, int32_t exclude_self, const int64_t* list_indptr,
                                       const int32_t* list_items, const int32_t* list_stamps, int32_t n_lists, const int32_t* row_list,
                                       const int32_t* row_limit, const int32_t* win_lo, const int32_t* win_hi, int32_t* idx,
                                       float* score, int64_t ldk, void* workspace, uint64_t workspace_bytes, void* stream) {
    const RowFilter f = {exclude_self, list_indptr, list_items, win_lo, win_hi, list_stamps, row_list, row_limit, n_lists};
    return topk_run(Q, ldq, Nq, C, ldc, Nc, D, norm, metric, k, f, true, idx, score, ldk, workspace, workspace_bytes, stream);
}

extern "C" int dae_topk_similarity_ex(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                                      int32_t norm, int32_t metric, int32_t k, int32_t exclude_self, const int64_t* excl_indptr,
                                      const int32_t* excl_items, int32_t* idx, float* score, int64_t ldk, void* workspace,
                                      uint64_t workspace_bytes, void* stream) {
    return dae_topk_similarity_win(Q, ldq, Nq, C, ldc, Nc, D, norm, metric, k, exclude_self, excl_indptr, excl_items, nullptr, nullptr,
                                   idx, score, ldk, workspace, workspace_bytes, stream);
}

extern "C" int dae_topk_similarity(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                                   int32_t norm, int32_t metric, int32_t k, int32_t exclude_self, int32_t* idx, float* score,
                                   int64_t ldk, void* workspace, uint64_t workspace_bytes, void* stream) {
    return dae_topk_similarity_ex(Q, ldq, Nq, C, ldc, Nc, D, norm, metric, k, exclude_self, nullptr, nullptr, idx, score, ldk, workspace,
                                  workspace_bytes, stream);
}
