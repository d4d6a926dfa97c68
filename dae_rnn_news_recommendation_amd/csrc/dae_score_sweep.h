// dae_score_sweep.h -- what the "without the N x N matrix" kernels share: dae_topk.hip, dae_rank.hip, dae_pairs.hip and
// dae_pair_hist.hip sweep the 128 x 128 score tiles of gemm_mainloop<float, 2> over two normalised operand images and differ
// only in the epilogue.  Here: the order-preserving keys, the score tile in LDS, the tile enumerations, the row filter of top-k and
// rank (exclusion lists, stamped lists, candidate windows: its fields, the list a row reads, the window prologue, its checks and
// its launch), and the host prologue (argument checks, workspace carve, normalisation, GemmParams) and launch of every entry.
// The *_images entries (dae_topk_images, dae_pair_hist_images) sweep images their caller built chunk by chunk
// (dae_sweep_image.hip: from dense rows or straight from CSR rows); their prologue is sweep_prepare_images.
#pragma once
#include "dae_gemm_tile.h"

namespace dae {

// ---- keys ----
// monotone 32-bit key of a score: a < b  <=>  key(a) < key(b); -0 < +0 adjacent
__device__ __forceinline__ uint32_t score_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float key_score(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// 64-bit key of a (score, index) pair: a larger key is a better pair, i.e. score descending, then index ascending -- a total
// order.  Key 0 lies below every finite score, ~0 above every pair.
__device__ __forceinline__ uint64_t pair_key(float s, int j) {
    if (s == 0.f) s = 0.f;                                      // -0 and +0 are one score
    return ((uint64_t)score_key(s) << 32) | (uint32_t)~(uint32_t)j;
}
__device__ __forceinline__ float pair_key_score(uint64_t x) { return key_score((uint32_t)(x >> 32)); }
__device__ __forceinline__ int32_t pair_key_index(uint64_t x) { return (int32_t)~(uint32_t)x; }

// ---- the score tile ----
// Wave (wm, wn) of gemm_mainloop<float, 2> holds the 64 x 64 quadrant (wm * 64, wn * 64) of the tile as acc[mt][nt][r], in the accumulator
// layout of dae_gemm_tile.h (acc_row / acc_col, relative to the quadrant).
// the accumulators as a [128][128] fp32 tile in LDS (over the dead staging ring: the caller's barriers frame it)
__device__ __forceinline__ void acc_to_tile(const f32x16 (&acc)[2][2], float* tile, int wm, int wn, int g, int c) {
    float* first = tile + (wm * 64 + 4 * g) * BN + wn * 64 + c;  // the lane's first value
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) first[acc_row(mt, r, 0) * BN + acc_col(nt, 0)] = acc[mt][nt][r];
}

// ---- tile enumerations ----
// tile (qt, ct), ct <= qt, of the lower triangle: t = qt (qt + 1) / 2 + ct
__device__ __forceinline__ void tri_tile(long long t, int& qt, int& ct) {
    long long q = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (q * (q + 1) / 2 > t) --q;
    while ((q + 1) * (q + 2) / 2 <= t) ++q;
    qt = (int)q; ct = (int)(t - q * (q + 1) / 2);
}

// first position of the ascending list X[0, n) whose item is >= v
__device__ __forceinline__ int lower_bound_i32(const int32_t* X, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (X[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}

// ---- the row filter ----
// May corpus column j compete in query row i?  dae_topk.hip and dae_rank.hip ask it per (row, column) and differ only in where
// their epilogue applies the answer; the terms, every one optional:
struct RowFilter {
    int exclude_self;             // the corpus is the query set itself: row i does not admit column i
    const int64_t* excl_indptr;   // [Nq + 1] exclusion CSR (*_tiles_kernel<true> only): row i's list is
    const int32_t* excl_items;    // excl_items[excl_indptr[i] .. excl_indptr[i + 1]), ascending and unique
    const int32_t* win_lo;        // [Nq] candidate windows (*_tiles_kernel<*, true> only): row i admits the columns
    const int32_t* win_hi;        // win_lo[i] <= j < win_hi[i]
    // shared stamped lists (*_tiles_kernel<true, *, true> only): excl_indptr [n_lists + 1] / excl_items are then the CSR of
    // n_lists lists, one stamp per item; row i reads list row_list[i] (outside [0, n_lists): none) and is barred from its items
    const int32_t* list_stamps;   // with list_stamps[p] <= row_limit[i]
    const int32_t* row_list;      // [Nq]
    const int32_t* row_limit;     // [Nq]
    int n_lists;
};

// the list one query row reads: items X[0, n) ascending and unique; SEQ: their stamps S[0, n) and the row's limit
struct RowList { const int32_t* X; const int32_t* S; int n, lim; };

// the list of row gi: its own CSR row, or (SEQ) the shared list row_list[gi] -- outside [0, n_lists): n == 0, never a stray read
template <bool SEQ>
__device__ __forceinline__ RowList row_list_of(const RowFilter& f, int gi) {
    RowList l = {nullptr, nullptr, 0, 0};
    int u = gi;
    if constexpr (SEQ) {
        u = f.row_list[gi];
        if (u < 0 || u >= f.n_lists) return l;
        l.lim = f.row_limit[gi];
    }
    const int64_t x0 = f.excl_indptr[u];
    l.X = f.excl_items + x0;
    if constexpr (SEQ) l.S = f.list_stamps + x0;
    l.n = (int)(f.excl_indptr[u + 1] - x0);
    return l;
}

// does the list bar column j: is j one of its items, and (SEQ) stamped at most lim?
template <bool SEQ>
__device__ __forceinline__ bool list_has(const RowList& l, int j) {
    const int lo = lower_bound_i32(l.X, l.n, j);
    if constexpr (SEQ) return lo < l.n && l.X[lo] == j && l.S[lo] <= l.lim;
    else return lo < l.n && l.X[lo] == j;
}

// Candidate windows: row i admits only the columns win_lo[i] <= j < win_hi[i].  The 128 (lo, hi) pairs of query tile qt, clamped
// to [0, Nc], go to LDS (wlo / whi; an empty window and the rows >= Nq become (0, 0)); un[0..1] receives the union of the
// non-empty ones, and [ct0, ct1) the share of workgroup `split` of `splits` in the union's corpus tiles (empty without a union).
__device__ __forceinline__ void window_prologue(const int32_t* win_lo, const int32_t* win_hi, int Nq, int Nc, int qt, int split, int splits,
                                                int* wlo, int* whi, int* un, int& ct0, int& ct1) {
    const int tid = threadIdx.x;
    if (tid == 0) { un[0] = INT32_MAX; un[1] = 0; }
    __syncthreads();
    if (tid < 128) {
        const int gi = qt * BM + tid;
        int lo = 0, hi = 0;
        if (gi < Nq) { lo = min(max(win_lo[gi], 0), Nc); hi = min(max(win_hi[gi], 0), Nc); }
        if (lo >= hi) lo = hi = 0;                              // does not widen the union
        else { atomicMin(&un[0], lo); atomicMax(&un[1], hi); }
        wlo[tid] = lo; whi[tid] = hi;
    }
    __syncthreads();
    const int t0 = un[1] > 0 ? un[0] / BN : 0, nt = un[1] > 0 ? (un[1] + BN - 1) / BN - t0 : 0;
    ct0 = t0 + (int)((int64_t)nt * split / splits); ct1 = t0 + (int)((int64_t)nt * (split + 1) / splits);
}

// ---- the running top-k of a score tile ----
// What dae_topk.hip (scores from the MFMA) and dae_words.hip (scores from bitmap profiles) do with a [128][128] fp32 score tile in
// LDS; the description stands at the top of dae_topk.hip.
constexpr int TOPK_MAX = 128;
constexpr int TOPK_SLOTS = 512;            // workgroups in flight on the MI355X: 256 CUs x 2 (the slice count is sized for it)
constexpr int TOPK_MAX_SPLITS = 32;        // bounds phase B's LDS (32 lists x 128 keys x 8 B)
constexpr int TOPK_TILE_BYTES = BM * BN * 4;
constexpr int TOPK_LDS = TOPK_TILE_BYTES + 128 * 8 + 128 * 4 + 4 * 2 * TOPK_MAX * 8;
constexpr int TOPK_WIN_LDS = TOPK_LDS + 2 * 128 * 4 + 16;   // + the query tile's windows and their union

// number of keys of the descending list L[0, n) above x
__device__ __forceinline__ int keys_above(const uint64_t* L, int n, uint64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (L[m] > x) lo = m + 1; else hi = m;
    }
    return lo;
}

// The epilogue of one score tile: `tile` holds the scores of query tile qt (rows) against corpus tile ct (columns); wave w merges the
// candidates of its rows 32w .. 32w+31 into the rows' sorted lists of slice `split`.  th / len: the rows' thresholds and list lengths,
// Ls / Cs: this wave's merge scratch, wlo / whi: the rows' windows (WIN only), row0 / col0: the global ids of image row / column 0
// (CHUNK only, else 0), k = p.k, lane / wave of the thread and below = the mask of the lanes under it: values the kernel keeps across its
// tile loop.  P: the kernel's parameter block -- Nq, Nc, Nqp, k, part ([splits][Nqp][k] sorted keys) and the RowFilter f.
// The caller's barriers frame it.
template <bool EXCL, bool WIN, bool SEQ, bool CHUNK, typename P>
__device__ __forceinline__ void topk_tile_epilogue(const P& p, const float* tile, uint64_t* th, int* len, uint64_t* Ls, uint64_t* Cs,
                                                   const int* wlo, const int* whi, int qt, int ct, int split, int row0, int col0, int k,
                                                   int lane, int wave, uint64_t below) {
    const int j0 = ct * BN + lane, j1 = j0 + 64;
    const int gj0 = col0 + j0, gj1 = col0 + j1;          // the candidates' ids
    for (int rr = 0; rr < 32; ++rr) {
        const int row = wave * 32 + rr, gi = qt * BM + row;
        if (gi >= p.Nq) break;
        int wl = 0, wh = INT32_MAX;
        if constexpr (WIN) {
            wl = wlo[row]; wh = whi[row];
            if (wh <= ct * BN || wl >= (ct + 1) * BN) continue;      // the row's window misses this tile (wave-uniform)
        }
        const uint64_t t = th[row];
        const bool ok0 = j0 < p.Nc && !(p.f.exclude_self && gj0 == row0 + gi) && (!WIN || (j0 >= wl && j0 < wh)),
                   ok1 = j1 < p.Nc && !(p.f.exclude_self && gj1 == row0 + gi) && (!WIN || (j1 >= wl && j1 < wh));
        const uint64_t c0 = ok0 ? pair_key(tile[row * BN + lane], gj0) : 0, c1 = ok1 ? pair_key(tile[row * BN + 64 + lane], gj1) : 0;
        bool in0 = c0 > t, in1 = c1 > t;
        uint64_t b0 = __ballot(in0), b1 = __ballot(in1);
        if ((b0 | b1) == 0) continue;
        if constexpr (EXCL) {                               // drop the candidates the row's list bars, then ballot again
            const RowList l = row_list_of<SEQ>(p.f, gi);
            if (l.n > 0) {
                if (in0 && list_has<SEQ>(l, gj0)) in0 = false;
                if (in1 && list_has<SEQ>(l, gj1)) in1 = false;
                b0 = __ballot(in0); b1 = __ballot(in1);
                if ((b0 | b1) == 0) continue;
            }
        }
        // ---- merge the candidates into the row's list ----
        const int n0 = __popcll(b0), n = n0 + __popcll(b1);
        const int m = len[row];
        uint64_t* L = p.part + ((int64_t)split * p.Nqp + gi) * k;
        const uint64_t e0 = lane < m ? L[lane] : 0, e1 = lane + 64 < m ? L[lane + 64] : 0;
        if (in0) Cs[__popcll(b0 & below)] = c0;
        if (in1) Cs[n0 + __popcll(b1 & below)] = c1;
        if (lane < m) Ls[lane] = e0;
        if (lane + 64 < m) Ls[lane + 64] = e1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        int r0 = lane, r1 = lane + 64, q0 = 0, q1 = 0;      // new positions: old entries / candidates
        for (int q = 0; q < n; ++q) {
            const uint64_t x = Cs[q];
            r0 += x > e0; r1 += x > e1; q0 += x > c0; q1 += x > c1;
        }
        if (in0) q0 += keys_above(Ls, m, c0);
        if (in1) q1 += keys_above(Ls, m, c1);
        if (lane < m && r0 < k) L[r0] = e0;
        if (lane + 64 < m && r1 < k) L[r1] = e1;
        if (in0 && q0 < k) L[q0] = c0;
        if (in1 && q1 < k) L[q1] = c1;
        const int m2 = min(k, m + n);
        if (m2 == k) {                                      // the k-th entry is the new threshold
            if (lane < m && r0 == k - 1) th[row] = e0;
            if (lane + 64 < m && r1 == k - 1) th[row] = e1;
            if (in0 && q0 == k - 1) th[row] = c0;
            if (in1 && q1 == k - 1) th[row] = c1;
        }
        if (lane == 0) len[row] = m2;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // Ls / Cs are rewritten by the next row's merge
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- host ----
static inline uint64_t al256(uint64_t b) { return (b + 255) / 256 * 256; }

// Phase B of a top-k sweep (dae_topk.hip: topk_merge_kernel<false>): one workgroup per query row merges the row's `splits` sorted
// lists part [splits][Nqp][k] / part_n [splits][Nqp] and writes idx / score [Nq x ldk], tails -1 / -inf.
int topk_merge_launch(const uint64_t* part, const int* part_n, int Nq, int Nqp, int splits, int k, int32_t* idx, float* score, int64_t ldk,
                      hipStream_t st);

// the two operand images every *_workspace starts with
static inline uint64_t sweep_images_bytes(int Nq, int Nc, int D) {
    const uint64_t Dp = pad128(D);
    return al256(pad128(Nq) * Dp * 4) + al256(pad128(Nc) * Dp * 4);
}

// corpus slices per query tile: `slots` workgroups in flight, at most one slice per corpus tile and at most `cap`
static inline int sweep_splits(int Nq, int Nc, int slots, int cap) {
    const int64_t qt = pad128(Nq) / BM, ct = pad128(Nc) / BN;
    int64_t s = slots / qt;
    if (s > ct) s = ct;
    if (s > cap) s = cap;
    return s < 1 ? 1 : (int)s;
}

struct SweepOperands {
    float *Qi, *Ci;               // normalised, zero-padded images [Nqp x Dp], [Ncp x Dp] (Ci == Qi when the corpus is Q)
    int64_t Nqp, Ncp, Dp;
    GemmParams g;                 // one K segment: A = Qi, Bt = Ci
    char* rest;                   // the workspace behind the images
};

// the K loop over two images of width Dp: one K segment, A = Qi, Bt = Ci
static inline void sweep_gemm_params(const float* Qi, const float* Ci, int64_t Dp, GemmParams& g) {
    memset(&g, 0, sizeof(g));
    g.seg[0].A = (const char*)Qi; g.seg[0].Bt = (const char*)Ci;
    g.seg[0].lda_b = g.seg[0].ldb_b = Dp * 4;
    g.seg[0].ktiles = g.ktiles_total = (int)(Dp * 4 / BKB);
    g.nseg = 1; g.splits = 1; g.out_scale = 1.f;
}

// The prologue of every entry point: the argument checks they share (messages prefixed with `who`; `need` is the entry's
// *_workspace), the images carved from the workspace and filled by row_normalize_kernel, and the K loop's parameters.
static inline int sweep_prepare(const char* who, const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                                int32_t norm, int32_t metric, void* workspace, uint64_t workspace_bytes, uint64_t need, hipStream_t st,
                                SweepOperands& o) {
    DAE_CHECK_ARG(C ? (Nc > 0 && ldc >= D) : Nc == Nq, "%s: bad corpus (C == NULL means the corpus is Q: pass Nc == Nq)", who);
    DAE_CHECK_ARG(norm >= 0 && norm <= 3, "%s: norm must be 0 (none), 1 (l1), 2 (l2) or 3 (max)", who);
    DAE_CHECK_ARG(metric == 0 || metric == 1, "%s: metric must be 0 (cosine) or 1 (linear kernel)", who);
    o.Nqp = pad128(Nq); o.Ncp = pad128(Nc); o.Dp = pad128(D);
    DAE_CHECK_ARG(o.Nqp * o.Dp * 4 < (1ll << 32) && o.Ncp * o.Dp * 4 < (1ll << 32), "%s: an operand image exceeds 4 GiB", who);
    DAE_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%llu < %llu bytes)", who, (unsigned long long)workspace_bytes,
                  (unsigned long long)need);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "%s: workspace must be 256-byte aligned", who);
    char* w = (char*)workspace;
    o.Qi = (float*)w;           w += al256(o.Nqp * o.Dp * 4);
    o.Ci = C ? (float*)w : o.Qi;  w += al256(o.Ncp * o.Dp * 4);
    o.rest = w;
    const int cosine = metric == 0 ? 1 : 0;
    if (int rc = launch_row_normalize(Q, ldq, Nq, D, norm, cosine, o.Qi, o.Dp, (int)o.Dp, (int)o.Nqp, st)) return rc;
    if (C)
        if (int rc = launch_row_normalize(C, ldc, Nc, D, norm, cosine, o.Ci, o.Dp, (int)o.Dp, (int)o.Ncp, st)) return rc;
    sweep_gemm_params(o.Qi, o.Ci, o.Dp, o.g);
    return 0;
}

// The prologue of the *_images entries, whose caller built the images (dae_sweep_image.hip): the checks of the two images
// [pad128(Nq) x pad128(D)], [pad128(Nc) x pad128(D)] (Ci == NULL: the corpus is Qi, pass Nc == Nq) and of the workspace, and the
// K loop's parameters.  No HIP call.
static inline int sweep_prepare_images(const char* who, const float* Qi, int32_t Nq, const float* Ci, int32_t Nc, int32_t D, void* workspace,
                                       uint64_t workspace_bytes, uint64_t need, SweepOperands& o) {
    DAE_CHECK_ARG(Qi && workspace && Nq > 0 && D > 0, "%s: bad input", who);
    DAE_CHECK_ARG(Ci ? Nc > 0 : Nc == Nq, "%s: bad corpus (Ci == NULL means the corpus is Qi: pass Nc == Nq)", who);
    o.Nqp = pad128(Nq); o.Ncp = pad128(Nc); o.Dp = pad128(D);
    DAE_CHECK_ARG(o.Nqp * o.Dp * 4 < (1ll << 32) && o.Ncp * o.Dp * 4 < (1ll << 32), "%s: an operand image exceeds 4 GiB", who);
    DAE_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%llu < %llu bytes)", who, (unsigned long long)workspace_bytes,
                  (unsigned long long)need);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0 && ((uintptr_t)Qi % 256) == 0 && ((uintptr_t)Ci % 256) == 0,
                  "%s: workspace and images must be 256-byte aligned", who);
    o.Qi = const_cast<float*>(Qi); o.Ci = const_cast<float*>(Ci ? Ci : Qi);
    o.rest = (char*)workspace;
    sweep_gemm_params(o.Qi, o.Ci, o.Dp, o.g);
    return 0;
}

// The pointer checks of a RowFilter, in front of everything else an entry checks (messages prefixed with `who`).  seq: the entry
// takes the shared stamped form, whose five arrays come together or not at all; without them n_lists does not count.
static inline int sweep_filter_check(const char* who, RowFilter& f, bool seq) {
    if (seq) {
        const int given = (f.excl_indptr != nullptr) + (f.excl_items != nullptr) + (f.list_stamps != nullptr) + (f.row_list != nullptr) +
                          (f.row_limit != nullptr);
        DAE_CHECK_ARG(given == 0 || given == 5,
                      "%s: list_indptr, list_items, list_stamps, row_list and row_limit go together (%d of the 5 are NULL)", who, 5 - given);
        DAE_CHECK_ARG(given == 0 || f.n_lists >= 0, "%s: n_lists must not be negative (got %d)", who, f.n_lists);
        if (!given) f.n_lists = 0;
    }
    DAE_CHECK_ARG((f.excl_indptr == nullptr) == (f.excl_items == nullptr),
                  "%s: excl_indptr and excl_items go together (exactly one of them is NULL)", who);
    DAE_CHECK_ARG((f.win_lo == nullptr) == (f.win_hi == nullptr), "%s: win_lo and win_hi go together (exactly one of them is NULL)", who);
    return 0;
}

// launches kernel K (GEMM_THREADS threads, `lds` bytes of dynamic LDS, one parameter block) through DAE_LAUNCH; the first launch
// of every instantiation raises the kernel's dynamic-LDS limit to `lds_max`
template <auto K, typename P>
static inline int sweep_launch(int64_t grid, int lds_max, int lds, hipStream_t st, const P& p) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    DAE_CHECK_HIP(attr);
    DAE_LAUNCH(K, dim3((unsigned)grid), dim3(GEMM_THREADS), lds, st, p);
    DAE_CHECK_LAUNCH();
    return 0;
}

// sweep_launch of KERNEL<EXCL, WIN, SEQ> for the terms the RowFilter f holds, with LDS bytes of dynamic LDS (WIN_LDS with windows)
#define DAE_SWEEP_LAUNCH_FILTERED(KERNEL, f, LDS, WIN_LDS, grid, st, p)                                                                 \
    ((f).list_stamps ? ((f).win_lo ? sweep_launch<KERNEL<true, true, true>>(grid, WIN_LDS, WIN_LDS, st, p)                             \
                                   : sweep_launch<KERNEL<true, false, true>>(grid, LDS, LDS, st, p))                                   \
     : (f).win_lo    ? ((f).excl_indptr ? sweep_launch<KERNEL<true, true>>(grid, WIN_LDS, WIN_LDS, st, p)                              \
                                        : sweep_launch<KERNEL<false, true>>(grid, WIN_LDS, WIN_LDS, st, p))                            \
                     : ((f).excl_indptr ? sweep_launch<KERNEL<true, false>>(grid, LDS, LDS, st, p)                                     \
                                        : sweep_launch<KERNEL<false, false>>(grid, LDS, LDS, st, p)))

}  // namespace dae
