// dae_mmr.hip -- diversification of recommendation lists on the device (dae_mmr_lists): Maximal Marginal Relevance with an optional
// de-dup threshold and an optional cap on the articles of one label.  A second epilogue on the list's own score tile of
// dae_dedup.hip: the gather, the K loop and acc_to_tile are the same (dae_list_tile.h); where de-duplication builds masks and scans
// them, this one runs a k-step selection loop.
//
// Rule.  A row is a list of L <= 128 candidate article indices with one fp32 relevance each (no order assumed).  Position p is VALID
// iff 0 <= list[p] < Na and rel[p] is finite.  s(q, p) is the score dae_pairwise_similarity gives row list[q] against column
// list[p].  State: m[p] = +0, alive = valid.  Each of at most k steps:
//   v[p]   = (lambda (x) rel[p]) (-) ((1 (-) lambda) (x) m[p]) for every alive p -- three roundings, never a contracted FMA (mmr_value);
//   select the alive p with the largest v[p], the lowest position among equals (-0 == +0); val = v[p], near = m[p]; p leaves alive;
//   m[p']  = fmaxf(m[p'], s(p, p')) -- a NaN score leaves m as it is; the penalty is max(0, max over the selected);
//   a finite threshold: every alive p' with s(p, p') >= threshold leaves;
//   max_per_label > 0 and c = label[list[p]] >= 0: once max_per_label selected entries carry c, every alive p' with label c leaves.
// (Should every alive v be NaN -- an infinite score under lambda = 1 -- the lowest alive position is taken.)
//
// Orientation.  tile[q][p] = s(q, p): row = the SELECTED article, column = the candidate.  After a selection the wave reads row q,
// tile[q][lane] and tile[q][lane + 64]: consecutive dwords, 32 distinct banks per 32-lane half of a ds_read_b32, conflict-free.  A
// column read would put all 64 lanes on one bank.  Is the tile bit-symmetric?  By the code it must be: A = Bt = the gather buffer, and
// element (q, p) is the fmaf chain over k, in k order, of the products a[q][k] * a[p][k] -- a product does not depend on the order of
// its factors, and the chain's order does not depend on where the element lies in the tile; pairwise_similarity's fp32 matrix of the
// test corpora compares equal to its transpose.  Nothing here relies on it: only rows of selected positions are read.
//
// One workgroup of GEMM_THREADS per list.  The list's ids, relevances and labels[list[p]] go to 1.5 KiB of LDS behind the tile
// (outside the staging ring, which the K loop overwrites); invalid positions get id -1.  After gemm_mainloop<float, 2> on tile (r, r)
// of the gather buffer and acc_to_tile, wave 0 alone runs the selection in registers: lane l owns positions l and l + 64 (lambda (x)
// rel, m, alive, label).  A step is two v's per lane, a wave maximum by __shfl_xor and one readfirstlane, two ballots that locate the
// lowest position holding the maximum, two v_readlane for val / near, the two LDS reads of row q, fmaxf, the threshold compare and,
// for the cap, two ballots of "label == c" and-ed with the selected set and popcounted.  The selected position is wave-uniform, so
// nothing diverges and the state never passes through LDS.  Lane 0 stores slot t as it is selected; the tails are filled as in de-dup.
// counts[2 i] = selected; [2 i + 1] = the selected whose rank among the valid positions is >= k (a popcount of the validity ballot
// below the position): how far the re-rank reached past the plain top-k.  No atomics.
// LDS: the 64 KiB staging ring / tile + 1.5 KiB list = 65.5 KiB, two workgroups per CU (de-dup: 66.5 KiB).  A list's result depends
// on its own tile alone: bit-identical run to run, independent of the grid and of the chunking (that of dae_dedup_lists).
#include "dae_list_tile.h"

#include <cmath>

namespace dae {

constexpr int MMR_LDS = DEDUP_TILE_BYTES + 3 * 128 * 4;

struct MmrParams {
    GemmParams g;                 // one K segment: A = Bt = the gather buffer
    const int32_t* lists;         // the chunk's first list
    const float* rel;             // the chunk's first row of relevances
    const int32_t* labels;        // [Na] or NULL
    int64_t ldl, ldr, ldo;
    int Na, L, k, max_per_label;
    float lambda, threshold;
    int32_t *out_idx, *out_pos;   // the chunk's first row
    float *out_val, *out_near;
    int32_t* counts;              // [R][2]
};

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
// lr (-) (oml (x) m), each a single correctly rounded fp32 operation.  hipcc contracts a - b * c into an FMA by default, and its
// __fmul_rn / __fsub_rn are the plain operators (they contract like any other); the pragma takes the permission away here.
__device__ __forceinline__ float mmr_value(float lr, float oml, float m) {
#pragma clang fp contract(off)
    const float penalty = oml * m;
    return lr - penalty;
}
// the float lane l of the wave holds (l wave-uniform)
__device__ __forceinline__ float lane_f32(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__global__ __launch_bounds__(GEMM_THREADS, 2) void mmr_tiles_kernel(MmrParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* tile = reinterpret_cast<float*>(lds);
    int* ids = reinterpret_cast<int*>(lds + DEDUP_TILE_BYTES);  // [128] the list, -1 where invalid (outside the staging ring)
    float* rels = reinterpret_cast<float*>(ids + 128);          // [128]
    int* labs = ids + 256;                                      // [128] labels[list[p]], -1 where invalid or without labels
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    if (tid < 128) {
        int id = -1, lab = -1;
        float rv = 0.f;
        if (tid < p.L) {
            id = p.lists[(int64_t)r * p.ldl + tid];
            rv = p.rel[(int64_t)r * p.ldr + tid];
        }
        if (id < 0 || id >= p.Na || !finite_f32(rv)) id = -1;
        if (id >= 0 && p.labels) lab = p.labels[id];
        ids[tid] = id; rels[tid] = rv; labs[tid] = lab;
    }
    f32x16 acc[2][2];
    gemm_mainloop<float, 2>(p.g, r, r, 0, p.g.ktiles_total, lds, acc);
    __syncthreads();                                            // every wave is done with the staging ring
    acc_to_tile(acc, tile, wave >> 1, wave & 1, lane >> 5, lane & 31);
    __syncthreads();
    if (wave != 0) return;
    // ---- the selection, in wave 0's registers: lane l owns positions l and l + 64 ----
    const float lam = p.lambda, oml = 1.f - lam, T = p.threshold;
    const bool thr_on = finite_f32(T);
    const int k = p.k, cap = p.max_per_label;
    const int lab0 = labs[lane], lab1 = labs[lane + 64];
    const float lr0 = lam * rels[lane], lr1 = lam * rels[lane + 64];        // lambda (x) rel: the same every step
    bool al0 = ids[lane] >= 0, al1 = ids[lane + 64] >= 0;
    float m0 = 0.f, m1 = 0.f;
    const uint64_t valid0 = __ballot(al0), valid1 = __ballot(al1);
    uint64_t sel0 = 0, sel1 = 0;                                // the selected set
    const float ninf = -INFINITY;
    int32_t* oi = p.out_idx + (int64_t)r * p.ldo;
    int32_t* op = p.out_pos + (int64_t)r * p.ldo;
    float* ov = p.out_val + (int64_t)r * p.ldo;
    float* on = p.out_near + (int64_t)r * p.ldo;
    int n = 0, beyond = 0;
    for (; n < k; ++n) {
        const uint64_t a0 = __ballot(al0), a1 = __ballot(al1);
        if (!(a0 | a1)) break;
        const float v0 = mmr_value(lr0, oml, m0), v1 = mmr_value(lr1, oml, m1);
        float best = fmaxf(al0 ? v0 : ninf, al1 ? v1 : ninf);   // (fmaxf passes a NaN by)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
        best = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(best)));
        uint64_t e0 = __ballot(al0 && v0 == best), e1 = __ballot(al1 && v1 == best);
        if (!(e0 | e1)) { e0 = a0; e1 = a1; }                   // every alive v is NaN
        const int q = e0 ? __ffsll((unsigned long long)e0) - 1 : 64 + __ffsll((unsigned long long)e1) - 1;
        const float val = q < 64 ? lane_f32(v0, q) : lane_f32(v1, q - 64);
        const float near = q < 64 ? lane_f32(m0, q) : lane_f32(m1, q - 64);
        const int c = labs[q];
        if (q < 64) { sel0 |= 1ull << q; al0 = al0 && lane != q; }
        else { sel1 |= 1ull << (q - 64); al1 = al1 && lane != q - 64; }
        const int rank = q < 64 ? __popcll(valid0 & ((1ull << q) - 1ull)) : __popcll(valid0) + __popcll(valid1 & ((1ull << (q - 64)) - 1ull));
        beyond += rank >= k;
        if (lane == 0) { oi[n] = ids[q]; op[n] = q; ov[n] = val; on[n] = near; }
        const float s0 = tile[q * BN + lane], s1 = tile[q * BN + lane + 64];     // row q: the selected against every candidate
        m0 = fmaxf(m0, s0); m1 = fmaxf(m1, s1);
        if (thr_on) { al0 = al0 && !(s0 >= T); al1 = al1 && !(s1 >= T); }
        if (cap > 0 && c >= 0) {
            const int have = __popcll(__ballot(lab0 == c) & sel0) + __popcll(__ballot(lab1 == c) & sel1);
            if (have >= cap) { al0 = al0 && lab0 != c; al1 = al1 && lab1 != c; }
        }
    }
    for (int t = n + lane; t < k; t += 64) { oi[t] = -1; op[t] = -1; ov[t] = ninf; on[t] = ninf; }
    if (lane == 0) { p.counts[2 * (int64_t)r] = n; p.counts[2 * (int64_t)r + 1] = beyond; }
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_mmr_lists_workspace(int32_t Nr, int32_t Na, int32_t D, int32_t L) { return list_workspace_bytes(Nr, Na, D, L); }

extern "C" int dae_mmr_lists(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t norm, int32_t metric, const int32_t* lists,
                             int64_t ldl, const float* rel, int64_t ldr, const int32_t* labels, int32_t max_per_label, int32_t Nr, int32_t L,
                             int32_t k, float lambda, float threshold, int32_t* out_idx, int32_t* out_pos, float* out_val, float* out_near,
                             int64_t ldo, int32_t* counts, void* workspace, uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(E && lists && rel && out_idx && out_pos && out_val && out_near && counts && workspace && Na > 0 && D > 0 && Nr > 0 && lde >= D,
                  "mmr_lists: bad input");
    DAE_CHECK_ARG(L >= 1 && L <= DEDUP_MAX, "mmr_lists: L must be in 1..%d (got %d)", DEDUP_MAX, L);
    DAE_CHECK_ARG(k >= 1 && k <= L, "mmr_lists: k must be in 1..L = %d (got %d)", L, k);
    DAE_CHECK_ARG(norm >= 0 && norm <= 3, "mmr_lists: norm must be 0 (none), 1 (l1), 2 (l2) or 3 (max)");
    DAE_CHECK_ARG(metric == 0 || metric == 1, "mmr_lists: metric must be 0 (cosine) or 1 (linear kernel)");
    DAE_CHECK_ARG(lambda >= 0.f && lambda <= 1.f, "mmr_lists: lambda must be in [0, 1] (got %g)", (double)lambda);      // (false for NaN)
    DAE_CHECK_ARG(!std::isnan(threshold), "mmr_lists: threshold is NaN");
    DAE_CHECK_ARG(max_per_label >= 0, "mmr_lists: max_per_label must not be negative (got %d)", max_per_label);
    DAE_CHECK_ARG(max_per_label == 0 || labels, "mmr_lists: max_per_label > 0 needs labels");
    DAE_CHECK_ARG(ldl >= L, "mmr_lists: ldl (%lld) must be >= L (%d)", (long long)ldl, L);
    DAE_CHECK_ARG(ldr >= L, "mmr_lists: ldr (%lld) must be >= L (%d)", (long long)ldr, L);
    DAE_CHECK_ARG(ldo >= k, "mmr_lists: ldo (%lld) must be >= k (%d)", (long long)ldo, k);
    ListWorkspace w;
    if (int rc = list_workspace_carve("mmr_lists", Na, D, Nr, workspace, workspace_bytes, w)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_row_normalize(E, lde, Na, D, norm, metric == 0 ? 1 : 0, w.image, w.Dp, (int)w.Dp, (int)w.Nap, st)) return rc;
    MmrParams p;
    memset(&p, 0, sizeof(p));
    sweep_gemm_params(w.gathered, w.gathered, w.Dp, p.g);
    p.labels = labels; p.ldl = ldl; p.ldr = ldr; p.ldo = ldo; p.Na = Na; p.L = L; p.k = k; p.max_per_label = max_per_label;
    p.lambda = lambda; p.threshold = threshold;
    for (int64_t i0 = 0; i0 < Nr; i0 += w.R) {
        const int64_t n = Nr - i0 < w.R ? Nr - i0 : w.R;
        p.lists = lists + i0 * ldl; p.rel = rel + i0 * ldr;
        p.out_idx = out_idx + i0 * ldo; p.out_pos = out_pos + i0 * ldo; p.out_val = out_val + i0 * ldo; p.out_near = out_near + i0 * ldo;
        p.counts = counts + 2 * i0;
        if (int rc = launch_list_gather(w.image, (int)w.Dp, Na, p.lists, ldl, L, n, w.gathered, w.valid, st)) return rc;
        if (int rc = sweep_launch<mmr_tiles_kernel>(n, MMR_LDS, MMR_LDS, st, p)) return rc;
    }
    return 0;
}
