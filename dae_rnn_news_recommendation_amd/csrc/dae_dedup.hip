// dae_dedup.hip -- greedy de-duplication of recommendation lists on the device (dae_dedup_lists): the last stage of the
// recommendation pipeline, "skip an article whose similarity to an article already selected reaches a threshold".
//
// Rule.  A row is an ordered list of L <= 128 candidate article indices, best first.  Walking it front to back, the candidate at
// position p is KEPT iff no candidate kept at a position q < p has s(p, q) >= threshold; the walk stops after k kept.  s(p, q) is
// the score dae_pairwise_similarity gives row list[p] against column list[q]: rows normalised by row_normalize_kernel
// (dae_similarity.hip) into a zero-padded fp32 image, products by gemm_mainloop<float, 2> (dae_gemm_tile.h) over the whole K range
// in one pass.  Entries < 0 or >= Na are skipped and never kept.  An index that occurs twice is, under cosine, a duplicate of
// itself: no special case.
//
// Three kernels per chunk of R lists:
//   row_normalize_kernel      once per call: the corpus image [pad128(Na) x Dp];
//   dedup_gather_kernel       copies the image rows a chunk's lists name into the gather buffer [R * 128 x Dp]: list r owns rows
//                             128 r .. 128 r + 127, row p = the image row list[p]; an invalid entry and the positions >= L are zero
//                             rows.  A pure copy, so a gathered row IS the image row, bit for bit.  Beside the buffer: the list's
//                             128-bit validity mask (two 64-bit words, from one ballot per 64 positions);
//   dedup_tiles_kernel        one workgroup of GEMM_THREADS per list: gemm_mainloop<float, 2> with A = Bt = the gather buffer, tile
//                             (r, r) -- exactly the list's 128 x 128 score tile, tile[p][q] = s(p, q).  acc_to_tile moves it to LDS
//                             over the dead staging ring, as the top-k epilogue does.  Then
//     mask build  all 256 threads: thread (p = tid & 127, h = tid >> 7) builds the 64-bit word h of row p's mask
//                 {q < p : valid(q) && tile[p][q] >= threshold} into 2 KiB of LDS.  A thread reads ALONG its row but its wave reads
//                 DOWN a column -- 64 rows x the same q would be one bank, a 32-way conflict per ds_read_b32 half -- so lane p starts
//                 at column (p & 63) and wraps: in step i it reads q = 64 h + ((i + p) & 63), 32 consecutive dwords mod 64 per
//                 32-lane half, conflict-free (banks of ds_read_b32: (a / 4) % 32);
//     scan        wave 0 alone: lane l holds the masks of positions l and l + 64 in registers, and the 128 serial steps are
//                 v_readlane + scalar logic on the 128-bit kept set (keep p iff valid(p) && !(mask[p] & kept)) -- no LDS round trip
//                 and no divergence, every lane computes the same kept set.  Afterwards lane l stores its own positions, if kept,
//                 at the rank popcount(kept below it) gives, and the tail of the row is filled with -1;
//     counts      [2 i] = kept; [2 i + 1] = the pairs q < p < min(k, L) of valid entries with s(p, q) >= threshold -- the duplicate
//                 pairs the plain top-k would have shown -- a popcount over the same masks, cut to that bound, and one wave sum.
// LDS: the 64 KiB staging ring / tile + 2 KiB masks + 0.5 KiB list = 66.5 KiB, two workgroups per CU.  A list's result depends on
// its own tile alone, so it is bit-identical run to run and independent of the grid and of the chunking.
//
// Chunking.  The workspace is the image, the gather buffer and the validity masks.  dae_dedup_lists_workspace asks for min(Nr, R0)
// lists, R0 the number whose gather buffer stays within DEDUP_GATHER_BYTES; the entry accepts any workspace that holds the image
// and one list and walks the rows in chunks of as many lists as fit (never more than R0: the K loop addresses the buffer with
// 32-bit byte offsets).  The sizes, the carve with its checks and the gather launch live in dae_list_tile.h: dae_mmr.hip (dae_mmr_lists)
// runs another epilogue on the same gather buffer and the same tile.
#include "dae_list_tile.h"

#include <cmath>

namespace dae {

constexpr int DEDUP_LDS = DEDUP_TILE_BYTES + 128 * 2 * 8 + 128 * 4;

// grid = 2 R: workgroup b copies the 64 rows of half (b & 1) of list (b >> 1), 16 rows per wave, 16 bytes per lane and step
__global__ __launch_bounds__(256) void dedup_gather_kernel(const float* __restrict__ image, int Dp, int Na, const int32_t* __restrict__ lists,
                                                           int64_t ldl, int L, float* __restrict__ gathered,
                                                           unsigned long long* __restrict__ valid) {
    __shared__ int ids[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x >> 1, half = blockIdx.x & 1;
    if (tid < 64) {
        const int p = half * 64 + tid;
        int id = p < L ? lists[(int64_t)r * ldl + p] : -1;
        if (id < 0 || id >= Na) id = -1;
        ids[tid] = id;
        const unsigned long long ok = __ballot(id >= 0);
        if (tid == 0) valid[2 * (int64_t)r + half] = ok;
    }
    __syncthreads();
    const int q4 = Dp >> 2;                                     // 16-byte pieces per row
    const f32x4* src = reinterpret_cast<const f32x4*>(image);
    f32x4* dst = reinterpret_cast<f32x4*>(gathered) + ((int64_t)r * DEDUP_MAX + half * 64 + wave * 16) * q4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int e = lane; e < 16 * q4; e += 64) {
        const int row = e / q4, c = e - row * q4;
        const int id = ids[wave * 16 + row];
        dst[e] = id >= 0 ? src[(int64_t)id * q4 + c] : zero;
    }
}

int launch_list_gather(const float* image, int Dp, int Na, const int32_t* lists, int64_t ldl, int L, int64_t n, float* gathered,
                       unsigned long long* valid, hipStream_t st) {
    DAE_LAUNCH(dedup_gather_kernel, dim3((unsigned)(2 * n)), dim3(256), 0, st, image, Dp, Na, lists, ldl, L, gathered, valid);
    DAE_CHECK_LAUNCH();
    return 0;
}

struct DedupParams {
    GemmParams g;                 // one K segment: A = Bt = the gather buffer
    const int32_t* lists;         // the chunk's first list
    int64_t ldl, ldo;
    const unsigned long long* valid;   // [R][2] validity masks of the chunk's lists
    int L, k;
    float threshold;
    int32_t *out_idx, *out_pos;   // the chunk's first row
    int32_t* counts;              // [R][2]
};

// the 64-bit value lane l of the wave holds (l wave-uniform)
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
// the bits below bit n of a 128-bit set, as its two words
__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1ull; }

__global__ __launch_bounds__(GEMM_THREADS, 2) void dedup_tiles_kernel(DedupParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* tile = reinterpret_cast<float*>(lds);
    uint64_t* masks = reinterpret_cast<uint64_t*>(lds + DEDUP_TILE_BYTES);      // [128][2]
    int* ids = reinterpret_cast<int*>(masks + 256);                             // [128] the list (outside the staging ring)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    if (tid < 128) ids[tid] = tid < p.L ? p.lists[(int64_t)r * p.ldl + tid] : -1;
    f32x16 acc[2][2];
    gemm_mainloop<float, 2>(p.g, r, r, 0, p.g.ktiles_total, lds, acc);
    __syncthreads();                                            // every wave is done with the staging ring
    acc_to_tile(acc, tile, wave >> 1, wave & 1, lane >> 5, lane & 31);
    __syncthreads();
    // (one address for the whole workgroup; through lane_u64 the two words are scalars, and with them the whole scan below)
    const uint64_t v0 = lane_u64(p.valid[2 * (int64_t)r], 0), v1 = lane_u64(p.valid[2 * (int64_t)r + 1], 0);
    {
        // word h of row pp's mask; the columns of word h are 64 h .. 64 h + 63, of which only those below pp count
        const int pp = tid & 127, h = tid >> 7;
        const uint64_t vh = h ? v1 : v0;
        const float T = p.threshold;
        uint64_t m = 0;
        if (64 * h < pp) {
            const float* row = tile + pp * BN + 64 * h;
#pragma unroll 8
            for (int i = 0; i < 64; ++i) {
                const int q = (i + pp) & 63;                    // the skewed start: see the head of the file
                m |= (uint64_t)(row[q] >= T) << q;
            }
            m &= vh & low_bits(pp - 64 * h);
        }
        masks[2 * pp + h] = m;
    }
    __syncthreads();
    if (wave != 0) return;
    // ---- the serial scan, in wave 0's registers ----
    const uint64_t a0 = masks[2 * lane], a1 = masks[2 * lane + 1];                 // position lane
    const uint64_t b0 = masks[2 * (lane + 64)], b1 = masks[2 * (lane + 64) + 1];   // position lane + 64
    uint64_t k0 = 0, k1 = 0;                                    // the kept set
    int n = 0;
    const int L = p.L, k = p.k;
    for (int q = 0; q < min(L, 64) && n < k; ++q) {
        const uint64_t m0 = lane_u64(a0, q);                    // (a position < 64 has no bits in word 1)
        if (((v0 >> q) & 1) && !(m0 & k0)) { k0 |= 1ull << q; ++n; }
    }
    for (int q = 64; q < L && n < k; ++q) {
        const uint64_t m0 = lane_u64(b0, q - 64), m1 = lane_u64(b1, q - 64);
        if (((v1 >> (q - 64)) & 1) && !((m0 & k0) | (m1 & k1))) { k1 |= 1ull << (q - 64); ++n; }
    }
    // ---- the row: lane l stores positions l and l + 64, if kept, at their rank among the kept ----
    int32_t* oi = p.out_idx + (int64_t)r * p.ldo;
    int32_t* op = p.out_pos + (int64_t)r * p.ldo;
    const uint64_t below = (1ull << lane) - 1ull;
    if ((k0 >> lane) & 1) { const int at = __popcll(k0 & below); oi[at] = ids[lane]; op[at] = lane; }
    if ((k1 >> lane) & 1) { const int at = __popcll(k0) + __popcll(k1 & below); oi[at] = ids[lane + 64]; op[at] = lane + 64; }
    for (int t = n + lane; t < k; t += 64) { oi[t] = -1; op[t] = -1; }
    // ---- the duplicate pairs among the first min(k, L) positions ----
    const int bound = min(k, L);
    const uint64_t lo0 = low_bits(bound), lo1 = low_bits(bound - 64);
    int dup = 0;
    if (lane < bound && ((v0 >> lane) & 1)) dup += __popcll(a0 & lo0) + __popcll(a1 & lo1);
    if (lane + 64 < bound && ((v1 >> lane) & 1)) dup += __popcll(b0 & lo0) + __popcll(b1 & lo1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dup += __shfl_xor(dup, o, 64);
    if (lane == 0) { p.counts[2 * (int64_t)r] = n; p.counts[2 * (int64_t)r + 1] = dup; }
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_dedup_lists_workspace(int32_t Nr, int32_t Na, int32_t D, int32_t L) { return list_workspace_bytes(Nr, Na, D, L); }

extern "C" int dae_dedup_lists(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t norm, int32_t metric, const int32_t* lists,
                               int64_t ldl, int32_t Nr, int32_t L, int32_t k, float threshold, int32_t* out_idx, int32_t* out_pos,
                               int64_t ldo, int32_t* counts, void* workspace, uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(E && lists && out_idx && out_pos && counts && workspace && Na > 0 && D > 0 && Nr > 0 && lde >= D, "dedup_lists: bad input");
    DAE_CHECK_ARG(L >= 1 && L <= DEDUP_MAX, "dedup_lists: L must be in 1..%d (got %d)", DEDUP_MAX, L);
    DAE_CHECK_ARG(k >= 1 && k <= L, "dedup_lists: k must be in 1..L = %d (got %d)", L, k);
    DAE_CHECK_ARG(norm >= 0 && norm <= 3, "dedup_lists: norm must be 0 (none), 1 (l1), 2 (l2) or 3 (max)");
    DAE_CHECK_ARG(metric == 0 || metric == 1, "dedup_lists: metric must be 0 (cosine) or 1 (linear kernel)");
    DAE_CHECK_ARG(!std::isnan(threshold), "dedup_lists: threshold is NaN");
    DAE_CHECK_ARG(ldl >= L, "dedup_lists: ldl (%lld) must be >= L (%d)", (long long)ldl, L);
    DAE_CHECK_ARG(ldo >= k, "dedup_lists: ldo (%lld) must be >= k (%d)", (long long)ldo, k);
    ListWorkspace w;
    if (int rc = list_workspace_carve("dedup_lists", Na, D, Nr, workspace, workspace_bytes, w)) return rc;
    const int64_t Dp = w.Dp, R = w.R;
    hipStream_t st = (hipStream_t)stream;
    float* image = w.image; float* gathered = w.gathered;
    unsigned long long* valid = w.valid;
    if (int rc = launch_row_normalize(E, lde, Na, D, norm, metric == 0 ? 1 : 0, image, Dp, (int)Dp, (int)w.Nap, st)) return rc;
    DedupParams p;
    memset(&p, 0, sizeof(p));
    sweep_gemm_params(gathered, gathered, Dp, p.g);
    p.ldl = ldl; p.ldo = ldo; p.valid = valid; p.L = L; p.k = k; p.threshold = threshold;
    for (int64_t i0 = 0; i0 < Nr; i0 += R) {
        const int64_t n = Nr - i0 < R ? Nr - i0 : R;
        p.lists = lists + i0 * ldl;
        p.out_idx = out_idx + i0 * ldo; p.out_pos = out_pos + i0 * ldo; p.counts = counts + 2 * i0;
        if (int rc = launch_list_gather(image, (int)Dp, Na, p.lists, ldl, L, n, gathered, valid, st)) return rc;
        if (int rc = sweep_launch<dedup_tiles_kernel>(n, DEDUP_LDS, DEDUP_LDS, st, p)) return rc;
    }
    return 0;
}
