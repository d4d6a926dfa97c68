// dae_pairs.hip -- every pair of rows whose similarity reaches a threshold, without the N x N matrix (dae_threshold_pairs).
//
// The scores are those of dae_topk_similarity / dae_pairwise_similarity: rows normalised by row_normalize_kernel
// (dae_similarity.hip) into zero-padded fp32 operand images, products by gemm_mainloop<float, 2> (dae_gemm_tile.h) over the
// whole K range in one pass, so a score does not depend on the grid.
//
// pairs_tiles_kernel: one 128 x 128 score tile per workgroup (256 threads, 4 waves), LDS = the 64 KiB staging ring of the K
// loop, two workgroups per CU.  With the corpus being the query set itself (self mode) only the tiles on or below the diagonal
// exist in the grid: block t is tile (qt, ct) with t = qt (qt + 1) / 2 + ct, ct <= qt.  The epilogue works on the accumulators
// (the tile never passes through LDS):
//   1. every lane tests its 64 values into a 64-bit hit mask: score >= threshold (false for NaN), i < Nq, j < Nc, and j < i in
//      self mode (the strict lower triangle: every unordered pair once, never the self pair);
//   2. one ballot: a wave without a hit is done;
//   3. a wave prefix sum of the lanes' hit counts, ONE atomicAdd on the 64-bit cursor for the whole wave and tile, then every hit
//      lane stores its records -- key (uint64) i << 32 | j and the fp32 score -- from its own offset, with plain stores.
// The cursor always counts; a record is stored only while its slot is below the capacity, so the count is exact when the
// buffer is too small.  Append order depends on scheduling: when the count fits, rocprim::radix_sort_pairs orders the records by
// key (i ascending, then j ascending) and pairs_unpack_kernel splits the keys into rows / cols, which makes the result
// bit-identical run to run and independent of the grid.
#include "dae_score_sweep.h"

#include <rocprim/rocprim.hpp>

#include <cmath>

namespace dae {

constexpr int PAIRS_LDS = lds_bytes_for(2);

struct PairsParams {
    GemmParams g;                 // one K segment: A = query image, Bt = corpus image
    int Nq, Nc, self, ctiles;
    float threshold;
    unsigned long long capacity;
    unsigned long long* cursor;   // qualifying pairs so far (counts past the capacity)
    uint64_t* keys;               // [capacity] unsorted records: (uint64) i << 32 | j
    float* vals;                  // [capacity] and their scores
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void pairs_tiles_kernel(PairsParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int qt, ct;
    if (p.self) tri_tile(blockIdx.x, qt, ct);
    else { qt = blockIdx.x / p.ctiles; ct = blockIdx.x % p.ctiles; }
    f32x16 acc[2][2];
    gemm_mainloop<float, 2>(p.g, qt, ct, 0, p.g.ktiles_total, lds, acc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int i0 = qt * BM + wm * 64 + 4 * g, j0 = ct * BN + wn * 64 + c;      // the lane's first value
    const float T = p.threshold;
    // bit (mt * 2 + nt) * 16 + r of `hits`: the lane's value acc[mt][nt][r] qualifies.  Row / column of a value: acc_row /
    // acc_col of dae_score_sweep.h.  (A mask in two VGPRs rather than 64 conditions kept in SGPR pairs.)
    uint64_t hits = 0;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + acc_row(mt, r, 0), j = j0 + acc_col(nt, 0);
                const bool hit = acc[mt][nt][r] >= T && i < p.Nq && j < p.Nc && (!p.self || j < i);
                hits |= (uint64_t)hit << ((mt * 2 + nt) * 16 + r);
            }
    if (__ballot(hits != 0) == 0) return;
    const int n = __popcll(hits);
    int incl = n;                                               // inclusive prefix sum of the lanes' counts
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    unsigned long long base = 0;
    if (lane == 63) base = atomicAdd(p.cursor, (unsigned long long)incl);
    base = __shfl(base, 63, 64);
    unsigned long long slot = base + (unsigned long long)(incl - n);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((hits >> ((mt * 2 + nt) * 16 + r)) & 1) {
                    const int i = i0 + acc_row(mt, r, 0), j = j0 + acc_col(nt, 0);
                    if (slot < p.capacity) {
                        p.keys[slot] = ((uint64_t)(uint32_t)i << 32) | (uint32_t)j;
                        p.vals[slot] = acc[mt][nt][r];
                    }
                    ++slot;
                }
}

__global__ __launch_bounds__(256) void pairs_unpack_kernel(const uint64_t* __restrict__ keys, unsigned long long n,
                                                           int32_t* __restrict__ rows, int32_t* __restrict__ cols) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) {
        const uint64_t k = keys[t];
        rows[t] = (int32_t)(k >> 32);
        cols[t] = (int32_t)(uint32_t)k;
    }
}

// the row index occupies key bits 32 .. 32 + bits(Nq - 1); the sort stops there
static int pairs_end_bit(int Nq) {
    int b = 1;
    while (b < 31 && (1ll << b) < (long long)Nq) ++b;
    return 32 + b;
}
static size_t pairs_sort_temp_bytes(size_t n, int Nq) {
    size_t bytes = 0;
    uint64_t* k = nullptr;
    float* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, n, 0, pairs_end_bit(Nq), (hipStream_t)0);
    return bytes;
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_threshold_pairs_workspace(int32_t Nq, int32_t Nc, int32_t D, uint64_t capacity) {
    if (Nq <= 0 || Nc <= 0 || D <= 0) return 0;
    // operand images, unsorted keys + scores, sorted keys, sort scratch, cursor
    return sweep_images_bytes(Nq, Nc, D) + 2 * al256(capacity * 8) + al256(capacity * 4) +
           al256(capacity ? pairs_sort_temp_bytes((size_t)capacity, Nq) : 0) + 256;
}

extern "C" int dae_threshold_pairs(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                                   int32_t norm, int32_t metric, float threshold, int32_t* rows, int32_t* cols, float* scores,
                                   uint64_t capacity, uint64_t* count_host, void* workspace, uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(Q && count_host && workspace && Nq > 0 && D > 0, "threshold_pairs: bad input");
    DAE_CHECK_ARG(ldq >= D, "threshold_pairs: ldq (%lld) must be >= D (%d)", (long long)ldq, D);
    DAE_CHECK_ARG(!std::isnan(threshold), "threshold_pairs: threshold is NaN");
    DAE_CHECK_ARG(capacity == 0 || (rows && cols && scores), "threshold_pairs: rows / cols / scores are NULL with capacity %llu",
                  (unsigned long long)capacity);
    hipStream_t st = (hipStream_t)stream;
    SweepOperands o;
    if (int rc = sweep_prepare("threshold_pairs", Q, ldq, Nq, C, ldc, Nc, D, norm, metric, workspace, workspace_bytes,
                               dae_threshold_pairs_workspace(Nq, Nc, D, capacity), st, o))
        return rc;
    const size_t temp_bytes = capacity ? pairs_sort_temp_bytes((size_t)capacity, Nq) : 0;
    char* w = o.rest;
    uint64_t* keys = (uint64_t*)w;        w += al256(capacity * 8);
    uint64_t* keys_s = (uint64_t*)w;      w += al256(capacity * 8);
    float* vals = (float*)w;              w += al256(capacity * 4);
    void* temp = w;                       w += al256(temp_bytes);
    unsigned long long* cursor = (unsigned long long*)w;
    DAE_CHECK_HIP(hipMemsetAsync(cursor, 0, 8, st));
    PairsParams p;
    memset(&p, 0, sizeof(p));
    p.g = o.g;
    p.Nq = Nq; p.Nc = Nc; p.self = C ? 0 : 1; p.ctiles = (int)(o.Ncp / BN); p.threshold = threshold;
    p.capacity = capacity; p.cursor = cursor; p.keys = keys; p.vals = vals;
    const int64_t qtiles = o.Nqp / BM;
    const int64_t tiles = p.self ? qtiles * (qtiles + 1) / 2 : qtiles * p.ctiles;
    DAE_CHECK_ARG(tiles < (1ll << 31), "threshold_pairs: %lld tiles exceed the grid", (long long)tiles);
    if (int rc = sweep_launch<pairs_tiles_kernel>(tiles, PAIRS_LDS, PAIRS_LDS, st, p)) return rc;
    unsigned long long count = 0;
    DAE_CHECK_HIP(hipMemcpyAsync(&count, cursor, 8, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    *count_host = count;
    if (count == 0 || count > capacity) return 0;
    size_t tb = temp_bytes;
    DAE_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, keys, keys_s, vals, scores, (size_t)count, 0, pairs_end_bit(Nq), st));
    DAE_LAUNCH(pairs_unpack_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, keys_s, count, rows, cols);
    DAE_CHECK_LAUNCH();
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}
