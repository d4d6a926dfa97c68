// dae_covisit.hip -- the co-visitation item-to-item recommender (dae_covisit_neighbors / dae_covisit_recommend): "readers of this
// article also read ...", from co-clicks alone, without an Na x Na matrix.  The rules are stated in include/dae_hip.h.
//
// Build (dae_covisit_neighbors): emit -> sort -> run-length -> select.
//   covisit_emit_kernel     one thread per click event p of a user: counts the records of its pairs (p, q), p < q <= p + w, with
//                           different items; one wave prefix sum and ONE integer atomicAdd on the 64-bit cursor per wave, then every
//                           lane stores its records -- the key a << bits | b per record -- from its own offset (the append of
//                           dae_pairs.hip).  The append order depends on scheduling; the records carry no payload, so the sorted
//                           array does not.  A record is stored only below the capacity, which is the host's upper bound of the
//                           record count (dae_covisit_record_bound): the buffers cannot be overrun.
//   covisit_clicks_kernel   clicks[a] by integer atomics (exact), a workgroup's hot articles summed in LDS first.
//   rocprim::radix_sort_keys (double buffer, the 2 * bits key bits in use), rocprim::run_length_encode: distinct pairs and counts.
//   covisit_rows_kernel     row_start[a] = the first distinct pair of article a (binary search), a = 0 .. Na.
//   covisit_select_short_kernel / covisit_select_long_kernel: the K best of every row under pair_key (dae_score_sweep.h: ordered score
//                           bits high, complemented index low -- a total order).  Rows are skewed (a hub has thousands of distinct
//                           neighbours, the median tens), so no wave ever walks a long row alone:
//                             degree <= 256: one wave per row, four rows per workgroup; the row's keys go to LDS once and every entry
//                               counts the keys above it -- its rank IS its output slot, no sort;
//                             degree  > 256: one workgroup per row, passes of 256 entries against a running K-best in LDS (kept in
//                               rank order, double buffered); an entry below the K-th best is dropped by one compare, and a pass in
//                               which no entry survives that compare costs one vote.
// Recommend (dae_covisit_recommend): one workgroup per user; see covisit_recommend_kernel.
// No floating-point atomics; every float is a fixed chain of single fp32 roundings (__fmul_rn, /, sqrtf, __fadd_rn), so the outputs
// are bit-identical run to run and equal the NumPy restatement (tests/covisit_reference.py).
#include "dae_score_sweep.h"

#include <rocprim/rocprim.hpp>

namespace dae {

constexpr int CV_THREADS = 256;
constexpr int CV_SHORT = 256;        // the longest row one wave selects
constexpr int CV_MAXK = 128;
constexpr int CV_MAXLAST = 32;
constexpr int CV_MAXENT = CV_MAXK * CV_MAXLAST;      // 4096 entries per user

// number of bits that hold an article index 0 .. Na - 1 (at least 1)
static inline int covisit_bits(int Na) {
    int b = 1;
    while (b < 31 && (1ll << b) < (long long)Na) ++b;
    return b;
}

// first user row whose end lies beyond event e: the user of event e
__device__ __forceinline__ int covisit_user_of(const int64_t* indptr, int M, int64_t e) {
    int lo = 0, hi = M;                                 // the answer u has indptr[u] <= e < indptr[u + 1]
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (indptr[m + 1] <= e) lo = m + 1; else hi = m;
    }
    return lo;
}

// clicks[a] += the occurrences of a.  Click logs are Zipf-like: a hub article takes a few percent of all clicks, and that many atomics
// on one address serialise.  A workgroup therefore first adds its CV_CLICK_EVENTS events into a direct-mapped table in LDS (slot
// a mod 1024, claimed by the first article that asks for it; an article that finds its slot taken goes to memory directly) and
// flushes the table with one atomic per slot in use.  Integer sums: exact, whatever the order.
constexpr int CV_CLICK_SLOTS = 1024;
constexpr int CV_CLICK_EVENTS = 16 * CV_THREADS;
__global__ __launch_bounds__(CV_THREADS) void covisit_clicks_kernel(const int32_t* __restrict__ items, int64_t nnz, int Na,
                                                                    int32_t* __restrict__ clicks) {
    __shared__ int tag[CV_CLICK_SLOTS], val[CV_CLICK_SLOTS];
    for (int h = threadIdx.x; h < CV_CLICK_SLOTS; h += CV_THREADS) { tag[h] = -1; val[h] = 0; }
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * CV_CLICK_EVENTS;
    for (int i = threadIdx.x; i < CV_CLICK_EVENTS; i += CV_THREADS) {
        const int64_t e = e0 + i;
        if (e >= nnz) break;
        const int a = items[e];
        if (a < 0 || a >= Na) continue;
        const int h = a & (CV_CLICK_SLOTS - 1);
        const int old = atomicCAS(&tag[h], -1, a);
        if (old == -1 || old == a) atomicAdd(&val[h], 1);
        else atomicAdd(&clicks[a], 1);
    }
    __syncthreads();
    for (int h = threadIdx.x; h < CV_CLICK_SLOTS; h += CV_THREADS)
        if (val[h] > 0) atomicAdd(&clicks[tag[h]], val[h]);
}

__global__ __launch_bounds__(CV_THREADS) void covisit_emit_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ items,
                                                                  int M, int64_t nnz, int Na, int window, int both, int bits,
                                                                  unsigned long long capacity, unsigned long long* cursor,
                                                                  uint64_t* __restrict__ keys) {
    const int64_t e = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int n = 0, a = -1;
    int64_t q1 = 0;                                     // the partners of event e are the events e < q <= q1
    if (e < nnz) {
        a = items[e];
        if (a >= 0 && a < Na) {
            const int u = covisit_user_of(indptr, M, e);
            const int64_t end = indptr[u + 1];
            q1 = e + window < end - 1 ? e + window : end - 1;
            for (int64_t q = e + 1; q <= q1; ++q) {
                const int b = items[q];
                n += (b != a && b >= 0 && b < Na) ? 1 : 0;
            }
            if (both) n *= 2;
        } else a = -1;
    }
    if (__ballot(n != 0) == 0) return;
    int incl = n;                                       // inclusive prefix sum of the lanes' counts
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    unsigned long long base = 0;
    if (lane == 63) base = atomicAdd(cursor, (unsigned long long)incl);
    base = __shfl(base, 63, 64);
    unsigned long long slot = base + (unsigned long long)(incl - n);
    if (n == 0) return;
    for (int64_t q = e + 1; q <= q1; ++q) {
        const int b = items[q];
        if (b == a || b < 0 || b >= Na) continue;
        if (slot < capacity) keys[slot] = ((uint64_t)(uint32_t)a << bits) | (uint32_t)b;
        ++slot;
        if (both) {
            if (slot < capacity) keys[slot] = ((uint64_t)(uint32_t)b << bits) | (uint32_t)a;
            ++slot;
        }
    }
}

__global__ __launch_bounds__(CV_THREADS) void covisit_rows_kernel(const uint64_t* __restrict__ uniq, const unsigned long long* __restrict__ n_pairs,
                                                                  int Na, int bits, int64_t* __restrict__ row_start) {
    const int64_t a = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    if (a > Na) return;
    const uint64_t want = (uint64_t)a << bits;
    int64_t lo = 0, hi = (int64_t)*n_pairs;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (uniq[m] < want) lo = m + 1; else hi = m;
    }
    row_start[a] = lo;
}

struct CovisitSelect {
    const uint64_t* uniq;         // distinct pairs a << bits | b, ascending
    const uint32_t* runs;         // and their counts
    const int64_t* row_start;     // [Na + 1]
    const int32_t* clicks;        // [Na]
    int Na, bits, cosine, K;
    int32_t* nbr; float* sim; int32_t* cnt; int64_t ld;
    int32_t* degree;
};

// the similarity of one distinct pair: fp32, one rounding per operation
__device__ __forceinline__ float covisit_sim(const CovisitSelect& p, int a, int b, uint32_t c) {
    const float fc = (float)c;
    if (!p.cosine) return fc;
    return fc / sqrtf(__fmul_rn((float)p.clicks[a], (float)p.clicks[b]));
}

// rows of at most CV_SHORT distinct neighbours: wave w of the workgroup selects row blockIdx.x * 4 + w
__global__ __launch_bounds__(CV_THREADS) void covisit_select_short_kernel(CovisitSelect p) {
    __shared__ uint64_t keys[4][CV_SHORT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t a64 = (int64_t)blockIdx.x * 4 + wave;
    const bool live = a64 < p.Na;
    const int a = (int)a64;
    int64_t r0 = 0;
    int n = 0;
    if (live) {
        r0 = p.row_start[a];
        const int64_t deg = p.row_start[a + 1] - r0;
        if (lane == 0) p.degree[a] = (int32_t)deg;
        n = deg <= CV_SHORT ? (int)deg : -1;            // -1: a long row, the other kernel's
    }
    const uint64_t bmask = (1ull << p.bits) - 1;
    uint32_t c4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = lane + 64 * r;
        c4[r] = 0;
        if (j < n) {
            const int b = (int)(p.uniq[r0 + j] & bmask);
            c4[r] = p.runs[r0 + j];
            keys[wave][j] = pair_key(covisit_sim(p, a, b, c4[r]), b);
        }
    }
    __syncthreads();
    if (n < 0) return;
    const int64_t out = (int64_t)a * p.ld;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = lane + 64 * r;
        if (j >= n) continue;
        const uint64_t mine = keys[wave][j];
        int rank = 0;
        for (int i = 0; i < n; ++i) rank += keys[wave][i] > mine ? 1 : 0;
        if (rank < p.K) {
            p.nbr[out + rank] = pair_key_index(mine);
            p.sim[out + rank] = pair_key_score(mine);
            p.cnt[out + rank] = (int32_t)c4[r];
        }
    }
    if (live)
        for (int t = n + lane; t < p.K; t += 64) { p.nbr[out + t] = -1; p.sim[out + t] = 0.f; p.cnt[out + t] = 0; }
}

// rows of more than CV_SHORT distinct neighbours: one workgroup per row
__global__ __launch_bounds__(CV_THREADS) void covisit_select_long_kernel(CovisitSelect p) {
    __shared__ uint64_t best[2][CV_MAXK];               // the running K-best in rank order, double buffered
    __shared__ uint32_t bcnt[2][CV_MAXK];
    __shared__ uint64_t fresh[CV_THREADS];              // the pass's entries that beat the K-th best (0: none)
    const int a = blockIdx.x, tid = threadIdx.x;
    const int64_t r0 = p.row_start[a];
    const int64_t deg = p.row_start[a + 1] - r0;
    if (deg <= CV_SHORT) return;
    const uint64_t bmask = (1ull << p.bits) - 1;
    int cur = 0, nb = 0;                                // the buffer in use and its fill, uniform over the workgroup
    for (int64_t j0 = 0; j0 < deg; j0 += CV_THREADS) {
        const int64_t j = j0 + tid;
        uint64_t mine = 0;
        uint32_t c = 0;
        if (j < deg) {
            const int b = (int)(p.uniq[r0 + j] & bmask);
            c = p.runs[r0 + j];
            mine = pair_key(covisit_sim(p, a, b, c), b);
            if (nb == p.K && mine < best[cur][p.K - 1]) mine = 0;
        }
        fresh[tid] = mine;
        if (!__syncthreads_or(mine != 0)) continue;     // (the barrier also orders the writes of fresh)
        const int nxt = cur ^ 1;
        // an old entry keeps its place among the old ones and moves down by the fresh entries above it
        if (tid < nb) {
            const uint64_t old = best[cur][tid];
            int rank = tid;
            for (int i = 0; i < CV_THREADS; ++i) rank += fresh[i] > old ? 1 : 0;
            if (rank < p.K) { best[nxt][rank] = old; bcnt[nxt][rank] = bcnt[cur][tid]; }
        }
        int added = 0;
        if (mine != 0) {
            int rank = 0;
            for (int i = 0; i < nb; ++i) rank += best[cur][i] > mine ? 1 : 0;
            for (int i = 0; i < CV_THREADS; ++i) rank += fresh[i] > mine ? 1 : 0;
            if (rank < p.K) { best[nxt][rank] = mine; bcnt[nxt][rank] = c; }
            added = 1;
        }
        const int total = nb + __syncthreads_count(added);
        nb = total < p.K ? total : p.K;
        cur = nxt;
    }
    const int64_t out = (int64_t)a * p.ld;
    for (int t = tid; t < p.K; t += CV_THREADS) {
        const bool has = t < nb;
        p.nbr[out + t] = has ? pair_key_index(best[cur][t]) : -1;
        p.sim[out + t] = has ? pair_key_score(best[cur][t]) : 0.f;
        p.cnt[out + t] = has ? (int32_t)bcnt[cur][t] : 0;
    }
}

// a log without a record: every row is a tail
__global__ __launch_bounds__(CV_THREADS) void covisit_empty_kernel(int Na, int K, int32_t* nbr, float* sim, int32_t* cnt, int64_t ld,
                                                                   int32_t* degree) {
    const int64_t t = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x;
    if (t >= (int64_t)Na * K) return;
    const int64_t a = t / K, s = t % K;
    nbr[a * ld + s] = -1; sim[a * ld + s] = 0.f; cnt[a * ld + s] = 0;
    if (s == 0) degree[a] = 0;
}

__global__ void covisit_totals_kernel(const unsigned long long* cursor, const unsigned long long* n_pairs, int64_t* totals) {
    totals[0] = cursor ? (int64_t)*cursor : 0;
    totals[1] = n_pairs ? (int64_t)*n_pairs : 0;
}

// ---- recommend ----
struct CovisitRecommend {
    const int32_t* nbr; const float* sim; int64_t ld; int Na, K;
    const int64_t* indptr; const int32_t* items;
    const int64_t* seen_indptr; const int32_t* seen_items;
    const int32_t* win_lo; const int32_t* win_hi;
    const float* age_weight;
    int last, k, cap;             // cap: the power of two that holds last * K entries -- the size of the key array
    int32_t* idx; float* score; int64_t ldo;
};

// bitonic sort of keys[0, S), S a power of two, by the whole workgroup; ends with a barrier
template <bool DESC>
__device__ __forceinline__ void covisit_sort(uint64_t* keys, int S) {
    for (int k2 = 2; k2 <= S; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (S >> 1); t += CV_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const bool up = ((i & k2) == 0) != DESC;
                const uint64_t x = keys[i], y = keys[i + j];
                if ((x > y) == up) { keys[i] = y; keys[i + j] = x; }
            }
            __syncthreads();
        }
}

// One workgroup per user.  Dynamic LDS: keys uint64[cap] then prod float[last * K] -- 8 * 4096 + 4 * 4096 = 48 KiB at the limits.
//   1. the sources are the user's last min(last, L) clicks, oldest first; wave w counts the filled slots of the rows of the sources
//      w, w + 4, ..., thread 0 turns the counts into offsets, and the same walk stores entry (source o, slot t) compactly as the key
//      candidate << 12 | o * K + t, with its product __fmul_rn(age_weight, sim) in prod[o * K + t];
//   2. a bitonic sort of the next power of two of the user's own entry count orders them by (candidate, source order);
//   3. the thread of a run's first entry sums the run in that order with __fadd_rn, looks the candidate up in the user's seen list
//      (binary search) and in the window, and keeps the survivor's pair_key in registers (0 otherwise) until every thread has read
//      its run; the keys then replace the entries;
//   4. a second bitonic sort, descending, and the first k keys are the list.
__global__ __launch_bounds__(CV_THREADS) void covisit_recommend_kernel(CovisitRecommend p) {
    extern __shared__ __attribute__((aligned(16))) char cv_lds[];
    uint64_t* keys = (uint64_t*)cv_lds;
    float* prod = (float*)(cv_lds + (size_t)p.cap * 8);
    __shared__ int src_item[CV_MAXLAST], src_fill[CV_MAXLAST], src_off[CV_MAXLAST + 1];
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t h0 = p.indptr[u];
    const int64_t L = p.indptr[u + 1] - h0;
    const int ns = (int)(L < p.last ? L : p.last);
    if (tid < ns) {
        const int x = p.items[h0 + L - ns + tid];
        src_item[tid] = (x >= 0 && x < p.Na) ? x : -1;
    }
    __syncthreads();
    for (int o = wave; o < ns; o += 4) {
        const int x = src_item[o];
        int f = 0;
        if (x >= 0)
            for (int t0 = 0; t0 < p.K; t0 += 64) {
                const int t = t0 + lane;
                const int c = t < p.K ? p.nbr[(int64_t)x * p.ld + t] : -1;
                f += __popcll(__ballot(c >= 0 && c < p.Na));
            }
        if (lane == 0) src_fill[o] = f;
    }
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int o = 0; o < ns; ++o) { src_off[o] = s; s += src_fill[o]; }
        src_off[ns] = s;
    }
    __syncthreads();
    const int E = src_off[ns];
    int32_t* oi = p.idx + (int64_t)u * p.ldo;
    float* os = p.score + (int64_t)u * p.ldo;
    if (E == 0) {
        for (int t = tid; t < p.k; t += CV_THREADS) { oi[t] = -1; os[t] = -INFINITY; }
        return;
    }
    int S = 1;
    while (S < E) S <<= 1;
    for (int o = wave; o < ns; o += 4) {
        const int x = src_item[o];
        if (x < 0) continue;
        const float w = p.age_weight[ns - 1 - o];
        int pos = src_off[o];
        for (int t0 = 0; t0 < p.K; t0 += 64) {
            const int t = t0 + lane;
            const int c = t < p.K ? p.nbr[(int64_t)x * p.ld + t] : -1;
            const bool ok = c >= 0 && c < p.Na;
            const uint64_t m = __ballot(ok);
            if (ok) {
                const int e = o * p.K + t;
                keys[pos + __popcll(m & ((1ull << lane) - 1))] = ((uint64_t)(uint32_t)c << 12) | (uint32_t)e;
                prod[e] = __fmul_rn(w, p.sim[(int64_t)x * p.ld + t]);
            }
            pos += __popcll(m);
        }
    }
    for (int i = E + tid; i < S; i += CV_THREADS) keys[i] = ~0ull;
    __syncthreads();
    covisit_sort<false>(keys, S);
    uint64_t res[CV_MAXENT / CV_THREADS];
    const int64_t x0 = p.seen_indptr[u];
    const int32_t* X = p.seen_items + x0;
    const int nx = (int)(p.seen_indptr[u + 1] - x0);
    int lo = 0, hi = p.Na;
    if (p.win_lo) { lo = p.win_lo[u]; hi = p.win_hi[u]; }
#pragma unroll
    for (int r = 0; r < CV_MAXENT / CV_THREADS; ++r) {
        const int i = tid + r * CV_THREADS;
        res[r] = 0;
        if (i >= E) continue;
        const int c = (int)(keys[i] >> 12);
        if (i > 0 && (int)(keys[i - 1] >> 12) == c) continue;           // not the first entry of its run
        float acc = 0.f;
        for (int j = i; j < E && (int)(keys[j] >> 12) == c; ++j) acc = __fadd_rn(acc, prod[keys[j] & 4095u]);
        if (c < lo || c >= hi) continue;
        const int at = lower_bound_i32(X, nx, c);
        if (at < nx && X[at] == c) continue;
        res[r] = pair_key(acc, c);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < CV_MAXENT / CV_THREADS; ++r) {
        const int i = tid + r * CV_THREADS;
        if (i < S) keys[i] = res[r];
    }
    __syncthreads();
    covisit_sort<true>(keys, S);
    for (int t = tid; t < p.k; t += CV_THREADS) {
        const uint64_t x = t < S ? keys[t] : 0;
        oi[t] = x ? pair_key_index(x) : -1;
        os[t] = x ? pair_key_score(x) : -INFINITY;
    }
}

// ---- host ----
// scratch of the two rocprim calls over n records of `bits2` key bits (they run one after the other: the larger of the two)
static bool covisit_temp_bytes(size_t n, int bits2, size_t& bytes) {
    uint64_t* k = nullptr;
    uint32_t* c = nullptr;
    unsigned long long* r = nullptr;
    rocprim::double_buffer<uint64_t> db(k, k);
    size_t sort_bytes = 0, rle_bytes = 0;
    if (rocprim::radix_sort_keys(nullptr, sort_bytes, db, n, 0, bits2, (hipStream_t)0) != hipSuccess) return false;
    if (rocprim::run_length_encode(nullptr, rle_bytes, k, n, k, c, r, (hipStream_t)0) != hipSuccess) return false;
    bytes = sort_bytes > rle_bytes ? sort_bytes : rle_bytes;
    return true;
}
// the part of the workspace whose size follows from the arguments alone: two key buffers, the run counts, the row starts, scalars
static uint64_t covisit_fixed_bytes(uint64_t bound, int Na) {
    return 2 * al256(bound * 8) + al256(bound * 4) + al256(((uint64_t)Na + 1) * 8) + 256;
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_covisit_record_bound(const int64_t* indptr_host, int32_t M, int32_t window, int32_t both) {
    if (!indptr_host || M <= 0 || window < 1) return 0;
    uint64_t total = 0;
    const uint64_t w = (uint64_t)window;
    for (int32_t u = 0; u < M; ++u) {
        const int64_t L = indptr_host[u + 1] - indptr_host[u];
        if (L < 2) continue;
        const uint64_t r = (uint64_t)L - 1;               // sum over p of min(w, L - 1 - p) = sum over r' = 0 .. L - 1 of min(w, r')
        total += r <= w ? r * (r + 1) / 2 : w * (w + 1) / 2 + (r - w) * w;
    }
    return both ? 2 * total : total;
}

extern "C" uint64_t dae_covisit_neighbors_workspace(uint64_t record_bound, int32_t Na, int32_t K) {
    if (Na < 1 || K < 1 || K > CV_MAXK || record_bound >= (1ull << 31)) return 0;
    if (record_bound == 0) return 0;                      // nothing to sort: the call needs no workspace
    size_t temp = 0;
    if (!covisit_temp_bytes((size_t)record_bound, 2 * covisit_bits(Na), temp)) return 0;
    return covisit_fixed_bytes(record_bound, Na) + al256(temp);
}

extern "C" int dae_covisit_neighbors(const int64_t* indptr, const int32_t* items, const int64_t* indptr_host, int32_t M, int64_t nnz,
                                     int32_t Na, int32_t window, int32_t both, int32_t normalize, int32_t K, int32_t* nbr, float* sim,
                                     int32_t* cnt, int64_t ld, int32_t* degree, int32_t* clicks, int64_t* totals, void* workspace,
                                     uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(nbr && sim && cnt && degree && clicks && totals, "covisit_neighbors: an output is NULL");
    DAE_CHECK_ARG(K >= 1 && K <= CV_MAXK, "covisit_neighbors: K (%d) must be in 1..%d", K, CV_MAXK);
    DAE_CHECK_ARG(window >= 1, "covisit_neighbors: window (%d) must be at least 1", window);
    DAE_CHECK_ARG(Na >= 1 && 2 * covisit_bits(Na) <= 62, "covisit_neighbors: Na (%d) must be at least 1 and fit 31 bits", Na);
    DAE_CHECK_ARG(ld >= K, "covisit_neighbors: ld (%lld) must be >= K (%d)", (long long)ld, K);
    DAE_CHECK_ARG(M >= 0 && nnz >= 0, "covisit_neighbors: M (%d) and nnz (%lld) must not be negative", M, (long long)nnz);
    DAE_CHECK_ARG(both == 0 || both == 1, "covisit_neighbors: both (%d) must be 0 or 1", both);
    DAE_CHECK_ARG(normalize == 0 || normalize == 1, "covisit_neighbors: normalize (%d) must be 0 (none) or 1 (cosine)", normalize);
    DAE_CHECK_ARG(M == 0 || indptr_host, "covisit_neighbors: indptr_host is NULL");
    DAE_CHECK_ARG(M == 0 || nnz == 0 || (indptr && items), "covisit_neighbors: indptr / items is NULL");
    DAE_CHECK_ARG(M == 0 || (indptr_host[0] == 0 && indptr_host[M] == nnz), "covisit_neighbors: indptr_host must start at 0 and end at nnz");
    DAE_CHECK_ARG((nnz + CV_THREADS - 1) / CV_THREADS < (1ll << 31), "covisit_neighbors: %lld events exceed the grid", (long long)nnz);
    const uint64_t bound = (M > 0 && nnz > 0) ? dae_covisit_record_bound(indptr_host, M, window, both) : 0;
    DAE_CHECK_ARG(bound < (1ull << 31), "covisit_neighbors: up to %llu records; one call takes fewer than 2^31 (build from fewer users)",
                  (unsigned long long)bound);
    const int bits = covisit_bits(Na);
    if (bound > 0) {
        // the record buffers are sized by the bound: checked before anything is launched, so they cannot be overrun
        DAE_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0, "covisit_neighbors: the workspace must be 256-byte aligned");
        DAE_CHECK_ARG(workspace_bytes >= covisit_fixed_bytes(bound, Na),
                      "covisit_neighbors: workspace too small (%llu bytes, the buffers of %llu records alone need %llu)",
                      (unsigned long long)workspace_bytes, (unsigned long long)bound, (unsigned long long)covisit_fixed_bytes(bound, Na));
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned egrid = (unsigned)((nnz + CV_THREADS - 1) / CV_THREADS);
    const int64_t cells = (int64_t)Na * K;
    DAE_CHECK_ARG((cells + CV_THREADS - 1) / CV_THREADS < (1ll << 31), "covisit_neighbors: Na x K exceeds the grid");
    unsigned long long records = 0;
    unsigned long long* cursor = nullptr;
    unsigned long long* n_pairs = nullptr;
    uint64_t *keys_a = nullptr, *keys_b = nullptr;
    uint32_t* runs = nullptr;
    int64_t* row_start = nullptr;
    void* temp = nullptr;
    size_t temp_bytes = 0;
    if (bound > 0) {
        DAE_CHECK_ARG(covisit_temp_bytes((size_t)bound, 2 * bits, temp_bytes), "covisit_neighbors: the size query of rocprim failed");
        DAE_CHECK_ARG(workspace_bytes >= covisit_fixed_bytes(bound, Na) + al256(temp_bytes),
                      "covisit_neighbors: workspace too small (%llu bytes, %llu records need %llu)", (unsigned long long)workspace_bytes,
                      (unsigned long long)bound, (unsigned long long)(covisit_fixed_bytes(bound, Na) + al256(temp_bytes)));
        char* w = (char*)workspace;
        keys_a = (uint64_t*)w;              w += al256(bound * 8);
        keys_b = (uint64_t*)w;              w += al256(bound * 8);
        runs = (uint32_t*)w;                w += al256(bound * 4);
        row_start = (int64_t*)w;            w += al256(((uint64_t)Na + 1) * 8);
        cursor = (unsigned long long*)w;    n_pairs = cursor + 1;   w += 256;
        temp = w;
        DAE_CHECK_HIP(hipMemsetAsync(cursor, 0, 16, st));
    }
    DAE_CHECK_HIP(hipMemsetAsync(clicks, 0, (size_t)Na * 4, st));
    if (nnz > 0 && M > 0) {
        DAE_LAUNCH(covisit_clicks_kernel, dim3((unsigned)((nnz + CV_CLICK_EVENTS - 1) / CV_CLICK_EVENTS)), dim3(CV_THREADS), 0, st, items, nnz,
                   (int)Na, clicks);
        DAE_CHECK_LAUNCH();
    }
    if (bound > 0) {
        DAE_LAUNCH(covisit_emit_kernel, dim3(egrid), dim3(CV_THREADS), 0, st, indptr, items, (int)M, nnz, (int)Na, (int)window, (int)both,
                   bits, (unsigned long long)bound, cursor, keys_a);
        DAE_CHECK_LAUNCH();
        DAE_CHECK_HIP(hipMemcpyAsync(&records, cursor, 8, hipMemcpyDeviceToHost, st));
        DAE_CHECK_HIP(hipStreamSynchronize(st));
        DAE_CHECK_ARG(records <= bound, "covisit_neighbors: the device log emitted %llu records, the host indptr bounds them by %llu",
                      records, (unsigned long long)bound);
    }
    if (records == 0) {
        DAE_LAUNCH(covisit_empty_kernel, dim3((unsigned)((cells + CV_THREADS - 1) / CV_THREADS)), dim3(CV_THREADS), 0, st, (int)Na, (int)K, nbr,
                   sim, cnt, ld, degree);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(covisit_totals_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)nullptr, (const unsigned long long*)nullptr,
                   totals);
        DAE_CHECK_LAUNCH();
        return 0;
    }
    rocprim::double_buffer<uint64_t> db(keys_a, keys_b);
    size_t tb = temp_bytes;
    DAE_CHECK_HIP(rocprim::radix_sort_keys(temp, tb, db, (size_t)records, 0, 2 * bits, st));
    uint64_t* sorted = db.current();
    uint64_t* uniq = db.alternate();
    tb = temp_bytes;
    DAE_CHECK_HIP(rocprim::run_length_encode(temp, tb, sorted, (size_t)records, uniq, runs, n_pairs, st));
    DAE_LAUNCH(covisit_rows_kernel, dim3((unsigned)(((int64_t)Na + 1 + CV_THREADS - 1) / CV_THREADS)), dim3(CV_THREADS), 0, st,
               (const uint64_t*)uniq, (const unsigned long long*)n_pairs, (int)Na, bits, row_start);
    DAE_CHECK_LAUNCH();
    CovisitSelect p;
    p.uniq = uniq; p.runs = runs; p.row_start = row_start; p.clicks = clicks;
    p.Na = Na; p.bits = bits; p.cosine = normalize; p.K = K;
    p.nbr = nbr; p.sim = sim; p.cnt = cnt; p.ld = ld; p.degree = degree;
    DAE_LAUNCH(covisit_select_short_kernel, dim3((unsigned)(((int64_t)Na + 3) / 4)), dim3(CV_THREADS), 0, st, p);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(covisit_select_long_kernel, dim3((unsigned)Na), dim3(CV_THREADS), 0, st, p);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(covisit_totals_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)cursor, (const unsigned long long*)n_pairs, totals);
    DAE_CHECK_LAUNCH();
    DAE_CHECK_HIP(hipStreamSynchronize(st));              // the workspace may be released on return
    return 0;
}

extern "C" int dae_covisit_recommend(const int32_t* nbr, const float* sim, int64_t ld, int32_t Na, int32_t K, const int64_t* indptr,
                                     const int32_t* items, int32_t M, const int64_t* seen_indptr, const int32_t* seen_items,
                                     const int32_t* win_lo, const int32_t* win_hi, const float* age_weight, int32_t last, int32_t k,
                                     int32_t* idx, float* score, int64_t ldo, void* stream) {
    DAE_CHECK_ARG(nbr && sim, "covisit_recommend: the table is NULL");
    DAE_CHECK_ARG(K >= 1 && K <= CV_MAXK, "covisit_recommend: K (%d) must be in 1..%d", K, CV_MAXK);
    DAE_CHECK_ARG(Na >= 1, "covisit_recommend: Na (%d) must be at least 1", Na);
    DAE_CHECK_ARG(ld >= K, "covisit_recommend: ld (%lld) must be >= K (%d)", (long long)ld, K);
    DAE_CHECK_ARG(last >= 1 && last <= CV_MAXLAST, "covisit_recommend: last (%d) must be in 1..%d", last, CV_MAXLAST);
    DAE_CHECK_ARG(k >= 1 && k <= CV_MAXK, "covisit_recommend: k (%d) must be in 1..%d", k, CV_MAXK);
    DAE_CHECK_ARG(ldo >= k, "covisit_recommend: ldo (%lld) must be >= k (%d)", (long long)ldo, k);
    DAE_CHECK_ARG(M >= 0, "covisit_recommend: M (%d) must not be negative", M);
    DAE_CHECK_ARG((win_lo == nullptr) == (win_hi == nullptr), "covisit_recommend: win_lo and win_hi go together");
    if (M == 0) return 0;
    DAE_CHECK_ARG(indptr && items && seen_indptr && seen_items && age_weight && idx && score,
                  "covisit_recommend: indptr / items / seen_indptr / seen_items / age_weight / idx / score is NULL");
    CovisitRecommend p;
    p.nbr = nbr; p.sim = sim; p.ld = ld; p.Na = Na; p.K = K;
    p.indptr = indptr; p.items = items; p.seen_indptr = seen_indptr; p.seen_items = seen_items;
    p.win_lo = win_lo; p.win_hi = win_hi; p.age_weight = age_weight;
    p.last = last; p.k = k;
    p.cap = 1;
    while (p.cap < last * K) p.cap <<= 1;
    p.idx = idx; p.score = score; p.ldo = ldo;
    const size_t lds = (size_t)p.cap * 8 + (size_t)last * K * 4;      // keys, then products: 48 KiB at last = 32, K = 128
    hipStream_t st = (hipStream_t)stream;
    DAE_LAUNCH(covisit_recommend_kernel, dim3((unsigned)M), dim3(CV_THREADS), lds, st, p);
    DAE_CHECK_LAUNCH();
    return 0;
}
