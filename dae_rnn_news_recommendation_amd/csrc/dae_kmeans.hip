// dae_kmeans.hip -- Lloyd iterations of spherical k-means on the device: dae_kmeans_assign, dae_kmeans_update.
//
// Both entries read sweep images (dae_sweep_image.hip): zero-padded fp32 [pad128(rows) x pad128(D)], built by the caller -- the row
// image once per fit, the centroid image before every assignment.
//
// Assignment (dae_kmeans_assign): the score sweep of dae_score_sweep.h with the smallest epilogue there is, an arg-max.
// kmeans_assign_tiles_kernel: grid = (query tiles) x (centroid slices), 256 threads (4 waves).  A workgroup walks the 128-column
// centroid tiles of its slice with gemm_mainloop<float, 2>; the score tile never leaves the accumulators.  In the accumulator layout
// of dae_gemm_tile.h a lane of wave (wm, wn) holds, of every tile, the rows wm * 64 + acc_row(mt, r, g) at the two columns
// wn * 64 + acc_col(nt, c): 32 rows x 2 columns.  So 32 (score, column) pairs per lane (64 VGPRs) carry the best of a row's columns
// this lane has seen; a lane's columns ascend from tile to tile and from nt = 0 to 1, so a strict > keeps the lowest column of equal
// scores (-0 == +0 under >, as under pair_key).  A padded column j >= K scores 0 and is gated out BEFORE the compare: it would win
// every row whose real scores are all negative.  After the last tile the pairs become 64-bit pair_keys (score descending, then column
// ascending: a total order), every row is reduced over the 32 lanes of its half wave by shuffles, and the two wn waves meet in 2 KiB
// of LDS over the dead staging ring.  With one slice the workgroup writes label and score itself; with several it writes one key per
// (slice, row) and kmeans_assign_finish_kernel takes the maximum.  (238 VGPRs, no scratch, two workgroups per CU; measured against
// the LDS-tile epilogue of top-k at k = 1 on the same prebuilt images, and against the route a user had, in profiles/kmeans_bench.txt.)
// Non-finite scores: a row whose scores are all -inf or NaN gets label -1 (dae_topk_similarity returns a column for -inf and lets a
// NaN win); on finite scores the two agree bit for bit.
// The host record: each query tile folds the fp64 sum of its 128 scores and the count of rows whose label differs from prev_labels
// in a fixed tree (tile_fold), kmeans_assign_fold_kernel adds the tile partials in a fixed order, and the entry downloads the two.
//
// Update (dae_kmeans_update): rocprim::radix_sort_pairs sorts (label, row id) by label -- a stable sort, so `order` is by (label,
// row id) and rows outside [0, K) (key K) form its tail; offsets / counts are binary searches in the sorted labels.  Every cluster is
// cut into segments of at most 256 consecutive members of `order`.  kmeans_partial_kernel, one workgroup per segment, sums the
// segment's image rows ascending in fp64, thread t owning the columns t, t + 256, ...; kmeans_centroid_kernel, one workgroup per
// cluster, adds the segment partials ascending (s_d), folds n2 = sum of s_d^2 in a fixed tree and writes fl32(s_d / sqrt(n2)).  An
// empty cluster, or one with n2 == 0, keeps its row.  No floating-point atomic anywhere: the result is bit-identical run to run, and
// every word of the workspace is written before it is read.
#include "dae_score_sweep.h"

#include <rocprim/rocprim.hpp>

namespace dae {

constexpr int KM_SLOTS = 512;              // workgroups in flight on the MI355X: 256 CUs x 2
constexpr int KM_MAX_SPLITS = 32;
constexpr int KM_LDS = lds_bytes_for(2);   // the staging ring; the epilogue's 4 KiB lie over it
constexpr int KM_SEG = 256;                // members per segment of the update

struct KmAssignParams {
    GemmParams g;                 // one K segment: A = row image, Bt = centroid image
    int N, K, Nqp, splits, ctiles;
    const int32_t* prev;          // [N] labels to count changes against, or NULL (every row counts)
    int32_t* labels;              // [N]
    float* scores;                // [N]
    uint64_t* part;               // [splits][Nqp] best key per (slice, row); splits > 1 only
    double* psum;                 // [Nqp / 128] fp64 score sum per query tile
    long long* pchg;              // [Nqp / 128] changed labels per query tile
};

// row gi's result from its best key: label and score are written, (s, chg) is its share of the host record
__device__ __forceinline__ void km_row_finish(const KmAssignParams& p, int gi, uint64_t key, double& s, long long& chg) {
    s = 0.0; chg = 0;
    if (gi >= p.N) return;
    const int32_t lab = key ? pair_key_index(key) : -1;           // key 0: no finite score (a NaN row)
    const float sc = key ? pair_key_score(key) : -__builtin_inff();
    p.labels[gi] = lab; p.scores[gi] = sc;
    s = (double)sc;
    chg = p.prev ? (p.prev[gi] != lab ? 1 : 0) : 1;
}

// the sums of a query tile's 128 (s, chg) in a fixed tree; every thread of the workgroup calls it (fs / fc: 128 items of LDS each)
__device__ __forceinline__ void km_tile_fold(double s, long long chg, double* fs, long long* fc, int tid, int qt, double* psum, long long* pchg) {
    if (tid < 128) { fs[tid] = s; fc[tid] = chg; }
    __syncthreads();
    for (int h = 64; h > 0; h >>= 1) {
        if (tid < h) { fs[tid] += fs[tid + h]; fc[tid] += fc[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) { psum[qt] = fs[0]; pchg[qt] = fc[0]; }
}

__global__ __launch_bounds__(GEMM_THREADS, 2) void kmeans_assign_tiles_kernel(KmAssignParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.x % p.splits, qt = blockIdx.x / p.splits;
    const int ct0 = (int)((int64_t)p.ctiles * split / p.splits), ct1 = (int)((int64_t)p.ctiles * (split + 1) / p.splits);
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    float bs[2][16];                                            // the best score of each of the lane's 32 rows so far
    int bj[2][16];                                              // and its column; -1: none yet
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { bs[mt][r] = -__builtin_inff(); bj[mt][r] = -1; }
    for (int ct = ct0; ct < ct1; ++ct) {
        f32x16 acc[2][2];
        gemm_mainloop<float, 2>(p.g, qt, ct, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int j = ct * BN + wn * 64 + acc_col(nt, c);
            if (j < p.K) {                                      // a padded column never competes
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float s = acc[mt][nt][r];
                        if (s > bs[mt][r]) { bs[mt][r] = s; bj[mt][r] = j; }
                    }
            }
        }
        __syncthreads();                                        // every wave is done with the staging ring
    }
    uint64_t* ex = reinterpret_cast<uint64_t*>(lds);            // [2 wn][128 rows] keys
    double* fs = reinterpret_cast<double*>(lds + 2048);
    long long* fc = reinterpret_cast<long long*>(lds + 3072);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            uint64_t key = bj[mt][r] >= 0 ? pair_key(bs[mt][r], bj[mt][r]) : 0;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {                  // the 32 lanes of a half wave hold one row
                const uint64_t other = __shfl_xor((unsigned long long)key, o, 64);
                key = other > key ? other : key;
            }
            if (c == 0) ex[wn * 128 + wm * 64 + acc_row(mt, r, g)] = key;
        }
    __syncthreads();
    uint64_t key = 0;
    if (tid < 128) key = ex[tid] > ex[128 + tid] ? ex[tid] : ex[128 + tid];
    const int gi = qt * BM + tid;
    if (p.splits > 1) {
        if (tid < 128) p.part[(int64_t)split * p.Nqp + gi] = key;
        return;
    }
    double s = 0.0; long long chg = 0;
    if (tid < 128) km_row_finish(p, gi, key, s, chg);
    km_tile_fold(s, chg, fs, fc, tid, qt, p.psum, p.pchg);
}

// splits > 1: the best of a row's slices; one workgroup of 128 threads per query tile
__global__ __launch_bounds__(128) void kmeans_assign_finish_kernel(KmAssignParams p) {
    __shared__ double fs[128];
    __shared__ long long fc[128];
    const int tid = threadIdx.x, qt = blockIdx.x, gi = qt * BM + tid;
    uint64_t key = 0;
    for (int s = 0; s < p.splits; ++s) {
        const uint64_t x = p.part[(int64_t)s * p.Nqp + gi];
        key = x > key ? x : key;
    }
    double s = 0.0; long long chg = 0;
    km_row_finish(p, gi, key, s, chg);
    km_tile_fold(s, chg, fs, fc, tid, qt, p.psum, p.pchg);
}

// the tile partials in a fixed order: thread t adds the tiles t, t + 256, ... ascending, then a fixed tree; out2: sum, changed
__global__ __launch_bounds__(256) void kmeans_assign_fold_kernel(const double* __restrict__ psum, const long long* __restrict__ pchg, int tiles,
                                                                 double* __restrict__ out2) {
    __shared__ double fs[256];
    __shared__ long long fc[256];
    const int tid = threadIdx.x;
    double s = 0.0; long long n = 0;
    for (int t = tid; t < tiles; t += 256) { s += psum[t]; n += pchg[t]; }
    fs[tid] = s; fc[tid] = n;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) { fs[tid] += fs[tid + h]; fc[tid] += fc[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) { out2[0] = fs[0]; out2[1] = (double)fc[0]; }
}

static int km_assign_splits(int N, int K) { return sweep_splits(N, K, KM_SLOTS, KM_MAX_SPLITS); }

// ---- update ----
// sort keys: the label, or K for a row that takes no part; the payload is the row id
__global__ __launch_bounds__(256) void kmeans_keys_kernel(const int32_t* __restrict__ labels, int N, int K, uint32_t* __restrict__ keys,
                                                          int32_t* __restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t l = (uint32_t)labels[i];
    keys[i] = l < (uint32_t)K ? l : (uint32_t)K;
    vals[i] = i;
}

__device__ __forceinline__ int lower_bound_u32(const uint32_t* X, int n, uint32_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (X[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}

// offsets[c] = first position of label c in the sorted labels (c <= K), counts[c] = members of cluster c (c < K)
__global__ __launch_bounds__(256) void kmeans_offsets_kernel(const uint32_t* __restrict__ keys_s, int N, int K, int64_t* __restrict__ offsets,
                                                             int32_t* __restrict__ counts) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > K) return;
    const int lo = lower_bound_u32(keys_s, N, (uint32_t)c);
    offsets[c] = lo;
    if (c < K) counts[c] = lower_bound_u32(keys_s, N, (uint32_t)c + 1u) - lo;
}

// segoff[c] = segments of the clusters before c (exclusive scan of ceil(counts / KM_SEG)), c <= K; one workgroup
__global__ __launch_bounds__(256) void kmeans_segments_kernel(const int32_t* __restrict__ counts, int K, int32_t* __restrict__ segoff) {
    __shared__ int tot[257];
    const int tid = threadIdx.x;
    const int chunk = (K + 255) / 256, c0 = min(tid * chunk, K), c1 = min(c0 + chunk, K);
    int n = 0;
    for (int c = c0; c < c1; ++c) n += (counts[c] + KM_SEG - 1) / KM_SEG;
    tot[tid + 1] = n;
    __syncthreads();
    if (tid == 0) {
        tot[0] = 0;
        for (int t = 0; t < 256; ++t) tot[t + 1] += tot[t];
    }
    __syncthreads();
    n = tot[tid];
    for (int c = c0; c < c1; ++c) { segoff[c] = n; n += (counts[c] + KM_SEG - 1) / KM_SEG; }
    if (tid == 255) segoff[K] = tot[256];
}

// one workgroup per segment: the fp64 sums of its members' image rows, members ascending; part [segments][Dp]
__global__ __launch_bounds__(256) void kmeans_partial_kernel(const float* __restrict__ Xi, int Dp, int K, const int32_t* __restrict__ order,
                                                             const int64_t* __restrict__ offsets, const int32_t* __restrict__ segoff,
                                                             double* __restrict__ part) {
    __shared__ int mem[KM_SEG];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= segoff[K]) return;
    int lo = 0, hi = K + 1;                                     // the cluster: the last c with segoff[c] <= b
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (segoff[m] <= b) lo = m + 1; else hi = m;
    }
    const int c = lo - 1;
    const int64_t start = offsets[c] + (int64_t)(b - segoff[c]) * KM_SEG;
    const int n = (int)min((int64_t)KM_SEG, offsets[c + 1] - start);
    if (tid < n) mem[tid] = order[start + tid];
    __syncthreads();
    for (int col = tid; col < Dp; col += 256) {
        double a = 0.0;
        for (int m = 0; m < n; ++m) a += (double)Xi[(int64_t)mem[m] * Dp + col];
        part[(int64_t)b * Dp + col] = a;
    }
}

// one workgroup per cluster: s_d = its segment partials added ascending, n2 = sum of s_d^2 (thread t over its columns ascending,
// then a fixed tree), centroid = fl32(s_d / sqrt(n2)); flag[c] = 1 for a cluster with members whose n2 is 0 (its row is kept)
__global__ __launch_bounds__(256) void kmeans_centroid_kernel(const double* __restrict__ part, int Dp, int D, const int32_t* __restrict__ segoff,
                                                              float* __restrict__ centroids, int64_t ldc, int32_t* __restrict__ flag) {
    __shared__ double fs[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int s0 = segoff[c], s1 = segoff[c + 1];
    if (s0 == s1) return;                                       // an empty cluster keeps its row
    double n2 = 0.0;
    for (int col = tid; col < Dp; col += 256) {
        double s = 0.0;
        for (int sg = s0; sg < s1; ++sg) s += part[(int64_t)sg * Dp + col];
        n2 += s * s;
    }
    fs[tid] = n2;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) fs[tid] += fs[tid + h];
        __syncthreads();
    }
    n2 = fs[0];
    if (tid == 0) flag[c] = n2 == 0.0 ? 1 : 0;
    if (n2 == 0.0) return;
    const double nrm = sqrt(n2);
    for (int col = tid; col < D; col += 256) {
        double s = 0.0;
        for (int sg = s0; sg < s1; ++sg) s += part[(int64_t)sg * Dp + col];
        centroids[(int64_t)c * ldc + col] = (float)(s / nrm);
    }
}

// out4: rows left out, clusters without members, clusters with members whose n2 is 0 (flag; NULL: not computed), segments; one workgroup
__global__ __launch_bounds__(256) void kmeans_update_record_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ flag,
                                                                   const int64_t* __restrict__ offsets, const int32_t* __restrict__ segoff,
                                                                   int N, int K, double* __restrict__ out4) {
    __shared__ int fe[256], fz[256];
    const int tid = threadIdx.x;
    int e = 0, z = 0;
    for (int c = tid; c < K; c += 256) {
        if (counts[c] == 0) ++e;
        else if (flag && flag[c]) ++z;
    }
    fe[tid] = e; fz[tid] = z;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) { fe[tid] += fe[tid + h]; fz[tid] += fz[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) {
        out4[0] = (double)((int64_t)N - offsets[K]);
        out4[1] = (double)fe[0];
        out4[2] = (double)fz[0];
        out4[3] = (double)segoff[K];
    }
}

// bits of the sort keys 0 .. K
static int km_end_bit(int K) {
    int b = 1;
    while (b < 32 && (1ll << b) <= (long long)K) ++b;
    return b;
}
// the scratch of the sort (rocprim sizes it for the current device's configuration); false when the query fails
static bool km_sort_temp_bytes(size_t n, int K, size_t& bytes) {
    bytes = 0;
    uint32_t* k = nullptr;
    int32_t* v = nullptr;
    return rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, n, 0, km_end_bit(K), (hipStream_t)0) == hipSuccess;
}
static int64_t km_max_segments(int N, int K) { return ((int64_t)N + KM_SEG - 1) / KM_SEG + K; }

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_kmeans_assign_workspace(int32_t N, int32_t K) {
    if (N <= 0 || K <= 0) return 0;
    const uint64_t Nqp = pad128(N), s = km_assign_splits(N, K);
    return al256(s * Nqp * 8) + 2 * al256(Nqp / BM * 8) + 256;
}

extern "C" int dae_kmeans_assign(const float* Xi, int32_t N, const float* Ci, int32_t K, int32_t D, const int32_t* prev_labels,
                                 int32_t* labels, float* scores, double* out_host, void* workspace, uint64_t workspace_bytes,
                                 void* stream) {
    DAE_CHECK_ARG(Xi && Ci && labels && scores && out_host && workspace, "kmeans_assign: Xi / Ci / labels / scores / out_host / workspace are NULL");
    DAE_CHECK_ARG(N > 0 && K > 0 && D > 0, "kmeans_assign: N, K and D must be positive (got %d, %d, %d)", N, K, D);
    SweepOperands o;
    if (int rc = sweep_prepare_images("kmeans_assign", Xi, N, Ci, K, D, workspace, workspace_bytes, dae_kmeans_assign_workspace(N, K), o)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int splits = km_assign_splits(N, K);
    const int64_t qtiles = o.Nqp / BM;
    KmAssignParams p;
    memset(&p, 0, sizeof(p));
    p.g = o.g;
    p.N = N; p.K = K; p.Nqp = (int)o.Nqp; p.splits = splits; p.ctiles = (int)(o.Ncp / BN);
    p.prev = prev_labels; p.labels = labels; p.scores = scores;
    char* w = o.rest;
    p.part = (uint64_t*)w;        w += al256((uint64_t)splits * o.Nqp * 8);
    p.psum = (double*)w;          w += al256(qtiles * 8);
    p.pchg = (long long*)w;       w += al256(qtiles * 8);
    double* out2 = (double*)w;
    if (int rc = sweep_launch<kmeans_assign_tiles_kernel>(qtiles * splits, KM_LDS, KM_LDS, st, p)) return rc;
    if (splits > 1) {
        DAE_LAUNCH(kmeans_assign_finish_kernel, dim3((unsigned)qtiles), dim3(128), 0, st, p);
        DAE_CHECK_LAUNCH();
    }
    DAE_LAUNCH(kmeans_assign_fold_kernel, dim3(1), dim3(256), 0, st, p.psum, p.pchg, (int)qtiles, out2);
    DAE_CHECK_LAUNCH();
    double h[2] = {0.0, 0.0};
    DAE_CHECK_HIP(hipMemcpyAsync(h, out2, 16, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    out_host[0] = h[0]; out_host[1] = h[1]; out_host[2] = (double)(qtiles * splits); out_host[3] = (double)splits;
    return 0;
}

extern "C" uint64_t dae_kmeans_update_workspace(int32_t N, int32_t K, int32_t D) {
    if (N <= 0 || K <= 0 || D <= 0) return 0;
    size_t temp_bytes = 0;
    if (!km_sort_temp_bytes((size_t)N, K, temp_bytes)) return 0;      // dae_kmeans_update then reports the failed query
    // unsorted and sorted labels, row ids, sort scratch, segment offsets, flags, segment partials, the record
    return 3 * al256((uint64_t)N * 4) + al256(temp_bytes) + 2 * al256(((uint64_t)K + 1) * 4) +
           al256((uint64_t)km_max_segments(N, K) * pad128(D) * 8) + 256;
}

extern "C" int dae_kmeans_update(const float* Xi, int32_t N, int32_t D, const int32_t* labels, int32_t K, float* centroids, int64_t ldc,
                                 int32_t* counts, int32_t* order, int64_t* offsets, double* out_host, void* workspace,
                                 uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(Xi && labels && counts && order && offsets && out_host && workspace,
                  "kmeans_update: Xi / labels / counts / order / offsets / out_host / workspace are NULL (centroids may be: the sort alone)");
    DAE_CHECK_ARG(N > 0 && K > 0 && D > 0, "kmeans_update: N, K and D must be positive (got %d, %d, %d)", N, K, D);
    DAE_CHECK_ARG(K < INT32_MAX, "kmeans_update: K must be below 2^31 - 1");
    DAE_CHECK_ARG(!centroids || ldc >= D, "kmeans_update: ldc (%lld) must be >= D (%d)", (long long)ldc, D);
    const int64_t Dp = pad128(D);
    DAE_CHECK_ARG(pad128(N) * Dp * 4 < (1ll << 32), "kmeans_update: an operand image exceeds 4 GiB");
    size_t temp_bytes = 0;
    DAE_CHECK_ARG(km_sort_temp_bytes((size_t)N, K, temp_bytes), "kmeans_update: the size query of rocprim::radix_sort_pairs failed");
    const uint64_t need = dae_kmeans_update_workspace(N, K, D);
    DAE_CHECK_ARG(workspace_bytes >= need, "kmeans_update: workspace too small (%llu < %llu bytes)", (unsigned long long)workspace_bytes,
                  (unsigned long long)need);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0 && ((uintptr_t)Xi % 256) == 0, "kmeans_update: workspace and image must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t maxseg = km_max_segments(N, K);
    DAE_CHECK_ARG(maxseg < (1ll << 31), "kmeans_update: %lld segments exceed the grid", (long long)maxseg);
    char* w = (char*)workspace;
    uint32_t* keys = (uint32_t*)w;        w += al256((uint64_t)N * 4);
    uint32_t* keys_s = (uint32_t*)w;      w += al256((uint64_t)N * 4);
    int32_t* vals = (int32_t*)w;          w += al256((uint64_t)N * 4);
    void* temp = w;                       w += al256(temp_bytes);
    int32_t* segoff = (int32_t*)w;        w += al256(((uint64_t)K + 1) * 4);
    int32_t* flag = (int32_t*)w;          w += al256(((uint64_t)K + 1) * 4);
    double* part = (double*)w;            w += al256((uint64_t)maxseg * Dp * 8);
    double* out4 = (double*)w;
    DAE_LAUNCH(kmeans_keys_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, labels, (int)N, (int)K, keys, vals);
    DAE_CHECK_LAUNCH();
    size_t tb = temp_bytes;
    DAE_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, keys, keys_s, vals, order, (size_t)N, 0, km_end_bit(K), st));
    DAE_LAUNCH(kmeans_offsets_kernel, dim3((unsigned)(((int64_t)K + 1 + 255) / 256)), dim3(256), 0, st, keys_s, (int)N, (int)K, offsets, counts);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(kmeans_segments_kernel, dim3(1), dim3(256), 0, st, counts, (int)K, segoff);
    DAE_CHECK_LAUNCH();
    if (centroids) {
        DAE_LAUNCH(kmeans_partial_kernel, dim3((unsigned)maxseg), dim3(256), 0, st, Xi, (int)Dp, (int)K, order, offsets, segoff, part);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(kmeans_centroid_kernel, dim3((unsigned)K), dim3(256), 0, st, part, (int)Dp, (int)D, segoff, centroids, ldc, flag);
        DAE_CHECK_LAUNCH();
    }
    DAE_LAUNCH(kmeans_update_record_kernel, dim3(1), dim3(256), 0, st, counts, centroids ? flag : (const int32_t*)nullptr, offsets, segoff, (int)N,
               (int)K, out4);
    DAE_CHECK_LAUNCH();
    double h[4] = {0.0, 0.0, 0.0, 0.0};
    DAE_CHECK_HIP(hipMemcpyAsync(h, out4, 32, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) out_host[i] = h[i];
    return 0;
}
