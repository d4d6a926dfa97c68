// dae_vectorize.hip -- from a count matrix to the training input, on CSR rows (dae_csr_column_stats, dae_csr_select_columns,
// dae_tfidf_transform): what sklearn's CountVectorizer._limit_features and TfidfTransformer do to a bag of words, without
// densifying or copying it to the host.  CSR conventions of dae_sweep_image_csr: int64 indptr (offsets relative to the arrays
// passed), int32 column ids ascending and unique within a row, fp32 values or NULL (every stored entry is 1); an entry whose
// column lies outside [0, F) is dropped and counted.
//
// All three are streaming kernels on very uneven rows (1 .. a few thousand entries): the per-row kernels give every row ONE wave,
// four rows to a 256-thread workgroup, and the wave walks its row in passes of 64 entries, so consecutive lanes read consecutive
// entries and a 5-entry row costs one partly filled pass, not a workgroup.  No LDS: the only reduction is a wave's.
//   column_stats   entry-parallel (a row's boundaries do not matter): df[c] += 1, tf[c] += (integer) count, 64-bit integer atomics
//                  -- exact and independent of scheduling.  The two counters of the host record are summed per wave first.
//   select_columns count per row -> rocprim::exclusive_scan -> fill; a lane's output slot inside a pass is the number of kept
//                  entries in the lanes below it (ballot + popcount), so a row keeps its ascending order.
//   tfidf          pass 1 folds lane l's entries l, l + 64, ... in ascending order into an fp64 sum, the wave sums by a fixed
//                  butterfly: the norm depends on the row alone, not on the launch or on other rows.  Pass 2 recomputes v (the row
//                  is in cache) and writes fl32(v / norm), so out_values may be values.
#include "dae_score_sweep.h"      // al256

#include <rocprim/rocprim.hpp>

#include <cmath>

namespace dae {

constexpr int VEC_ROWS = 4;                 // rows (waves) per workgroup
constexpr int VEC_STATS_BLOCKS = 2048;      // grid of the entry-parallel kernel (grid-stride)

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// counts[0] += entries whose value is not an integer in [0, 2^24], counts[1] += entries dropped for their column
__global__ __launch_bounds__(256) void csr_column_stats_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                               const float* __restrict__ values, int rows, int F,
                                                               unsigned long long* __restrict__ df, unsigned long long* __restrict__ tf,
                                                               unsigned long long* __restrict__ counts) {
    const int64_t q0 = indptr[0], q1 = indptr[rows];
    unsigned long long bad = 0, dropped = 0;
    for (int64_t q = q0 + (int64_t)blockIdx.x * 256 + threadIdx.x; q < q1; q += (int64_t)gridDim.x * 256) {
        const int c = indices[q];
        if (c < 0 || c >= F) { ++dropped; continue; }
        atomicAdd(df + c, 1ull);                                    // an explicit zero is a stored entry: it counts
        const float v = values ? values[q] : 1.f;
        if (v >= 0.f && v <= 16777216.f && v == truncf(v)) {
            if (v != 0.f) atomicAdd(tf + c, (unsigned long long)v);
        } else {
            ++bad;                                                  // NaN lands here too; nothing is added to tf
        }
    }
    bad = wave_sum_u64(bad);
    dropped = wave_sum_u64(dropped);
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(counts, bad);
        if (dropped) atomicAdd(counts + 1, dropped);
    }
}

// cnt[i] = kept entries of row i (i < rows), cnt[rows] = 0 (the scan's last output is the total); counts[0] += dropped entries
__global__ __launch_bounds__(256) void csr_select_count_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int rows,
                                                               int F, const int32_t* __restrict__ remap, int64_t* __restrict__ cnt,
                                                               unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * VEC_ROWS + (threadIdx.x >> 6);      // 64-bit: rows may be close to 2^31
    if (i > rows) return;
    if (i == rows) {
        if (lane == 0) cnt[rows] = 0;
        return;
    }
    const int64_t p0 = indptr[i], p1 = indptr[i + 1];
    unsigned kept = 0, dropped = 0;
    for (int64_t q = p0 + lane; q < p1; q += 64) {
        const int c = indices[q];
        if (c < 0 || c >= F) ++dropped;
        else if (remap[c] >= 0) ++kept;
    }
    kept = wave_sum_u32(kept);
    dropped = wave_sum_u32(dropped);
    if (lane == 0) {
        cnt[i] = kept;
        if (dropped) atomicAdd(counts, (unsigned long long)dropped);
    }
}

// out_indptr holds the scanned counts; the caller has checked out_indptr[rows] <= capacity, so no slot lies past the buffers
__global__ __launch_bounds__(256) void csr_select_fill_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                              const float* __restrict__ values, int rows, int F,
                                                              const int32_t* __restrict__ remap, const int64_t* __restrict__ out_indptr,
                                                              int32_t* __restrict__ out_indices, float* __restrict__ out_values) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * VEC_ROWS + (threadIdx.x >> 6);      // 64-bit: rows may be close to 2^31
    if (i >= rows) return;
    const int64_t p0 = indptr[i], p1 = indptr[i + 1];
    int64_t o = out_indptr[i];
    const int64_t o_end = out_indptr[i + 1];
    for (int64_t base = p0; base < p1; base += 64) {                // the bound is wave-uniform: every lane takes part in the ballot
        const int64_t q = base + lane;
        int m = -1;
        if (q < p1) {
            const int c = indices[q];
            if (c >= 0 && c < F) m = remap[c];
        }
        const unsigned long long mask = __ballot(m >= 0);
        const int64_t slot = o + __popcll(mask & ((1ull << lane) - 1ull));
        if (m >= 0 && slot < o_end) {
            out_indices[slot] = m;
            if (out_values) out_values[slot] = values ? values[q] : 1.f;
        }
        o += __popcll(mask);
    }
}

// v of one stored entry: fl32(t * idf[c]), t = count or fl32(1 + log((double) count)); a dropped entry is 0 and takes no part
__device__ __forceinline__ float tfidf_value(const int32_t* __restrict__ indices, const float* values, const float* __restrict__ idf,
                                             int F, int sublinear, int64_t q, bool& dropped) {
    const int c = indices[q];
    dropped = c < 0 || c >= F;
    if (dropped) return 0.f;
    float t = values ? values[q] : 1.f;
    if (sublinear) t = (float)(1.0 + log((double)t));
    return idf ? t * idf[c] : t;
}

__global__ __launch_bounds__(256) void tfidf_transform_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                              const float* values, int rows, int F, const float* __restrict__ idf,
                                                              int sublinear, int norm, float* out_values,
                                                              unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * VEC_ROWS + (threadIdx.x >> 6);      // 64-bit: rows may be close to 2^31
    if (i >= rows) return;
    const int64_t p0 = indptr[i], p1 = indptr[i + 1];
    unsigned n_dropped = 0;
    bool dropped;
    double scale = 0.0;                                             // 0: the row keeps its v
    if (norm != 0) {
        double a = 0.0;
        for (int64_t q = p0 + lane; q < p1; q += 64) {
            const double v = (double)tfidf_value(indices, values, idf, F, sublinear, q, dropped);
            a += norm == 1 ? fabs(v) : v * v;                       // v * v is exact in fp64
        }
        a = wave_sum_f64(a);
        if (norm == 2) a = sqrt(a);
        if (a != 0.0 && isfinite(a)) scale = a;
    }
    for (int64_t q = p0 + lane; q < p1; q += 64) {
        const float v = tfidf_value(indices, values, idf, F, sublinear, q, dropped);
        n_dropped += dropped ? 1u : 0u;
        out_values[q] = scale != 0.0 ? (float)((double)v / scale) : v;
    }
    n_dropped = wave_sum_u32(n_dropped);
    if (lane == 0 && n_dropped) atomicAdd(counts, (unsigned long long)n_dropped);
}

static int csr_checks(const char* who, const void* indptr, const void* indices, int32_t rows, int32_t F, const void* workspace,
                      uint64_t workspace_bytes, uint64_t need) {
    DAE_CHECK_ARG(indptr && indices, "%s: indptr / indices are NULL (values may be: a binary matrix)", who);
    DAE_CHECK_ARG(rows > 0 && F > 0, "%s: rows and F must be positive (got %d, %d)", who, rows, F);
    DAE_CHECK_ARG(workspace && ((uintptr_t)workspace % 256) == 0, "%s: workspace must be non-NULL and 256-byte aligned", who);
    DAE_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%llu < %llu bytes)", who, (unsigned long long)workspace_bytes,
                  (unsigned long long)need);
    return 0;
}

static unsigned row_blocks(int64_t rows) { return (unsigned)((rows + VEC_ROWS - 1) / VEC_ROWS); }

static size_t select_scan_temp_bytes(size_t n) {
    size_t bytes = 0;
    int64_t* p = nullptr;
    (void)rocprim::exclusive_scan(nullptr, bytes, p, p, (int64_t)0, n, rocprim::plus<int64_t>(), (hipStream_t)0);
    return bytes;
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_csr_column_stats_workspace(void) { return 256; }

extern "C" int dae_csr_column_stats(const int64_t* indptr, const int32_t* indices, const float* values, int32_t rows, int32_t F, int64_t* df,
                                    int64_t* tf, uint64_t* counts2_host, void* workspace, uint64_t workspace_bytes, void* stream) {
    if (int rc = csr_checks("csr_column_stats", indptr, indices, rows, F, workspace, workspace_bytes, dae_csr_column_stats_workspace())) return rc;
    DAE_CHECK_ARG(df && tf && counts2_host, "csr_column_stats: df / tf / counts2_host are NULL");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* counts = (unsigned long long*)workspace;
    DAE_CHECK_HIP(hipMemsetAsync(counts, 0, 16, st));
    DAE_LAUNCH(csr_column_stats_kernel, dim3(VEC_STATS_BLOCKS), dim3(256), 0, st, indptr, indices, values, (int)rows, (int)F,
               (unsigned long long*)df, (unsigned long long*)tf, counts);
    DAE_CHECK_LAUNCH();
    unsigned long long host[2] = {0, 0};
    DAE_CHECK_HIP(hipMemcpyAsync(host, counts, 16, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    counts2_host[0] = host[0];
    counts2_host[1] = host[1];
    return 0;
}

extern "C" uint64_t dae_csr_select_columns_workspace(int32_t rows) {
    if (rows <= 0) return 0;
    // the per-row counts (+ the total's slot), the scan's scratch, the dropped counter
    return al256(((uint64_t)rows + 1) * 8) + al256(select_scan_temp_bytes((size_t)rows + 1)) + 256;
}

extern "C" int dae_csr_select_columns(const int64_t* indptr, const int32_t* indices, const float* values, int32_t rows, int32_t F,
                                      const int32_t* remap, int64_t* out_indptr, int32_t* out_indices, float* out_values, uint64_t capacity,
                                      int64_t* out2_host, void* workspace, uint64_t workspace_bytes, void* stream) {
    if (int rc = csr_checks("csr_select_columns", indptr, indices, rows, F, workspace, workspace_bytes, dae_csr_select_columns_workspace(rows)))
        return rc;
    DAE_CHECK_ARG(remap && out_indptr && out2_host, "csr_select_columns: remap / out_indptr / out2_host are NULL");
    DAE_CHECK_ARG(capacity == 0 || out_indices, "csr_select_columns: out_indices is NULL with capacity %llu", (unsigned long long)capacity);
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)rows + 1;
    size_t temp_bytes = select_scan_temp_bytes(n);
    char* w = (char*)workspace;
    int64_t* cnt = (int64_t*)w;                     w += al256(n * 8);
    void* temp = w;                                 w += al256(temp_bytes);
    unsigned long long* counts = (unsigned long long*)w;
    DAE_CHECK_HIP(hipMemsetAsync(counts, 0, 8, st));
    DAE_LAUNCH(csr_select_count_kernel, dim3(row_blocks((int64_t)rows + 1)), dim3(256), 0, st, indptr, indices, (int)rows, (int)F, remap, cnt, counts);
    DAE_CHECK_LAUNCH();
    DAE_CHECK_HIP(rocprim::exclusive_scan(temp, temp_bytes, cnt, out_indptr, (int64_t)0, n, rocprim::plus<int64_t>(), st));
    long long nnz = 0;
    unsigned long long dropped = 0;
    DAE_CHECK_HIP(hipMemcpyAsync(&nnz, out_indptr + rows, 8, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipMemcpyAsync(&dropped, counts, 8, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    out2_host[0] = nnz;
    out2_host[1] = (int64_t)dropped;
    DAE_CHECK_ARG((uint64_t)nnz <= capacity, "csr_select_columns: %lld kept entries exceed the capacity %llu (nothing was written to "
                  "out_indices / out_values)", nnz, (unsigned long long)capacity);
    if (nnz == 0) return 0;
    DAE_LAUNCH(csr_select_fill_kernel, dim3(row_blocks(rows)), dim3(256), 0, st, indptr, indices, values, (int)rows, (int)F, remap,
               (const int64_t*)out_indptr, out_indices, out_values);
    DAE_CHECK_LAUNCH();
    return 0;
}

extern "C" uint64_t dae_tfidf_transform_workspace(void) { return 256; }

extern "C" int dae_tfidf_transform(const int64_t* indptr, const int32_t* indices, const float* values, int32_t rows, int32_t F, const float* idf,
                                   int32_t sublinear, int32_t norm, float* out_values, uint64_t* dropped_host, void* workspace,
                                   uint64_t workspace_bytes, void* stream) {
    if (int rc = csr_checks("tfidf_transform", indptr, indices, rows, F, workspace, workspace_bytes, dae_tfidf_transform_workspace())) return rc;
    DAE_CHECK_ARG(out_values && dropped_host, "tfidf_transform: out_values / dropped_host are NULL");
    DAE_CHECK_ARG(sublinear == 0 || sublinear == 1, "tfidf_transform: sublinear must be 0 or 1");
    DAE_CHECK_ARG(norm >= 0 && norm <= 2, "tfidf_transform: norm must be 0 (none), 1 (l1) or 2 (l2)");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* counts = (unsigned long long*)workspace;
    DAE_CHECK_HIP(hipMemsetAsync(counts, 0, 8, st));
    DAE_LAUNCH(tfidf_transform_kernel, dim3(row_blocks(rows)), dim3(256), 0, st, indptr, indices, values, (int)rows, (int)F, idf, (int)sublinear,
               (int)norm, out_values, counts);
    DAE_CHECK_LAUNCH();
    unsigned long long dropped = 0;
    DAE_CHECK_HIP(hipMemcpyAsync(&dropped, counts, 8, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    *dropped_host = dropped;
    return 0;
}
