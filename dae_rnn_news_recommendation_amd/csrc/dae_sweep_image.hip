// dae_sweep_image.hip -- operand images of the score sweeps, built on their own (dae_sweep_image_dense, dae_sweep_image_csr).
//
// Every sweep of dae_score_sweep.h multiplies two normalised, zero-padded fp32 images [pad128(rows) x pad128(D)].  The plain
// entries build both images inside the call from dense fp32 rows (sweep_prepare).  The entries here build ONE image of a chunk
// of rows, from dense rows (row_normalize_kernel, dae_similarity.hip) or straight from CSR rows (csr_row_normalize_kernel,
// below), so that a caller can hold a sparse matrix as CSR and sweep it a bounded number of rows at a time
// (dae_topk_images, dae_pair_hist_images; helpers.most_similar / label_similarity_stats with chunk_rows=).
//
// csr_row_normalize_kernel writes, bit for bit, the image rows row_normalize_kernel writes for the densified rows.  Thread tid of
// that kernel folds the entries j = tid (mod 256) in ascending j into a + |x|, a + x * x or fmaxf(a, |x|), a >= 0, and a zero
// entry is the identity of all three.  So: one 256-thread workgroup per row and the same block_reduce; the row passes through
// LDS in windows of CSR_WIN columns (a multiple of 256, so a column keeps its thread) -- the window is zeroed, the row's stored
// entries inside it are scattered (column ids ascending and unique: no two land on one word), and thread tid folds window words
// tid, tid + 256, ... exactly as the dense kernel folds x[j].  A window without stored entries is skipped by the folds.  The last
// pass writes (w * s1) * s2 of every window word, i.e. the dense kernel's expression on the same value, in coalesced rows.
// An entry whose column lies outside [0, D) or whose position breaks the ascending order is dropped, never written.
#include "dae_score_sweep.h"

namespace dae {

constexpr int CSR_WIN = 8192;              // columns per LDS window (32 KiB)

__global__ __launch_bounds__(256) void csr_row_normalize_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                                const float* __restrict__ values, int N, int D, int norm, int cosine,
                                                                float* __restrict__ Y, int64_t ldy, int Dp) {
    __shared__ float win[CSR_WIN];
    __shared__ float red[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    float* y = Y + (int64_t)i * ldy;
    if (i >= N) {                                       // padding rows of the operand image
        for (int j = tid; j < Dp; j += 256) y[j] = 0.f;
        return;
    }
    const int64_t p0 = indptr[i];
    const int n = (int)(indptr[i + 1] - p0);
    const int32_t* cols = indices + p0;
    const float* vals = values ? values + p0 : nullptr;
    auto block_reduce = [&](float v, bool is_max) {
        v = is_max ? wave_max(v) : wave_sum(v);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
    };
    // the stored entries [q0, q1) of the columns [base, base + CSR_WIN) as a dense window in LDS; q0 is carried from window to window
    auto fill = [&](int base, int q0, int q1) {
        __syncthreads();                                // the last reader of the window before
        for (int j = tid; j < CSR_WIN; j += 256) win[j] = 0.f;
        __syncthreads();
        for (int q = q0 + tid; q < q1; q += 256) {
            const int c = cols[q] - base;
            if (c >= 0 && c < CSR_WIN && base + c < D) win[c] = vals ? vals[q] : 1.f;
        }
        __syncthreads();
    };
    float s1 = 1.f;
    if (norm != 0) {
        float a = 0.f;
        for (int base = 0, q0 = 0; base < D && q0 < n; base += CSR_WIN) {
            const int q1 = q0 + lower_bound_i32(cols + q0, n - q0, base + CSR_WIN);
            if (q1 == q0) continue;
            fill(base, q0, q1);
            const int lim = min(CSR_WIN, D - base);
            for (int j = tid; j < lim; j += 256) {
                const float v = win[j];
                a = norm == 1 ? a + fabsf(v) : norm == 2 ? a + v * v : fmaxf(a, fabsf(v));
            }
            q0 = q1;
        }
        a = block_reduce(a, norm == 3);
        if (norm == 2) a = sqrtf(a);
        s1 = a == 0.f ? 1.f : 1.f / a;
    }
    float s2 = 1.f;
    if (cosine) {
        float a = 0.f;
        for (int base = 0, q0 = 0; base < D && q0 < n; base += CSR_WIN) {
            const int q1 = q0 + lower_bound_i32(cols + q0, n - q0, base + CSR_WIN);
            if (q1 == q0) continue;
            fill(base, q0, q1);
            const int lim = min(CSR_WIN, D - base);
            for (int j = tid; j < lim; j += 256) { const float v = win[j] * s1; a += v * v; }
            q0 = q1;
        }
        a = sqrtf(block_reduce(a, false));
        s2 = a == 0.f ? 1.f : 1.f / a;
    }
    for (int base = 0, q0 = 0; base < Dp; base += CSR_WIN) {
        const int lim = min(CSR_WIN, Dp - base);
        const int q1 = q0 < n ? q0 + lower_bound_i32(cols + q0, n - q0, base + CSR_WIN) : q0;
        if (q1 == q0) {
            for (int j = tid; j < lim; j += 256) y[base + j] = 0.f;
            continue;
        }
        fill(base, q0, q1);
        for (int j = tid; j < lim; j += 256) y[base + j] = base + j < D ? (win[j] * s1) * s2 : 0.f;
        q0 = q1;
    }
}

// what dae_sweep_image_dense and dae_sweep_image_csr check alike, in front of every HIP call
static int image_checks(const char* who, const void* image, int32_t rows, int32_t D, int32_t norm, int32_t metric, uint64_t image_bytes) {
    DAE_CHECK_ARG(rows > 0 && D > 0, "%s: rows and D must be positive (got %d, %d)", who, rows, D);
    DAE_CHECK_ARG(norm >= 0 && norm <= 3, "%s: norm must be 0 (none), 1 (l1), 2 (l2) or 3 (max)", who);
    DAE_CHECK_ARG(metric == 0 || metric == 1, "%s: metric must be 0 (cosine) or 1 (linear kernel)", who);
    DAE_CHECK_ARG(pad128(rows) * pad128(D) * 4 < (1ll << 32), "%s: an operand image exceeds 4 GiB", who);
    DAE_CHECK_ARG(image_bytes >= al256(pad128(rows) * pad128(D) * 4), "%s: image too small (%llu < %llu bytes)", who,
                  (unsigned long long)image_bytes, (unsigned long long)al256(pad128(rows) * pad128(D) * 4));
    DAE_CHECK_ARG(((uintptr_t)image % 256) == 0, "%s: image must be 256-byte aligned", who);
    return 0;
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_sweep_image_bytes(int32_t rows, int32_t D) {
    if (rows <= 0 || D <= 0) return 0;
    return al256((uint64_t)pad128(rows) * (uint64_t)pad128(D) * 4);
}

extern "C" int dae_sweep_image_dense(const float* X, int64_t ldx, int32_t rows, int32_t D, int32_t norm, int32_t metric, float* image,
                                     uint64_t image_bytes, void* stream) {
    DAE_CHECK_ARG(X && image, "sweep_image_dense: X / image are NULL");
    if (int rc = image_checks("sweep_image_dense", image, rows, D, norm, metric, image_bytes)) return rc;
    DAE_CHECK_ARG(ldx >= D, "sweep_image_dense: ldx (%lld) must be >= D (%d)", (long long)ldx, D);
    const int64_t Dp = pad128(D);
    return launch_row_normalize(X, ldx, rows, D, norm, metric == 0 ? 1 : 0, image, Dp, (int)Dp, (int)pad128(rows), (hipStream_t)stream);
}

extern "C" int dae_sweep_image_csr(const int64_t* indptr, const int32_t* indices, const float* values, int32_t rows, int32_t D,
                                   int32_t norm, int32_t metric, float* image, uint64_t image_bytes, void* stream) {
    DAE_CHECK_ARG(indptr && indices && image, "sweep_image_csr: indptr / indices / image are NULL (values may be: a binary matrix)");
    if (int rc = image_checks("sweep_image_csr", image, rows, D, norm, metric, image_bytes)) return rc;
    const int64_t Dp = pad128(D);
    DAE_LAUNCH(csr_row_normalize_kernel, dim3((unsigned)pad128(rows)), dim3(256), 0, (hipStream_t)stream, indptr, indices, values, (int)rows,
               (int)D, (int)norm, metric == 0 ? 1 : 0, image, Dp, (int)Dp);
    DAE_CHECK_LAUNCH();
    return 0;
}
