// dae_als.hip -- implicit-feedback matrix factorisation by alternating least squares (Hu, Koren, Volinsky 2008) with a conjugate
// gradient solve per row (dae_als_interactions / dae_als_gram / dae_als_solve_rows / dae_als_loss).  The rules are stated in
// include/dae_hip.h.
//
// Interactions (dae_als_interactions): keys -> sort -> run-length -> rows, the machinery of dae_covisit.hip, twice.
//   als_keys_kernel         one thread per click event: the key user << ib | item (an item outside [0, Na) gets the key of row M, which
//                           sorts behind every row and is counted out).
//   rocprim::radix_sort_keys over the bits in use, rocprim::run_length_encode: the distinct (user, item) pairs and their counts.
//   als_rows_kernel         row_ptr[r] = the first pair of row r (binary search), r = 0 .. rows.
//   als_unpack_kernel       user_idx / user_cnt, and the key item << ub | user of the other orientation;
//   rocprim::radix_sort_pairs (key, count), als_rows_kernel and als_unpack2_kernel give item_ptr / item_idx / item_cnt.
// Gram (dae_als_gram): fp64 partials of row blocks (a 16 x 16 thread tile, every thread T x T outputs), then a reduction over the
//   blocks ascending.  The blocks depend on N alone.
// Solve (dae_als_solve_rows): every vector of a row's CG (x, r, p, Ap; F <= 128 floats) lives in registers, four components per lane
//   of a *group* of GS = the power of two >= F / 4 lanes (32 lanes at F = 128, 16 at 64, one at F <= 4), and every group of the wave
//   holds the same copy.  One gathered factor row is one float4 per lane of a group, so a wave works on 64 / GS entries at once and
//   the reduction of the entry's dot product stays inside the group (xor shuffles; both partners compute the same sum, so every
//   lane ends with the same bits).  A p = G p + sum_j alpha cnt_j (y_j . p) y_j is a sum of scaled rows: group gg of the Gt groups at
//   work takes the rows k = gg, gg + Gt, ... of G and then the entries j = gg, gg + Gt, ... in ascending order, the groups of a wave
//   are added by xor shuffles, and the waves of a workgroup ascending through LDS.
//     rows of at most ALS_LONG entries: one wave per row (als_solve_short_kernel: 8 waves per workgroup, persistent, G staged in LDS
//       once per workgroup -- 64 KiB at F = 128, two workgroups = 16 waves per CU); a longer row is appended to a list;
//     longer rows: one workgroup of 16 waves per row (als_solve_long_kernel), G read through L2.
//   Which groups add which terms depends on F and on which of the two kernels runs the row, i.e. on the row's length, and on nothing
//   else; fp contraction is off, so every product and every sum is one fp32 rounding.
// Loss (dae_als_loss): sum_u x_u^T (Y^T Y) x_u = <X^T X, Y^T Y>, both Grams in fp64 by the Gram kernels; the observed entries and
//   lambda |x_u|^2 as one fp64 partial per row, lambda |y_i|^2 one per row of Y, the F^2 products one each; one array, summed in a
//   fixed order (256 chunks, then one).  No atomics.
#include "dae_common.h"

#include <rocprim/rocprim.hpp>

#pragma clang fp contract(off)

namespace dae {

constexpr int ALS_MAXF = 128;
constexpr int ALS_MAXCG = 32;
constexpr int ALS_LONG = 256;              // the longest row one wave solves
constexpr int ALS_THREADS = 512;           // als_solve_short_kernel: 8 rows per workgroup
constexpr int ALS_WAVES = ALS_THREADS / 64;
constexpr int ALS_HUB_THREADS = 1024;      // als_solve_long_kernel: 16 waves per row
constexpr int ALS_HUB_WAVES = ALS_HUB_THREADS / 64;
constexpr int ALS_GRID = 2048;             // persistent workgroups of either solve kernel
constexpr int ALS_GRAM_BLOCKS = 256;       // at most this many row blocks of a Gram
constexpr int ALS_SUM_BLOCKS = 256;

static inline uint64_t als_al256(uint64_t b) { return (b + 255) / 256 * 256; }
// number of bits that hold the values 0 .. n - 1 (at least 1)
static inline int als_bits(int64_t n) {
    int b = 1;
    while (b < 32 && (1ll << b) < n) ++b;
    return b;
}
static inline int als_group_log2(int F) {
    int l = 0;
    while ((4 << l) < F) ++l;
    return l;                              // F <= 128: at most 5 (32 lanes)
}
static inline bool als_vec4(const float* base, int64_t ld, int F) { return F % 4 == 0 && ld % 4 == 0 && ((uintptr_t)base & 15) == 0; }

// ---- interactions ----
__device__ __forceinline__ int als_user_of(const int64_t* indptr, int M, int64_t e) {
    int lo = 0, hi = M;                    // the answer u has indptr[u] <= e < indptr[u + 1]
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (indptr[m + 1] <= e) lo = m + 1; else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(256) void als_keys_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ items, int M,
                                                       int64_t nnz, int Na, int ib, uint64_t* __restrict__ keys) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int a = items[e];
    const bool ok = a >= 0 && a < Na;
    const uint64_t u = ok ? (uint64_t)als_user_of(indptr, M, e) : (uint64_t)M;
    keys[e] = (u << ib) | (ok ? (uint64_t)(uint32_t)a : 0ull);
}

// row_ptr[r] = the first of the n sorted keys that is >= r << shift, r = 0 .. rows; n comes from n_dev
__global__ __launch_bounds__(256) void als_rows_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ n_dev, int rows,
                                                       int shift, int64_t* __restrict__ row_ptr) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > rows) return;
    const uint64_t want = (uint64_t)r << shift;
    int64_t lo = 0, hi = *n_dev;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (keys[m] < want) lo = m + 1; else hi = m;
    }
    row_ptr[r] = lo;
}

__global__ void als_count_kernel(const unsigned long long* __restrict__ n_runs, int64_t* __restrict__ n64) { *n64 = (int64_t)*n_runs; }

// the pairs below user_ptr[M] (the runs of valid items): user_idx / user_cnt and the key of the other orientation
__global__ __launch_bounds__(256) void als_unpack_kernel(const uint64_t* __restrict__ uniq, const uint32_t* __restrict__ runs,
                                                         const int64_t* __restrict__ n_pairs, int ib, int ub, int64_t cap,
                                                         int32_t* __restrict__ idx, int32_t* __restrict__ cnt, uint64_t* __restrict__ keys2) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= *n_pairs || j >= cap) return;
    const uint64_t k = uniq[j];
    const uint64_t item = k & ((1ull << ib) - 1), user = k >> ib;
    idx[j] = (int32_t)item;
    cnt[j] = (int32_t)runs[j];
    keys2[j] = (item << ub) | user;
}

__global__ __launch_bounds__(256) void als_unpack2_kernel(const uint64_t* __restrict__ keys2, const uint32_t* __restrict__ vals,
                                                          const int64_t* __restrict__ n_pairs, int ub, int64_t cap, int32_t* __restrict__ idx,
                                                          int32_t* __restrict__ cnt) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= *n_pairs || j >= cap) return;
    idx[j] = (int32_t)(keys2[j] & ((1ull << ub) - 1));
    cnt[j] = (int32_t)vals[j];
}

// totals = {events with a valid item, distinct pairs}: the runs behind n_pairs are the one run of the key of row M
__global__ void als_totals_kernel(const uint32_t* __restrict__ runs, const int64_t* __restrict__ n_runs, const int64_t* __restrict__ n_pairs,
                                  int64_t nnz, int64_t* __restrict__ totals) {
    int64_t bad = 0;
    for (int64_t j = *n_pairs; j < *n_runs; ++j) bad += runs[j];
    totals[0] = nnz - bad;
    totals[1] = *n_pairs;
}

__global__ __launch_bounds__(256) void als_zero_ptr_kernel(int64_t* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// ---- Gram ----
// Block b sums the rows [b * rows_per_block, (b + 1) * rows_per_block) ascending in fp64 (the product of two floats is exact in
// fp64).  Thread (ty, tx) of the 16 x 16 tile owns the outputs (ty + 16 i, tx + 16 j), i, j < T.
template <int T>
__global__ __launch_bounds__(256) void als_gram_partial_kernel(const float* __restrict__ Y, int64_t ldy, int N, int F, int rows_per_block,
                                                               double* __restrict__ part) {
    constexpr int W = 16 * T;
    __shared__ float tile[16][W + 1];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
    double acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = 0.0;
    for (int64_t c0 = r0; c0 < r1; c0 += 16) {
        __syncthreads();
        for (int e = tid; e < 16 * W; e += 256) {
            const int r = e / W, c = e % W;
            tile[r][c] = (c0 + r < r1 && c < F) ? Y[(c0 + r) * ldy + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < 16; ++r) {
            double av[T], bv[T];
#pragma unroll
            for (int i = 0; i < T; ++i) { av[i] = (double)tile[r][ty + 16 * i]; bv[i] = (double)tile[r][tx + 16 * i]; }
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] += av[i] * bv[j];
        }
    }
    double* out = part + (int64_t)blockIdx.x * F * F;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int a = ty + 16 * i, b = tx + 16 * j;
            if (a < F && b < F) out[a * F + b] = acc[i][j];
        }
}

// the blocks ascending; G = fl32(sum + lambda on the diagonal), G64 = the sum itself (either may be NULL)
__global__ __launch_bounds__(256) void als_gram_reduce_kernel(const double* __restrict__ part, int nb, int F, float lambda,
                                                              float* __restrict__ G, double* __restrict__ G64) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= F * F) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(int64_t)b * F * F + e];
    if (G64) G64[e] = s;
    if (G) G[e] = (float)(e / F == e % F ? s + (double)lambda : s);
}

static inline int als_gram_blocks(int N) {
    const int nb = (N + 63) / 64;
    return nb < 1 ? 1 : (nb > ALS_GRAM_BLOCKS ? ALS_GRAM_BLOCKS : nb);
}

// launches the two Gram kernels; part holds als_gram_blocks(N) * F * F doubles
static int als_gram_launch(const float* Y, int64_t ldy, int N, int F, float lambda, float* G, double* G64, double* part, hipStream_t st) {
    const int nb = als_gram_blocks(N);
    const int rpb = (N + nb - 1) / nb;
    if (F <= 16) DAE_LAUNCH(als_gram_partial_kernel<1>, dim3(nb), dim3(256), 0, st, Y, ldy, N, F, rpb, part);
    else if (F <= 32) DAE_LAUNCH(als_gram_partial_kernel<2>, dim3(nb), dim3(256), 0, st, Y, ldy, N, F, rpb, part);
    else if (F <= 64) DAE_LAUNCH(als_gram_partial_kernel<4>, dim3(nb), dim3(256), 0, st, Y, ldy, N, F, rpb, part);
    else DAE_LAUNCH(als_gram_partial_kernel<8>, dim3(nb), dim3(256), 0, st, Y, ldy, N, F, rpb, part);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(als_gram_reduce_kernel, dim3((F * F + 255) / 256), dim3(256), 0, st, (const double*)part, nb, F, lambda, G, G64);
    DAE_CHECK_LAUNCH();
    return 0;
}

// ---- solve ----
struct AlsSolve {
    const int64_t* ptr; const int32_t* idx; const int32_t* cnt; int R;
    const float* Y; int64_t ldy; int N, F;
    const float* G; float alpha; int steps;
    float* X; int64_t ldx;
    int gl;                       // log2 of the group size
    int vecY, vecX, vecG;         // the rows may be read as float4
    int32_t* long_rows; unsigned* n_long;
};

// components c0 .. c0 + 3 of a row of F floats; zeros beyond F
__device__ __forceinline__ float4 als_ld4(const float* __restrict__ row, int c0, int F, int vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 >= F) return v;
    if (vec) return *reinterpret_cast<const float4*>(row + c0);
    v.x = row[c0];
    if (c0 + 1 < F) v.y = row[c0 + 1];
    if (c0 + 2 < F) v.z = row[c0 + 2];
    if (c0 + 3 < F) v.w = row[c0 + 3];
    return v;
}

// a . b over the group's lanes: four products summed ascending, then xor shuffles -- the same bits in every lane of the group
__device__ __forceinline__ float als_dot(const float4& a, const float4& b, int gs) {
    float s = a.x * b.x;
    s = s + a.y * b.y;
    s = s + a.z * b.z;
    s = s + a.w * b.w;
    for (int o = 1; o < gs; o <<= 1) s = s + __shfl_xor(s, o, 64);
    return s;
}

__device__ __forceinline__ void als_axpy(float4& y, float a, const float4& x) {
    y.x = y.x + a * x.x; y.y = y.y + a * x.y; y.z = y.z + a * x.z; y.w = y.w + a * x.w;
}

template <int NW>
__device__ __forceinline__ void als_team_sync() {
    if (NW == 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// the groups of a wave by xor shuffles, then (NW > 1) the waves ascending through wpart [NW][128]
template <int NW>
__device__ __forceinline__ void als_combine(float4& acc, int gs, int wave, int g, int c0, float* wpart) {
    for (int o = gs; o < 64; o <<= 1) {
        acc.x = acc.x + __shfl_xor(acc.x, o, 64); acc.y = acc.y + __shfl_xor(acc.y, o, 64);
        acc.z = acc.z + __shfl_xor(acc.z, o, 64); acc.w = acc.w + __shfl_xor(acc.w, o, 64);
    }
    if (NW > 1) {
        if (g == 0) *reinterpret_cast<float4*>(wpart + wave * ALS_MAXF + c0) = acc;
        __syncthreads();
        acc = *reinterpret_cast<const float4*>(wpart + c0);
        for (int w = 1; w < NW; ++w) {
            const float4 t = *reinterpret_cast<const float4*>(wpart + w * ALS_MAXF + c0);
            acc.x = acc.x + t.x; acc.y = acc.y + t.y; acc.z = acc.z + t.z; acc.w = acc.w + t.w;
        }
        __syncthreads();
    }
}

// Av = G v + sum_j alpha cnt_j (y_j . v) y_j of one row, for the vector v every group holds; FIRST: also b = sum_j (1 + alpha cnt_j) y_j.
// Gs: the rows of G, gld floats apart (LDS or global); vbuf: 128 floats of LDS the team shares.
template <int NW, bool FIRST>
__device__ __forceinline__ float4 als_apply(const AlsSolve& p, int64_t e0, int n, const float4& v, const float* Gs, int gld, int vecG,
                                            float* vbuf, float* wpart, int wave, int lane, float4& b) {
    const int gs = 1 << p.gl, ng = 64 >> p.gl;
    const int g = lane >> p.gl, c0 = (lane & (gs - 1)) * 4;
    const int gg = wave * ng + g, Gt = NW * ng;
    constexpr int U = NW > 1 ? 8 : 4;      // gathered rows in flight per lane (the order of a group's terms does not depend on it)
    if (gg == 0) *reinterpret_cast<float4*>(vbuf + c0) = v;
    als_team_sync<NW>();
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < p.F; k0 += Gt) {
        const int k = k0 + gg;
        if (k < p.F) als_axpy(acc, vbuf[k], als_ld4(Gs + (int64_t)k * gld, c0, p.F, vecG));
    }
    if (FIRST) b = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j0 = 0; j0 < n; j0 += U * Gt) {
        int it[U];
        float a[U];
        float4 y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * Gt + gg;
            it[u] = -1; a[u] = 0.f;
            if (j < n) {
                const int i = p.idx[e0 + j];
                if (i >= 0 && i < p.N) { it[u] = i; a[u] = p.alpha * (float)p.cnt[e0 + j]; }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            y[u] = it[u] >= 0 ? als_ld4(p.Y + (int64_t)it[u] * p.ldy, c0, p.F, p.vecY) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float d = als_dot(y[u], v, gs);
            als_axpy(acc, a[u] * d, y[u]);
            if (FIRST && it[u] >= 0) als_axpy(b, 1.f + a[u], y[u]);
        }
    }
    als_combine<NW>(acc, gs, wave, g, c0, wpart);
    if (FIRST) als_combine<NW>(b, gs, wave, g, c0, wpart);
    return acc;
}

// one row, by a team of NW waves; every lane of the team takes every branch alike (the scalars have the same bits in every lane)
template <int NW>
__device__ __forceinline__ void als_row(const AlsSolve& p, int row, int64_t e0, int n, const float* Gs, int gld, int vecG, float* vbuf,
                                        float* wpart, int wave, int lane) {
    const int gs = 1 << p.gl;
    const int g = lane >> p.gl, c0 = (lane & (gs - 1)) * 4;
    float* xrow = p.X + (int64_t)row * p.ldx;
    float4 x = als_ld4(xrow, c0, p.F, p.vecX);
    float4 b, Ap;
    float4 r = als_apply<NW, true>(p, e0, n, x, Gs, gld, vecG, vbuf, wpart, wave, lane, b);
    r.x = b.x - r.x; r.y = b.y - r.y; r.z = b.z - r.z; r.w = b.w - r.w;
    float4 d = r;
    float rs = als_dot(r, r, gs);
    for (int it = 0; it < p.steps; ++it) {
        if (rs <= 1e-20f) break;
        Ap = als_apply<NW, false>(p, e0, n, d, Gs, gld, vecG, vbuf, wpart, wave, lane, b);
        const float dAd = als_dot(d, Ap, gs);
        if (!(dAd > 0.f)) break;
        const float a = rs / dAd;
        als_axpy(x, a, d);
        als_axpy(r, -a, Ap);
        const float rsn = als_dot(r, r, gs);
        const float beta = rsn / rs;
        d.x = r.x + beta * d.x; d.y = r.y + beta * d.y; d.z = r.z + beta * d.z; d.w = r.w + beta * d.w;
        rs = rsn;
    }
    if (wave == 0 && g == 0) {
        if (c0 < p.F) xrow[c0] = x.x;
        if (c0 + 1 < p.F) xrow[c0 + 1] = x.y;
        if (c0 + 2 < p.F) xrow[c0 + 2] = x.z;
        if (c0 + 3 < p.F) xrow[c0 + 3] = x.w;
    }
}

// dynamic LDS: G as F rows of gld = 4 * group size floats, zero padded
__global__ __launch_bounds__(ALS_THREADS) void als_solve_short_kernel(AlsSolve p) {
    extern __shared__ __attribute__((aligned(16))) float als_g[];
    __shared__ __attribute__((aligned(16))) float vbuf[ALS_WAVES][ALS_MAXF];
    const int gld = 4 << p.gl;
    for (int e = threadIdx.x; e < p.F * gld; e += ALS_THREADS) {
        const int k = e / gld, c = e % gld;
        als_g[e] = c < p.F ? p.G[k * p.F + c] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t base = (int64_t)blockIdx.x * ALS_WAVES; base < p.R; base += (int64_t)gridDim.x * ALS_WAVES) {
        const int64_t row = base + wave;
        if (row >= p.R) continue;
        const int64_t e0 = p.ptr[row];
        const int64_t n = p.ptr[row + 1] - e0;
        if (n > ALS_LONG) {
            if (lane == 0) p.long_rows[atomicAdd(p.n_long, 1u)] = (int32_t)row;      // (the order of the list decides nothing)
            continue;
        }
        if (n <= 0) {
            for (int c = lane; c < p.F; c += 64) p.X[row * p.ldx + c] = 0.f;
            continue;
        }
        als_row<1>(p, (int)row, e0, (int)n, als_g, gld, 1, vbuf[wave], nullptr, 0, lane);
    }
}

__global__ __launch_bounds__(ALS_HUB_THREADS) void als_solve_long_kernel(AlsSolve p) {
    __shared__ __attribute__((aligned(16))) float vbuf[ALS_MAXF];
    __shared__ __attribute__((aligned(16))) float wpart[ALS_HUB_WAVES * ALS_MAXF];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned n_long = *p.n_long;
    for (unsigned i = blockIdx.x; i < n_long; i += gridDim.x) {
        const int row = p.long_rows[i];
        const int64_t e0 = p.ptr[row];
        const int64_t n = p.ptr[row + 1] - e0;
        als_row<ALS_HUB_WAVES>(p, row, e0, (int)n, p.G, p.F, p.vecG, vbuf, wpart, wave, lane);
        __syncthreads();
    }
}

// ---- loss ----
struct AlsLoss {
    const int64_t* ptr; const int32_t* idx; const int32_t* cnt; int R;
    const float* X; int64_t ldx; const float* Y; int64_t ldy; int N, F;
    float alpha, lambda;
    int gl, vecX, vecY;
    double* part;                 // [R]
};

__device__ __forceinline__ double als_dot64(const float4& a, const float4& b, int gs) {
    double s = (double)a.x * (double)b.x;
    s += (double)a.y * (double)b.y;
    s += (double)a.z * (double)b.z;
    s += (double)a.w * (double)b.w;
    for (int o = 1; o < gs; o <<= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// part[u] = sum over the row's entries of c (1 - s)^2 - s^2, s = x_u . y_i, c = 1 + alpha cnt, plus lambda |x_u|^2: one wave per row
__global__ __launch_bounds__(256) void als_loss_rows_kernel(AlsLoss p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.R) return;
    const int gs = 1 << p.gl, ng = 64 >> p.gl;
    const int g = lane >> p.gl, lg = lane & (gs - 1), c0 = lg * 4;
    const float4 x = als_ld4(p.X + row * p.ldx, c0, p.F, p.vecX);
    const int64_t e0 = p.ptr[row];
    const int64_t n = p.ptr[row + 1] - e0;
    double acc = 0.0;
    for (int64_t j0 = 0; j0 < n; j0 += ng) {
        const int64_t j = j0 + g;
        int i = -1;
        double c = 0.0;
        if (j < n) {
            i = p.idx[e0 + j];
            c = 1.0 + (double)p.alpha * (double)p.cnt[e0 + j];
            if (i < 0 || i >= p.N) i = -1;
        }
        const float4 y = i >= 0 ? als_ld4(p.Y + (int64_t)i * p.ldy, c0, p.F, p.vecY) : make_float4(0.f, 0.f, 0.f, 0.f);
        const double s = als_dot64(x, y, gs);
        if (i >= 0 && lg == 0) acc += c * (1.0 - s) * (1.0 - s) - s * s;
    }
    const double xx = als_dot64(x, x, gs);
    if (lane == 0) acc += (double)p.lambda * xx;
    for (int o = 1; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) p.part[row] = acc;
}

// part[i] = lambda |y_i|^2, one thread per row
__global__ __launch_bounds__(256) void als_loss_norm_kernel(const float* __restrict__ Y, int64_t ldy, int N, int F, float lambda,
                                                            double* __restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    for (int c = 0; c < F; ++c) { const double v = (double)Y[i * ldy + c]; s += v * v; }
    part[i] = (double)lambda * s;
}

__global__ __launch_bounds__(256) void als_loss_frob_kernel(const double* __restrict__ A, const double* __restrict__ B, int n,
                                                            double* __restrict__ part) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) part[e] = A[e] * B[e];
}

// out[b] = the sum of in[b * chunk, (b + 1) * chunk): thread t adds its elements t, t + 256, ... ascending, then a fixed tree
__global__ __launch_bounds__(256) void als_sum_kernel(const double* __restrict__ in, int64_t n, int64_t chunk, double* __restrict__ out) {
    __shared__ double sh[256];
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) s += in[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// ---- host ----
static bool als_temp_bytes(size_t n, int bits1, int bits2, size_t& bytes) {
    uint64_t* k = nullptr;
    uint32_t* c = nullptr;
    unsigned long long* r = nullptr;
    rocprim::double_buffer<uint64_t> dk(k, k);
    rocprim::double_buffer<uint32_t> dv(c, c);
    size_t s1 = 0, s2 = 0, s3 = 0;
    if (rocprim::radix_sort_keys(nullptr, s1, dk, n, 0, bits1, (hipStream_t)0) != hipSuccess) return false;
    if (rocprim::run_length_encode(nullptr, s2, k, n, k, c, r, (hipStream_t)0) != hipSuccess) return false;
    if (rocprim::radix_sort_pairs(nullptr, s3, dk, dv, n, 0, bits2, (hipStream_t)0) != hipSuccess) return false;
    bytes = s1 > s2 ? s1 : s2;
    bytes = bytes > s3 ? bytes : s3;
    return true;
}
// two key buffers, two count buffers, the scalars
static uint64_t als_inter_fixed_bytes(uint64_t nnz) { return 2 * als_al256(nnz * 8) + 2 * als_al256(nnz * 4) + 256; }

static uint64_t als_loss_fixed_bytes(int R, int N, int F) {
    const int nb = als_gram_blocks(R > N ? R : N);
    const uint64_t ff = (uint64_t)F * F;
    return 2 * als_al256(ff * 8) + als_al256((uint64_t)nb * ff * 8) + als_al256(((uint64_t)R + N + ff) * 8) + als_al256(ALS_SUM_BLOCKS * 8);
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_als_interactions_workspace(int64_t nnz, int32_t M, int32_t Na) {
    if (nnz <= 0 || nnz >= (1ll << 31) || M < 1 || Na < 1) return 0;
    size_t temp = 0;
    if (!als_temp_bytes((size_t)nnz, als_bits(Na) + als_bits((int64_t)M + 1), als_bits(Na) + als_bits(M), temp)) return 0;
    return als_inter_fixed_bytes((uint64_t)nnz) + als_al256(temp);
}

extern "C" int dae_als_interactions(const int64_t* indptr, const int32_t* items, int32_t M, int64_t nnz, int32_t Na, int64_t* user_ptr,
                                    int32_t* user_idx, int32_t* user_cnt, int64_t* item_ptr, int32_t* item_idx, int32_t* item_cnt,
                                    int64_t cap, int64_t* totals, void* workspace, uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(user_ptr && user_idx && user_cnt && item_ptr && item_idx && item_cnt && totals, "als_interactions: an output is NULL");
    DAE_CHECK_ARG(M >= 0 && nnz >= 0, "als_interactions: M (%d) and nnz (%lld) must not be negative", M, (long long)nnz);
    DAE_CHECK_ARG(Na >= 1, "als_interactions: Na (%d) must be at least 1", Na);
    DAE_CHECK_ARG(nnz < (1ll << 31), "als_interactions: %lld events; one call takes fewer than 2^31 (build from fewer users)", (long long)nnz);
    DAE_CHECK_ARG(cap >= nnz, "als_interactions: cap (%lld) must be >= nnz (%lld)", (long long)cap, (long long)nnz);
    DAE_CHECK_ARG(nnz == 0 || M >= 1, "als_interactions: %lld events without a user", (long long)nnz);
    DAE_CHECK_ARG(nnz == 0 || (indptr && items), "als_interactions: indptr / items is NULL");
    if (nnz > 0) {
        DAE_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0, "als_interactions: the workspace must be 256-byte aligned");
        DAE_CHECK_ARG(workspace_bytes >= als_inter_fixed_bytes((uint64_t)nnz),
                      "als_interactions: workspace too small (%llu bytes, the buffers of %lld events alone need %llu)",
                      (unsigned long long)workspace_bytes, (long long)nnz, (unsigned long long)als_inter_fixed_bytes((uint64_t)nnz));
    }
    hipStream_t st = (hipStream_t)stream;
    if (nnz == 0) {
        DAE_LAUNCH(als_zero_ptr_kernel, dim3((unsigned)(((int64_t)M + 1 + 255) / 256)), dim3(256), 0, st, user_ptr, (int64_t)M + 1);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(als_zero_ptr_kernel, dim3((unsigned)(((int64_t)Na + 1 + 255) / 256)), dim3(256), 0, st, item_ptr, (int64_t)Na + 1);
        DAE_CHECK_LAUNCH();
        DAE_LAUNCH(als_zero_ptr_kernel, dim3(1), dim3(256), 0, st, totals, (int64_t)2);
        DAE_CHECK_LAUNCH();
        return 0;
    }
    const int ib = als_bits(Na), ub = als_bits(M), ub1 = als_bits((int64_t)M + 1);
    size_t temp_bytes = 0;
    DAE_CHECK_ARG(als_temp_bytes((size_t)nnz, ib + ub1, ib + ub, temp_bytes), "als_interactions: the size query of rocprim failed");
    DAE_CHECK_ARG(workspace_bytes >= als_inter_fixed_bytes((uint64_t)nnz) + als_al256(temp_bytes),
                  "als_interactions: workspace too small (%llu bytes, %lld events need %llu)", (unsigned long long)workspace_bytes,
                  (long long)nnz, (unsigned long long)(als_inter_fixed_bytes((uint64_t)nnz) + als_al256(temp_bytes)));
    char* w = (char*)workspace;
    uint64_t* keys_a = (uint64_t*)w;    w += als_al256((uint64_t)nnz * 8);
    uint64_t* keys_b = (uint64_t*)w;    w += als_al256((uint64_t)nnz * 8);
    uint32_t* runs_a = (uint32_t*)w;    w += als_al256((uint64_t)nnz * 4);
    uint32_t* runs_b = (uint32_t*)w;    w += als_al256((uint64_t)nnz * 4);
    unsigned long long* n_runs = (unsigned long long*)w;
    int64_t* n_runs64 = (int64_t*)w + 1;
    w += 256;
    void* temp = w;
    const unsigned egrid = (unsigned)((nnz + 255) / 256);
    DAE_LAUNCH(als_keys_kernel, dim3(egrid), dim3(256), 0, st, indptr, items, (int)M, nnz, (int)Na, ib, keys_a);
    DAE_CHECK_LAUNCH();
    rocprim::double_buffer<uint64_t> db(keys_a, keys_b);
    size_t tb = temp_bytes;
    DAE_CHECK_HIP(rocprim::radix_sort_keys(temp, tb, db, (size_t)nnz, 0, ib + ub1, st));
    uint64_t* sorted = db.current();
    uint64_t* uniq = db.alternate();
    tb = temp_bytes;
    DAE_CHECK_HIP(rocprim::run_length_encode(temp, tb, sorted, (size_t)nnz, uniq, runs_a, n_runs, st));
    DAE_LAUNCH(als_count_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)n_runs, n_runs64);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(als_rows_kernel, dim3((unsigned)(((int64_t)M + 1 + 255) / 256)), dim3(256), 0, st, (const uint64_t*)uniq,
               (const int64_t*)n_runs64, (int)M, ib, user_ptr);
    DAE_CHECK_LAUNCH();
    const int64_t* n_pairs_dev = user_ptr + M;
    DAE_LAUNCH(als_unpack_kernel, dim3(egrid), dim3(256), 0, st, (const uint64_t*)uniq, (const uint32_t*)runs_a, n_pairs_dev, ib, ub, cap,
               user_idx, user_cnt, sorted);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(als_totals_kernel, dim3(1), dim3(1), 0, st, (const uint32_t*)runs_a, (const int64_t*)n_runs64, n_pairs_dev, nnz, totals);
    DAE_CHECK_LAUNCH();
    int64_t n_pairs = 0;
    DAE_CHECK_HIP(hipMemcpyAsync(&n_pairs, n_pairs_dev, 8, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    DAE_CHECK_ARG(n_pairs >= 0 && n_pairs <= nnz, "als_interactions: %lld pairs of %lld events", (long long)n_pairs, (long long)nnz);
    const uint64_t* keys2 = sorted;
    const uint32_t* vals2 = runs_a;
    if (n_pairs > 0) {
        rocprim::double_buffer<uint64_t> dk(sorted, uniq);
        rocprim::double_buffer<uint32_t> dv(runs_a, runs_b);
        tb = temp_bytes;
        DAE_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, dk, dv, (size_t)n_pairs, 0, ib + ub, st));
        keys2 = dk.current();
        vals2 = dv.current();
    }
    DAE_LAUNCH(als_rows_kernel, dim3((unsigned)(((int64_t)Na + 1 + 255) / 256)), dim3(256), 0, st, keys2, n_pairs_dev, (int)Na, ub, item_ptr);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(als_unpack2_kernel, dim3(egrid), dim3(256), 0, st, keys2, vals2, n_pairs_dev, ub, cap, item_idx, item_cnt);
    DAE_CHECK_LAUNCH();
    DAE_CHECK_HIP(hipStreamSynchronize(st));              // the workspace may be released on return
    return 0;
}

extern "C" uint64_t dae_als_gram_workspace(int32_t N, int32_t F) {
    if (N < 1 || F < 1 || F > ALS_MAXF) return 0;
    return als_al256((uint64_t)als_gram_blocks(N) * F * F * 8);
}

extern "C" int dae_als_gram(const float* Y, int64_t ldy, int32_t N, int32_t F, float lambda, float* G, void* workspace,
                            uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(F >= 1 && F <= ALS_MAXF, "als_gram: F (%d) must be in 1..%d", F, ALS_MAXF);
    DAE_CHECK_ARG(N >= 1, "als_gram: N (%d) must be at least 1", N);
    DAE_CHECK_ARG(Y && G, "als_gram: Y / G is NULL");
    DAE_CHECK_ARG(ldy >= F, "als_gram: ldy (%lld) must be >= F (%d)", (long long)ldy, F);
    DAE_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0, "als_gram: the workspace must be 256-byte aligned");
    DAE_CHECK_ARG(workspace_bytes >= dae_als_gram_workspace(N, F), "als_gram: workspace too small (%llu bytes, %llu needed)",
                  (unsigned long long)workspace_bytes, (unsigned long long)dae_als_gram_workspace(N, F));
    return als_gram_launch(Y, ldy, N, F, lambda, G, nullptr, (double*)workspace, (hipStream_t)stream);
}

extern "C" uint64_t dae_als_solve_rows_workspace(int32_t R) {
    if (R < 1) return 0;
    return 256 + als_al256((uint64_t)R * 4);
}

extern "C" int dae_als_solve_rows(const int64_t* ptr, const int32_t* idx, const int32_t* cnt, int32_t R, const float* Y, int64_t ldy,
                                  int32_t N, int32_t F, const float* G, float alpha, int32_t cg_steps, float* X, int64_t ldx,
                                  void* workspace, uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(F >= 1 && F <= ALS_MAXF, "als_solve_rows: F (%d) must be in 1..%d", F, ALS_MAXF);
    DAE_CHECK_ARG(cg_steps >= 1 && cg_steps <= ALS_MAXCG, "als_solve_rows: cg_steps (%d) must be in 1..%d", cg_steps, ALS_MAXCG);
    DAE_CHECK_ARG(R >= 0 && N >= 1, "als_solve_rows: R (%d) must not be negative and N (%d) must be at least 1", R, N);
    DAE_CHECK_ARG(ldy >= F && ldx >= F, "als_solve_rows: ldy (%lld) and ldx (%lld) must be >= F (%d)", (long long)ldy, (long long)ldx, F);
    DAE_CHECK_ARG(alpha == alpha, "als_solve_rows: alpha is NaN");
    if (R == 0) return 0;
    DAE_CHECK_ARG(ptr && idx && cnt && Y && G && X, "als_solve_rows: ptr / idx / cnt / Y / G / X is NULL");
    DAE_CHECK_ARG((const float*)X != Y, "als_solve_rows: the factors to update must not be the fixed factors");
    DAE_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0, "als_solve_rows: the workspace must be 256-byte aligned");
    DAE_CHECK_ARG(workspace_bytes >= dae_als_solve_rows_workspace(R), "als_solve_rows: workspace too small (%llu bytes, %llu needed)",
                  (unsigned long long)workspace_bytes, (unsigned long long)dae_als_solve_rows_workspace(R));
    static const int attr_rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(als_solve_short_kernel),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, ALS_MAXF * ALS_MAXF * 4);
    DAE_CHECK_ARG(attr_rc == 0, "als_solve_rows: hipFuncSetAttribute failed (%d)", attr_rc);
    hipStream_t st = (hipStream_t)stream;
    AlsSolve p;
    p.ptr = ptr; p.idx = idx; p.cnt = cnt; p.R = R;
    p.Y = Y; p.ldy = ldy; p.N = N; p.F = F; p.G = G; p.alpha = alpha; p.steps = cg_steps;
    p.X = X; p.ldx = ldx;
    p.gl = als_group_log2(F);
    p.vecY = als_vec4(Y, ldy, F); p.vecX = als_vec4(X, ldx, F); p.vecG = als_vec4(G, F, F);
    p.n_long = (unsigned*)workspace;
    p.long_rows = (int32_t*)((char*)workspace + 256);
    DAE_CHECK_HIP(hipMemsetAsync(p.n_long, 0, 4, st));
    const int64_t blocks = ((int64_t)R + ALS_WAVES - 1) / ALS_WAVES;
    const size_t lds = (size_t)F * (4 << p.gl) * 4;
    DAE_LAUNCH(als_solve_short_kernel, dim3((unsigned)(blocks < ALS_GRID ? blocks : ALS_GRID)), dim3(ALS_THREADS), lds, st, p);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(als_solve_long_kernel, dim3((unsigned)(R < ALS_GRID ? R : ALS_GRID)), dim3(ALS_HUB_THREADS), 0, st, p);
    DAE_CHECK_LAUNCH();
    return 0;
}

extern "C" uint64_t dae_als_loss_workspace(int32_t R, int32_t N, int32_t F) {
    if (R < 1 || N < 1 || F < 1 || F > ALS_MAXF) return 0;
    return als_loss_fixed_bytes(R, N, F);
}

extern "C" int dae_als_loss(const int64_t* ptr, const int32_t* idx, const int32_t* cnt, int32_t R, const float* X, int64_t ldx,
                            const float* Y, int64_t ldy, int32_t N, int32_t F, float alpha, float lambda, double* loss, void* workspace,
                            uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(F >= 1 && F <= ALS_MAXF, "als_loss: F (%d) must be in 1..%d", F, ALS_MAXF);
    DAE_CHECK_ARG(R >= 1 && N >= 1, "als_loss: R (%d) and N (%d) must be at least 1", R, N);
    DAE_CHECK_ARG(ptr && idx && cnt && X && Y && loss, "als_loss: ptr / idx / cnt / X / Y / loss is NULL");
    DAE_CHECK_ARG(ldy >= F && ldx >= F, "als_loss: ldy (%lld) and ldx (%lld) must be >= F (%d)", (long long)ldy, (long long)ldx, F);
    DAE_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0, "als_loss: the workspace must be 256-byte aligned");
    DAE_CHECK_ARG(workspace_bytes >= als_loss_fixed_bytes(R, N, F), "als_loss: workspace too small (%llu bytes, %llu needed)",
                  (unsigned long long)workspace_bytes, (unsigned long long)als_loss_fixed_bytes(R, N, F));
    hipStream_t st = (hipStream_t)stream;
    const int nb = als_gram_blocks(R > N ? R : N);
    const int ff = F * F;
    char* w = (char*)workspace;
    double* gx = (double*)w;        w += als_al256((uint64_t)ff * 8);
    double* gy = (double*)w;        w += als_al256((uint64_t)ff * 8);
    double* gpart = (double*)w;     w += als_al256((uint64_t)nb * ff * 8);
    double* part = (double*)w;      w += als_al256(((uint64_t)R + N + ff) * 8);
    double* sums = (double*)w;
    int rc = als_gram_launch(X, ldx, R, F, 0.f, nullptr, gx, gpart, st);
    if (rc) return rc;
    rc = als_gram_launch(Y, ldy, N, F, 0.f, nullptr, gy, gpart, st);
    if (rc) return rc;
    AlsLoss p;
    p.ptr = ptr; p.idx = idx; p.cnt = cnt; p.R = R; p.X = X; p.ldx = ldx; p.Y = Y; p.ldy = ldy; p.N = N; p.F = F;
    p.alpha = alpha; p.lambda = lambda; p.gl = als_group_log2(F);
    p.vecX = als_vec4(X, ldx, F); p.vecY = als_vec4(Y, ldy, F);
    p.part = part;
    DAE_LAUNCH(als_loss_rows_kernel, dim3((unsigned)(((int64_t)R + 3) / 4)), dim3(256), 0, st, p);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(als_loss_norm_kernel, dim3((unsigned)(((int64_t)N + 255) / 256)), dim3(256), 0, st, Y, ldy, (int)N, (int)F, lambda, part + R);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(als_loss_frob_kernel, dim3((unsigned)((ff + 255) / 256)), dim3(256), 0, st, (const double*)gx, (const double*)gy, ff,
               part + R + N);
    DAE_CHECK_LAUNCH();
    const int64_t total = (int64_t)R + N + ff;
    const int64_t chunk = (total + ALS_SUM_BLOCKS - 1) / ALS_SUM_BLOCKS;
    DAE_LAUNCH(als_sum_kernel, dim3(ALS_SUM_BLOCKS), dim3(256), 0, st, (const double*)part, total, chunk, sums);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(als_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)sums, (int64_t)ALS_SUM_BLOCKS, (int64_t)ALS_SUM_BLOCKS, loss);
    DAE_CHECK_LAUNCH();
    return 0;
}
