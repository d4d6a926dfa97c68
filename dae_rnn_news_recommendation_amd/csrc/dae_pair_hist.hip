// dae_pair_hist.hip -- related / unrelated score histograms of all row pairs, without the N x N matrix (dae_pair_hist).
//
// The scores are those of dae_threshold_pairs: rows normalised by row_normalize_kernel (dae_similarity.hip) into zero-padded
// fp32 operand images, products by gemm_mainloop<float, 2> (dae_gemm_tile.h) over the whole K range in one pass, so a score
// does not depend on the grid.  What is new is an epilogue that REDUCES the scores by label class instead of storing them.
//
// pair_hist_tiles_kernel: 256 threads (4 waves), a fixed grid of G workgroups (two per CU, capped at the tile count);
// workgroup w walks the strip of 128 x 128 tiles w, w + G, w + 2G, ... of the lower-triangle enumeration of pairs_tiles_kernel
// (self mode: t = qt (qt + 1) / 2 + ct, ct <= qt) or of the full qtiles x ctiles grid (with candidates).
// LDS = the 64 KiB staging ring of the K loop + the two class histograms, 2 x bins x uint32, which live there for the whole
// strip: 80 KiB at 2048 bins, two workgroups per CU.  The tile's 128 + 128 labels overlay the ring between two K loops.
// Epilogue on the accumulators (the tile never passes through LDS), per value: valid when i < Nq, j < Nc, j < i in self mode
// and both labels >= 0; class = labels equal; bin = clamp(floor((s - lo) * bins / (hi - lo)), 0, bins - 1) in fp32 exactly as
// written (IEEE subtract, multiply, divide; no contraction is possible); one LDS atomic add without return on hist[class][bin];
// per-lane running NaN count, score_key min / max per class and fp64 sum per class.  NaN scores enter no bin.
// End of the strip (and after every 2^17 tiles, so that no uint32 counter can wrap: a tile adds at most 16 384): the non-zero
// LDS counters go to the global uint64[2][bins] histogram by atomic adds -- integers, so the result is bit-identical run to
// run and independent of the grid -- and the lanes' running values are reduced over the wave and the workgroup into one
// record per workgroup; the host folds the records in index order (the fp64 sums are therefore bit-identical run to run).
//
// dae_pair_hist_images runs the same kernel, unchanged, on images the caller built (dae_sweep_image.hip) with an explicit range:
// the strict lower triangle of an operand swept in row chunks is its diagonal blocks in self mode plus the blocks below them in
// full mode; counts add as integers, min / max combine, the caller adds the fp64 sums block by block.  dae_sweep_image_norm2_max
// exposes row_norm2_max_kernel so that the automatic range of the linear kernel can be rebuilt from the chunks (a maximum).
#include "dae_score_sweep.h"

#include <cmath>
#include <vector>

namespace dae {

constexpr int PAIR_HIST_MAX_BINS = 2048;
constexpr int PAIR_HIST_RING = lds_bytes_for(2);
constexpr int PAIR_HIST_MAX_GRID = 1024;     // records in the workspace; the grid is 2 x CUs (512 on the MI355X), capped here
constexpr int PAIR_HIST_FLUSH_TILES = 1 << 17;
constexpr int PAIR_NORM_BLOCKS = 256;

struct PairHistRecord {           // one per workgroup
    double sum[2];                // related, unrelated
    unsigned long long n_nan;
    uint32_t kmin[2], kmax[2];
};

struct PairHistParams {
    GemmParams g;                 // one K segment: A = query image, Bt = corpus image
    int Nq, Nc, self, ctiles, bins;
    long long tiles;
    float lo, span, fbins;        // span = hi - lo (fp32)
    const int32_t* labels_q;      // [Nq]
    const int32_t* labels_c;      // [Nc] (= labels_q in self mode)
    unsigned long long* hist;     // [2][bins]: related, unrelated
    PairHistRecord* rec;          // [gridDim.x]
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void pair_hist_tiles_kernel(PairHistParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(lds + PAIR_HIST_RING);      // [2][bins], alive for the whole strip
    int32_t* lab = reinterpret_cast<int32_t*>(lds);                          // [128 query | 128 corpus] labels, over the dead ring
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int bins = p.bins;
    for (int b = tid; b < 2 * bins; b += GEMM_THREADS) hist[b] = 0;
    double sum_r = 0.0, sum_u = 0.0;
    unsigned long long n_nan = 0;
    uint32_t kmin_r = 0xffffffffu, kmax_r = 0, kmin_u = 0xffffffffu, kmax_u = 0;
    auto flush = [&]() {                                        // LDS counters -> global histogram; leaves them zero
        __syncthreads();
        for (int b = tid; b < 2 * bins; b += GEMM_THREADS) {
            const uint32_t v = hist[b];
            if (v) { atomicAdd(&p.hist[b], (unsigned long long)v); hist[b] = 0; }
        }
        __syncthreads();
    };
    int done = 0;
    for (long long t = blockIdx.x; t < p.tiles; t += gridDim.x) {
        int qt, ct;
        if (p.self) tri_tile(t, qt, ct);
        else { qt = (int)(t / p.ctiles); ct = (int)(t % p.ctiles); }
        f32x16 acc[2][2];
        gemm_mainloop<float, 2>(p.g, qt, ct, 0, p.g.ktiles_total, lds, acc);
        __syncthreads();                                        // every wave is done with the staging ring
        {
            const int i = (tid < 128 ? qt * BM : ct * BN - 128) + tid;         // rows past the end carry the missing label
            lab[tid] = tid < 128 ? (i < p.Nq ? p.labels_q[i] : -1) : (i < p.Nc ? p.labels_c[i] : -1);
        }
        __syncthreads();
        const int li0 = wm * 64 + 4 * g, lj0 = 128 + wn * 64 + c;          // the lane's first value
        const int32_t lc0 = lab[lj0], lc1 = lab[lj0 + 32];
        const bool tri = p.self && qt == ct;                    // the diagonal tile: only j < i counts
        const int i0 = qt * BM + li0, j0 = ct * BN + wn * 64 + c;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int li = li0 + acc_row(mt, r, 0);
                const int32_t lq = lab[li];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int32_t lc = nt ? lc1 : lc0;
                    const int i = i0 + acc_row(mt, r, 0), j = j0 + acc_col(nt, 0);
                    if ((lq | lc) < 0 || (tri && j >= i)) continue;
                    const float s = acc[mt][nt][r];
                    if (s != s) { ++n_nan; continue; }
                    float x = floorf(__fdiv_rn(__fmul_rn(__fsub_rn(s, p.lo), p.fbins), p.span));
                    x = fminf(fmaxf(x, 0.f), p.fbins - 1.f);
                    const uint32_t k = score_key(s);
                    if (lq == lc) {
                        atomicAdd(&hist[(int)x], 1u);
                        kmin_r = min(kmin_r, k); kmax_r = max(kmax_r, k); sum_r += (double)s;
                    } else {
                        atomicAdd(&hist[bins + (int)x], 1u);
                        kmin_u = min(kmin_u, k); kmax_u = max(kmax_u, k); sum_u += (double)s;
                    }
                }
            }
        if ((++done & (PAIR_HIST_FLUSH_TILES - 1)) == 0) flush();
        __syncthreads();                                        // the labels are the next K loop's staging ring
    }
    flush();
    // the strip's running values: wave, then workgroup, in a fixed shape (scratch: the ring, dead after the last tile)
    PairHistRecord* wrec = reinterpret_cast<PairHistRecord*>(lds);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum_r += __shfl_xor(sum_r, o, 64); sum_u += __shfl_xor(sum_u, o, 64);
        n_nan += __shfl_xor(n_nan, o, 64);
        kmin_r = min(kmin_r, (uint32_t)__shfl_xor((int)kmin_r, o, 64)); kmax_r = max(kmax_r, (uint32_t)__shfl_xor((int)kmax_r, o, 64));
        kmin_u = min(kmin_u, (uint32_t)__shfl_xor((int)kmin_u, o, 64)); kmax_u = max(kmax_u, (uint32_t)__shfl_xor((int)kmax_u, o, 64));
    }
    if (lane == 0) {
        PairHistRecord& w = wrec[wave];
        w.sum[0] = sum_r; w.sum[1] = sum_u; w.n_nan = n_nan;
        w.kmin[0] = kmin_r; w.kmin[1] = kmin_u; w.kmax[0] = kmax_r; w.kmax[1] = kmax_u;
    }
    __syncthreads();
    if (tid == 0) {
        PairHistRecord o;
        o.sum[0] = (wrec[0].sum[0] + wrec[1].sum[0]) + (wrec[2].sum[0] + wrec[3].sum[0]);
        o.sum[1] = (wrec[0].sum[1] + wrec[1].sum[1]) + (wrec[2].sum[1] + wrec[3].sum[1]);
        o.n_nan = wrec[0].n_nan + wrec[1].n_nan + wrec[2].n_nan + wrec[3].n_nan;
        for (int k = 0; k < 2; ++k) {
            o.kmin[k] = min(min(wrec[0].kmin[k], wrec[1].kmin[k]), min(wrec[2].kmin[k], wrec[3].kmin[k]));
            o.kmax[k] = max(max(wrec[0].kmax[k], wrec[1].kmax[k]), max(wrec[2].kmax[k], wrec[3].kmax[k]));
        }
        p.rec[blockIdx.x] = o;
    }
}

// largest squared row 2-norm of an operand image (fp64), one partial per block: the automatic range of the linear kernel
__global__ __launch_bounds__(256) void row_norm2_max_kernel(const float* __restrict__ Y, int64_t ldy, int N, int Dp, double* __restrict__ part) {
    __shared__ double red[256];
    double best = 0.0;
    for (int i = blockIdx.x; i < N; i += gridDim.x) {
        const float* y = Y + (int64_t)i * ldy;
        double a = 0.0;
        for (int j = threadIdx.x; j < Dp; j += 256) { const double v = (double)y[j]; a += v * v; }
        red[threadIdx.x] = a;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        best = fmax(best, red[0]);                              // NaN rows drop out: their scores are NaN and enter no bin
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = best;
}

}  // namespace dae

using namespace dae;

extern "C" int32_t dae_pair_hist_max_bins(void) { return PAIR_HIST_MAX_BINS; }

// the workspace of pair_hist_sweep: labels, global histogram, per-workgroup records
static uint64_t pair_hist_sweep_bytes(int32_t Nq, int32_t Nc, int32_t bins) {
    return al256(pad128(Nq) * 4) + al256(pad128(Nc) * 4) + al256(2 * (uint64_t)bins * 8) + al256(PAIR_HIST_MAX_GRID * sizeof(PairHistRecord));
}

extern "C" uint64_t dae_pair_hist_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t bins) {
    if (Nq <= 0 || Nc <= 0 || D <= 0 || bins <= 0) return 0;
    // operand images, the sweep's share, norm partials of the automatic range
    return sweep_images_bytes(Nq, Nc, D) + pair_hist_sweep_bytes(Nq, Nc, bins) + al256(2 * PAIR_NORM_BLOCKS * 8);
}

extern "C" uint64_t dae_pair_hist_images_workspace(int32_t Nq, int32_t Nc, int32_t bins) {
    if (Nq <= 0 || Nc <= 0 || bins <= 0) return 0;
    return pair_hist_sweep_bytes(Nq, Nc, bins);
}

extern "C" uint64_t dae_sweep_image_norm2_max_workspace(void) { return al256(PAIR_NORM_BLOCKS * 8); }

// the largest squared row 2-norm (fp64) of the first `rows` rows of an image of width Dp, from the partials of row_norm2_max_kernel
static int image_norm2_max(const float* image, int32_t rows, int64_t Dp, double* npart, double* out_host, hipStream_t st) {
    DAE_LAUNCH(row_norm2_max_kernel, dim3(PAIR_NORM_BLOCKS), dim3(256), 0, st, image, Dp, (int)rows, (int)Dp, npart);
    DAE_CHECK_LAUNCH();
    double h[PAIR_NORM_BLOCKS];
    DAE_CHECK_HIP(hipMemcpyAsync(h, npart, PAIR_NORM_BLOCKS * 8, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    double m = 0.0;
    for (int k = 0; k < PAIR_NORM_BLOCKS; ++k) m = std::fmax(m, h[k]);
    *out_host = m;
    return 0;
}

extern "C" int dae_sweep_image_norm2_max(const float* image, int32_t rows, int32_t D, double* out_host, void* workspace,
                                         uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(image && out_host && workspace, "sweep_image_norm2_max: image / out / workspace are NULL");
    DAE_CHECK_ARG(rows > 0 && D > 0, "sweep_image_norm2_max: rows and D must be positive (got %d, %d)", rows, D);
    DAE_CHECK_ARG(pad128(rows) * pad128(D) * 4 < (1ll << 32), "sweep_image_norm2_max: an operand image exceeds 4 GiB");
    DAE_CHECK_ARG(workspace_bytes >= dae_sweep_image_norm2_max_workspace() && ((uintptr_t)workspace % 256) == 0,
                  "sweep_image_norm2_max: workspace too small / unaligned");
    return image_norm2_max(image, rows, pad128(D), (double*)workspace, out_host, (hipStream_t)stream);
}

// The sweep of dae_pair_hist and dae_pair_hist_images over two prepared images (g), lo < hi: labels up, histogram cleared,
// pair_hist_tiles_kernel, and the host's fold of the records into out16.  w: pair_hist_sweep_bytes of workspace.
static int pair_hist_sweep(const GemmParams& g, int32_t Nq, const int32_t* labels_q_host, int self, int32_t Nc, const int32_t* labels_c_host,
                           float lo, float hi, int32_t bins, uint64_t* hist_host, double* out16_host, char* w, hipStream_t st) {
    const int64_t Nqp = pad128(Nq), Ncp = pad128(Nc), qtiles = Nqp / BM, ctiles = Ncp / BN;
    const int64_t tiles = self ? qtiles * (qtiles + 1) / 2 : qtiles * ctiles;
    for (int k = 0; k < 16; ++k) out16_host[k] = std::nan("");
    int32_t* lq = (int32_t*)w;                  w += al256(Nqp * 4);
    int32_t* lc = self ? lq : (int32_t*)w;      w += al256(Ncp * 4);
    unsigned long long* hist = (unsigned long long*)w;   w += al256(2 * (uint64_t)bins * 8);
    PairHistRecord* rec = (PairHistRecord*)w;
    DAE_CHECK_HIP(hipMemcpyAsync(lq, labels_q_host, (size_t)Nq * 4, hipMemcpyHostToDevice, st));
    if (!self) DAE_CHECK_HIP(hipMemcpyAsync(lc, labels_c_host, (size_t)Nc * 4, hipMemcpyHostToDevice, st));
    DAE_CHECK_HIP(hipMemsetAsync(hist, 0, 2 * (size_t)bins * 8, st));
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        DAE_CHECK_HIP(hipGetDevice(&dev));
        DAE_CHECK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        cus = n > 0 ? n : 1;
    }
    int64_t grid = 2 * (int64_t)cus;
    if (grid > PAIR_HIST_MAX_GRID) grid = PAIR_HIST_MAX_GRID;
    if (grid > tiles) grid = tiles;
    PairHistParams p;
    memset(&p, 0, sizeof(p));
    p.g = g;
    p.Nq = Nq; p.Nc = Nc; p.self = self; p.ctiles = (int)ctiles; p.bins = bins; p.tiles = tiles;
    p.lo = lo; p.span = hi - lo; p.fbins = (float)bins;
    p.labels_q = lq; p.labels_c = lc; p.hist = hist; p.rec = rec;
    if (int rc = sweep_launch<pair_hist_tiles_kernel>(grid, PAIR_HIST_RING + 2 * PAIR_HIST_MAX_BINS * 4, PAIR_HIST_RING + 2 * bins * 4, st, p))
        return rc;
    std::vector<PairHistRecord> r((size_t)grid);
    DAE_CHECK_HIP(hipMemcpyAsync(hist_host, hist, 2 * (size_t)bins * 8, hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipMemcpyAsync(r.data(), rec, (size_t)grid * sizeof(PairHistRecord), hipMemcpyDeviceToHost, st));
    DAE_CHECK_HIP(hipStreamSynchronize(st));
    uint64_t n[2] = {0, 0}, n_nan = 0;
    for (int k = 0; k < 2; ++k)
        for (int b = 0; b < bins; ++b) n[k] += hist_host[(size_t)k * bins + b];
    double sum[2] = {0.0, 0.0};
    uint32_t kmin[2] = {0xffffffffu, 0xffffffffu}, kmax[2] = {0, 0};
    for (const PairHistRecord& o : r) {                         // index order: the sums are bit-identical run to run
        n_nan += o.n_nan;
        for (int k = 0; k < 2; ++k) {
            sum[k] += o.sum[k];
            kmin[k] = o.kmin[k] < kmin[k] ? o.kmin[k] : kmin[k];
            kmax[k] = o.kmax[k] > kmax[k] ? o.kmax[k] : kmax[k];
        }
    }
    out16_host[0] = (double)n[0]; out16_host[1] = (double)n[1]; out16_host[2] = (double)n_nan;
    for (int k = 0; k < 2; ++k)
        if (n[k]) {
            out16_host[3 + k] = sum[k];
            out16_host[5 + 2 * k] = (double)key_score(kmin[k]);
            out16_host[6 + 2 * k] = (double)key_score(kmax[k]);
        }
    out16_host[9] = (double)lo; out16_host[10] = (double)hi;
    out16_host[11] = (double)grid; out16_host[12] = (double)tiles;
    return 0;
}

extern "C" int dae_pair_hist_images(const float* Qi, int32_t Nq, const int32_t* labels_q_host, const float* Ci, int32_t Nc,
                                    const int32_t* labels_c_host, int32_t D, float lo, float hi, int32_t bins, uint64_t* hist_host,
                                    double* out16_host, void* workspace, uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(labels_q_host && hist_host && out16_host, "pair_hist_images: labels_q / hist / out16 are NULL");
    DAE_CHECK_ARG(!Ci || labels_c_host, "pair_hist_images: with Ci, labels_c is needed");
    DAE_CHECK_ARG(bins >= 2 && bins <= PAIR_HIST_MAX_BINS, "pair_hist_images: bins must be in 2..%d (got %d)", PAIR_HIST_MAX_BINS, bins);
    DAE_CHECK_ARG(std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo),
                  "pair_hist_images: lo / hi must be finite with lo < hi (there is no automatic range here) and hi - lo must not overflow fp32");
    SweepOperands o;
    if (int rc = sweep_prepare_images("pair_hist_images", Qi, Nq, Ci, Nc, D, workspace, workspace_bytes,
                                      dae_pair_hist_images_workspace(Nq, Nc, bins), o))
        return rc;
    const int64_t qtiles = o.Nqp / BM, ctiles = o.Ncp / BN;
    DAE_CHECK_ARG((Ci ? qtiles * ctiles : qtiles * (qtiles + 1) / 2) < (1ll << 31), "pair_hist_images: the tiles exceed the enumeration");
    return pair_hist_sweep(o.g, Nq, labels_q_host, Ci ? 0 : 1, Nc, labels_c_host, lo, hi, bins, hist_host, out16_host, o.rest, (hipStream_t)stream);
}

extern "C" int dae_pair_hist(const float* Q, int64_t ldq, int32_t Nq, const int32_t* labels_q_host, const float* C, int64_t ldc,
                             int32_t Nc, const int32_t* labels_c_host, int32_t D, int32_t norm, int32_t metric, float lo, float hi,
                             int32_t bins, uint64_t* hist_host, double* out16_host, void* workspace, uint64_t workspace_bytes,
                             void* stream) {
    DAE_CHECK_ARG(Q && labels_q_host && workspace && Nq > 0 && D > 0, "pair_hist: bad input");
    DAE_CHECK_ARG(hist_host && out16_host, "pair_hist: hist / out16 are NULL");
    DAE_CHECK_ARG(ldq >= D, "pair_hist: ldq (%lld) must be >= D (%d)", (long long)ldq, D);
    DAE_CHECK_ARG(C ? (Nc > 0 && ldc >= D && labels_c_host) : Nc == Nq,
                  "pair_hist: bad corpus (C == NULL means the corpus is Q: pass Nc == Nq; with C, labels_c is needed)");
    DAE_CHECK_ARG(bins >= 2 && bins <= PAIR_HIST_MAX_BINS, "pair_hist: bins must be in 2..%d (got %d)", PAIR_HIST_MAX_BINS, bins);
    DAE_CHECK_ARG(std::isfinite(lo) && std::isfinite(hi), "pair_hist: lo / hi must be finite (lo >= hi asks for the automatic range)");
    DAE_CHECK_ARG(lo >= hi || std::isfinite(hi - lo), "pair_hist: hi - lo overflows fp32");
    const int self = C ? 0 : 1;
    const int64_t Nqp = pad128(Nq), Ncp = pad128(Nc), qtiles = Nqp / BM, ctiles = Ncp / BN;
    const int64_t tiles = self ? qtiles * (qtiles + 1) / 2 : qtiles * ctiles;
    DAE_CHECK_ARG(tiles < (1ll << 31), "pair_hist: %lld tiles exceed the enumeration", (long long)tiles);
    hipStream_t st = (hipStream_t)stream;
    SweepOperands o;
    if (int rc = sweep_prepare("pair_hist", Q, ldq, Nq, C, ldc, Nc, D, norm, metric, workspace, workspace_bytes,
                               dae_pair_hist_workspace(Nq, Nc, D, bins), st, o))
        return rc;
    for (int k = 0; k < 16; ++k) out16_host[k] = std::nan("");
    const float *Qi = o.Qi, *Ci = o.Ci;
    const int64_t Dp = o.Dp;
    if (lo >= hi) {                                             // the automatic range
        if (metric == 0) { lo = -1.f; hi = 1.f; }
        else {
            // Cauchy-Schwarz: |score| <= (largest row norm of Qi) x (largest row norm of Ci), rounded up by one part in 2^20
            double* npart = (double*)(o.rest + pair_hist_sweep_bytes(Nq, Nc, bins));
            double mq = 0.0, mc = 0.0;
            if (int rc = image_norm2_max(Qi, Nq, Dp, npart, &mq, st)) return rc;
            if (C) { if (int rc = image_norm2_max(Ci, Nc, Dp, npart + PAIR_NORM_BLOCKS, &mc, st)) return rc; }
            else mc = mq;
            const double M = std::sqrt(mq) * std::sqrt(mc) * (1.0 + 1.0 / 1048576.0);
            float Mf = (float)M;
            if ((double)Mf < M) Mf = std::nextafterf(Mf, INFINITY);
            if (!(Mf > 0.f) || !std::isfinite(Mf)) Mf = 1.f;    // all-zero rows (every score is 0) / overflowing norms
            lo = -Mf; hi = Mf;
        }
    }
    return pair_hist_sweep(o.g, Nq, labels_q_host, self, Nc, labels_c_host, lo, hi, bins, hist_host, out16_host, o.rest, st);
}
