// dae_user_fit.hip -- the training step of the decay user model (dae_user_pair_loss): pairwise ranking loss of the relevance
// R(u, a) = (alpha . u) . a over click histories, with its gradients with respect to alpha and beta, in one walk of every
// history.  "Embedding-based News Recommendation for Millions of Users" (KDD'17) learns alpha (one weight per embedding
// dimension) and the decay beta this way; E is fixed, so there is no backward pass.
//
// Per user, events oldest first (definition: include/dae_hip.h).  The state before event e is s / z; beside it runs the
// derivative chain g = ds/dbeta, zg = dz/dbeta.  Event e is scored against each of its sampled negatives n:
//     D = E[items[e]] - E[n];   x = (sum alpha s D) / z;   xb = (sum alpha g D) / z - x zg / z
//     loss += softplus(-x);   c = -sigmoid(-x);   dalpha += c s D / z;   dbeta += c xb
// then folded in:  g = f g + f' s;  zg = f zg + f' z;  s = f s + E[item];  z = f z + 1   (old s, z on the right).
// Neither the [events x H] matrix of states nor its beta-derivative is ever stored.
//
// Layout.  One wave per user over all of H: a lane owns CPL = 4 / 8 / 16 columns (H <= 256 / 512 / 1024) in groups of four
// adjacent ones, columns 256 k + 4 lane .. + 3 -- in registers s, g, alpha and the dalpha accumulator, 4 CPL floats, plus the
// 1 + UF_NB rows of the event in flight.  The column a lane owns does NOT depend on the load path: VEC (16-byte aligned E, lde
// and H multiples of 4) reads a group with one 16-byte load, the scalar path reads the same four columns with four 4-byte
// loads.  So both paths run the same arithmetic on the same values in the same order, and the margins are bit-identical
// between them (a strided view and its contiguous copy agree whatever their alignment).
// A wave reads 64 item ids, factors and negative ids with one load per lane each and hands them out by readlane, as
// user_states_kernel does.  The rows of ONE event are in flight per wave: prefetching the next event's 1 + UF_NB rows would add
// 5 CPL registers (40 at CPL 8: a wave per SIMD less), and the other waves of the SIMD are there to cover the gather's latency (at
// CPL 8 each waiting wave has 10 KB in flight).
// n_neg > UF_NB: the history is walked once per chunk of UF_NB negatives (the chain is recomputed: 4 fused multiply-adds per
// column and event against 5 operations per column and pair), so the registers do not grow with n_neg.
//
// Reductions.  The two dot products of a pair are summed per lane in column order with fmaf, then over the wave by the DPP
// tree of dae_common.h (wave64_sum_hi), both trees interleaved; lane 63's sum is broadcast by readlane.  What follows the sums --
// the one IEEE division per pair that gives x, exp, log1p, the sigmoid -- runs once per event for its UF_NB pairs, lane j taking
// pair j; lane j also keeps the loss, dbeta and pair count of the j-th negatives, and the lanes are added up at the end.
//
// Accumulation.  fp32 accumulators never span more than 64 events of one user: dalpha is added up in fp32 within a block of 64
// events and then moved into fp64; loss and dbeta go into fp64 pair by pair.  Across its users a wave accumulates in fp64 and
// keeps one [64 CPL + 3] partial in the workspace (fp64 sums and the bits of an int64 pair count); user_pair_fold_kernel adds the partials in wave
// order.  No atomics.  The grid is a function of M and the CU count alone, user u belongs to wave u mod waves, so everything
// is bit-identical run to run; the margins and the pair count do not depend on the grid or the user order at all.
//
// Scheduling.  waves = min(ceil4(M), 32 per CU, UF_MAX_WAVES): more waves than are resident at once (registers allow 4 per SIMD
// at CPL 8, i.e. 16 per CU), so the dispatcher backfills a CU as soon as a workgroup's users are done, and the
// modular assignment spreads neighbouring users -- and with them any run of long histories -- over all waves.  The longest
// single history still is one wave's work: a wave owns a whole user because the chain is sequential.
#include "dae_common.h"

#include <algorithm>

namespace dae {

constexpr int UF_THREADS = 256;             // 4 waves per workgroup
constexpr int UF_NB = 4;                    // negatives scored per walk of a history
constexpr int UF_MAX_WAVES = 8192;          // bounds the workspace without knowing the device (32 waves on each of 256 CUs)
constexpr int UF_MAX_H = 1024;
constexpr int UF_MAX_NEG = 16;

struct UserFitArgs {
    const float* E; int64_t lde; int Na, H;
    const int64_t* indptr; const int32_t* items; const float* decay; const float* ddecay; float beta;
    const float* alpha; const int32_t* negatives; int n_neg;
    int64_t M; int waves;
    double* part; float* margin;
};

__device__ __forceinline__ float lane_bcast(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// the CPL columns of a row that the lane owns; cc holds their offsets, clamped into the row
__device__ __forceinline__ double lane_bcast64(double v, int l) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(b >> 32), l);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

template <int CPL, bool VEC>
__device__ __forceinline__ void load_row(const float* r, const int (&cc)[CPL], float (&x)[CPL]) {
    if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < CPL / 4; ++k) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(r + cc[4 * k]);
#pragma unroll
            for (int q = 0; q < 4; ++q) x[4 * k + q] = v[q];
        }
    } else {
#pragma unroll
        for (int q = 0; q < CPL; ++q) x[q] = r[cc[q]];
    }
}

template <int CPL, bool VEC>
__global__ __launch_bounds__(UF_THREADS) void user_pair_loss_kernel(UserFitArgs a) {
    const int lane = threadIdx.x & 63;
    const int w = (int)blockIdx.x * (UF_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= a.waves) return;
    // A column past H reads a column inside the row instead (the last one; VEC: the last group of four) and carries alpha = 0: it adds
    // exact zeros to both dot products, and its dalpha is never written.
    int cc[CPL]; float al[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int col = (q >> 2) * 256 + lane * 4 + (q & 3);
        cc[q] = VEC ? min(col - (q & 3), a.H - 4) + (q & 3) : min(col, a.H - 1);
        al[q] = col < a.H ? a.alpha[col] : 0.f;
    }
    // the wave's fp64 partial lives in the workspace: only this wave touches it, each lane its own columns, in program order
    // (a row of the partials has all 64 CPL columns, so that no store needs a mask; the fold reads the first H and what follows the columns)
    double* o = a.part + (int64_t)w * (64 * CPL + 3);
    volatile double* ol = o + lane * 4;              // volatile: the sums stay in memory instead of being promoted to 2 CPL registers
#pragma unroll
    for (int q = 0; q < CPL; ++q) ol[(q >> 2) * 256 + (q & 3)] = 0.0;
    double loss64 = 0.0, dbeta64 = 0.0;
    int64_t pairs = 0;
    const int nchunks = (a.n_neg + UF_NB - 1) / UF_NB;
    for (int64_t u = w; u < a.M; u += a.waves) {
        const int64_t e0 = a.indptr[u], e1 = a.indptr[u + 1];
        for (int c = 0; c < nchunks; ++c) {
            const int j0 = c * UF_NB;
            float s[CPL], g[CPL], z = 0.f, zg = 0.f;
#pragma unroll
            for (int q = 0; q < CPL; ++q) { s[q] = 0.f; g[q] = 0.f; }
            for (int64_t base = e0; base < e1; base += 64) {
                const int64_t ke = min(base + lane, e1 - 1);
                const int raw = a.items[ke];
                const int it = min(max(raw, 0), a.Na - 1);              // a caller error (see dae_hip.h) must not become a stray read
                float f = a.decay ? a.decay[ke] : a.beta;
                float fp = a.decay ? (a.ddecay ? a.ddecay[ke] : 0.f) : 1.f;
                if (ke == e0) { f = 0.f; fp = 0.f; }                    // the first event starts the chain: s = E[item], z = 1, g = zg = 0
                int ng[UF_NB];
#pragma unroll
                for (int j = 0; j < UF_NB; ++j) {
                    int v = j0 + j < a.n_neg ? a.negatives[ke * a.n_neg + j0 + j] : -1;
                    if (v == raw || ke == e0) v = -1;                   // not a pair: the positive itself, or nothing to predict from
                    ng[j] = v;
                }
                const int n = (int)min((int64_t)64, e1 - base);
                float da[CPL];
#pragma unroll
                for (int q = 0; q < CPL; ++q) da[q] = 0.f;
                for (int i = 0; i < n; ++i) {
                    const int row = __builtin_amdgcn_readlane(it, i);
                    const float fi = lane_bcast(f, i), fpi = lane_bcast(fp, i);
                    int nj[UF_NB];
                    float P[CPL], N[UF_NB][CPL];
                    load_row<CPL, VEC>(a.E + (int64_t)row * a.lde, cc, P);
#pragma unroll
                    for (int j = 0; j < UF_NB; ++j) {
                        nj[j] = __builtin_amdgcn_readlane(ng[j], i);
                        load_row<CPL, VEC>(a.E + (int64_t)min(max(nj[j], 0), a.Na - 1) * a.lde, cc, N[j]);
                    }
                    // lane j < UF_NB takes the two sums of pair j: what follows the dot products is done once for the pairs of an event
                    float vd1 = 0.f, vd2 = 0.f;
                    int okbits = 0;
#pragma unroll
                    for (int j = 0; j < UF_NB; ++j) {
                        if (nj[j] >= 0) {                               // the same in every lane
                            float p1 = 0.f, p2 = 0.f;
#pragma unroll
                            for (int q = 0; q < CPL; ++q) {
                                const float D = P[q] - N[j][q];
                                N[j][q] = s[q] * D;                     // kept for dalpha
                                p1 = fmaf(al[q], N[j][q], p1);
                                p2 = fmaf(g[q], al[q] * D, p2);
                            }
                            const float d1 = lane_bcast(wave64_sum_hi(p1), 63), d2 = lane_bcast(wave64_sum_hi(p2), 63);
                            vd1 = lane == j ? d1 : vd1;
                            vd2 = lane == j ? d2 : vd2;
                            okbits |= 1 << j;
                        }
                    }
                    float x = 0.f;
                    if (okbits) {
                        const bool ok = lane < UF_NB && ((okbits >> lane) & 1);
                        const float rz = 1.0f / z;
                        x = ok ? vd1 / z : 0.f;                         // the one division that defines the margin
                        const float xb = (vd2 - x * zg) * rz;
                        const float ee = __expf(-fabsf(x));             // ~2 ulp of a value <= 1
                        const float r = 1.0f / (1.0f + ee);
                        const float c = -(x >= 0.f ? ee * r : r);       // -sigmoid(-x)
                        loss64 += ok ? (double)(fmaxf(-x, 0.f) + log1pf(ee)) : 0.0;
                        dbeta64 += ok ? (double)(c * xb) : 0.0;
                        pairs += ok ? 1 : 0;
                        const float czv = c * rz;
#pragma unroll
                        for (int j = 0; j < UF_NB; ++j) {
                            if (nj[j] >= 0) {
                                const float cz = lane_bcast(czv, j);
#pragma unroll
                                for (int q = 0; q < CPL; ++q) da[q] = fmaf(cz, N[j][q], da[q]);
                            }
                        }
                    }
                    if (a.margin && lane < UF_NB && j0 + lane < a.n_neg) a.margin[(base + i) * a.n_neg + j0 + lane] = x;
#pragma unroll
                    for (int q = 0; q < CPL; ++q) {
                        g[q] = fmaf(fi, g[q], fpi * s[q]);
                        s[q] = fmaf(fi, s[q], P[q]);
                    }
                    zg = fmaf(fi, zg, fpi * z);
                    z = fmaf(fi, z, 1.0f);
                }
#pragma unroll
                for (int q = 0; q < CPL; ++q)
                    ol[(q >> 2) * 256 + (q & 3)] += (double)da[q];
            }
        }
    }
    // lane j holds the sums of the j-th negative of every chunk: add them in lane order
    double lsum = 0.0, bsum = 0.0;
    int64_t psum = 0;
#pragma unroll
    for (int j = 0; j < UF_NB; ++j) {
        lsum += lane_bcast64(loss64, j);
        bsum += lane_bcast64(dbeta64, j);
        psum += __builtin_bit_cast(int64_t, lane_bcast64(__builtin_bit_cast(double, pairs), j));
    }
    if (lane == 0) { o[64 * CPL] = lsum; o[64 * CPL + 1] = bsum; o[64 * CPL + 2] = __builtin_bit_cast(double, psum); }
}

// adds the per-wave partials (rows of cols + 3 doubles, the last one the bits of an int64) in wave order: thread h < H makes dalpha[h], H the loss, H + 1 dbeta, H + 2 the pair count
__global__ __launch_bounds__(256) void user_pair_fold_kernel(const double* part, int waves, int H, int cols, double* loss,
                                                             double* dalpha, double* dbeta, int64_t* n_pairs) {
    const int h = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (h < H + 2) {
        double v = 0.0;
        const int k = h < H ? h : cols + h - H;
        for (int w = 0; w < waves; ++w) v += part[(int64_t)w * (cols + 3) + k];
        if (h < H) dalpha[h] = v;
        else if (h == H) *loss = v;
        else *dbeta = v;
    } else if (h == H + 2) {
        int64_t n = 0;
        for (int w = 0; w < waves; ++w) n += __builtin_bit_cast(int64_t, part[(int64_t)w * (cols + 3) + cols + 2]);
        *n_pairs = n;
    }
}

static int part_cols(int H) { return H <= 256 ? 256 : H <= 512 ? 512 : 1024; }      // 64 x the columns per lane

static int64_t wave_cap(int64_t M) {
    const int64_t w = (std::max<int64_t>(M, 1) + 3) / 4 * 4;
    return w < UF_MAX_WAVES ? w : UF_MAX_WAVES;
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_user_pair_loss_workspace(int64_t M, int32_t H) {
    if (M < 0 || H <= 0 || H > UF_MAX_H) return 0;
    return (uint64_t)wave_cap(M) * (uint64_t)(part_cols(H) + 3) * 8;
}

extern "C" int dae_user_pair_loss(const float* E, int64_t lde, int32_t Na, int32_t H, const int64_t* indptr, const int32_t* items,
                                  int64_t M, int64_t nnz, float beta, const float* decay, const float* ddecay, const float* alpha,
                                  const int32_t* negatives, int32_t n_neg, double* loss, double* dalpha, double* dbeta,
                                  int64_t* n_pairs, float* margin, void* workspace, uint64_t workspace_bytes, void* stream) {
    DAE_CHECK_ARG(M >= 0 && nnz >= 0, "user_pair_loss: negative count (M = %lld, nnz = %lld)", (long long)M, (long long)nnz);
    DAE_CHECK_ARG(H > 0 && H <= UF_MAX_H, "user_pair_loss: H must be in 1..%d (got %d)", UF_MAX_H, H);
    DAE_CHECK_ARG(Na > 0, "user_pair_loss: Na must be positive (got %d)", Na);
    DAE_CHECK_ARG(n_neg >= 1 && n_neg <= UF_MAX_NEG, "user_pair_loss: n_neg must be in 1..%d (got %d)", UF_MAX_NEG, n_neg);
    DAE_CHECK_ARG(E && indptr && alpha, "user_pair_loss: E / indptr / alpha are NULL");
    DAE_CHECK_ARG((items && negatives) || nnz == 0, "user_pair_loss: items / negatives are NULL");
    DAE_CHECK_ARG(loss && dalpha && dbeta && n_pairs, "user_pair_loss: loss / dalpha / dbeta / n_pairs are NULL");
    DAE_CHECK_ARG(lde >= H, "user_pair_loss: lde (%lld) must be >= H (%d)", (long long)lde, H);
    DAE_CHECK_ARG(decay || !ddecay, "user_pair_loss: ddecay without decay");
    DAE_CHECK_ARG(decay || (beta >= 0.f && beta <= 1.f), "user_pair_loss: beta must be in [0, 1] (got %g)", (double)beta);
    const uint64_t need = dae_user_pair_loss_workspace(M, H);
    DAE_CHECK_ARG(workspace && workspace_bytes >= need, "user_pair_loss: workspace too small (%llu bytes, need %llu)",
                  (unsigned long long)(workspace ? workspace_bytes : 0), (unsigned long long)need);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "user_pair_loss: workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int waves = 0;
    if (M > 0) {
        static int cus = 0;
        if (cus == 0) {
            int dev = 0, n = 0;
            DAE_CHECK_HIP(hipGetDevice(&dev));
            DAE_CHECK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
            cus = n > 0 ? n : 1;
        }
        waves = (int)std::min<int64_t>(wave_cap(M), (int64_t)cus * 32);
    }
    UserFitArgs a;
    a.E = E; a.lde = lde; a.Na = Na; a.H = H; a.indptr = indptr; a.items = items; a.decay = decay; a.ddecay = ddecay; a.beta = beta;
    a.alpha = alpha; a.negatives = negatives; a.n_neg = n_neg; a.M = M; a.waves = waves;
    a.part = (double*)workspace; a.margin = margin;
    if (waves > 0) {
        const dim3 grid((unsigned)(waves / (UF_THREADS / 64))), block(UF_THREADS);
        const bool vec = H % 4 == 0 && lde % 4 == 0 && ((uintptr_t)E % 16) == 0;
        const int cpl = part_cols(H) / 64;
        void (*kern)(UserFitArgs) = nullptr;
        if (cpl == 4) kern = vec ? user_pair_loss_kernel<4, true> : user_pair_loss_kernel<4, false>;
        else if (cpl == 8) kern = vec ? user_pair_loss_kernel<8, true> : user_pair_loss_kernel<8, false>;
        else kern = vec ? user_pair_loss_kernel<16, true> : user_pair_loss_kernel<16, false>;
        DAE_LAUNCH(kern, grid, block, 0, st, a);
        DAE_CHECK_LAUNCH();
    }
    DAE_LAUNCH(user_pair_fold_kernel, dim3((unsigned)((H + 3 + 255) / 256)), dim3(256), 0, st, a.part, waves, (int)H, part_cols(H), loss, dalpha,
               dbeta, n_pairs);
    DAE_CHECK_LAUNCH();
    return 0;
}
