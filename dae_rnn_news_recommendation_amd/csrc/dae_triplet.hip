// dae_triplet.hip -- online triplet miners on the dot-product Gram matrix D = h h^T.
//
// batch_all  (triplet_loss_utils.py:79-131): the reference materialises ~8 tensors of B^3 elements
//   (2 GB each at B=800).  Here one workgroup per anchor streams its D row into LDS, compacts the
//   positives (same label, != anchor) and negatives (different label) in index order, and sweeps the
//   |P| x |N| rectangle once per role with the operands in registers/LDS -- nothing B^3 ever exists.
//   Outputs per anchor: sum softplus(D[a,n]-D[a,p]), #positive triplets, and the un-normalised
//   gradient row G[a,:] (sum of sigmoids with the role's sign).  N_valid / data_weight are integer
//   closed forms of the label histogram (dae_label_stats).
// batch_hard (triplet_loss_utils.py:202-259): one workgroup per anchor, wavefront-shuffle max/min
//   reductions; reproduces the reference's quirks literally (invalid negatives contribute 0, invalid
//   positives are shifted by the row max, float-equality data_weight, gradient ties split equally,
//   gradient through the row-max shift).
#include <type_traits>

#include "dae_common.h"
#include "dae_kernels.h"
#include "dae_miner_tile.h"

namespace dae {

constexpr int TRIP_THREADS = 256;
constexpr int TRIP_MAX_B = 4096;

// block-wide helpers (256 threads = 4 waves)
__device__ __forceinline__ float block_sum_f(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ unsigned block_sum_u(unsigned v, unsigned* red) {
    v = wave_sum_u32(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max_f(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_min_f(float v, float* red) {
    v = wave_min(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

// softplus(t) and sigmoid(t) from one exp (TF: -log_sigmoid(-t) = softplus(t); SoftplusGrad = sigmoid)
__device__ __forceinline__ void softplus_sigmoid(float t, float& sp, float& sg) {
    const float en = __expf(-fabsf(t));                       // in (0,1]
    const float r = __frcp_rn(1.0f + en);
    const float l = en < 1e-4f ? en * (1.0f - 0.5f * en) : __logf(1.0f + en);
    sp = fmaxf(t, 0.f) + l;
    sg = t >= 0.f ? r : en * r;
}
__device__ __forceinline__ float sigmoid_only(float t) {
    const float en = __expf(-fabsf(t));
    const float r = __frcp_rn(1.0f + en);
    return t >= 0.f ? r : en * r;
}

// Sweep of the |P| x |N| rectangle of one anchor.  Work split: WAVE w owns the positives p = w, w+4, w+8, ...
// and walks ALL negatives in chunks of 64*Q (lane l keeps negatives k0 + q*64 + l, q < Q, in registers), so a
// positive's gradient is complete inside one wave and the per-positive overhead is amortised over Q pairs per
// lane.  Each (p, n) pair is evaluated once: softplus for the loss, sigmoid for both gradient roles.
//   positive role: sum over the wave's lanes with a wavefront DPP reduction (VALU operand path, no LDS round
//                  trip), accumulated by lane 63 into gpos[p] -- a single owner, fixed order, deterministic;
//   negative role: per-wave partial sums in registers, parked in gneg_w[wave][k] and added up over the 4 waves
//                  in wave order at the end.
// Lanes without a negative carry v = -inf: v - u = -inf gives softplus = 0, sigmoid = 0, "positive" = false,
// so the hot loop needs no masks.
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

// FACT = true: exp(v - u) is formed as E_n * F_p with E_n = exp(v_n - m) (one per lane register) and F_p = exp(m - u_p)
// (one LDS value per positive), m = mid-range of the anchor's D row -- one transcendental less per pair.  Used when
// the row's range is <= 80 so that neither factor nor the product can overflow; otherwise the direct form runs.
template <bool POS_ONLY, int Q, bool FACT, bool FIRST>
__device__ __forceinline__ void sweep_pairs(const float* __restrict__ pu, const float* __restrict__ pf, float mid,
                                            const float* __restrict__ nv, int nP, int nN,
                                            int k0, int wave, int lane, float* __restrict__ gpos,
                                            unsigned* __restrict__ cpos, float* __restrict__ gneg_w,
                                            unsigned* __restrict__ cneg_w, float& loss, unsigned& cnt) {
    float v[Q], gs[Q], ev[Q];
    unsigned rc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int k = k0 + q * 64 + lane;
        v[q] = (k < nN) ? nv[k] : -INFINITY;
        ev[q] = FACT ? __builtin_amdgcn_exp2f((v[q] - mid) * kLog2e) : 0.f;      // exp(-inf) = 0 for padding lanes
        gs[q] = 0.f; rc[q] = 0u;
    }
    // two positives per iteration (p and p+4): their DPP reduction chains and LDS traffic interleave
    for (int p = wave; p < nP; p += 8) {
        const bool has2 = (p + 4) < nP;
        float u[2], fp[2], sgp[2];
        unsigned cp[2];
        u[0] = pu[p]; u[1] = has2 ? pu[p + 4] : INFINITY;               // u = +inf -> t = -inf -> contributes nothing
        fp[0] = FACT ? pf[p] : 0.f; fp[1] = (FACT && has2) ? pf[p + 4] : 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            sgp[h] = 0.f; cp[h] = 0u;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float t = v[q] - u[h];                            // triplet_distance[a,p,n]  (:106)
                float sp, sg;
                if constexpr (FACT) {
                    const float e = ev[q] * fp[h];                      // exp(t)
                    const float w = 1.0f + e;
                    const float r = __builtin_amdgcn_rcpf(w);
                    float lg = kLn2 * __builtin_amdgcn_logf(w);
                    asm volatile("" : "+v"(lg));                        // keep the log unconditional: no per-pair branch
                    sp = e < 1e-4f ? e * (1.0f - 0.5f * e) : lg;       // softplus(t) = log1p(exp(t))  (:126)
                    sg = e * r;                                         // sigmoid(t) = SoftplusGrad
                } else {
                    const float en = __builtin_amdgcn_exp2f(-fabsf(t) * kLog2e);    // exp(-|t|) in [0,1]
                    const float w = 1.0f + en;
                    const float r = __builtin_amdgcn_rcpf(w);
                    float lg = kLn2 * __builtin_amdgcn_logf(w);
                    asm volatile("" : "+v"(lg));
                    const float l = en < 1e-4f ? en * (1.0f - 0.5f * en) : lg;   // log1p(en)
                    sp = fmaxf(t, 0.f) + l;                             // softplus(t) = -log_sigmoid(-t)  (:126)
                    sg = t >= 0.f ? r : en * r;                         // sigmoid(t) = SoftplusGrad
                }
                const bool pos = t > 1e-16f;                            // (:114)
                loss += POS_ONLY ? (pos ? sp : 0.f) : sp;
                const float sgu = POS_ONLY ? (pos ? sg : 0.f) : sg;
                gs[q] += sgu;
                sgp[h] += sgu;
                cnt += pos ? 1u : 0u;
                if (POS_ONLY) { rc[q] += pos ? 1u : 0u; cp[h] += pos ? 1u : 0u; }
            }
        }
        sgp[0] = wave64_sum_hi(sgp[0]);
        sgp[1] = wave64_sum_hi(sgp[1]);
        if (POS_ONLY) { cp[0] = wave_sum_u32(cp[0]); cp[1] = wave_sum_u32(cp[1]); }
        if (lane == 63) {
            if (FIRST) { gpos[p] = sgp[0]; if (has2) gpos[p + 4] = sgp[1]; }
            else { gpos[p] += sgp[0]; if (has2) gpos[p + 4] += sgp[1]; }
            if (POS_ONLY) {
                if (FIRST) { cpos[p] = cp[0]; if (has2) cpos[p + 4] = cp[1]; }
                else { cpos[p] += cp[0]; if (has2) cpos[p + 4] += cp[1]; }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int k = k0 + q * 64 + lane;
        if (k < nN) { gneg_w[k] = gs[q]; if (POS_ONLY) cneg_w[k] = rc[q]; }
    }
}

// Pair-packed sweep (row range <= 40, all triplets counted): lane registers hold the negatives as float2 pairs so the
// element-wise work runs on packed-fp32 VALU ops (v_pk_mul/add_f32: two pairs per instruction), and the two
// transcendentals are SHARED by the two pairs of a register: with w = 1 + exp(t),
//     log w_a + log w_b = log(w_a w_b),      1/w_a = w_b / (w_a w_b),      1/w_b = w_a / (w_a w_b)
// -- one v_log_f32 and one v_rcp_f32 (quarter-rate instructions) per TWO triplets instead of two each.  Only sums of
// log terms are ever needed (the loss is a sum), and range <= 40 bounds w_a w_b by e^80 < FLT_MAX.  log1p accuracy for
// small exp(t) comes from the first-order correction  log1p(e) = log(fl(1+e)) + (e - (fl(1+e) - 1)) / fl(1+e)
// instead of a per-pair select.  ~12 issue slots per triplet against ~27 for sweep_pairs (2 x 4 of them transcendental).
typedef float f32x2 __attribute__((ext_vector_type(2)));
// FAST (bf16 training mode): sigmoid(t) = e/(1+e) = 1 - 1/w, so only the sums of r = 1/w are accumulated and turned into
// sums of sigmoids at the end (count of lane slots minus sum r; padding slots have e = 0 -> r = 1 -> sigmoid 0, so they need
// no mask), and the first-order log1p correction is dropped: log(fl(1+e)) is within 2^-24 ABSOLUTE of log1p(e) per triplet.
// 11 issue slots per triplet instead of 18.  The caller checks the anchor's mean term against that absolute bound and
// re-runs the anchor with FAST = false when it could exceed 2e-6 relative (well-separated embeddings: every term tiny).
template <int Q2, bool FIRST, bool FAST>
__device__ __forceinline__ void sweep_pairs2(const float* __restrict__ pu, const float* __restrict__ pf, float mid,
                                             const float* __restrict__ nv, int nP, int nN, int k0, int wave, int lane,
                                             float* __restrict__ gpos, float* __restrict__ gneg_w, float& loss_log2,
                                             float& loss_corr, unsigned& cnt_wave) {
    f32x2 v2[Q2], ev2[Q2], gs2[Q2];
#pragma unroll
    for (int q = 0; q < Q2; ++q) {
        const int k = k0 + (2 * q) * 64 + lane;
        v2[q].x = (k < nN) ? nv[k] : -INFINITY;
        v2[q].y = (k + 64 < nN) ? nv[k + 64] : -INFINITY;
        ev2[q].x = __builtin_amdgcn_exp2f((v2[q].x - mid) * kLog2e);          // exp(-inf) = 0 for padding lanes
        ev2[q].y = __builtin_amdgcn_exp2f((v2[q].y - mid) * kLog2e);
        gs2[q] = f32x2{0.f, 0.f};
    }
    f32x2 corr2 = {0.f, 0.f};
    int iters = 0;
    for (int p = wave; p < nP; p += 8) {
        ++iters;
        const bool has2 = (p + 4) < nP;
        float u[2], fp[2], sgp[2];
        u[0] = pu[p]; u[1] = has2 ? pu[p + 4] : INFINITY;               // u = +inf -> t = -inf, F_p = 0 -> contributes nothing
        fp[0] = pf[p]; fp[1] = has2 ? pf[p + 4] : 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x2 sgp2 = {0.f, 0.f};
#pragma unroll
            for (int q = 0; q < Q2; ++q) {
                const f32x2 t2 = v2[q] - u[h];                           // triplet_distance[a,p,n]  (:106)
                if constexpr (FAST) {
                    const f32x2 w2 = ev2[q] * fp[h] + 1.0f;              // 1 + exp(t)   (one packed fma)
                    const float P = w2.x * w2.y;
                    const float R = __builtin_amdgcn_rcpf(P);
                    loss_log2 += __builtin_amdgcn_logf(P);               // log2(w_a) + log2(w_b)
                    const f32x2 r2 = f32x2{w2.y, w2.x} * R;              // 1/w_a, 1/w_b  = 1 - sigmoid(t)
                    gs2[q] += r2;
                    sgp2 += r2;
                } else {
                    const f32x2 e2 = ev2[q] * fp[h];                     // exp(t)
                    const f32x2 w2 = e2 + 1.0f;
                    const float P = w2.x * w2.y;
                    const float R = __builtin_amdgcn_rcpf(P);
                    loss_log2 += __builtin_amdgcn_logf(P);               // log2(w_a) + log2(w_b)
                    const f32x2 r2 = f32x2{w2.y, w2.x} * R;              // 1/w_a, 1/w_b
                    corr2 += (e2 - (w2 - 1.0f)) * r2;                    // log1p correction (natural units)
                    const f32x2 sg2 = e2 * r2;                           // sigmoid(t) = SoftplusGrad
                    gs2[q] += sg2;
                    sgp2 += sg2;
                }
                cnt_wave += (unsigned)__popcll(__ballot(t2.x > 1e-16f)) + (unsigned)__popcll(__ballot(t2.y > 1e-16f));   // (:114)
            }
            sgp[h] = sgp2.x + sgp2.y;
        }
        sgp[0] = wave64_sum_hi(sgp[0]);
        sgp[1] = wave64_sum_hi(sgp[1]);
        if constexpr (FAST) {                                            // sum of sigmoids = lane slots - sum of r
            sgp[0] = (float)(128 * Q2) - sgp[0];
            sgp[1] = (float)(128 * Q2) - sgp[1];
        }
        if (lane == 63) {
            if (FIRST) { gpos[p] = sgp[0]; if (has2) gpos[p + 4] = sgp[1]; }
            else { gpos[p] += sgp[0]; if (has2) gpos[p + 4] += sgp[1]; }
        }
    }
    loss_corr += corr2.x + corr2.y;
    const float slots = (float)(2 * iters);                              // positives walked by this wave (incl. the u = +inf filler)
#pragma unroll
    for (int q = 0; q < Q2; ++q) {
        const int k = k0 + (2 * q) * 64 + lane;
        if (k < nN) gneg_w[k] = FAST ? slots - gs2[q].x : gs2[q].x;
        if (k + 64 < nN) gneg_w[k + 64] = FAST ? slots - gs2[q].y : gs2[q].y;
    }
}

#if defined(DAE_MINER_PROBE) && (DAE_MINER_PROBE & 4)
// probe build (tools only): thread 0 stamps the 100 MHz wall clock at each stage into role_cnt (8 x uint64 per workgroup;
// the plan's role_cnt buffer is large enough) -- read back by tools/miner_timeline.py
#define MINER_STAMP(i) do { if (!POS_ONLY && threadIdx.x == 0) reinterpret_cast<unsigned long long*>(role_cnt)[(size_t)blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define MINER_STAMP(i) do { } while (0)
#endif
// One anchor: everything the workgroup does for row `ar` of D / G (batch element a0 + ar).
template <bool POS_ONLY>
__device__ __forceinline__ void batch_all_anchor(char* smem, const int ar, const float* __restrict__ D_slabs, int d_splits,
                                                 int64_t slab_stride, int64_t ldd, const int32_t* __restrict__ labels, int B, int Bp,
                                                 float* __restrict__ loss_part, uint32_t* __restrict__ npos_part,
                                                 float* __restrict__ G, uint32_t* __restrict__ role_cnt, int fast, int a0,
                                                 const int32_t* __restrict__ cls) {
    // positives are compacted from the front of val[]/idx[], negatives from the back (nP + nN <= B)
    float* val = reinterpret_cast<float*>(smem);             // [Bp]
    int* idx = reinterpret_cast<int*>(val + Bp);              // [Bp]
    float* gpos = reinterpret_cast<float*>(idx + Bp);         // [Bp]    positive-role gradient sums (one owner wave each)
    float* pf = gpos + Bp;                                    // [Bp]    F_p = exp(mid - u_p) of the factorised sweep
    float* gneg = pf + Bp;                                    // [4][Bp] per-wave negative-role partial sums (>= 1024 floats: the count's sorted runs)
    int* scan = reinterpret_cast<int*>(gneg + (4 * Bp > 1024 ? 4 * Bp : 1024));        // [2][TRIP_THREADS + 1]
    float* red = reinterpret_cast<float*>(scan + 2 * (TRIP_THREADS + 1));   // [4]
    unsigned* redu = reinterpret_cast<unsigned*>(red + 4);    // [4]
    unsigned* cpos = POS_ONLY ? redu + 4 : nullptr;           // [Bp]    (pos_only role counts)
    unsigned* cneg = POS_ONLY ? cpos + Bp : nullptr;          // [4][Bp]

    // anchors [a0, a0 + gridDim.x) of the batch: row `ar` of D / G / the partial arrays belongs to batch element a = a0 + ar
    // (a0 = 0 and a square D for a whole batch; a0 > 0 when a rank mines ITS anchors against an all-gathered batch)
    const int a = a0 + ar;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    MINER_STAMP(0);
    const int32_t la = labels[a];
    float* Grow = G + (int64_t)ar * Bp;
    uint32_t* Rrow = POS_ONLY ? role_cnt + (int64_t)ar * Bp : nullptr;

    // zero the gradient row (covers j == a and j >= B) and the positive-role accumulators
    // every j < B other than the anchor is a positive or a negative and is written at the end: only the anchor's own
    // entry and the padding columns need zeros
    for (int j = tid; j < Bp; j += TRIP_THREADS) {
        if (j >= B || j == a) { Grow[j] = 0.f; if (POS_ONLY) Rrow[j] = 0u; }
        gpos[j] = 0.f;
        if (POS_ONLY) cpos[j] = 0u;
    }

    // ---- deterministic compaction in index order (ballot ranks; coalesced label / D-row reads) ----
    // element j = k*256 + tid; its slot = (#positives before it in index order) = prefix over (k, wave) + rank in wave
    const int K = (B + TRIP_THREADS - 1) / TRIP_THREADS;           // <= 16 for B <= 4096
    int* cntP = scan;                                              // [K][4]
    int* cntN = scan + 64;                                         // [K][4]
    int nP = 0, nN = 0;
    float* pu = val;                      // positives: val[0 .. nP)
    float *nv;                            // negatives: val[Bp-nN .. Bp)
    int *pidx = idx, *nidx;
    constexpr int KU = 4;
    // CLASS-SORTED batch (the training loops sort every mini-batch by label; the label block verifies it and publishes each
    // row's class range in `cls`): positives are the index range [cs, ce) minus the anchor, negatives the rest -- destinations
    // are index arithmetic, so there are no ballots, no count arrays and no barrier before the scatter; the row's min / max
    // ride along.  Same slots as the compaction below (index order), so everything downstream is identical.
    const bool ranged = cls != nullptr && K <= KU && cls[0] != 0;
    float lo = INFINITY, hi = -INFINITY;
    if (ranged) {
        const int cs = cls[1 + 2 * a], ce = cls[2 + 2 * a];
        nP = ce - cs - 1; nN = B - (ce - cs);
        nv = val + (Bp - nN);
        nidx = idx + (Bp - nN);
        float dj[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) dj[k] = 0.f;
        for (int s0 = 0; s0 < d_splits; s0 += 4) {          // 4 K-slices of the Gram matrix at a time: 16 loads in flight
            float dd[4][KU];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* Drow = D_slabs + (int64_t)min(s0 + u, d_splits - 1) * slab_stride + (int64_t)ar * ldd;
#pragma unroll
                for (int k = 0; k < KU; ++k) {
                    const int j = k * TRIP_THREADS + tid;
                    dd[u][k] = Drow[min(j, B - 1)];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < KU; ++k) dj[k] += (s0 + u < d_splits) ? dd[u][k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int j = k * TRIP_THREADS + tid;
            if (j < B && j != a) {
                const float d = dj[k];
                if (j >= cs && j < ce) { const int o = j - cs - (j > a ? 1 : 0); pu[o] = d; pidx[o] = j; }
                else { const int o = j < cs ? j : j - (ce - cs); nv[o] = d; nidx[o] = j; }
                lo = fminf(lo, d); hi = fmaxf(hi, d);
            }
        }
        lo = wave_min(lo); hi = wave_max(hi);
        if (lane == 0) { red[wave] = lo; reinterpret_cast<float*>(redu)[wave] = hi; }
    } else if (K <= KU) {
        // usual mini-batch (B <= 1024): every global load of the prologue is issued up front -- labels and the D row
        // (d_splits slabs) of all K strips -- so the block pays ONE memory latency instead of 2K dependent ones
        int32_t lj[KU];
        float dj[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int j = k * TRIP_THREADS + tid;
            lj[k] = (j < B) ? labels[j] : la;
            dj[k] = 0.f;
        }
        for (int s0 = 0; s0 < d_splits; s0 += 4) {          // 4 K-slices of the Gram matrix at a time: 16 loads in flight
            float dd[4][KU];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* Drow = D_slabs + (int64_t)(s0 + u) * slab_stride + (int64_t)ar * ldd;
#pragma unroll
                for (int k = 0; k < KU; ++k) {
                    const int j = k * TRIP_THREADS + tid;
                    dd[u][k] = (j < B && s0 + u < d_splits) ? Drow[j] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < KU; ++k) dj[k] += dd[u][k];
        }
        unsigned long long bp[KU], bn[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int j = k * TRIP_THREADS + tid;
            const bool isP = (j < B) && (lj[k] == la) && (j != a);
            const bool isN = (j < B) && (lj[k] != la);
            bp[k] = __ballot(isP); bn[k] = __ballot(isN);
            if (lane == 0) { cntP[k * 4 + wave] = __popcll(bp[k]); cntN[k * 4 + wave] = __popcll(bn[k]); }
        }
        __syncthreads();
        int beforeP[KU], beforeN[KU];
        {
            int offP = 0, offN = 0;
#pragma unroll
            for (int k = 0; k < KU; ++k) {
                beforeP[k] = offP; beforeN[k] = offN;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int cp = cntP[k * 4 + w], cn = cntN[k * 4 + w];
                    if (w < wave) { beforeP[k] += cp; beforeN[k] += cn; }
                    offP += cp; offN += cn;
                }
            }
            nP = offP; nN = offN;
        }
        nv = val + (Bp - nN);
        nidx = idx + (Bp - nN);
        const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int j = k * TRIP_THREADS + tid;
            const bool isP = (bp[k] >> lane) & 1ull, isN = (bn[k] >> lane) & 1ull;
            if (isP) { const int o = beforeP[k] + __popcll(bp[k] & lt); pu[o] = dj[k]; pidx[o] = j; }
            if (isN) { const int o = beforeN[k] + __popcll(bn[k] & lt); nv[o] = dj[k]; nidx[o] = j; }
        }
    } else {
    for (int k = 0; k < K; ++k) {
        const int j = k * TRIP_THREADS + tid;
        const int32_t lj = (j < B) ? labels[j] : la;
        const bool isP = (j < B) && (lj == la) && (j != a);
        const bool isN = (j < B) && (lj != la);
        const unsigned long long bp = __ballot(isP), bn = __ballot(isN);
        if (lane == 0) { cntP[k * 4 + wave] = __popcll(bp); cntN[k * 4 + wave] = __popcll(bn); }
    }
    __syncthreads();
    for (int e = 0; e < K * 4; ++e) { nP += cntP[e]; nN += cntN[e]; }
    nv = val + (Bp - nN);
    nidx = idx + (Bp - nN);
    {
        int offP = 0, offN = 0;           // running prefix over (k', wave') < (k, wave)
        for (int k = 0; k < K; ++k) {
            int beforeP = offP, beforeN = offN;
            for (int w = 0; w < 4; ++w) {
                if (w < wave) { beforeP += cntP[k * 4 + w]; beforeN += cntN[k * 4 + w]; }
                offP += cntP[k * 4 + w]; offN += cntN[k * 4 + w];
            }
            const int j = k * TRIP_THREADS + tid;
            const int32_t lj = (j < B) ? labels[j] : la;
            const bool isP = (j < B) && (lj == la) && (j != a);
            const bool isN = (j < B) && (lj != la);
            const unsigned long long bp = __ballot(isP), bn = __ballot(isN);
            const unsigned long long lt = (1ull << lane) - 1ull;
            float d = 0.f;
            if (j < B)
                for (int sl = 0; sl < d_splits; ++sl) d += D_slabs[(int64_t)sl * slab_stride + (int64_t)ar * ldd + j];
            if (isP) { const int o = beforeP + __popcll(bp & lt); pu[o] = d; pidx[o] = j; }
            if (isN) { const int o = beforeN + __popcll(bn & lt); nv[o] = d; nidx[o] = j; }
        }
    }
    }
    __syncthreads();
    MINER_STAMP(1);
    // range of the anchor's D row over its positives and negatives -> factorised or direct sweep (uniform choice)
    if (ranged) {
        const float* rh = reinterpret_cast<const float*>(redu);
        lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        hi = fmaxf(fmaxf(rh[0], rh[1]), fmaxf(rh[2], rh[3]));
        __syncthreads();                                     // red / redu are reused by the block sums at the end
    } else {
        for (int k = tid; k < nP; k += TRIP_THREADS) { lo = fminf(lo, pu[k]); hi = fmaxf(hi, pu[k]); }
        for (int k = tid; k < nN; k += TRIP_THREADS) { lo = fminf(lo, nv[k]); hi = fmaxf(hi, nv[k]); }
        lo = block_min_f(lo, red);
        hi = block_max_f(hi, red);
    }
    const bool fact = (hi - lo) <= 80.0f;                    // also false for NaN/inf rows
    const bool fact2 = !POS_ONLY && (hi - lo) <= 40.0f;      // pair-packed sweep: products of two (1 + exp(t)) stay finite
    const float mid = 0.5f * (hi + lo);
    if (fact)
        for (int k = tid; k < nP; k += TRIP_THREADS) pf[k] = __builtin_amdgcn_exp2f((mid - pu[k]) * kLog2e);
    __syncthreads();

    MINER_STAMP(2);
    float loss = 0.f;
    unsigned cnt = 0u;
    float* gneg_w = gneg + wave * Bp;
    unsigned* cneg_w = POS_ONLY ? cneg + wave * Bp : nullptr;
    // chunks of 128*q2 negatives, q2 <= 5 register pairs per lane; equal-sized chunks when one is not enough
    const int need2 = (nN + 127) / 128;
    const int nch2 = (need2 + 4) / 5;
    const int q2 = nch2 > 0 ? (need2 + nch2 - 1) / nch2 : 1;
    auto packed_sweeps = [&](auto FASTV) {
        constexpr bool FAST = decltype(FASTV)::value;
        float loss_log2 = 0.f, loss_corr = 0.f;
        unsigned cnt_wave = 0u;
        for (int k0 = 0; k0 < nN; k0 += q2 * 128) {
            const bool first = (k0 == 0);
#define DAE_SWEEP2(QV)                                                                                                  \
    do {                                                                                                                \
        if (first) sweep_pairs2<QV, true, FAST>(pu, pf, mid, nv, nP, nN, k0, wave, lane, gpos, gneg_w, loss_log2, loss_corr, cnt_wave);   \
        else sweep_pairs2<QV, false, FAST>(pu, pf, mid, nv, nP, nN, k0, wave, lane, gpos, gneg_w, loss_log2, loss_corr, cnt_wave);        \
    } while (0)
            switch (q2) {
                case 5: DAE_SWEEP2(5); break;
                case 4: DAE_SWEEP2(4); break;
                case 3: DAE_SWEEP2(3); break;
                case 2: DAE_SWEEP2(2); break;
                default: DAE_SWEEP2(1); break;
            }
#undef DAE_SWEEP2
        }
        loss = kLn2 * loss_log2 + loss_corr;
        cnt = lane == 0 ? cnt_wave : 0u;
    };
    bool redo = false;
    if (fact2) {
        if (fast) {
            packed_sweeps(std::true_type{});
            // |log(fl(1+e)) - log1p(e)| <= 2^-24 per triplet: accept when that is below 2e-6 of the anchor's sum, i.e. the mean
            // term is >= 0.03 (softplus(t) at t = -3.5); otherwise (every triplet far on the satisfied side) take the exact form
            const float lsum = block_sum_f(loss, red);
            redo = !(lsum >= 0.03f * (float)nP * (float)nN);
            if (redo) { __syncthreads(); packed_sweeps(std::false_type{}); }
        } else {
            packed_sweeps(std::false_type{});
        }
    }
    for (int k0 = 0; !fact2 && k0 < nN;) {
        const int need = (nN - k0 + 63) / 64;                 // negatives per lane still to cover
        // menu of register-resident widths; the smallest one >= need (6 caps a chunk at 384 negatives; this legacy path shares the register budget of the pair-packed one)
        const int q = need <= 4 ? need : 6;
        const bool first = (k0 == 0);
#define DAE_SWEEP(QV)                                                                                                    \
    do {                                                                                                                 \
        if (fact) {                                                                                                      \
            if (first) sweep_pairs<POS_ONLY, QV, true, true>(pu, pf, mid, nv, nP, nN, k0, wave, lane, gpos, cpos, gneg_w, cneg_w, loss, cnt);   \
            else sweep_pairs<POS_ONLY, QV, true, false>(pu, pf, mid, nv, nP, nN, k0, wave, lane, gpos, cpos, gneg_w, cneg_w, loss, cnt);       \
        } else {                                                                                                         \
            if (first) sweep_pairs<POS_ONLY, QV, false, true>(pu, pf, mid, nv, nP, nN, k0, wave, lane, gpos, cpos, gneg_w, cneg_w, loss, cnt);  \
            else sweep_pairs<POS_ONLY, QV, false, false>(pu, pf, mid, nv, nP, nN, k0, wave, lane, gpos, cpos, gneg_w, cneg_w, loss, cnt);      \
        }                                                                                                                \
    } while (0)
        switch (q) {
            case 6: DAE_SWEEP(6); break;
            case 4: DAE_SWEEP(4); break;
            case 3: DAE_SWEEP(3); break;
            case 2: DAE_SWEEP(2); break;
            default: DAE_SWEEP(1); break;
        }
#undef DAE_SWEEP
        k0 += q * 64;
    }
    __syncthreads();
    MINER_STAMP(3);
    for (int k = tid; k < nP; k += TRIP_THREADS) {
        Grow[pidx[k]] = -gpos[k];
        if (POS_ONLY) Rrow[pidx[k]] = cpos[k];
    }
    for (int k = tid; k < nN; k += TRIP_THREADS) {
        Grow[nidx[k]] = (gneg[k] + gneg[Bp + k]) + (gneg[2 * Bp + k] + gneg[3 * Bp + k]);
        if (POS_ONLY) Rrow[nidx[k]] = cneg[k] + cneg[Bp + k] + cneg[2 * Bp + k] + cneg[3 * Bp + k];
    }
    const float ltot = block_sum_f(loss, red);
    const unsigned ctot = block_sum_u(cnt, redu);
    if (tid == 0) { loss_part[ar] = ltot; npos_part[ar] = ctot; }
    MINER_STAMP(4);
#if defined(DAE_MINER_PROBE) && (DAE_MINER_PROBE & 4)
    if (!POS_ONLY && tid == 0) {
        unsigned hw; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        reinterpret_cast<unsigned long long*>(role_cnt)[(size_t)blockIdx.x * 8 + 5] = ((unsigned long long)xcc << 32) | hw;
        reinterpret_cast<unsigned long long*>(role_cnt)[(size_t)blockIdx.x * 8 + 6] = ((unsigned long long)nP << 32) | (unsigned)nN;
    }
#endif
}

// Workgroup -> anchors.  The launch has min(n_anchors, nslots) workgroups, nslots = what the chip holds at once (3 per CU):
// with 800 anchors on 768 slots the 32 workgroups of a second round used to start when the first ones ended and finished at
// 1.6 x the median (profiles/r02_miner_timeline.txt).  Now every workgroup is resident from the start and walks the anchor list in
// SNAKE order -- b, 2 nslots - 1 - b, 2 nslots + b, ... -- so with `order` (anchors by descending sweep cost, from the label
// block) the workgroups that take a second anchor are the ones whose first was the cheapest, and the second is the cheapest
// of all: classic longest-processing-time packing.  Every anchor is still computed by one workgroup, alone, in the same way.
template <bool POS_ONLY, int OCC>
__global__ __launch_bounds__(TRIP_THREADS, OCC) void batch_all_kernel(const float* __restrict__ D_slabs, int d_splits,
                                                                 int64_t slab_stride, int64_t ldd,
                                                                 const int32_t* __restrict__ labels, int B, int Bp,
                                                                 float* __restrict__ loss_part, uint32_t* __restrict__ npos_part,
                                                                 float* __restrict__ G, uint32_t* __restrict__ role_cnt, int fast, int a0,
                                                                 const int32_t* __restrict__ order, int n_anchors,
                                                                 const int32_t* __restrict__ cls) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nslots = gridDim.x, b = blockIdx.x;
    bool first = true;
    for (int r = 0; r * nslots < n_anchors; ++r) {     // round r hands out the anchors [r nslots, (r + 1) nslots), odd rounds from the far end
        const int k = (r & 1) ? (r + 1) * nslots - 1 - b : r * nslots + b;
        if (k >= n_anchors) continue;
        const int ar = order ? order[k] : k;
        if (!first) __syncthreads();                   // the previous anchor's LDS image is dead
        first = false;
        batch_all_anchor<POS_ONLY>(smem, ar, D_slabs, d_splits, slab_stride, ldd, labels, B, Bp, loss_part, npos_part, G, role_cnt, fast, a0, cls);
    }
}


// ------------------------------------------------------------------------------------------------
// batch_all, lane-grid form (dae_miner_tile.h): the kernel of the usual mini-batch (B <= 1024, all valid triplets).
// One workgroup per anchor, ALL anchors resident at once (<= 128 VGPRs: 4 workgroups per CU = 1024 slots), so there is no
// second round of workgroups and no packing.  Per anchor: D row -> positives / negatives (class ranges of a label-sorted batch,
// else ballot compaction), exact count of the positive triplets from sorted runs, sweep variant by the row's range:
//   range <= 40: pair-shared reciprocal, LOGW = 8 / 4 / 2 factors per logarithm (range <= 10 / 20 / 40); FAST (bf16 steps) or exact
//   range <= 80: one reciprocal and one logarithm per cell (exp(t) = E_n F_p still finite)
//   otherwise (and NaN / inf rows): exp(-|t|) per cell, the reference-literal stable form
// ------------------------------------------------------------------------------------------------
#if defined(DAE_MINER_PROBE) && (DAE_MINER_PROBE & 4)
#define TILE_STAMP(i) do { if (threadIdx.x == 0) reinterpret_cast<unsigned long long*>(role_cnt)[(size_t)blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define TILE_STAMP(i) do { } while (0)
#endif
enum { MT_FAST = 0, MT_EXACT = 1, MT_CELL = 2, MT_DIRECT = 3, MT_FAST_SCALED = 4 };

// Sweep variants without the pair trick, same lane grid and the same outputs as tile_sweep.
//   DIRECT = false: w = 1 + E_n F_p per cell, one v_rcp_f32 and one v_log_f32 per cell (row range <= 80)
//   DIRECT = true : t = v_n - u_p, en = exp(-|t|), softplus = max(t, 0) + log1p(en), sigmoid = t >= 0 ? 1/(1+en) : en/(1+en)
template <int Q2, bool DIRECT>
__device__ __forceinline__ void tile_sweep_cells(const float* __restrict__ pu, const float* __restrict__ pf, const float* __restrict__ nv, float mid,
                                                 int nP, int nN, int k0, bool first, float* __restrict__ gpos, float* __restrict__ gneg_w,
                                                 float& loss) {
    const int tid = threadIdx.x, lane = tid & 63, b = tid & 15, a = tid >> 4;
    float x[2 * Q2], gs[2 * Q2];                                            // E_n (or v_n when DIRECT) and the column sums
#pragma unroll
    for (int m = 0; m < 2 * Q2; ++m) {
        const int k = k0 + 16 * m + b;
        const float v = (k < nN) ? nv[k] : -INFINITY;
        x[m] = DIRECT ? v : __builtin_amdgcn_exp2f((v - mid) * kMtLog2e);
        gs[m] = 0.f;
    }
    const int T = (nP + 15) >> 4;
    for (int t = 0; t < T; ++t) {
        const int j = a + 16 * t;
        const float f = (j < nP) ? (DIRECT ? pu[j] : pf[j]) : (DIRECT ? INFINITY : 0.f);   // u = +inf -> t = -inf -> contributes nothing
        float rs = 0.f;
#pragma unroll
        for (int m = 0; m < 2 * Q2; ++m) {
            float sp, sg;
            if constexpr (DIRECT) {
                const float tt = x[m] - f;
                const float en = __builtin_amdgcn_exp2f(-fabsf(tt) * kMtLog2e);
                const float w = 1.0f + en;
                const float r = __builtin_amdgcn_rcpf(w);
                const float lg = 0.6931471805599453f * __builtin_amdgcn_logf(w);
                const float l = en < 1e-4f ? en * (1.0f - 0.5f * en) : lg;
                sp = fmaxf(tt, 0.f) + l;
                sg = tt >= 0.f ? r : en * r;
                if (!(tt == tt)) { sp = tt; sg = tt; }                      // NaN rows stay NaN
                if (tt == -INFINITY) { sp = 0.f; sg = 0.f; }
            } else {
                const float e = x[m] * f;
                const float w = 1.0f + e;
                const float r = __builtin_amdgcn_rcpf(w);
                const float lg = 0.6931471805599453f * __builtin_amdgcn_logf(w);
                sp = e < 1e-4f ? e * (1.0f - 0.5f * e) : lg;
                sg = e * r;
            }
            loss += sp; gs[m] += sg; rs += sg;
        }
        rs = row16_sum(rs);
        if (b == 0 && j < nP) { if (first) gpos[j] = rs; else gpos[j] += rs; }
    }
#pragma unroll
    for (int m = 0; m < 2 * Q2; ++m) {
        const float c = mt_cross_row_sum(gs[m]);
        const int k = k0 + 16 * m + b;
        if (lane < 16 && k < nN) gneg_w[k] = c;
    }
}

// all chunks of the anchor's negatives through tile_sweep (plain functions, pointers by value: closures that capture the LDS
// pointers by reference end up in scratch as GENERIC pointers and every LDS access of the sweep becomes a flat_load / flat_store)
template <bool FAST, int LOGW, bool SCALED = false>
__device__ __forceinline__ float tile_pair_sweeps(const float* pf, const float* nv, float mid, int nP, int nN, int q2, float* gpos, float* gneg_w,
                                                  float half_range = 0.f) {
    float loss_log2 = 0.f, loss_corr = 0.f;
    const float esc = SCALED ? __builtin_amdgcn_exp2f(-half_range * kMtLog2e) : 1.0f;
    for (int k0 = 0; k0 < nN; k0 += 32 * q2) {
        const bool first = (k0 == 0);
        switch (q2) {
            case 12: tile_sweep<12, FAST, LOGW, 2, SCALED>(pf, nv, mid, nP, nN, k0, first, gpos, gneg_w, loss_log2, loss_corr, 0, 1, esc); break;
            case 10: tile_sweep<10, FAST, LOGW, 2, SCALED>(pf, nv, mid, nP, nN, k0, first, gpos, gneg_w, loss_log2, loss_corr, 0, 1, esc); break;
            case 8: tile_sweep<8, FAST, LOGW, 2, SCALED>(pf, nv, mid, nP, nN, k0, first, gpos, gneg_w, loss_log2, loss_corr, 0, 1, esc); break;
            case 6: tile_sweep<6, FAST, LOGW, 2, SCALED>(pf, nv, mid, nP, nN, k0, first, gpos, gneg_w, loss_log2, loss_corr, 0, 1, esc); break;
            default: tile_sweep<4, FAST, LOGW, 2, SCALED>(pf, nv, mid, nP, nN, k0, first, gpos, gneg_w, loss_log2, loss_corr, 0, 1, esc); break;
        }
    }
    return kLn2 * loss_log2 + loss_corr;
}
// LOGW factors (1 + exp(t)) <= 1 + e^range are multiplied before one v_log_f32: their product must stay finite
template <bool FAST>
__device__ __forceinline__ float tile_pair_sweeps_by_range(float range, const float* pf, const float* nv, float mid, int nP, int nN, int q2,
                                                           float* gpos, float* gneg_w) {
    if (range <= 10.0f) return tile_pair_sweeps<FAST, 8>(pf, nv, mid, nP, nN, q2, gpos, gneg_w);
    if (range <= 20.0f) return tile_pair_sweeps<FAST, 4>(pf, nv, mid, nP, nN, q2, gpos, gneg_w);
    return tile_pair_sweeps<FAST, 2>(pf, nv, mid, nP, nN, q2, gpos, gneg_w);
}
template <bool DIRECT>
__device__ __forceinline__ float tile_cell_sweeps(const float* pu, const float* pf, const float* nv, float mid, int nP, int nN, float* gpos,
                                                  float* gneg_w) {
    float loss = 0.f;
    for (int k0 = 0; k0 < nN; k0 += 128) tile_sweep_cells<4, DIRECT>(pu, pf, nv, mid, nP, nN, k0, k0 == 0, gpos, gneg_w, loss);
    return loss;
}

template <int OCC>
__global__ __launch_bounds__(TRIP_THREADS, OCC) void batch_all_tile_kernel(const float* __restrict__ D_slabs, int d_splits, int64_t slab_stride,
                                                                           int64_t ldd, const int32_t* __restrict__ labels, int B, int Bp,
                                                                           float* __restrict__ loss_part, uint32_t* __restrict__ npos_part,
                                                                           float* __restrict__ G, uint32_t* __restrict__ role_cnt, int fast, int a0,
                                                                           const int32_t* __restrict__ order, const int32_t* __restrict__ cls) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* val = reinterpret_cast<float*>(smem);             // [Bp]  positives from the front, negatives from the back
    int* idx = reinterpret_cast<int*>(val + Bp);              // [Bp]
    float* gpos = reinterpret_cast<float*>(idx + Bp);         // [Bp]
    float* pf = gpos + Bp;                                    // [Bp]  F_p = exp(mid - u_p)
    float* gneg = pf + Bp;                                    // [4][Bp] per-wave negative-role partial sums; before the sweeps: the count's sorted runs (1024)
    int* scan = reinterpret_cast<int*>(gneg + (4 * Bp > 1024 ? 4 * Bp : 1024));   // [2][16]
    float* red = reinterpret_cast<float*>(scan + 32);         // [8]
    unsigned* redu = reinterpret_cast<unsigned*>(red + 8);    // [4]

    const int ar = order ? order[blockIdx.x] : (int)blockIdx.x;
    const int a = a0 + ar;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    TILE_STAMP(0);
    float* Grow = G + (int64_t)ar * Bp;
    for (int j = tid; j < Bp; j += TRIP_THREADS) {
        if (j >= B || j == a) Grow[j] = 0.f;
        gpos[j] = 0.f;
    }
    constexpr int KU = 4;                                     // B <= 1024: element j = k * 256 + tid
    int nP = 0, nN = 0;
    float* pu = val;
    float* nv;
    int *pidx = idx, *nidx;
    float lo = INFINITY, hi = -INFINITY;
    float dj[KU];
#pragma unroll
    for (int k = 0; k < KU; ++k) dj[k] = 0.f;
    const bool ranged = cls != nullptr && cls[0] != 0;
    int32_t lj[KU];
    const int32_t la = ranged ? 0 : labels[a];
    if (!ranged) {
#pragma unroll
        for (int k = 0; k < KU; ++k) { const int j = k * TRIP_THREADS + tid; lj[k] = (j < B) ? labels[j] : la; }
    }
    for (int s0 = 0; s0 < d_splits; s0 += 4) {                // 4 K-slices of the Gram matrix at a time: 16 loads in flight
        float dd[4][KU];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* Drow = D_slabs + (int64_t)min(s0 + u, d_splits - 1) * slab_stride + (int64_t)ar * ldd;
#pragma unroll
            for (int k = 0; k < KU; ++k) dd[u][k] = Drow[min(k * TRIP_THREADS + tid, B - 1)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < KU; ++k) dj[k] += (s0 + u < d_splits) ? dd[u][k] : 0.f;
    }
    if (ranged) {
        // class-sorted batch: positives are the index range [cs, ce) minus the anchor, negatives the rest (index arithmetic only)
        const int cs = cls[1 + 2 * a], ce = cls[2 + 2 * a];
        nP = ce - cs - 1; nN = B - (ce - cs);
        nv = val + (Bp - nN); nidx = idx + (Bp - nN);
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int j = k * TRIP_THREADS + tid;
            if (j < B && j != a) {
                const float d = dj[k];
                if (j >= cs && j < ce) { const int o = j - cs - (j > a ? 1 : 0); pu[o] = d; pidx[o] = j; }
                else { const int o = j < cs ? j : j - (ce - cs); nv[o] = d; nidx[o] = j; }
                lo = fminf(lo, d); hi = fmaxf(hi, d);
            }
        }
    } else {
        // deterministic compaction in index order (ballot ranks)
        int* cntP = scan; int* cntN = scan + 16;
        unsigned long long bp[KU], bn[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int j = k * TRIP_THREADS + tid;
            const bool isP = (j < B) && (lj[k] == la) && (j != a);
            const bool isN = (j < B) && (lj[k] != la);
            bp[k] = __ballot(isP); bn[k] = __ballot(isN);
            if (lane == 0) { cntP[k * 4 + wave] = __popcll(bp[k]); cntN[k * 4 + wave] = __popcll(bn[k]); }
        }
        __syncthreads();
        int beforeP[KU], beforeN[KU];
        int offP = 0, offN = 0;
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            beforeP[k] = offP; beforeN[k] = offN;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int cp = cntP[k * 4 + w], cn = cntN[k * 4 + w];
                if (w < wave) { beforeP[k] += cp; beforeN[k] += cn; }
                offP += cp; offN += cn;
            }
        }
        nP = offP; nN = offN;
        nv = val + (Bp - nN); nidx = idx + (Bp - nN);
        const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int j = k * TRIP_THREADS + tid;
            const bool isP = (bp[k] >> lane) & 1ull, isN = (bn[k] >> lane) & 1ull;
            if (isP) { const int o = beforeP[k] + __popcll(bp[k] & lt); pu[o] = dj[k]; pidx[o] = j; }
            if (isN) { const int o = beforeN[k] + __popcll(bn[k] & lt); nv[o] = dj[k]; nidx[o] = j; }
            if (isP || isN) { lo = fminf(lo, dj[k]); hi = fmaxf(hi, dj[k]); }
        }
    }
    lo = wave_min(lo); hi = wave_max(hi);
    if (lane == 0) { red[wave] = lo; red[4 + wave] = hi; }
    __syncthreads();
    lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    const float range = hi - lo;                              // NaN for NaN rows, inf for inf rows: every comparison below is then false
    const float mid = 0.5f * (hi + lo);
    // (40, 80]: bf16 steps take the SCALED pair sweep (factors carried as e^-c (1 + exp(t)), c = range / 2), exact mode one reciprocal per cell
    const int kind = range <= 40.0f ? (fast ? MT_FAST : MT_EXACT) : (range <= 80.0f ? (fast ? MT_FAST_SCALED : MT_CELL) : MT_DIRECT);
    if (kind != MT_DIRECT)
        for (int k = tid; k < nP; k += TRIP_THREADS) pf[k] = __builtin_amdgcn_exp2f((mid - pu[k]) * kMtLog2e);
    TILE_STAMP(1);
    // exact count of the positive triplets (its sorted runs live in the gneg region, which the sweeps write only at a chunk's end)
    unsigned cnt = count_positive_triplets(pu, nP, nv, nN, gneg);
    __syncthreads();
    TILE_STAMP(2);
#if defined(DAE_MINER_PROBE) && (DAE_MINER_PROBE & 4)
    const long long sweep_c0 = clock64();
#endif

    float loss = 0.f;
    float* gneg_w = gneg + wave * Bp;
    const int need2 = (nN + 31) / 32;                         // register pairs per lane that cover the negatives (16 columns x 2)
    const int nch = (need2 + 11) / 12;
    int q2 = nch > 0 ? (need2 + nch - 1) / nch : 4;
    q2 = (q2 + 1) & ~1;
    if (q2 < 4) q2 = 4;
    if (kind == MT_FAST) {
        loss = tile_pair_sweeps_by_range<true>(range, pf, nv, mid, nP, nN, q2, gpos, gneg_w);
        // FAST drops the first-order log1p correction: |log(fl(1+e)) - log1p(e)| <= 2^-24 per triplet.  Accept when that is below
        // 2e-6 of the anchor's sum (mean term >= 0.03 = softplus(-3.5)); otherwise every triplet is far on the satisfied side: exact form
        const float lsum = block_sum_f(loss, red);
        if (!(lsum >= 0.03f * (float)nP * (float)nN)) { __syncthreads(); loss = tile_pair_sweeps_by_range<false>(range, pf, nv, mid, nP, nN, q2, gpos, gneg_w); }
    } else if (kind == MT_FAST_SCALED) {
        loss = tile_pair_sweeps<true, 2, true>(pf, nv, mid, nP, nN, q2, gpos, gneg_w, 0.5f * range);
        const float lsum = block_sum_f(loss, red);            // same acceptance test as above; the fallback is the per-cell sweep
        if (!(lsum >= 0.03f * (float)nP * (float)nN)) { __syncthreads(); loss = tile_cell_sweeps<false>(pu, pf, nv, mid, nP, nN, gpos, gneg_w); }
    } else if (kind == MT_EXACT) {
        loss = tile_pair_sweeps_by_range<false>(range, pf, nv, mid, nP, nN, q2, gpos, gneg_w);
    } else if (kind == MT_CELL) {
        loss = tile_cell_sweeps<false>(pu, pf, nv, mid, nP, nN, gpos, gneg_w);
    } else {
        loss = tile_cell_sweeps<true>(pu, pf, nv, mid, nP, nN, gpos, gneg_w);
    }
    __syncthreads();
    TILE_STAMP(3);
#if defined(DAE_MINER_PROBE) && (DAE_MINER_PROBE & 4)
    const unsigned long long sweep_cycles = (unsigned long long)(clock64() - sweep_c0);
#endif
    for (int k = tid; k < nP; k += TRIP_THREADS) Grow[pidx[k]] = -gpos[k];
    for (int k = tid; k < nN; k += TRIP_THREADS) Grow[nidx[k]] = (gneg[k] + gneg[Bp + k]) + (gneg[2 * Bp + k] + gneg[3 * Bp + k]);
    const float ltot = block_sum_f(loss, red);
    const unsigned ctot = block_sum_u(cnt, redu);
    if (tid == 0) { loss_part[ar] = ltot; npos_part[ar] = ctot; }
    TILE_STAMP(4);
#if defined(DAE_MINER_PROBE) && (DAE_MINER_PROBE & 4)
    if (tid == 0) {
        unsigned hw; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        const unsigned long long kd = kind <= MT_EXACT ? (range <= 10.f ? 8 : range <= 20.f ? 4 : 2) : (kind == MT_CELL ? 1 : kind == MT_FAST_SCALED ? 3 : 15);
        reinterpret_cast<unsigned long long*>(role_cnt)[(size_t)blockIdx.x * 8 + 5] = (kd << 40) | ((unsigned long long)xcc << 32) | hw;
        reinterpret_cast<unsigned long long*>(role_cnt)[(size_t)blockIdx.x * 8 + 6] = ((unsigned long long)nP << 32) | (unsigned)nN;
        reinterpret_cast<unsigned long long*>(role_cnt)[(size_t)blockIdx.x * 8 + 7] = (sweep_cycles << 32) | (unsigned long long)__float_as_uint(range);
    }
#endif
}

}  // namespace dae
namespace dae {

// ------------------------------------------------------------------------------------------------
// batch_hard
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRIP_THREADS) void batch_hard_kernel(const float* __restrict__ D_slabs, int d_splits,
                                                                  int64_t slab_stride, int64_t ldd,
                                                                  const int32_t* __restrict__ labels, int B, int Bp,
                                                                  float* __restrict__ loss_part, uint32_t* __restrict__ cnt_part,
                                                                  int32_t* __restrict__ dw, float* __restrict__ G, int a0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* drow = reinterpret_cast<float*>(smem);            // [Bp]
    float* red = drow + Bp;                                   // [4]
    unsigned* redu = reinterpret_cast<unsigned*>(red + 4);    // [4]
    const int ar = blockIdx.x, a = a0 + ar, tid = threadIdx.x;        // see batch_all_kernel
    const int32_t la = labels[a];
    float* Grow = G + (int64_t)ar * Bp;

    float mx = -INFINITY;
    for (int j = tid; j < B; j += TRIP_THREADS) {
        float d = 0.f;
        for (int s = 0; s < d_splits; ++s) d += D_slabs[(int64_t)s * slab_stride + (int64_t)ar * ldd + j];
        drow[j] = d;
        mx = fmaxf(mx, d);
    }
    const float rowmax = block_max_f(mx, red);                               // :227
    float mn = INFINITY, hnl = -INFINITY;
    for (int j = tid; j < B; j += TRIP_THREADS) {
        const int32_t lj = labels[j];
        const float ap = (lj == la && j != a) ? 1.f : 0.f;                   // :223-224
        const float an = (lj != la) ? 1.f : 0.f;                             // :236-237
        const float d = drow[j];
        mn = fminf(mn, d + rowmax * (1.0f - ap));                            // :228
        hnl = fmaxf(hnl, an * d);                                            // :240  (invalid -> 0, not -inf)
    }
    const float hp = block_min_f(mn, red);                                   // :231
    const float hn = block_max_f(hnl, red);                                  // :243
    const float dist = fmaxf(hn - hp, 0.f);                                  // :247
    const bool cnt = dist > 0.f;                                             // :249
    // tie counts for the gradient split (TF reduce_min/max gradient = indicator / num_selected)
    unsigned c_n = 0, c_p = 0, c_m = 0, c_pinv = 0;
    for (int j = tid; j < B; j += TRIP_THREADS) {
        const int32_t lj = labels[j];
        const float ap = (lj == la && j != a) ? 1.f : 0.f;
        const float an = (lj != la) ? 1.f : 0.f;
        const float d = drow[j];
        const bool tp = (d + rowmax * (1.0f - ap)) == hp;
        c_n += (an * d == hn);
        c_p += tp;
        c_pinv += (tp && ap == 0.f);
        c_m += (d == rowmax);
    }
    const unsigned n_n = block_sum_u(c_n, redu), n_p = block_sum_u(c_p, redu);
    const unsigned n_m = block_sum_u(c_m, redu), n_pinv = block_sum_u(c_pinv, redu);
    const float gd = cnt ? sigmoid_only(dist) : 0.f;                         // softplus' = sigmoid; * triplet_count
    const float g_n = gd / (float)n_n;
    const float g_p = -gd / (float)n_p;
    const float g_m = (g_p * (float)n_pinv) / (float)n_m;                    // gradient through the row-max shift
    for (int j = tid; j < Bp; j += TRIP_THREADS) {
        float g = 0.f;
        if (j < B) {
            const int32_t lj = labels[j];
            const float ap = (lj == la && j != a) ? 1.f : 0.f;
            const float an = (lj != la) ? 1.f : 0.f;
            const float d = drow[j];
            if (an * d == hn) g += an * g_n;
            if ((d + rowmax * (1.0f - ap)) == hp) g += g_p;
            if (d == rowmax) g += g_m;
            if (cnt) {                                                       // data_weight :251-253
                const int w = (d == hp) + (d == hn) + (j == a);
                if (w) atomicAdd(&dw[j], w);
            }
        }
        Grow[j] = g;
    }
    if (tid == 0) {
        loss_part[ar] = cnt ? softplus_tf(dist) : 0.f;                       // :256
        cnt_part[ar] = cnt ? 1u : 0u;
    }
}

}  // namespace dae

using namespace dae;

extern "C" int dae_triplet_batch_all(const float* D_slabs, int32_t d_splits, int64_t slab_stride, int64_t ldd,
                                     const int32_t* labels, int32_t B, int32_t Bp, int32_t mode, float* loss_part,
                                     uint32_t* npos_part, float* G, uint32_t* role_cnt, void* stream) {
    return dae_triplet_batch_all_rows(D_slabs, d_splits, slab_stride, ldd, labels, B, Bp, 0, B, mode, loss_part, npos_part, G, role_cnt, stream);
}

extern "C" int dae_triplet_batch_all_rows(const float* D_slabs, int32_t d_splits, int64_t slab_stride, int64_t ldd,
                                          const int32_t* labels, int32_t B, int32_t Bp, int32_t a0, int32_t n_anchors, int32_t mode,
                                          float* loss_part, uint32_t* npos_part, float* G, uint32_t* role_cnt, void* stream) {
    return launch_batch_all(D_slabs, d_splits, slab_stride, ldd, labels, B, Bp, a0, n_anchors, mode, loss_part, npos_part, G, role_cnt, nullptr,
                            (hipStream_t)stream);
}

static int g_miner_pack = 1;       // 0: one workgroup per anchor (A/B; plan option "miner_pack")
void dae::set_miner_pack(int on) { g_miner_pack = on ? 1 : 0; }
static int g_miner_tile = 1;       // 0: the former wave-per-positive kernel also for B <= 1024 (A/B and equivalence tests; plan option "miner_tile")
void dae::set_miner_tile(int on) { g_miner_tile = on ? 1 : 0; }

// order: optional dispatch order of the anchors (LabelJob::order; whole-batch launches only)
int dae::launch_batch_all(const float* D_slabs, int d_splits, int64_t slab_stride, int64_t ldd, const int32_t* labels, int B, int Bp, int a0,
                          int n_anchors, int mode, float* loss_part, uint32_t* npos_part, float* G, uint32_t* role_cnt, const int32_t* order,
                          hipStream_t st, const int32_t* cls) {
    DAE_CHECK_ARG(!order || (a0 == 0 && n_anchors == B), "batch_all: a dispatch order needs the whole batch");
    DAE_CHECK_ARG(!cls || (a0 == 0 && n_anchors == B), "batch_all: class ranges need the whole batch");
    DAE_CHECK_ARG(a0 >= 0 && n_anchors > 0 && a0 + n_anchors <= B, "batch_all: anchors [%d, %d) outside the batch of %d", a0, a0 + n_anchors, B);
    const int pos_only = mode & DAE_MINER_POS_ONLY, fast = (mode & DAE_MINER_FAST) ? 1 : 0;
    DAE_CHECK_ARG(D_slabs && labels && loss_part && npos_part && G, "batch_all: null input");
    DAE_CHECK_ARG(B > 0 && B <= Bp && Bp <= TRIP_MAX_B, "batch_all: batch %d (padded %d) exceeds the supported %d", B, Bp, TRIP_MAX_B);
    DAE_CHECK_ARG(!pos_only || role_cnt, "batch_all: role_cnt required with pos_triplets_only");
    // val + idx + 4 per-wave gradient rows (+ 4 count rows when pos_only) + scans + reductions
    const size_t lds = (size_t)Bp * (pos_only ? 52 : 32) + (4 * Bp < 1024 ? (size_t)(1024 - 4 * Bp) * 4 : 0) + 2 * (TRIP_THREADS + 1) * sizeof(int) +
                       8 * sizeof(float);
    DAE_CHECK_ARG(lds <= 160 * 1024, "batch_all: batch %d needs %zu B of LDS (> 160 KiB)", B, lds);
    if (!pos_only && Bp <= 1024 && g_miner_tile) {
        // the lane-grid kernel: one workgroup per anchor, all of them resident (4 per CU)
        const size_t tl = (size_t)Bp * 16 + (size_t)(4 * Bp > 1024 ? 4 * Bp : 1024) * 4 + 32 * sizeof(int) + 12 * sizeof(float);
        static const int tile_attr_rc =          // once per process, thread-safe (function-local static initialiser)
            (int)hipFuncSetAttribute(reinterpret_cast<const void*>(batch_all_tile_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        DAE_CHECK_ARG(tile_attr_rc == 0, "batch_all: hipFuncSetAttribute failed (%d)", tile_attr_rc);
        DAE_LAUNCH(batch_all_tile_kernel<4>, dim3(n_anchors), dim3(TRIP_THREADS), tl, st, D_slabs, d_splits, slab_stride, ldd, labels, B, Bp,
                           loss_part, npos_part, G, role_cnt, fast, a0, /*order=*/nullptr, cls);   // every anchor is resident: the dispatch order is moot
        DAE_CHECK_LAUNCH();
        return 0;
    }
    typedef void (*ba_fn)(const float*, int, int64_t, int64_t, const int32_t*, int, int, float*, uint32_t*, float*, uint32_t*, int, int, const int32_t*, int, const int32_t*);
    ba_fn k = pos_only ? batch_all_kernel<true, 3> : batch_all_kernel<false, 3>;      // 3 workgroups per CU (168 VGPRs)
    static const int attr_rc = [] {
        int rc = 0;
        const ba_fn all[2] = {batch_all_kernel<true, 3>, batch_all_kernel<false, 3>};
        for (ba_fn f : all) rc |= (int)hipFuncSetAttribute(reinterpret_cast<const void*>(f), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        return rc;
    }();
    DAE_CHECK_ARG(attr_rc == 0, "batch_all: hipFuncSetAttribute failed (%d)", attr_rc);
    // at most one resident round: 3 workgroups per CU (168 VGPRs); the workgroups walk the anchor list in snake order (see the kernel)
    static const int cus = [] {                  // the device's CU count is read once; the resident slots follow THIS call's LDS footprint
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        return n;
    }();
    DAE_CHECK_ARG(cus > 0, "batch_all: cannot read the device's compute-unit count");
    const int per_cu = (int)((160 * 1024) / lds) < 3 ? (int)((160 * 1024) / lds) : 3;
    const int slots = cus * (per_cu < 1 ? 1 : per_cu);
    const int nwg = (g_miner_pack && n_anchors > slots) ? slots : n_anchors;
    DAE_LAUNCH(k, dim3(nwg), dim3(TRIP_THREADS), lds, st, D_slabs, d_splits, slab_stride, ldd, labels, B, Bp, loss_part, npos_part, G,
                       role_cnt, fast, a0, order, n_anchors, cls);
    DAE_CHECK_LAUNCH();
    return 0;
}

extern "C" int dae_triplet_batch_hard(const float* D_slabs, int32_t d_splits, int64_t slab_stride, int64_t ldd,
                                      const int32_t* labels, int32_t B, int32_t Bp, float* loss_part, uint32_t* cnt_part,
                                      int32_t* dw, float* G, void* stream) {
    return dae_triplet_batch_hard_rows(D_slabs, d_splits, slab_stride, ldd, labels, B, Bp, 0, B, loss_part, cnt_part, dw, G, stream);
}

extern "C" int dae_triplet_batch_hard_rows(const float* D_slabs, int32_t d_splits, int64_t slab_stride, int64_t ldd,
                                           const int32_t* labels, int32_t B, int32_t Bp, int32_t a0, int32_t n_anchors,
                                           float* loss_part, uint32_t* cnt_part, int32_t* dw, float* G, void* stream) {
    DAE_CHECK_ARG(a0 >= 0 && n_anchors > 0 && a0 + n_anchors <= B, "batch_hard: anchors [%d, %d) outside the batch of %d", a0, a0 + n_anchors, B);
    DAE_CHECK_ARG(D_slabs && labels && loss_part && cnt_part && dw && G, "batch_hard: null input");
    DAE_CHECK_ARG(B > 0 && B <= Bp && Bp <= 4 * TRIP_MAX_B, "batch_hard: batch %d too large", B);
    hipStream_t st = (hipStream_t)stream;
    DAE_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)Bp * sizeof(int32_t), st));
    const size_t lds = (size_t)Bp * 4 + 64;
    // Bp = 16384 needs 65 600 B, above the 64 KiB a kernel may take without asking: raise the limit once per process (as launch_batch_all does)
    static const int attr_rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(batch_hard_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        4 * TRIP_MAX_B * 4 + 64);
    DAE_CHECK_ARG(attr_rc == 0, "batch_hard: hipFuncSetAttribute failed (%d)", attr_rc);
    DAE_LAUNCH(batch_hard_kernel, dim3(n_anchors), dim3(TRIP_THREADS), lds, st, D_slabs, d_splits, slab_stride, ldd, labels, B, Bp,
                       loss_part, cnt_part, dw, G, a0);
    DAE_CHECK_LAUNCH();
    return 0;
}
