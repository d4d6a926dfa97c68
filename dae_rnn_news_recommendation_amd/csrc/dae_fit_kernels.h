// dae_fit_kernels.h -- the cell-independent kernels of the recurrent trainers, shared by dae_gru_fit.hip and dae_rnn_fit.hip: the
// loss on the stashed states (gru_loss_kernel, gru_loss_fold_kernel) and the 64 x 64 transpose that makes the K-contiguous images
// of the weight-gradient GEMMs (gru_transpose_kernel).  What they compute and why: the head of dae_gru_fit.hip.
// (static: the header is compiled into two translation units of one library)
#pragma once
#include "dae_gru_step.h"

namespace dae {

constexpr int GF_MAX_NEG = 16;
constexpr int GF_MAX_SPLITS = 16;

struct GruLossParams {
    const float* E; int64_t lde; int Na, H, Hp;
    const int32_t* items; const int32_t* negatives; int n_neg; int64_t nnz;
    float* hg;                    // [R x Hp] in: the state after the row's event; out: G
    const int64_t* row_event;     // [R]
    int64_t R;
    double* rowloss; int32_t* rowpairs; float* margin;
};

static __global__ __launch_bounds__(256) void gru_loss_kernel(GruLossParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= p.R) return;
    const int64_t ev = p.row_event[row];
    if (ev < 0) {                                               // padding: its row of HG is zero already
        if (lane == 0) { p.rowloss[row] = 0.0; p.rowpairs[row] = 0; }
        return;
    }
    const int64_t e = min(ev + 1, p.nnz - 1);                    // the event this state predicts (ev + 1 by the schedule's contract)
    const int raw = p.items[e];
    const float* pos = p.E + (int64_t)min(max(raw, 0), p.Na - 1) * p.lde;
    float* h = p.hg + row * p.Hp;
    float cj[GF_MAX_NEG];
    int nj[GF_MAX_NEG];
    double loss = 0.0;
    int pairs = 0;
#pragma unroll
    for (int j = 0; j < GF_MAX_NEG; ++j) {
        cj[j] = 0.f; nj[j] = -1;
        if (j < p.n_neg) {
            const int v = p.negatives[e * p.n_neg + j];
            if (v >= 0 && v != raw) {                           // the same in every lane
                nj[j] = min(v, p.Na - 1);
                const float* ng = p.E + (int64_t)nj[j] * p.lde;
                float s = 0.f;
                for (int col = lane; col < p.H; col += 64) s = fmaf(h[col], pos[col] - ng[col], s);
                const float x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave64_sum_hi(s)), 63));
                const float ee = expf(-fabsf(x));
                const float rr = 1.0f / (1.0f + ee);
                cj[j] = -(x >= 0.f ? ee * rr : rr);             // -sigmoid(-x)
                loss += (double)(fmaxf(-x, 0.f) + log1pf(ee));  // softplus(-x)
                ++pairs;
                if (p.margin && lane == 0) p.margin[e * p.n_neg + j] = x;
            }
        }
    }
    for (int col = lane; col < p.Hp; col += 64) {
        float gsum = 0.f;
        if (col < p.H) {
            const float pv = pos[col];
#pragma unroll
            for (int j = 0; j < GF_MAX_NEG; ++j)
                if (nj[j] >= 0) gsum = fmaf(cj[j], pv - p.E[(int64_t)nj[j] * p.lde + col], gsum);
        }
        h[col] = gsum;
    }
    if (lane == 0) { p.rowloss[row] = loss; p.rowpairs[row] = pairs; }
}

// one workgroup: thread t adds the rows t, t + 256, ... in ascending order, then the 256 sums are added pairwise in LDS
static __global__ __launch_bounds__(256) void gru_loss_fold_kernel(const double* __restrict__ rowloss, const int32_t* __restrict__ rowpairs, int64_t R,
                                                            double* __restrict__ loss, int64_t* __restrict__ n_pairs) {
    __shared__ double sl[256];
    __shared__ long long sp[256];
    double l = 0.0;
    long long n = 0;
    for (int64_t r = threadIdx.x; r < R; r += 256) { l += rowloss[r]; n += rowpairs[r]; }
    sl[threadIdx.x] = l; sp[threadIdx.x] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sp[threadIdx.x] += sp[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { *loss = sl[0]; *n_pairs = sp[0]; }
}

// dst[c][r] = src[r][c] on 64 x 64 tiles through LDS; grid (rows / 64, cols / 64).  GATHER: src row r is E[items[row_event[r]]]
// (columns >= H and the padding rows read as zero) instead of a row of a stash image.
template <bool GATHER>
static __global__ __launch_bounds__(256) void gru_transpose_kernel(const float* __restrict__ src, int64_t ld_src, const int64_t* __restrict__ row_event,
                                                            const int32_t* __restrict__ items, int Na, int H, float* __restrict__ dst,
                                                            int64_t ld_dst) {
    __shared__ float t[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int c0 = (int)blockIdx.y * 64;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int rr = ty + 4 * k;
        float v = 0.f;
        if constexpr (GATHER) {
            const int64_t e = row_event[r0 + rr];
            if (e >= 0 && c0 + tx < H) v = src[(int64_t)min(max(items[e], 0), Na - 1) * ld_src + c0 + tx];
        } else {
            v = src[(r0 + rr) * ld_src + c0 + tx];
        }
        t[rr][tx] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int cc = ty + 4 * k;
        dst[(int64_t)(c0 + cc) * ld_dst + r0 + tx] = t[tx][cc];
    }
}

// rows of the stash a call can need at most: every step's slab is padded to 128 rows
static inline int64_t gf_rows_bound(int64_t nnz, int64_t T) { return pad128(nnz + 128 * T); }

}  // namespace dae
