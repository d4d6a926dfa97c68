// dae_gru_step.h -- the time step of the GRU user model, shared by inference (dae_gru.hip) and training (dae_gru_fit.hip):
// the gate arithmetic, the per-article input projection's bias kernel and gru_step_kernel.  The layout and the reasons for it: the head of dae_gru.hip.
#pragma once
#include "dae_score_sweep.h"      // gemm_mainloop, al256, sweep_launch

namespace dae {

constexpr int GRU_RING = lds_bytes_for(2);
constexpr int GRU_LDS = GRU_RING + 128 * 4 + 128 * 8;

// logistic with expf (not the fast __expf of sigmoidf_): the recurrence feeds its own output back up to T times
__device__ __forceinline__ float gru_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    const float r = 1.0f / (1.0f + e);
    return x >= 0.f ? r : e * r;
}

// (static: the header is compiled into two translation units of one library)
// P += the biases that do not depend on h (rows < Na, columns < H of every gate block); bhn = the zero-padded image of b_hn
static __global__ __launch_bounds__(256) void gru_bias_kernel(float* __restrict__ P, int Na, int H, int Hp, const float* __restrict__ b_ih,
                                                       const float* __restrict__ b_hh, float* __restrict__ bhn) {
    const int a = blockIdx.x;
    if (a == Na) {                                              // the extra block
        for (int j = threadIdx.x; j < Hp; j += 256) bhn[j] = j < H ? b_hh[2 * H + j] : 0.f;
        return;
    }
    float* p = P + (int64_t)a * 3 * Hp;
    for (int q = threadIdx.x; q < 3 * Hp; q += 256) {
        const int g = q / Hp, j = q - g * Hp;
        if (j < H) p[q] += g < 2 ? b_ih[g * H + j] + b_hh[g * H + j] : b_ih[g * H + j];
    }
}

struct GruStepParams {
    GemmParams g;                 // one K segment: A = previous state buffer, Bt = W_hh image (gate g = tile rows g * Hp / 128 ...)
    const float* hprev;           // = g.seg[0].A
    float* hnext;                 // [pad128(M) x Hp]
    const float* P;               // [pad128(Na) x 3 Hp]
    const float* bhn;             // [Hp]
    const int64_t* indptr; const int32_t* items; const int32_t* order;
    float* U; int64_t ldu;
    int64_t nnz;
    int Na, H, Hp, t, active, all_states, skip_k;
};

// what the training form (dae_gru_fit.hip) adds: the step's rows of the time-major stash.  Every pointer is the step's own slab,
// row = sorted position, [pad128(active) x Hp]; hprev / hnext are the slabs of the step and of the step after it.
struct GruTrainParams : GruStepParams {
    float *sr, *sz, *sn, *sq;     // r, z, n and q = W_hn h + b_hn
    float* hout;                  // the state after the step (the loss kernel's operand)
    int64_t* row_event;           // [pad128(active)] the event of the row, -1 in the padding
    int next;                     // rows of hnext that hold a state: the users with a further step (the rest of its 128-row blocks is zeroed)
};

// P = GruStepParams: inference.  P = GruTrainParams: the same arithmetic, and every value the backward pass needs goes to the stash
// when it is first complete (r after the first K loop, q and n after the second, z and h' after the third), so the training form
// keeps no more values live than the inference form; rows >= active and columns >= H of the stash are written as exact zeros.
template <bool SKIP_K, typename P = GruStepParams>
__global__ __launch_bounds__(GEMM_THREADS, 1) void gru_step_kernel(P p) {
    constexpr bool TRAIN = !__is_same(P, GruStepParams);
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int* s_item = reinterpret_cast<int*>(lds + GRU_RING);                       // the tile's users: item of this step,
    long long* s_urow = reinterpret_cast<long long*>(lds + GRU_RING + 128 * 4);  // row of U to write (-1: none)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int tiles_n = p.Hp / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
    if (tid < 128) {
        const int i = tm * BM + tid;
        int it = 0;
        long long urow = -1;
        [[maybe_unused]] long long ev = -1;
        if (i < p.active) {
            const int64_t u = p.order[i];
            const int64_t e0 = p.indptr[u], e1 = p.indptr[u + 1];
            // e0 + t by the schedule's contract; a caller error (see dae_hip.h) must not become a stray read
            const int64_t e = max(min(min(e0 + p.t, e1 - 1), p.nnz - 1), (int64_t)0);
            it = min(max(p.items[e], 0), p.Na - 1);
            urow = p.all_states ? e : (e == e1 - 1 ? u : -1);
            ev = e;
        }
        s_item[tid] = it;
        s_urow[tid] = urow;
        if constexpr (TRAIN) { if (tn == 0) p.row_event[i] = ev; }
    }
    __syncthreads();
    const int Hp = p.Hp;
    const int col0 = tn * BN + wn * 64 + c;                     // this lane's columns: col0, col0 + 32
    const int rbase = wm * 64 + 4 * g;                          // its rows: rbase + acc_row(mt, r, 0)
    f32x16 acc[2][2], keep[2][2];                               // keep: r, then n
    // ---- r = sigmoid(P_r + acc) ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, tn, 0, p.g.ktiles_total, lds, acc);
    {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* pr = p.P + (int64_t)s_item[rbase + acc_row(mt, r, 0)] * (3 * Hp) + col0;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) keep[mt][nt][r] = gru_sigmoid(pr[nt * 32] + acc[mt][nt][r]);
                if constexpr (TRAIN) {
                    const int i = tm * BM + rbase + acc_row(mt, r, 0);
                    float* o = p.sr + (int64_t)i * Hp + col0;
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) o[nt * 32] = (i < p.active && col0 + nt * 32 < p.H) ? keep[mt][nt][r] : 0.f;
                }
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four rows' P values in flight, not all 32 (VGPRs)
            }
    }
    __syncthreads();                                            // every wave is done with the staging ring
    // ---- n = tanh(P_n + r * (acc + b_hn)) ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, 2 * tiles_n + tn, 0, p.g.ktiles_total, lds, acc);
    {
        const float bn0 = p.bhn[col0], bn1 = p.bhn[col0 + 32];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* pr = p.P + (int64_t)s_item[rbase + acc_row(mt, r, 0)] * (3 * Hp) + 2 * Hp + col0;
                if constexpr (TRAIN) {
                    const int i = tm * BM + rbase + acc_row(mt, r, 0);
                    const bool live = i < p.active;
                    const float q0 = acc[mt][0][r] + bn0, q1 = acc[mt][1][r] + bn1;
                    keep[mt][0][r] = tanhf(pr[0] + keep[mt][0][r] * q0);
                    keep[mt][1][r] = tanhf(pr[32] + keep[mt][1][r] * q1);
                    float* oq = p.sq + (int64_t)i * Hp + col0;
                    float* on = p.sn + (int64_t)i * Hp + col0;
                    const bool in0 = live && col0 < p.H, in1 = live && col0 + 32 < p.H;
                    oq[0] = in0 ? q0 : 0.f;  oq[32] = in1 ? q1 : 0.f;
                    on[0] = in0 ? keep[mt][0][r] : 0.f;  on[32] = in1 ? keep[mt][1][r] : 0.f;
                } else {
                    keep[mt][0][r] = tanhf(pr[0] + keep[mt][0][r] * (acc[mt][0][r] + bn0));
                    keep[mt][1][r] = tanhf(pr[32] + keep[mt][1][r] * (acc[mt][1][r] + bn1));
                }
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
    }
    __syncthreads();
    // ---- z = sigmoid(P_z + acc), h' = (1 - z) n + z h ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, tiles_n + tn, 0, p.g.ktiles_total, lds, acc);
    {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = rbase + acc_row(mt, r, 0);
                const int i = tm * BM + lrow;
                if (i < p.active) {
                    const float* pr = p.P + (int64_t)s_item[lrow] * (3 * Hp) + Hp + col0;
                    const float* hp = p.hprev + (int64_t)i * Hp + col0;
                    float* hn = p.hnext + (int64_t)i * Hp + col0;
                    const long long urow = s_urow[lrow];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const float z = gru_sigmoid(pr[nt * 32] + acc[mt][nt][r]);
                        const float h = hp[nt * 32];
                        const bool in = col0 + nt * 32 < p.H;
                        const float v = in ? (1.0f - z) * keep[mt][nt][r] + z * h : 0.f;
                        if constexpr (TRAIN) {
                            p.sz[(int64_t)i * Hp + col0 + nt * 32] = in ? z : 0.f;
                            p.hout[(int64_t)i * Hp + col0 + nt * 32] = v;
                            if (i < ((p.next + BM - 1) & ~(BM - 1))) hn[nt * 32] = i < p.next ? v : 0.f;
                        } else {
                            hn[nt * 32] = v;
                            if (urow >= 0 && in) p.U[urow * p.ldu + col0 + nt * 32] = v;
                        }
                    }
                } else if constexpr (TRAIN) {
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        p.sz[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                        p.hout[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                        if (i < ((p.next + BM - 1) & ~(BM - 1))) p.hnext[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                    }
                }
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
    }
}

}  // namespace dae
