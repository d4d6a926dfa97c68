// dae_rnn_step.h -- the time steps of the LSTM and plain-RNN user models, shared by inference (dae_rnn.hip) and training
// (dae_rnn_fit.hip): the input projection's bias kernel, lstm_step_kernel and rnn_step_kernel.  The layout and the reasons for
// it: the head of dae_rnn.hip.
#pragma once
#include "dae_gru_step.h"       // gru_sigmoid and, through dae_score_sweep.h, gemm_mainloop, sweep_launch, al256

namespace dae {

constexpr int RNN_LDS = GRU_RING + 128 * 4 + 128 * 8;                // ring, items, U rows
constexpr int LSTM_LDS = RNN_LDS + 128 * 8;                         // and C rows

// (static: the header is compiled into two translation units of one library)
// P += b_ih + b_hh (rows < Na, columns < H of each of the G gate blocks)
static __global__ __launch_bounds__(256) void rnn_bias_kernel(float* __restrict__ P, int H, int Hp, int G, const float* __restrict__ b_ih,
                                                       const float* __restrict__ b_hh) {
    float* p = P + (int64_t)blockIdx.x * G * Hp;
    for (int q = threadIdx.x; q < G * Hp; q += 256) {
        const int g = q / Hp, j = q - g * Hp;
        if (j < H) p[q] += b_ih[g * H + j] + b_hh[g * H + j];
    }
}

struct RnnStepParams {
    GemmParams g;                 // one K segment: A = previous state buffer, Bt = W_hh image (gate q = tile rows q * Hp / 128 ...)
    const float* hprev;           // = g.seg[0].A
    float* hnext;                 // [pad128(M) x Hp]
    float* cell;                  // LSTM: [pad128(M) x Hp], updated in place
    const float* P;               // [pad128(Na) x G Hp]
    const int64_t* indptr; const int32_t* items; const int32_t* order;
    float* U; int64_t ldu;
    float* C; int64_t ldc;        // LSTM: [M x ldc] or NULL
    int64_t nnz;
    int Na, H, Hp, t, active, all_states;
};

// what the training forms (dae_rnn_fit.hip) add: the step's rows of the time-major stash.  Every pointer is the step's own slab,
// row = sorted position, [pad128(active) x Hp]; hprev / hnext are the slabs of the step and of the step after it.  The training
// forms run with all_states = 1 and U = C = cell = NULL: the U row of a tile's user is then the row's event, which goes to row_event.
struct RnnTrainParams : RnnStepParams {
    float* hout;                  // the state after the step (the loss kernel's operand)
    float* sh;                    // RNN: a second copy of it, which the backward step replaces by da
    int64_t* row_event;           // [pad128(active)] the event of the row, -1 in the padding
    int next;                     // rows of hnext that hold a state: the users with a further step (the rest of its 128-row blocks is zeroed)
};

struct LstmTrainParams : RnnTrainParams {
    float *si, *sf, *sg, *so;     // the gates i, f, g, o
    float* sc;                    // c', the cell after the step
    const float* cprev;           // the cell before it: slab s - 1 of the c' image, same sorted position (a slab of zeros at step 0)
};

// the tile's users: the item of this step, the row of U to write and (CELL: the LSTM) the row of C to write (-1: none)
template <bool CELL>
__device__ __forceinline__ void rnn_tile_rows(const RnnStepParams& p, int tm, int tid, int* s_item, long long* s_urow, long long* s_crow) {
    if (tid < 128) {
        const int i = tm * BM + tid;
        int it = 0;
        long long urow = -1;
        [[maybe_unused]] long long crow = -1;
        if (i < p.active) {
            const int64_t u = p.order[i];
            const int64_t e0 = p.indptr[u], e1 = p.indptr[u + 1];
            // e0 + t by the schedule's contract; a caller error (see dae_hip.h) must not become a stray read
            const int64_t e = max(min(min(e0 + p.t, e1 - 1), p.nnz - 1), (int64_t)0);
            it = min(max(p.items[e], 0), p.Na - 1);
            urow = p.all_states ? e : (e == e1 - 1 ? u : -1);
            if constexpr (CELL) crow = (p.C && e == e1 - 1) ? u : -1;
        }
        s_item[tid] = it;
        s_urow[tid] = urow;
        if constexpr (CELL) s_crow[tid] = crow;
    }
    __syncthreads();
}

// P = RnnStepParams: inference.  P = LstmTrainParams: the same arithmetic in the same order, and every value the backward pass
// needs goes to the stash when it is first complete (i after the first K loop, g after the second -- before it is multiplied into
// the carry --, f and c' after the third, o and h' after the fourth), so the training form keeps no more values live than the
// inference form; rows >= active and columns >= H of the stash are written as exact zeros.  The cell is read from cprev and
// written to sc instead of being updated in place.
template <bool SKIP_K, typename P = RnnStepParams>
__global__ __launch_bounds__(GEMM_THREADS, 1) void lstm_step_kernel(P p) {
    constexpr bool TRAIN = !__is_same(P, RnnStepParams);
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int* s_item = reinterpret_cast<int*>(lds + GRU_RING);
    long long* s_urow = reinterpret_cast<long long*>(lds + GRU_RING + 128 * 4);
    long long* s_crow = reinterpret_cast<long long*>(lds + GRU_RING + 128 * 4 + 128 * 8);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int tiles_n = p.Hp / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
    rnn_tile_rows<true>(p, tm, tid, s_item, s_urow, s_crow);
    if constexpr (TRAIN) { if (tid < 128 && tn == 0) p.row_event[tm * BM + tid] = s_urow[tid]; }
    const int Hp = p.Hp;
    const int col0 = tn * BN + wn * 64 + c;                     // this lane's columns: col0, col0 + 32
    const int rbase = wm * 64 + 4 * g;                          // its rows: rbase + acc_row(mt, r, 0)
    f32x16 acc[2][2], keep[2][2];                               // keep: i, then i * g, then c'
    // ---- i = sigmoid(P_i + acc) ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* pr = p.P + (int64_t)s_item[rbase + acc_row(mt, r, 0)] * (4 * Hp) + col0;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) keep[mt][nt][r] = gru_sigmoid(pr[nt * 32] + acc[mt][nt][r]);
            if constexpr (TRAIN) {
                const int i = tm * BM + rbase + acc_row(mt, r, 0);
                float* o = p.si + (int64_t)i * Hp + col0;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) o[nt * 32] = (i < p.active && col0 + nt * 32 < p.H) ? keep[mt][nt][r] : 0.f;
            }
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four rows' P values in flight, not all 32 (VGPRs)
        }
    __syncthreads();                                            // every wave is done with the staging ring
    // ---- g = tanh(P_g + acc), carry = i * g ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, 2 * tiles_n + tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* pr = p.P + (int64_t)s_item[rbase + acc_row(mt, r, 0)] * (4 * Hp) + 2 * Hp + col0;
            if constexpr (TRAIN) {
                const int i = tm * BM + rbase + acc_row(mt, r, 0);
                float* o = p.sg + (int64_t)i * Hp + col0;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float gg = tanhf(pr[nt * 32] + acc[mt][nt][r]);
                    o[nt * 32] = (i < p.active && col0 + nt * 32 < p.H) ? gg : 0.f;
                    keep[mt][nt][r] = keep[mt][nt][r] * gg;
                }
            } else {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) keep[mt][nt][r] = keep[mt][nt][r] * tanhf(pr[nt * 32] + acc[mt][nt][r]);
            }
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    __syncthreads();
    // ---- f = sigmoid(P_f + acc), c' = f * c + carry ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, tiles_n + tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = rbase + acc_row(mt, r, 0);
            const int i = tm * BM + lrow;
            if (i < p.active) {
                const float* pr = p.P + (int64_t)s_item[lrow] * (4 * Hp) + Hp + col0;
                if constexpr (TRAIN) {
                    const float* cp = p.cprev + (int64_t)i * Hp + col0;
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const float f = gru_sigmoid(pr[nt * 32] + acc[mt][nt][r]);
                        const bool in = col0 + nt * 32 < p.H;
                        const float v = in ? f * cp[nt * 32] + keep[mt][nt][r] : 0.f;
                        p.sf[(int64_t)i * Hp + col0 + nt * 32] = in ? f : 0.f;
                        p.sc[(int64_t)i * Hp + col0 + nt * 32] = v;
                        keep[mt][nt][r] = v;
                    }
                } else {
                    float* cp = p.cell + (int64_t)i * Hp + col0;
                    const long long crow = s_crow[lrow];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const float f = gru_sigmoid(pr[nt * 32] + acc[mt][nt][r]);
                        const bool in = col0 + nt * 32 < p.H;
                        const float v = in ? f * cp[nt * 32] + keep[mt][nt][r] : 0.f;
                        cp[nt * 32] = v;
                        keep[mt][nt][r] = v;
                        if (crow >= 0 && in) p.C[crow * p.ldc + col0 + nt * 32] = v;
                    }
                }
            } else if constexpr (TRAIN) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    p.sf[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                    p.sc[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                }
            }
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    __syncthreads();
    // ---- o = sigmoid(P_o + acc), h' = o * tanh(c') ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, 3 * tiles_n + tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = rbase + acc_row(mt, r, 0);
            const int i = tm * BM + lrow;
            if (i < p.active) {
                const float* pr = p.P + (int64_t)s_item[lrow] * (4 * Hp) + 3 * Hp + col0;
                float* hn = p.hnext + (int64_t)i * Hp + col0;
                const long long urow = s_urow[lrow];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float o = gru_sigmoid(pr[nt * 32] + acc[mt][nt][r]);
                    const bool in = col0 + nt * 32 < p.H;
                    const float v = in ? o * tanhf(keep[mt][nt][r]) : 0.f;
                    if constexpr (TRAIN) {
                        p.so[(int64_t)i * Hp + col0 + nt * 32] = in ? o : 0.f;
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
                    p.so[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                    p.hout[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                    if (i < ((p.next + BM - 1) & ~(BM - 1))) p.hnext[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                }
            }
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
}

// P = RnnStepParams: inference.  P = RnnTrainParams: the same arithmetic; h' goes to hout (which the loss kernel replaces by G), to
// sh (which keeps it for the backward step's 1 - h'^2) and, for the users with a further step, to hnext.
template <bool SKIP_K, typename P = RnnStepParams>
__global__ __launch_bounds__(GEMM_THREADS, 2) void rnn_step_kernel(P p) {
    constexpr bool TRAIN = !__is_same(P, RnnStepParams);
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int* s_item = reinterpret_cast<int*>(lds + GRU_RING);
    long long* s_urow = reinterpret_cast<long long*>(lds + GRU_RING + 128 * 4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, c = lane & 31;
    const int tiles_n = p.Hp / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
    rnn_tile_rows<false>(p, tm, tid, s_item, s_urow, nullptr);
    if constexpr (TRAIN) { if (tid < 128 && tn == 0) p.row_event[tm * BM + tid] = s_urow[tid]; }
    const int Hp = p.Hp;
    const int col0 = tn * BN + wn * 64 + c;
    const int rbase = wm * 64 + 4 * g;
    f32x16 acc[2][2];
    // ---- h' = tanh(P + acc) ----
    if constexpr (SKIP_K) zero_acc(acc);
    else gemm_mainloop<float, 2>(p.g, tm, tn, 0, p.g.ktiles_total, lds, acc);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = rbase + acc_row(mt, r, 0);
            const int i = tm * BM + lrow;
            if (i < p.active) {
                const float* pr = p.P + (int64_t)s_item[lrow] * Hp + col0;
                float* hn = p.hnext + (int64_t)i * Hp + col0;
                const long long urow = s_urow[lrow];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const bool in = col0 + nt * 32 < p.H;
                    const float v = in ? tanhf(pr[nt * 32] + acc[mt][nt][r]) : 0.f;
                    if constexpr (TRAIN) {
                        p.hout[(int64_t)i * Hp + col0 + nt * 32] = v;
                        p.sh[(int64_t)i * Hp + col0 + nt * 32] = v;
                        if (i < ((p.next + BM - 1) & ~(BM - 1))) hn[nt * 32] = i < p.next ? v : 0.f;
                    } else {
                        hn[nt * 32] = v;
                        if (urow >= 0 && in) p.U[urow * p.ldu + col0 + nt * 32] = v;
                    }
                }
            } else if constexpr (TRAIN) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    p.hout[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                    p.sh[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                    if (i < ((p.next + BM - 1) & ~(BM - 1))) p.hnext[(int64_t)i * Hp + col0 + nt * 32] = 0.f;
                }
            }
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
}

}  // namespace dae
