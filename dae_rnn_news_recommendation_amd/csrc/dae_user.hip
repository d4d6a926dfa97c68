// dae_user.hip -- user states from browsing histories (dae_user_states): the decaying model of "Embedding-based News
// Recommendation for Millions of Users" (KDD'17), a decay-weighted mean of the embeddings of the articles a user has read.
//
// Per user, events oldest first:   s = d_e * s + E[items[e]],   z = d_e * z + 1,   state_e = s / z      (s: H floats, z: one)
//
// Layout.  One wave per (user, 256-column chunk of H): a lane owns 4 columns, so H = 500 is two waves per user and the longest
// history -- the tail of a skewed batch -- is walked by ceil(H / 256) waves side by side.  The recurrence is a dependent chain
// per column, but the rows it needs are known up front: a wave reads 64 item ids (and factors) with one load per lane, then
// issues the row loads of US_BATCH events back to back before the first fused multiply-add of the batch, as encode_csr_kernel
// does with its W rows.  VEC: a lane's 4 columns are adjacent (one 16-byte load per row) when E, U and their strides are
// 16-byte aligned and H is a multiple of 4; otherwise the lane's columns are 64 apart (four coalesced 4-byte loads).
//
// Arithmetic: one fmaf per column and event for s, one fmaf for z (every lane computes the same z), one IEEE division per
// output.  The order is the event order, there are no atomics and no cross-lane sums, and both output modes run the same
// instructions on the same values: the result is bit-identical run to run, independent of the order of the users, of VEC
// and of the grid, and the last all_states row of a user equals its last-state row bit for bit.
#include "dae_common.h"

namespace dae {

constexpr int US_THREADS = 256;             // 4 waves: 4 (user, chunk) pairs per workgroup
constexpr int US_CHUNK = 256;               // columns per wave
constexpr int US_BATCH = 8;                 // row loads in flight per lane (4 VGPRs each)

struct UserArgs {
    const float* E; int64_t lde; int Na, H;
    const int64_t* indptr; const int32_t* items; const float* decay; float beta;
    int64_t M; int chunks; int all_states;
    float* U; int64_t ldu;
};

template <bool VEC>
__global__ __launch_bounds__(US_THREADS) void user_states_kernel(UserArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (US_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t u = w / a.chunks;
    if (u >= a.M) return;
    const int c0 = (int)(w % a.chunks) * US_CHUNK;
    int col[4]; bool on[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        col[q] = VEC ? c0 + lane * 4 + q : c0 + q * 64 + lane;
        on[q] = col[q] < a.H;
    }
    const int64_t e0 = a.indptr[u], e1 = a.indptr[u + 1];
    float s[4] = {0.f, 0.f, 0.f, 0.f}, z = 0.f;
    // columns past H read column 0 of the row (in bounds) and are never written
    const float* Eb = a.E + (VEC ? (on[0] ? col[0] : 0) : 0);
    for (int64_t base = e0; base < e1; base += 64) {
        const int64_t ke = min(base + lane, e1 - 1);
        int it = a.items[ke];
        it = min(max(it, 0), a.Na - 1);                             // a caller error (see dae_hip.h) must not become a stray read
        float dv = a.decay ? a.decay[ke] : a.beta;
        if (ke == e0) dv = 0.f;                                     // a user's first factor is ignored
        const int n = (int)min((int64_t)64, e1 - base);
        for (int b = 0; b < n; b += US_BATCH) {
            f32x4 x[US_BATCH]; float d[US_BATCH];
#pragma unroll
            for (int j = 0; j < US_BATCH; ++j) {
                const int l = min(b + j, n - 1);
                const int row = __builtin_amdgcn_readlane(it, l);
                d[j] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dv), l));
                const float* r = Eb + (int64_t)row * a.lde;
                if constexpr (VEC) {
                    x[j] = *reinterpret_cast<const f32x4*>(r);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) x[j][q] = r[on[q] ? col[q] : 0];
                }
            }
#pragma unroll
            for (int j = 0; j < US_BATCH; ++j) {
                if (b + j < n) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) s[q] = fmaf(d[j], s[q], x[j][q]);
                    z = fmaf(d[j], z, 1.0f);
                    if (a.all_states) {
                        float* o = a.U + (base + b + j) * a.ldu;
                        if constexpr (VEC) {
                            if (on[0]) *reinterpret_cast<f32x4*>(o + col[0]) = f32x4{s[0] / z, s[1] / z, s[2] / z, s[3] / z};
                        } else {
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                if (on[q]) o[col[q]] = s[q] / z;
                        }
                    }
                }
            }
        }
    }
    if (!a.all_states) {
        float* o = a.U + u * a.ldu;
        const bool any = e1 > e0;
        if constexpr (VEC) {
            if (on[0]) *reinterpret_cast<f32x4*>(o + col[0]) = any ? f32x4{s[0] / z, s[1] / z, s[2] / z, s[3] / z} : f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (on[q]) o[col[q]] = any ? s[q] / z : 0.f;
        }
    }
}

}  // namespace dae

using namespace dae;

extern "C" int dae_user_states(const float* E, int64_t lde, int32_t Na, int32_t H, const int64_t* indptr, const int32_t* items,
                               int64_t M, int64_t nnz, float beta, const float* decay, int32_t all_states, float* U, int64_t ldu,
                               void* stream) {
    DAE_CHECK_ARG(M >= 0 && nnz >= 0, "user_states: negative count (M = %lld, nnz = %lld)", (long long)M, (long long)nnz);
    DAE_CHECK_ARG(H > 0, "user_states: H must be positive (got %d)", H);
    DAE_CHECK_ARG(Na > 0, "user_states: Na must be positive (got %d)", Na);
    DAE_CHECK_ARG(E && indptr, "user_states: E / indptr are NULL");
    DAE_CHECK_ARG(items || nnz == 0, "user_states: items is NULL");
    DAE_CHECK_ARG(U || (all_states ? nnz : M) == 0, "user_states: U is NULL");
    DAE_CHECK_ARG(lde >= H && ldu >= H, "user_states: lde (%lld) and ldu (%lld) must be >= H (%d)", (long long)lde, (long long)ldu, H);
    DAE_CHECK_ARG(decay || (beta >= 0.f && beta <= 1.f), "user_states: beta must be in [0, 1] (got %g)", (double)beta);
    if (M == 0) return 0;
    const int chunks = (H + US_CHUNK - 1) / US_CHUNK;
    const int64_t blocks = (M * chunks + US_THREADS / 64 - 1) / (US_THREADS / 64);
    DAE_CHECK_ARG(blocks < (1ll << 31), "user_states: M x ceil(H / %d) = %lld waves exceed the grid", US_CHUNK, (long long)(M * chunks));
    UserArgs a;
    a.E = E; a.lde = lde; a.Na = Na; a.H = H; a.indptr = indptr; a.items = items; a.decay = decay; a.beta = beta;
    a.M = M; a.chunks = chunks; a.all_states = all_states ? 1 : 0; a.U = U; a.ldu = ldu;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = H % 4 == 0 && lde % 4 == 0 && ldu % 4 == 0 && ((uintptr_t)E % 16) == 0 && ((uintptr_t)U % 16) == 0;
    if (vec) DAE_LAUNCH(user_states_kernel<true>, dim3((unsigned)blocks), dim3(US_THREADS), 0, st, a);
    else DAE_LAUNCH(user_states_kernel<false>, dim3((unsigned)blocks), dim3(US_THREADS), 0, st, a);
    DAE_CHECK_LAUNCH();
    return 0;
}
