// dae_words.hip -- the word-based user model (section 5.1 of "Embedding-based News Recommendation for Millions of Users"): an article
// is the set of its words (a CSR row over a vocabulary of V columns), a user is the set of the words of the articles clicked, and
// the relevance R(u, a) is the sum of article a's entry weights over the words the two share.  The rules are stated in
// include/dae_hip.h; here is how they run.
//
// Profiles (dae_word_profiles).  Word-major bitmaps per tile of 128 users: bits [ceil(M / 128)][V][4] uint32, bit (u & 31) of word
// (u & 127) >> 5 of cell (u >> 7, w) says "user u has word w" -- 16 bytes per (tile, word), which is what the score kernel reads per
// article entry.  The buffer is zeroed, then word_profile_kernel, one wave per user, walks the rows of the clicked articles and sets
// bits with integer atomicOr (exact, whatever the schedule); word_sizes_kernel counts every user's set bits in a pass over the bitmap
// (one bit test per (user, word), two partial counts per user added through LDS): no atomics.
//
// Entry weights (dae_word_entry_weights): e_p = x_p, or fl32(term_weights[c_p] * x_p), once per stored entry (x_p = 1 without
// values); an entry whose column lies outside [0, V) gets +0 and is never looked up.
//
// Scores.  s_0 = +0, s_i = fl32(s_{i-1} + (c_i in profile(u) ? e_i : +0)) over a's entries in storage order (ascending columns), one
// __fadd_rn per entry: no product, so nothing can be contracted, and s never becomes -0.  Three places compute it by that sequence
// -- the sweep below, the target's score and the fix-up of the rank -- so their results are bit-equal.
//
// Top-k (dae_word_topk), phase A = word_topk_kernel: grid = (user tiles) x (corpus slices) of sweep_splits / window_prologue, 256
// threads.  Per 128-article tile thread t owns article j = t & 127 and the 64 users of half h = t >> 7: 64 partial scores in VGPRs.
// The tile's CSR rows go through LDS in passes of WORD_PASS entries per article: the 256 threads load entry i of article a for
// (a, i) = (s / WORD_PASS, s % WORD_PASS), so a wave reads two runs of 32 consecutive entries, and store it at [i][a] with a row
// stride of 129 words, which makes thread j's read of [i][j] conflict-free (the transposing store is 4-way conflicted; it is 1 / 128
// of the work).  Slots behind a row's end hold (column 0, weight +0).  Per entry a thread loads the 8 bytes of its half of the
// column's mask (the V x 16 byte table of the user tile stays in L2) and does 64 select-adds: v_bfe_i32 spreads user q's bit over a
// word, v_and keeps e or +0, v_add.  Four entries' masks are in flight at a time.  The staging lies over the score tile, which is
// dead while the scores are in registers; then the 128 x 128 scores go to LDS as the [128][128] fp32 tile of acc_to_tile (row = user,
// column = article: a lane's 64 stores have stride 128 words, the 64 lanes of a store are consecutive -- conflict-free) and the
// epilogue is top-k's (topk_tile_epilogue, dae_score_sweep.h).  Phase B is topk_merge_kernel<false> (topk_merge_launch).
// LDS: 64 KiB tile / staging (33 KiB used) + 9.5 KiB top-k scratch + 1 KiB windows + 1.5 KiB row starts = 76 KiB: two workgroups
// per CU.  VGPRs: 64 scores + 8 masks + 8 staged words + addresses, far below the 256 that two workgroups per CU leave a wave.
//
// Rank (dae_word_rank): word_target_kernel, one wave per user, computes the target's score (lane 0: the adds are sequential) and
// writes tkey = pair_key(score, t), target_score and rank = 1 (0 without a target); word_rank_kernel is the sweep with a counting
// epilogue straight from the registers -- per user q of the half one ballot of key > tkey[q] over the wave's 64 articles and a
// popcount, lane q keeping user q's count for the slice; columns >= Na and columns outside the user's window are masked, the
// target has an equal key -- counts meet in LDS integer atomics and one integer atomic per row goes to rank; word_fixup_kernel, one
// wave per user, lane per seen item, recomputes the score of every seen item inside the window and takes 1 off rank where its key
// is above the target's.  Integers only: bit-identical run to run and independent of the grid.
#include "dae_score_sweep.h"

namespace dae {

constexpr int WORD_PASS = 32;                      // entries per article and staging pass
constexpr int WORD_LDW = 129;                      // row stride of the staged [WORD_PASS][128] arrays, in words
constexpr int WORD_STAGE_BYTES = 2 * WORD_PASS * WORD_LDW * 4;
static_assert(WORD_STAGE_BYTES <= TOPK_TILE_BYTES, "the staging lies over the score tile");
constexpr int WORD_ROWS_BYTES = 128 * 8 + 128 * 4 + 16;       // the tile's row starts, row lengths and the longest length
constexpr int WORD_TOPK_LDS = TOPK_WIN_LDS + WORD_ROWS_BYTES;
constexpr int WORD_RANK_LDS = WORD_STAGE_BYTES + 128 * 8 + 128 * 4 + 2 * 128 * 4 + 16 + WORD_ROWS_BYTES;
constexpr int WORD_RANK_SLOTS = 512;

struct WordCsr {
    const int64_t* indptr;        // [Na + 1]
    const int32_t* indices;       // [nnz] ascending and unique per row
    const float* weights;         // [nnz] entry weights (dae_word_entry_weights)
    int64_t nnz;
    int Na, V;
};

// row a's entries [r0, r0 + n), clamped to the arrays: a caller error must not become a stray read
__device__ __forceinline__ void word_row(const WordCsr& A, int a, int64_t& r0, int& n) {
    const int64_t b = min(max(A.indptr[a], (int64_t)0), A.nnz), e = min(max(A.indptr[a + 1], b), A.nnz);
    r0 = b;
    n = (int)min(e - b, (int64_t)INT32_MAX);
}

// the 16-byte cell of user tile qt and word w
__device__ __forceinline__ const uint32_t* word_cell(const uint32_t* bits, int V, int qt, int w) { return bits + ((int64_t)qt * V + w) * 4; }

// R(u, a) by the sequence of the sweep
__device__ __forceinline__ float word_pair_score(const WordCsr& A, const uint32_t* bits, int u, int a) {
    int64_t r0; int n;
    word_row(A, a, r0, n);
    const uint32_t* B = word_cell(bits, A.V, u >> 7, 0) + ((u & 127) >> 5);
    const int sh = u & 31;
    float s = 0.f;
    for (int i = 0; i < n; ++i) {
        const int c = A.indices[r0 + i];
        if ((unsigned)c >= (unsigned)A.V) continue;
        const uint32_t m = (uint32_t)((int32_t)(B[(int64_t)c * 4] << (31 - sh)) >> 31);
        s = __fadd_rn(s, __uint_as_float(__float_as_uint(A.weights[r0 + i]) & m));
    }
    return s;
}

__global__ __launch_bounds__(256) void word_weights_kernel(const int32_t* __restrict__ indices, const float* __restrict__ values, int64_t nnz,
                                                           int V, const float* __restrict__ tw, float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnz) return;
    const int c = indices[p];
    float e = 0.f;
    if ((unsigned)c < (unsigned)V) {
        const float x = values ? values[p] : 1.f;
        e = tw ? __fmul_rn(tw[c], x) : x;
    }
    out[p] = e;
}

// one wave per user, four users per workgroup
__global__ __launch_bounds__(256) void word_profile_kernel(const int64_t* __restrict__ hp, const int32_t* __restrict__ hi, int64_t hnnz, int M,
                                                           int max_events, WordCsr A, uint32_t* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int64_t u64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u64 >= M) return;
    const int u = (int)u64;
    const int64_t h0 = min(max(hp[u], (int64_t)0), hnnz), h1 = min(max(hp[u + 1], h0), hnnz);
    const int64_t first = max_events > 0 && h1 - h0 > max_events ? h1 - max_events : h0;
    uint32_t* B = bits + (int64_t)(u >> 7) * A.V * 4 + ((u & 127) >> 5);
    const uint32_t bit = 1u << (u & 31);
    for (int64_t e = first; e < h1; ++e) {
        const int a = hi[e];
        if (a < 0 || a >= A.Na) continue;
        int64_t r0; int n;
        word_row(A, a, r0, n);
        for (int i = lane; i < n; i += 64) {
            const int c = A.indices[r0 + i];
            if ((unsigned)c < (unsigned)A.V) atomicOr(&B[(int64_t)c * 4], bit);
        }
    }
}

// one workgroup per user tile: thread t counts the words w = t >> 7, (t >> 7) + 2, ... of user t & 127
__global__ __launch_bounds__(256) void word_sizes_kernel(const uint32_t* __restrict__ bits, int M, int V, int32_t* __restrict__ sizes) {
    __shared__ int part[256];
    const int tid = threadIdx.x, r = tid & 127;
    const uint32_t* B = word_cell(bits, V, blockIdx.x, 0) + (r >> 5);
    int n = 0;
    for (int w = tid >> 7; w < V; w += 2) n += (int)((B[(int64_t)w * 4] >> (r & 31)) & 1u);
    part[tid] = n;
    __syncthreads();
    const int u = blockIdx.x * 128 + tid;
    if (tid < 128 && u < M) sizes[u] = part[tid] + part[tid + 128];
}

struct WordSweep {
    WordCsr A;
    const uint32_t* bits;         // [ceil(M / 128)][V][4]
    int Nq, Nc, Nqp, k, splits, ctiles;       // Nq = M users, Nc = Na articles (the names topk_tile_epilogue reads)
    uint64_t* part;               // [splits][Nqp][k] sorted keys (top-k)
    int* part_n;                  // [splits][Nqp]
    RowFilter f;
    const uint64_t* tkey;         // [Nqp] target keys (rank)
    int32_t* rank;                // [Nq]
};

// The scores of user tile qt against article tile ct: acc[q] = R(qt * 128 + h * 64 + q, ct * 128 + j) for the thread's article
// j = tid & 127 and half h = tid >> 7.  stage: WORD_STAGE_BYTES of LDS, rs / rl / mx: WORD_ROWS_BYTES.  Ends behind a barrier.
__device__ __forceinline__ void word_score_tile(const WordSweep& p, int qt, int ct, char* stage, int64_t* rs, int* rl, int* mx, float (&acc)[64]) {
    const int tid = threadIdx.x, j = tid & 127, h = tid >> 7;
    int* sc = reinterpret_cast<int*>(stage);
    float* se = reinterpret_cast<float*>(stage) + WORD_PASS * WORD_LDW;
    if (tid == 0) *mx = 0;
    __syncthreads();                                            // the last tile's readers of rs / rl / mx and of the score tile are done
    if (tid < 128) {
        const int a = ct * BN + tid;
        int64_t r0 = 0; int n = 0;
        if (a < p.Nc) word_row(p.A, a, r0, n);
        rs[tid] = r0; rl[tid] = n;
        if (n > 0) atomicMax(mx, n);
    }
#pragma unroll
    for (int q = 0; q < 64; ++q) acc[q] = 0.f;
    __syncthreads();
    const int longest = *mx, mine = rl[j];
    const char* cell = reinterpret_cast<const char*>(word_cell(p.bits, p.A.V, qt, 0)) + h * 8;
    for (int p0 = 0; p0 < longest; p0 += WORD_PASS) {
        // ---- stage entries [p0, p0 + WORD_PASS) of the tile's 128 rows ----
#pragma unroll 4
        for (int s = tid; s < 128 * WORD_PASS; s += 256) {
            const int a = s / WORD_PASS, i = s % WORD_PASS;
            int c = 0; float e = 0.f;
            if (p0 + i < rl[a]) {
                const int64_t g = rs[a] + p0 + i;
                c = p.A.indices[g]; e = p.A.weights[g];
                if ((unsigned)c >= (unsigned)p.A.V) { c = 0; e = 0.f; }
            }
            sc[i * WORD_LDW + a] = c; se[i * WORD_LDW + a] = e;
        }
        __syncthreads();
        const int n = min(max(mine - p0, 0), WORD_PASS);
        for (int i0 = 0; i0 < WORD_PASS; i0 += 4) {
            if (__ballot(i0 < n) == 0) break;                   // wave-uniform: no lane of the wave has an entry left in this pass
            uint2 m[4]; uint32_t e[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int c = sc[(i0 + x) * WORD_LDW + j];
                e[x] = __float_as_uint(se[(i0 + x) * WORD_LDW + j]);
                m[x] = *reinterpret_cast<const uint2*>(cell + (int64_t)c * 16);
            }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
#pragma unroll
                for (int q = 0; q < 32; ++q) {
                    acc[q] = __fadd_rn(acc[q], __uint_as_float(e[x] & (uint32_t)((int32_t)(m[x].x << (31 - q)) >> 31)));
                    acc[q + 32] = __fadd_rn(acc[q + 32], __uint_as_float(e[x] & (uint32_t)((int32_t)(m[x].y << (31 - q)) >> 31)));
                }
            }
        }
        __syncthreads();                                        // the staging is rewritten by the next pass, or becomes the score tile
    }
}

template <bool EXCL, bool WIN>
__global__ __launch_bounds__(GEMM_THREADS, 2) void word_topk_kernel(WordSweep p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* tile = reinterpret_cast<float*>(lds);
    uint64_t* th = reinterpret_cast<uint64_t*>(lds + TOPK_TILE_BYTES);
    int* len = reinterpret_cast<int*>(th + 128);
    const int tid = threadIdx.x, wave = tid >> 6;
    uint64_t* Ls = reinterpret_cast<uint64_t*>(len + 128) + wave * 2 * TOPK_MAX;
    uint64_t* Cs = Ls + TOPK_MAX;
    int* wlo = reinterpret_cast<int*>(lds + TOPK_LDS);
    int* whi = wlo + 128;
    int64_t* rs = reinterpret_cast<int64_t*>(lds + TOPK_WIN_LDS);
    int* rl = reinterpret_cast<int*>(rs + 128);
    int* mx = rl + 128;
    const int split = blockIdx.x % p.splits, qt = blockIdx.x / p.splits;
    int ct0 = (int)((int64_t)p.ctiles * split / p.splits), ct1 = (int)((int64_t)p.ctiles * (split + 1) / p.splits);
    if (tid < 128) { th[tid] = 0; len[tid] = 0; }
    if constexpr (WIN) window_prologue(p.f.win_lo, p.f.win_hi, p.Nq, p.Nc, qt, split, p.splits, wlo, whi, whi + 128, ct0, ct1);
    const int j = tid & 127, h = tid >> 7, lane = tid & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int ct = ct0; ct < ct1; ++ct) {
        float acc[64];
        word_score_tile(p, qt, ct, lds, rs, rl, mx, acc);
#pragma unroll
        for (int q = 0; q < 64; ++q) tile[(h * 64 + q) * BN + j] = acc[q];
        __syncthreads();
        topk_tile_epilogue<EXCL, WIN, false, false>(p, tile, th, len, Ls, Cs, wlo, whi, qt, ct, split, 0, 0, p.k, lane, wave, below);
        // word_score_tile starts with a barrier: the tile is not rewritten before every wave is through its rows
    }
    __syncthreads();
    if (tid < 128 && qt * BM + tid < p.Nq) p.part_n[(int64_t)split * p.Nqp + qt * BM + tid] = len[tid];
}

// one wave per user, four users per workgroup
__global__ __launch_bounds__(256) void word_target_kernel(WordCsr A, const uint32_t* __restrict__ bits, int M, const int32_t* __restrict__ targets,
                                                          uint64_t* __restrict__ tkey, int32_t* __restrict__ rank,
                                                          float* __restrict__ target_score) {
    const int64_t u64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u64 >= M || (threadIdx.x & 63) != 0) return;
    const int u = (int)u64, t = targets[u];
    if (t < 0 || t >= A.Na) {                                   // no target (an index past the corpus is a caller error: not read)
        tkey[u] = ~0ull;                                        // above every key: nothing is counted
        rank[u] = 0;
        target_score[u] = -__builtin_inff();
        return;
    }
    const float s = word_pair_score(A, bits, u, t);
    tkey[u] = pair_key(s, t);
    rank[u] = 1;
    target_score[u] = s;
}

template <bool WIN>
__global__ __launch_bounds__(GEMM_THREADS, 2) void word_rank_kernel(WordSweep p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint64_t* tk = reinterpret_cast<uint64_t*>(lds + WORD_STAGE_BYTES);
    int* cnt = reinterpret_cast<int*>(tk + 128);
    int* wlo = cnt + 128;
    int* whi = wlo + 128;
    int64_t* rs = reinterpret_cast<int64_t*>(whi + 128 + 4);
    int* rl = reinterpret_cast<int*>(rs + 128);
    int* mx = rl + 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int split = blockIdx.x % p.splits, qt = blockIdx.x / p.splits;
    int ct0 = (int)((int64_t)p.ctiles * split / p.splits), ct1 = (int)((int64_t)p.ctiles * (split + 1) / p.splits);
    if (tid < 128) {
        const int gi = qt * BM + tid;
        tk[tid] = gi < p.Nq ? p.tkey[gi] : ~0ull;
        cnt[tid] = 0;
    }
    if constexpr (WIN) window_prologue(p.f.win_lo, p.f.win_hi, p.Nq, p.Nc, qt, split, p.splits, wlo, whi, whi + 128, ct0, ct1);
    const int j = tid & 127, h = tid >> 7;
    int n = 0;                                                  // lane q: keys above the target of user h * 64 + q among this wave's articles
    for (int ct = ct0; ct < ct1; ++ct) {
        float acc[64];
        word_score_tile(p, qt, ct, lds, rs, rl, mx, acc);       // its first barrier also orders tk / cnt / the windows
        const int gj = ct * BN + j;
        const bool ok = gj < p.Nc;
        int ln = lane;
        asm volatile("" : "+v"(ln));                           // per tile: keeps the 64 lane == q masks out of the SGPRs that live across the sweep
#pragma unroll
        for (int q = 0; q < 64; ++q) {
            const int row = h * 64 + q;
            bool in = ok && pair_key(acc[q], gj) > tk[row];
            if constexpr (WIN) in = in && gj >= wlo[row] && gj < whi[row];
            const int c = __popcll(__ballot(in));
            n += ln == q ? c : 0;
            if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four users' ballots in flight, not all 64 (SGPRs)
        }
    }
    __syncthreads();
    if (n) atomicAdd(&cnt[h * 64 + lane], n);
    __syncthreads();
    if (tid < 128 && qt * BM + tid < p.Nq && cnt[tid] != 0) atomicAdd(&p.rank[qt * BM + tid], cnt[tid]);
}

// one wave per user, four users per workgroup; lane l takes the seen items l, l + 64, ...
__global__ __launch_bounds__(256) void word_fixup_kernel(WordCsr A, const uint32_t* __restrict__ bits, int M, const int64_t* __restrict__ xp,
                                                         const int32_t* __restrict__ xi, const int32_t* __restrict__ win_lo,
                                                         const int32_t* __restrict__ win_hi, const uint64_t* __restrict__ tkey,
                                                         int32_t* __restrict__ rank) {
    const int lane = threadIdx.x & 63;
    const int64_t u64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u64 >= M) return;
    const int u = (int)u64;
    const uint64_t t = tkey[u];
    if (t == ~0ull) return;                                     // no target: nothing was counted
    int lo = 0, hi = A.Na;
    if (win_lo) { lo = min(max(win_lo[u], 0), A.Na); hi = min(max(win_hi[u], 0), A.Na); }
    const int64_t x0 = xp[u];
    const int64_t nx = xp[u + 1] - x0;
    int sub = 0;
    for (int64_t i = lane; i < nx; i += 64) {
        const int a = xi[x0 + i];
        if (a < lo || a >= hi) continue;                        // outside the window (or the corpus): the sweep did not count it
        if (i > 0 && xi[x0 + i - 1] == a) continue;             // a repeated item is taken off once
        sub += pair_key(word_pair_score(A, bits, u, a), a) > t ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sub += __shfl_xor(sub, o, 64);
    if (lane == 0 && sub) rank[u] -= sub;
}

static uint64_t word_bitmap_bytes(int64_t M, int64_t V) { return (uint64_t)(pad128(M) / 128) * (uint64_t)V * 16; }
static int word_topk_splits(int M, int Na) { return sweep_splits(M, Na, TOPK_SLOTS, TOPK_MAX_SPLITS); }
static int word_rank_splits(int M, int Na) { return sweep_splits(M, Na, WORD_RANK_SLOTS, WORD_RANK_SLOTS); }

// the checks the three entries share
static int word_check(const char* who, const void* bitmaps, int32_t M, int32_t V, const int64_t* art_indptr, const int32_t* art_indices,
                      const float* weights, int64_t nnz, int32_t Na) {
    DAE_CHECK_ARG(M >= 1 && V >= 1 && Na >= 1, "%s: M (%d), V (%d) and Na (%d) must be at least 1", who, M, V, Na);
    DAE_CHECK_ARG(nnz >= 0, "%s: nnz (%lld) must not be negative", who, (long long)nnz);
    DAE_CHECK_ARG(bitmaps && art_indptr && (nnz == 0 || (art_indices && weights)), "%s: bitmaps / art_indptr / art_indices / weights is NULL", who);
    DAE_CHECK_ARG(((uintptr_t)bitmaps % 16) == 0, "%s: bitmaps must be 16-byte aligned", who);
    return 0;
}

static void word_sweep_params(WordSweep& p, const void* bitmaps, int32_t M, int32_t V, const int64_t* art_indptr, const int32_t* art_indices,
                              const float* weights, int64_t nnz, int32_t Na, const RowFilter& f) {
    memset(&p, 0, sizeof(p));
    p.A.indptr = art_indptr; p.A.indices = art_indices; p.A.weights = weights; p.A.nnz = nnz; p.A.Na = Na; p.A.V = V;
    p.bits = (const uint32_t*)bitmaps;
    p.Nq = M; p.Nc = Na; p.Nqp = (int)pad128(M); p.ctiles = (int)(pad128(Na) / BN);
    p.f = f;
}

}  // namespace dae

using namespace dae;

extern "C" uint64_t dae_word_profiles_bytes(int32_t M, int32_t V) {
    if (M <= 0 || V <= 0) return 0;
    return word_bitmap_bytes(M, V);
}

extern "C" int dae_word_profiles(const int64_t* hist_indptr, const int32_t* hist_items, int64_t hist_nnz, int32_t M, int32_t max_events,
                                 const int64_t* art_indptr, const int32_t* art_indices, int64_t nnz, int32_t Na, int32_t V, void* bitmaps,
                                 uint64_t bitmap_bytes, int32_t* sizes, void* stream) {
    DAE_CHECK_ARG(M >= 1 && V >= 1 && Na >= 1, "word_profiles: M (%d), V (%d) and Na (%d) must be at least 1", M, V, Na);
    DAE_CHECK_ARG(hist_nnz >= 0 && nnz >= 0, "word_profiles: hist_nnz (%lld) and nnz (%lld) must not be negative", (long long)hist_nnz,
                  (long long)nnz);
    DAE_CHECK_ARG(max_events >= 0, "word_profiles: max_events (%d) must not be negative (0: every click)", max_events);
    DAE_CHECK_ARG(hist_indptr && (hist_nnz == 0 || hist_items), "word_profiles: hist_indptr / hist_items is NULL");
    DAE_CHECK_ARG(art_indptr && (nnz == 0 || art_indices), "word_profiles: art_indptr / art_indices is NULL");
    DAE_CHECK_ARG(bitmaps && sizes, "word_profiles: bitmaps / sizes is NULL");
    DAE_CHECK_ARG(((uintptr_t)bitmaps % 16) == 0, "word_profiles: bitmaps must be 16-byte aligned");
    DAE_CHECK_ARG(bitmap_bytes >= word_bitmap_bytes(M, V), "word_profiles: bitmaps too small (%llu < %llu bytes)",
                  (unsigned long long)bitmap_bytes, (unsigned long long)word_bitmap_bytes(M, V));
    hipStream_t st = (hipStream_t)stream;
    DAE_CHECK_HIP(hipMemsetAsync(bitmaps, 0, word_bitmap_bytes(M, V), st));
    WordCsr A = {art_indptr, art_indices, nullptr, nnz, Na, V};
    DAE_LAUNCH(word_profile_kernel, dim3((unsigned)(((int64_t)M + 3) / 4)), dim3(256), 0, st, hist_indptr, hist_items, hist_nnz, (int)M,
               (int)max_events, A, (uint32_t*)bitmaps);
    DAE_CHECK_LAUNCH();
    DAE_LAUNCH(word_sizes_kernel, dim3((unsigned)(pad128(M) / 128)), dim3(256), 0, st, (const uint32_t*)bitmaps, (int)M, (int)V, sizes);
    DAE_CHECK_LAUNCH();
    return 0;
}

extern "C" uint64_t dae_word_entry_weights_bytes(int64_t nnz) { return nnz <= 0 ? 0 : al256((uint64_t)nnz * 4); }

extern "C" int dae_word_entry_weights(const int32_t* art_indices, const float* art_values, int64_t nnz, int32_t V, const float* term_weights,
                                      float* weights, void* stream) {
    DAE_CHECK_ARG(nnz >= 0 && V >= 1, "word_entry_weights: nnz (%lld) must not be negative and V (%d) at least 1", (long long)nnz, V);
    if (nnz == 0) return 0;
    DAE_CHECK_ARG(art_indices && weights, "word_entry_weights: art_indices / weights is NULL");
    DAE_CHECK_ARG((nnz + 255) / 256 < (1ll << 31), "word_entry_weights: %lld entries exceed the grid", (long long)nnz);
    DAE_LAUNCH(word_weights_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, (hipStream_t)stream, art_indices, art_values, nnz, (int)V,
               term_weights, weights);
    DAE_CHECK_LAUNCH();
    return 0;
}

extern "C" uint64_t dae_word_topk_workspace(int32_t M, int32_t Na, int32_t k) {
    if (M <= 0 || Na <= 0 || k <= 0) return 0;
    const uint64_t Mp = pad128(M), s = word_topk_splits(M, Na);
    return al256(s * Mp * (uint64_t)k * 8) + al256(s * Mp * 4);
}

extern "C" int dae_word_topk(const void* bitmaps, int32_t M, int32_t V, const int64_t* art_indptr, const int32_t* art_indices,
                             const float* weights, int64_t nnz, int32_t Na, int32_t k, const int64_t* excl_indptr, const int32_t* excl_items,
                             const int32_t* win_lo, const int32_t* win_hi, int32_t* idx, float* score, int64_t ldk, void* workspace,
                             uint64_t workspace_bytes, void* stream) {
    RowFilter f = {0, excl_indptr, excl_items, win_lo, win_hi, nullptr, nullptr, nullptr, 0};
    if (int rc = sweep_filter_check("word_topk", f, false)) return rc;
    if (int rc = word_check("word_topk", bitmaps, M, V, art_indptr, art_indices, weights, nnz, Na)) return rc;
    DAE_CHECK_ARG(idx && score && workspace, "word_topk: idx / score / workspace is NULL");
    DAE_CHECK_ARG(k >= 1 && k <= TOPK_MAX, "word_topk: k must be in 1..%d (got %d)", TOPK_MAX, k);
    DAE_CHECK_ARG(ldk >= k, "word_topk: ldk (%lld) must be >= k (%d)", (long long)ldk, k);
    const uint64_t need = dae_word_topk_workspace(M, Na, k);
    DAE_CHECK_ARG(workspace_bytes >= need, "word_topk: workspace too small (%llu < %llu bytes)", (unsigned long long)workspace_bytes,
                  (unsigned long long)need);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "word_topk: workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    WordSweep p;
    word_sweep_params(p, bitmaps, M, V, art_indptr, art_indices, weights, nnz, Na, f);
    const int splits = word_topk_splits(M, Na);
    p.k = k; p.splits = splits;
    p.part = (uint64_t*)workspace; p.part_n = (int*)((char*)workspace + al256((uint64_t)splits * p.Nqp * k * 8));
    const int64_t grid = (int64_t)p.Nqp / BM * splits;
    if (int rc = f.win_lo ? (f.excl_indptr ? sweep_launch<word_topk_kernel<true, true>>(grid, WORD_TOPK_LDS, WORD_TOPK_LDS, st, p)
                                           : sweep_launch<word_topk_kernel<false, true>>(grid, WORD_TOPK_LDS, WORD_TOPK_LDS, st, p))
                          : (f.excl_indptr ? sweep_launch<word_topk_kernel<true, false>>(grid, WORD_TOPK_LDS, WORD_TOPK_LDS, st, p)
                                           : sweep_launch<word_topk_kernel<false, false>>(grid, WORD_TOPK_LDS, WORD_TOPK_LDS, st, p)))
        return rc;
    return topk_merge_launch(p.part, p.part_n, M, p.Nqp, splits, k, idx, score, ldk, st);
}

extern "C" uint64_t dae_word_rank_workspace(int32_t M) { return M <= 0 ? 0 : al256((uint64_t)pad128(M) * 8); }

extern "C" int dae_word_rank(const void* bitmaps, int32_t M, int32_t V, const int64_t* art_indptr, const int32_t* art_indices,
                             const float* weights, int64_t nnz, int32_t Na, const int64_t* excl_indptr, const int32_t* excl_items,
                             const int32_t* win_lo, const int32_t* win_hi, const int32_t* targets, int32_t* rank, float* target_score,
                             void* workspace, uint64_t workspace_bytes, void* stream) {
    RowFilter f = {0, excl_indptr, excl_items, win_lo, win_hi, nullptr, nullptr, nullptr, 0};
    if (int rc = sweep_filter_check("word_rank", f, false)) return rc;
    if (int rc = word_check("word_rank", bitmaps, M, V, art_indptr, art_indices, weights, nnz, Na)) return rc;
    DAE_CHECK_ARG(targets && rank && target_score && workspace, "word_rank: targets / rank / target_score / workspace is NULL");
    const uint64_t need = dae_word_rank_workspace(M);
    DAE_CHECK_ARG(workspace_bytes >= need, "word_rank: workspace too small (%llu < %llu bytes)", (unsigned long long)workspace_bytes,
                  (unsigned long long)need);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "word_rank: workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    WordSweep p;
    word_sweep_params(p, bitmaps, M, V, art_indptr, art_indices, weights, nnz, Na, f);
    uint64_t* tkey = (uint64_t*)workspace;
    p.splits = word_rank_splits(M, Na);
    p.tkey = tkey; p.rank = rank;
    const unsigned waves = (unsigned)(((int64_t)M + 3) / 4);
    DAE_LAUNCH(word_target_kernel, dim3(waves), dim3(256), 0, st, p.A, p.bits, (int)M, targets, tkey, rank, target_score);
    DAE_CHECK_LAUNCH();
    const int64_t grid = (int64_t)p.Nqp / BM * p.splits;
    if (int rc = f.win_lo ? sweep_launch<word_rank_kernel<true>>(grid, WORD_RANK_LDS, WORD_RANK_LDS, st, p)
                          : sweep_launch<word_rank_kernel<false>>(grid, WORD_RANK_LDS, WORD_RANK_LDS, st, p))
        return rc;
    if (f.excl_indptr) {
        DAE_LAUNCH(word_fixup_kernel, dim3(waves), dim3(256), 0, st, p.A, p.bits, (int)M, excl_indptr, excl_items, win_lo, win_hi,
                   (const uint64_t*)tkey, rank);
        DAE_CHECK_LAUNCH();
    }
    return 0;
}
