// dae_gemm_tile.h -- the LDS image of an operand tile, the accumulator layout of the 32 x 32 MFMA and the 128 x 128 K loop
// (gemm_mainloop), shared by the GEMM kernels of dae_gemm.hip / dae_gemm_w8.h and the score sweeps of dae_score_sweep.h.
// The two formats are DEFINED here, once ("the tile image", "the accumulator layout" below); why the tiles have these shapes:
// the head of dae_gemm.hip.
#pragma once
#include "dae_kernels.h"

namespace dae {

constexpr int BM = 128, BN = 128;
constexpr int BKB = 128;                 // K-tile width in bytes
constexpr int GEMM_THREADS = 256;
constexpr int TILE_BYTES = BM * BKB;     // 16 KiB per operand per stage
constexpr int STAGE_BYTES = 2 * TILE_BYTES;
// NST = number of LDS stages of the global_load_lds ring (0 = legacy register staging, 2 buffers)
constexpr int lds_bytes_for(int nst) { return (nst < 2 ? 2 : nst) * STAGE_BYTES; }
constexpr int wg_per_cu_for(int nst) { return nst <= 2 ? 2 : 1; }

struct GemmSeg {
    const char* A;
    const char* Bt;
    int64_t lda_b, ldb_b;   // leading dimensions in BYTES
    int ktiles;             // K_seg * sizeof(T) / 128
};

constexpr int GEMM_MAX_SEG = 6;    // K segments of one contraction: split-bf16 operands need (hi,hi) (hi,lo) (lo,hi) per product (dW with a valued x~^T: 2 x 3)
struct GemmParams {
    GemmSeg seg[GEMM_MAX_SEG];
    const char* bt2[GEMM_MAX_SEG];   // gemm_dw_pc<PAIR> only: a second Bt operand of the segment (same leading dimension) that shares its A tiles, or NULL
    int nseg;                  // non-empty segments, walked in order
    int epi_vec;               // gemm_nt_pc: 1 = LDS-staged epilogue (16-byte pieces, all 8 waves), 0 = dword stores from the accumulator layout (A/B)
    int ktiles_total;
    int tiles_m, tiles_n, splits;
    unsigned long long* trace;   // dae_gemm_trace only: [blocks][4 waves][8] shader-clock sums per K-loop phase
    float out_scale;           // fp32-output kernels: C = out_scale * accumulator (1 except for the dW gradient of scaled 16-bit delta images)
};

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    static __device__ __forceinline__ void run(const i32x4& a, const i32x4& b, f32x16& c) {
        // the 16-bit storage format of this build (dae_common.h): fp16 images multiply on v_mfma_f32_32x32x16_f16, bf16 images on ..._bf16 (same rate)
        if constexpr (kF16) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
        else c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static __device__ __forceinline__ void run(const i32x4& a, const i32x4& b, f32x16& c) {
        f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0], bf[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1], bf[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[2], bf[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[3], bf[3], c, 0, 0, 0);
    }
};

// ---- the tile image ----
// An operand tile in LDS is [rows][128 bytes] = eight 16-byte slots per row, and logical slot s of row `row` lives in physical slot
// s ^ tile_swz(row): the 16 lanes of a ds_read_b128 lane group (rows distinct mod 16) then hit 16 distinct slots of the 256-byte bank row
// (conflict-free).  LDS-DMA writes the image lane-linear in 1-KiB pieces of 8 rows (lane l lands at byte 16 l of its piece), so the
// swizzle sits on the per-lane SOURCE address (dma_src); the MFMA fragments come back with ds_read_b128 at frag_row + frag_slot, 32-row
// blocks FRAG_BLOCK bytes apart.  tile_image_ok() below proves at compile time that the two sides agree.
constexpr int PIECE_BYTES = 1024, PIECE_ROWS = PIECE_BYTES / BKB;
constexpr int FRAG_BLOCK = 32 * BKB;     // bytes between the 32-row MFMA blocks of a tile: the immediate offsets of the fragment reads
__host__ __device__ constexpr int tile_swz(int row) { return (row >> 1) & 7; }

// DMA side.  Piece i of wave `wave` (of WAVES that fill the tile) is piece i * WAVES + wave of the tile; lane `lane` of it fills one
// cell of row piece_row.  dma_src: the byte offset of the 16 bytes this lane must fetch, relative to the K tile's first byte of panel
// row 0 -- panel row row0 + piece_row (clamped to row_last: tiles that overhang the panel re-read its last row), leading dimension ld bytes.
__host__ __device__ constexpr int piece_row(int piece, int lane) { return piece * PIECE_ROWS + (lane >> 3); }
__host__ __device__ constexpr int piece_slot(int piece, int lane) { return (lane & 7) ^ tile_swz(piece_row(piece, lane)); }
template <int WAVES>
__host__ __device__ constexpr uint32_t dma_src(int i, int wave, int lane, int row0, uint32_t ld, int row_last = INT32_MAX) {
    const int row = row0 + piece_row(i * WAVES + wave, lane);
    return (uint32_t)(row < row_last ? row : row_last) * ld + (uint32_t)(piece_slot(i * WAVES + wave, lane) << 4);
}
__device__ __forceinline__ uint32_t lds_addr(const char* l) { return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)l; }
// 16 bytes per lane, global -> LDS (global_load_lds_dwordx4): the wave's 1 KiB lands lane-linear at l
__device__ __forceinline__ void glds16(const char* g, char* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
template <int WAVES> __device__ __forceinline__ void glds_piece(int i, int wave, const char* src, char* tile) {
    glds16(src, tile + (i * WAVES + wave) * PIECE_BYTES);
}
// the offsets of all N pieces of a wave
template <int WAVES, int N>
__device__ __forceinline__ void dma_srcs(uint32_t (&vo)[N], int wave, int lane, int row0, uint32_t ld, int row_last = INT32_MAX) {
#pragma unroll
    for (int i = 0; i < N; ++i) vo[i] = dma_src<WAVES>(i, wave, lane, row0, ld, row_last);
}

// Fragment side.  Lane (g = lane >> 5, r = lane & 31) reads row r of a 32-row block (first row row0, a multiple of 32) and, for the
// 16-byte k chunk kk of 4, the logical slot kk * 2 + g.
__host__ __device__ constexpr uint32_t frag_row(int row0, int lane) { return (uint32_t)((row0 + (lane & 31)) * BKB); }
__host__ __device__ constexpr uint32_t frag_slot(int kk, int lane) { return (uint32_t)(((kk * 2 + (lane >> 5)) ^ tile_swz(lane & 31)) << 4); }
__device__ __forceinline__ void frag_slots(int lane, uint32_t (&so)[4]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) so[kk] = frag_slot(kk, lane);
}

// the DMA mapping is a bijection of (piece, lane) onto the (row, logical slot) cells of a ROWS-row tile, every cell inside its 128-byte
// row, and the fragment side addresses exactly the cell where the DMA put logical slot kk * 2 + g of its row.  (The proof covers dma_src,
// frag_row and frag_slot and takes the hardware's destination -- piece * PIECE_BYTES + 16 * lane, what glds_piece passes -- as given; the
// writers that build the image with ds_write, stage_write and gemm_encode_bits_pc's build_a, and the offset code a kernel keeps written
// out are outside it.)
template <int ROWS, int WAVES> constexpr bool tile_image_ok() {
    int at[ROWS * 8] = {};                   // 1 + the 16-byte LDS cell that holds logical slot s of row r, at r * 8 + s
    for (int piece = 0; piece < ROWS / PIECE_ROWS; ++piece)
        for (int lane = 0; lane < 64; ++lane) {
            const int row = piece_row(piece, lane), cell = (piece * PIECE_BYTES >> 4) + lane;
            const int slot = (int)(dma_src<WAVES>(piece / WAVES, piece % WAVES, lane, 0, 0u) >> 4);
            if (row >= ROWS || slot > 7 || (cell >> 3) != row || at[row * 8 + slot]) return false;
            at[row * 8 + slot] = 1 + cell;
        }
    for (int row = 0; row < ROWS; ++row)
        for (int kk = 0; kk < 4; ++kk)
            for (int g = 0; g < 2; ++g) {
                const int lane = g * 32 + (row & 31);
                if (frag_row(row & ~31, lane) + frag_slot(kk, lane) != (uint32_t)(at[row * 8 + kk * 2 + g] - 1) << 4) return false;
            }
    return true;
}
static_assert(tile_image_ok<64, 4>() && tile_image_ok<128, 4>() && tile_image_ok<160, 4>() && tile_image_ok<256, 8>(),
              "the LDS-DMA side and the fragment side of the tile image disagree");

// ---- the accumulator layout of v_mfma_f32_32x32x* ----
// A 32 x 32 block lives in 16 registers per lane: lane (g = lane >> 5, c = lane & 31) holds in register r the value of row
// (r & 3) + 8 * (r >> 2) + 4 * g, column c.  For a wave tile of mt x nt blocks, acc[mt][nt][r] sits at (acc_row(mt, r, g), acc_col(nt, c))
// of the wave tile: a lane's values are its first one's place, (4 * g, c), plus the compile-time offsets acc_row(mt, r, 0), acc_col(nt, 0).
__host__ __device__ constexpr int acc_row(int mt, int r, int g) { return mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * g; }
__host__ __device__ constexpr int acc_col(int nt, int c) { return nt * 32 + c; }
template <int M, int N> __device__ __forceinline__ void zero_acc(f32x16 (&acc)[M][N]) {
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// segment of K tile kt: its index, the tile's position inside it and the first K tile AFTER it (where the stream switches operands)
template <typename P>
__device__ __forceinline__ int seg_locate(const P& p, int kt, int& k_in_seg, int& seg_end) {
    int sg = 0, base = 0;
    while (sg + 1 < p.nseg && kt >= base + p.seg[sg].ktiles) { base += p.seg[sg].ktiles; ++sg; }
    k_in_seg = kt - base;
    seg_end = base + p.seg[sg].ktiles;
    return sg;
}
__device__ __forceinline__ void seg_of(const GemmParams& p, int kt, const char*& A, const char*& Bt,
                                       int64_t& lda, int64_t& ldb, int64_t& kbyte) {
    int k, end;
    const int s = seg_locate(p, kt, k, end);
    A = p.seg[s].A; Bt = p.seg[s].Bt; lda = p.seg[s].lda_b; ldb = p.seg[s].ldb_b;
    kbyte = (int64_t)k * BKB;
}

// ---- staging: register path ----
struct StageRegs { i32x4 a[4], b[4]; };

__device__ __forceinline__ void stage_load(const GemmParams& p, int kt, int row0_m, int row0_n, int tid, StageRegs& r) {
    const char *A, *Bt; int64_t lda, ldb, kb;
    seg_of(p, kt, A, Bt, lda, ldb, kb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = tid + GEMM_THREADS * i;
        int row = c >> 3, slot = c & 7;
        r.a[i] = *reinterpret_cast<const i32x4*>(A + (int64_t)(row0_m + row) * lda + kb + slot * 16);
        r.b[i] = *reinterpret_cast<const i32x4*>(Bt + (int64_t)(row0_n + row) * ldb + kb + slot * 16);
    }
}
__device__ __forceinline__ void stage_write(char* stage, int tid, const StageRegs& r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = tid + GEMM_THREADS * i;
        int row = c >> 3, slot = c & 7;
        int off = row * BKB + ((slot ^ tile_swz(row)) << 4);
        *reinterpret_cast<i32x4*>(stage + off) = r.a[i];
        *reinterpret_cast<i32x4*>(stage + TILE_BYTES + off) = r.b[i];
    }
}

// ---- counted waits ----
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }
// vmcnt(PIECES * n): n younger stages of PIECES LDS-DMA pieces per wave each may stay in flight; n is at most NMAX (a ring of NMAX + 1 stages).
// A compare chain over template constants, so that exactly the waits of the NMAX + 1 reachable counts are emitted.
template <int PIECES, int NMAX> __device__ __forceinline__ void wait_vm_stages(int n) {
    static_assert(PIECES * NMAX < 64, "vmcnt is a 6-bit counter");
    if constexpr (NMAX == 0) wait_vm<0>();
    else if (n >= NMAX) wait_vm<PIECES * NMAX>();
    else wait_vm_stages<PIECES, NMAX - 1>(n);
}

// ---- fragment reads and MFMA groups ----
// All fragment reads of a K tile (ds_read_b128) are issued back to back and the MFMA groups wait with COUNTED lgkmcnt: the first MFMAs
// start as soon as their fragments land and the LDS latency of the rest hides behind them.  rocprofv3 showed ~50 % of wave time parked
// in lgkmcnt(0) with the compiler's own read->wait(0)->MFMA x4 schedule, and hipcc turns any source-level hoisting back into a full
// wait, so the reads are inline asm (invisible to its scoreboard) with hand-placed waits.  Every wait is followed by sched_barrier(0),
// and so is every MFMA block that an asm read or wait follows: register-only MFMAs may otherwise be moved across an asm statement
// (guide 5.4 rule 18) -- which is why each sched_barrier(0) of the K loops stays exactly where it is (tools/check_gemm_asm.py replays
// the result).
template <int OFF = 0> __device__ __forceinline__ i32x4 lds_read_b128(uint32_t addr) {   // OFF: 0..3 blocks of FRAG_BLOCK bytes, as an immediate
    static_assert(OFF % FRAG_BLOCK == 0 && OFF >= 0 && OFF <= 3 * FRAG_BLOCK && FRAG_BLOCK == 4096, "the offsets are spelled out below");
    i32x4 v;
    if constexpr (OFF == 0) asm volatile("ds_read_b128 %0, %1" : "=&v"(v) : "v"(addr));
    else if constexpr (OFF == 4096) asm volatile("ds_read_b128 %0, %1 offset:4096" : "=&v"(v) : "v"(addr));
    else if constexpr (OFF == 8192) asm volatile("ds_read_b128 %0, %1 offset:8192" : "=&v"(v) : "v"(addr));
    else asm volatile("ds_read_b128 %0, %1 offset:12288" : "=&v"(v) : "v"(addr));
    return v;
}
// the fragments of one k chunk for NB consecutive 32-row blocks of a tile; addr = slot base + frag_row + frag_slot
template <int NB> __device__ __forceinline__ void read_frags(i32x4 (&f)[NB], uint32_t addr) {
    static_assert(NB >= 1 && NB <= 4, "immediate offsets up to 3 blocks");
    f[0] = lds_read_b128(addr);
    if constexpr (NB > 1) f[1] = lds_read_b128<FRAG_BLOCK>(addr);
    if constexpr (NB > 2) f[2] = lds_read_b128<2 * FRAG_BLOCK>(addr);
    if constexpr (NB > 3) f[3] = lds_read_b128<3 * FRAG_BLOCK>(addr);
}
// acc[nt] += a . b[nt]; acc[mt][nt] += a[mt] . b[nt] (row blocks outer)
template <typename T, int NT> __device__ __forceinline__ void mma_row(const i32x4& a, const i32x4 (&b)[NT], f32x16 (&acc)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) Mma<T>::run(a, b[nt], acc[nt]);
}
template <typename T, int MT, int NT> __device__ __forceinline__ void mma_block(const i32x4 (&a)[MT], const i32x4 (&b)[NT], f32x16 (&acc)[MT][NT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) mma_row<T>(a[mt], b, acc[mt]);
}
// ... once all but the youngest CNT fragment reads have landed
template <typename T, int CNT, int MT, int NT> __device__ __forceinline__ void mma_group(const i32x4 (&a)[MT], const i32x4 (&b)[NT], f32x16 (&acc)[MT][NT]) {
    wait_lgkm<CNT>();
    __builtin_amdgcn_sched_barrier(0);
    mma_block<T>(a, b, acc);
}

// One K tile of MFMA work for a wave of the register-staged path: 16 fragment reads (64 VGPRs), four groups at lgkmcnt 12/8/4/0.
template <typename T>
__device__ __forceinline__ void compute_stage(const char* stage, int wm, int wn, int lane, f32x16 (&acc)[2][2]) {
    const uint32_t pa = lds_addr(stage) + frag_row(wm * 64, lane), pb = lds_addr(stage) + TILE_BYTES + frag_row(wn * 64, lane);
    i32x4 a[4][2], b[4][2];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        read_frags(a[kk], pa + frag_slot(kk, lane));
        read_frags(b[kk], pb + frag_slot(kk, lane));
    }
    mma_group<T, 12>(a[0], b[0], acc);
    mma_group<T, 8>(a[1], b[1], acc);
    mma_group<T, 4>(a[2], b[2], acc);
    mma_group<T, 0>(a[3], b[3], acc);
    __builtin_amdgcn_sched_barrier(0);
}

// K loop.  NST >= 2: ring of NST LDS stages filled by global_load_lds with COUNTED vmcnt waits -- tile i+NST-1 is
// requested right after the barrier of iteration i (its buffer was last read in iteration i-1), and the wait in
// front of the barrier only retires tile i, leaving up to NST-2 younger tiles (8 LDS-DMA ops per wave each) in
// flight across the barrier.  One raw s_barrier per K tile; __syncthreads() would drain the DMA queue (its
// fence waits vmcnt(0) while LDS-DMA writes are pending).
template <typename T, int NST, bool TRACE = false>
__device__ __forceinline__ void gemm_mainloop(const GemmParams& p, int tm, int tn, int kt0, int kt1, char* lds,
                                              f32x16 (&acc)[2][2]) {
    // TRACE (dae_gemm_trace): s_memtime stamps between the phases of every K iteration, summed per wave:
    //   [0] phase (a): 8 MFMAs (+DMA)  [1] waits (vmcnt, lgkmcnt)  [2] barrier  [3] phases (c,d,e): reads, 8 MFMAs + DMA, reads
    //   [4] iterations
    unsigned long long tsum[5] = {0, 0, 0, 0, 0}, tprev = 0;
#define DAE_STAMP(K)                                                         \
    if constexpr (TRACE) {                                                   \
        const unsigned long long t__ = __builtin_amdgcn_s_memtime();         \
        tsum[K] += t__ - tprev;                                              \
        tprev = t__;                                                         \
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int row0_m = tm * BM, row0_n = tn * BN;
    zero_acc(acc);
    const int nk = kt1 - kt0;
    if (nk <= 0) return;

    if constexpr (NST >= 2) {
        // ---- LDS-DMA addressing: this lane's 16-byte chunk of each of its 4 pieces per operand, as a 32-bit byte offset
        //      from a uniform (SGPR) panel pointer that advances by one K tile per stage ----
        // (This loop keeps dma_src, frag_row / frag_slot and its read / MFMA macros written out: through the helpers the offsets regroup
        //  -- up to 18 VGPRs fewer, so another reported occupancy in 16 kernels -- and the compiler's own waits move in the score sweeps:
        //  profiles/gemm_tile_refactor.md.  Not covered by tile_image_ok: keep equal to the helpers by hand.)
        uint32_t voA[4], voB[4];
        const char *gA = nullptr, *gB = nullptr;
        int kt_dma = kt0, seg_end = 0;
        auto seg_setup = [&](int kt) {
            int k;
            const int sg = seg_locate(p, kt, k, seg_end);
            const uint32_t lda = (uint32_t)p.seg[sg].lda_b, ldb = (uint32_t)p.seg[sg].ldb_b;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (i * 4 + wave) * 8 + (lane >> 3);
                const uint32_t ss = (uint32_t)(((lane & 7) ^ ((row >> 1) & 7)) << 4);
                voA[i] = (uint32_t)(row0_m + row) * lda + ss;
                voB[i] = (uint32_t)(row0_n + row) * ldb + ss;
            }
            gA = p.seg[sg].A + (int64_t)k * BKB;
            gB = p.seg[sg].Bt + (int64_t)k * BKB;
        };
        seg_setup(kt0);
        auto dma_piece = [&](int i, char* slot) {        // piece i of both operands of the stage at (gA, gB)
            glds_piece<4>(i, wave, gA + voA[i], slot);
            glds_piece<4>(i, wave, gB + voB[i], slot + TILE_BYTES);
        };
        auto dma_advance = [&]() {
            ++kt_dma;
            if (kt_dma == seg_end && kt_dma < p.ktiles_total) seg_setup(kt_dma);
            else { gA += BKB; gB += BKB; }
        };
        // Stage s lives in slot s % NST.  Rolling schedule of iteration i (fragment registers R0 = kk 0,1 and R1 = kk 2,3):
        //   (a) 8 MFMAs on R0(i)            [NST >= 3: + second half of the DMA of stage i+NST-1]
        //   (b) wait: stage i+1 landed, my LDS reads of tile i done; s_barrier
        //   (c) 8 ds_read_b128 of tile i+1 -> R0
        //   (d) 8 MFMAs on R1(i)            + DMA of stage i+NST into slot i % NST (first half when NST >= 3)
        //   (e) 8 ds_read_b128 of tile i+1 -> R1
        // so the fragment reads of the next tile and the LDS-DMA issue run under the MFMAs of this tile; the only exposed
        // latency per K tile is the barrier.  Reads past the last tile fetch stale LDS and are never consumed.
        constexpr bool SPLIT = NST >= 3;
        const int r = lane & 31, g = lane >> 5;
        const int swz = (r >> 1) & 7;
        const uint32_t lbase = lds_addr(lds);
        const uint32_t offa = (wm * 64 + r) * BKB, offb = TILE_BYTES + (wn * 64 + r) * BKB;
        uint32_t so[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) so[kk] = (uint32_t)(((kk * 2 + g) ^ swz) << 4);
        i32x4 fa[4][2], fb[4][2];
#define DAE_READ_KK(KK, SLOTBASE)                                          \
    fa[KK][0] = lds_read_b128((SLOTBASE) + offa + so[KK]);                 \
    fa[KK][1] = lds_read_b128<FRAG_BLOCK>((SLOTBASE) + offa + so[KK]);     \
    fb[KK][0] = lds_read_b128((SLOTBASE) + offb + so[KK]);                 \
    fb[KK][1] = lds_read_b128<FRAG_BLOCK>((SLOTBASE) + offb + so[KK]);
#define DAE_MMA2(KK, MT)                                                   \
    Mma<T>::run(fa[KK][MT], fb[KK][0], acc[MT][0]);                        \
    Mma<T>::run(fa[KK][MT], fb[KK][1], acc[MT][1]);                        \
    __builtin_amdgcn_sched_barrier(0);

        // ---- prologue: request stages 0..NST-2 (+ first half of NST-1 when SPLIT, else all of NST-1) ----
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            if (st < nk) {
                char* slot = lds + st * STAGE_BYTES;
                if (SPLIT && st == NST - 1) { dma_piece(0, slot); dma_piece(1, slot); }
                else { dma_piece(0, slot); dma_piece(1, slot); dma_piece(2, slot); dma_piece(3, slot); dma_advance(); }
            }
        }
        if (nk >= NST) { if constexpr (SPLIT) wait_vm<(NST - 2) * 8 + 4>(); else wait_vm<(NST - 1) * 8>(); }
        else wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        DAE_READ_KK(0, lbase) DAE_READ_KK(1, lbase) DAE_READ_KK(2, lbase) DAE_READ_KK(3, lbase)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (TRACE) tprev = __builtin_amdgcn_s_memtime();
        int cur = 0;                                      // slot of tile i
        for (int i = 0; i < nk; ++i) {
            const int nxt = cur + 1 == NST ? 0 : cur + 1;
            // (a)
            wait_lgkm<8>();
            __builtin_amdgcn_sched_barrier(0);
            DAE_MMA2(0, 0)
            if constexpr (SPLIT) { if (i + NST - 1 < nk) dma_piece(2, lds + (cur == 0 ? NST - 1 : cur - 1) * STAGE_BYTES); __builtin_amdgcn_sched_barrier(0); }
            DAE_MMA2(0, 1)
            DAE_MMA2(1, 0)
            if constexpr (SPLIT) { if (i + NST - 1 < nk) { dma_piece(3, lds + (cur == 0 ? NST - 1 : cur - 1) * STAGE_BYTES); dma_advance(); } __builtin_amdgcn_sched_barrier(0); }
            DAE_MMA2(1, 1)
            DAE_STAMP(0)
            // (b)
            {
                const int ahead = min(NST - 2, nk - 2 - i);
                if (ahead >= 2) wait_vm<16>();
                else if (ahead == 1) wait_vm<8>();
                else wait_vm<0>();
            }
            wait_lgkm<0>();
            DAE_STAMP(1)
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            DAE_STAMP(2)
            // (c)
            {
                const uint32_t nb = lbase + nxt * STAGE_BYTES;
                DAE_READ_KK(0, nb) DAE_READ_KK(1, nb)
                __builtin_amdgcn_sched_barrier(0);
                // (d): R1 landed at (b)
                char* slot = lds + cur * STAGE_BYTES;
                const bool more = i + NST < nk;
                DAE_MMA2(2, 0)
                if (more) dma_piece(0, slot);
                __builtin_amdgcn_sched_barrier(0);
                DAE_MMA2(2, 1)
                if (more) dma_piece(1, slot);
                __builtin_amdgcn_sched_barrier(0);
                DAE_MMA2(3, 0)
                if constexpr (!SPLIT) { if (more) dma_piece(2, slot); __builtin_amdgcn_sched_barrier(0); }
                DAE_MMA2(3, 1)
                if constexpr (!SPLIT) { if (more) { dma_piece(3, slot); dma_advance(); } __builtin_amdgcn_sched_barrier(0); }
                // (e)
                DAE_READ_KK(2, nb) DAE_READ_KK(3, nb)
                __builtin_amdgcn_sched_barrier(0);
            }
            DAE_STAMP(3)
            cur = nxt;
        }
        wait_lgkm<0>();                                       // drain the stale tail reads before the LDS is reused
#undef DAE_READ_KK
#undef DAE_MMA2
        if constexpr (TRACE) {
            if (lane == 0) {
                unsigned long long* o = p.trace + ((size_t)blockIdx.x * 4 + wave) * 8;
                o[0] = tsum[0]; o[1] = tsum[1]; o[2] = tsum[2]; o[3] = tsum[3]; o[4] = (unsigned long long)nk;
            }
        }
#undef DAE_STAMP
    } else {
        StageRegs regs;
        stage_load(p, kt0, row0_m, row0_n, tid, regs);
        stage_write(lds, tid, regs);
        __syncthreads();
        for (int kt = kt0; kt < kt1; ++kt) {
            char* cur = lds + ((kt - kt0) & 1) * STAGE_BYTES;
            char* nxt = lds + (((kt - kt0) & 1) ^ 1) * STAGE_BYTES;
            const bool more = (kt + 1 < kt1);
            if (more) stage_load(p, kt + 1, row0_m, row0_n, tid, regs);
            compute_stage<T>(cur, wm, wn, lane, acc);
            if (more) stage_write(nxt, tid, regs);
            __syncthreads();
        }
    }
}

}  // namespace dae
