// dae_gemm_tile.h -- the 128 x 128 MFMA tile and its K loop (gemm_mainloop), shared by the GEMM kernels of dae_gemm.hip and the
// fused similarity + top-k kernel of dae_topk.hip.  Tiling, LDS image and staging: see the head of dae_gemm.hip.
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
        int off = row * BKB + ((slot ^ ((row >> 1) & 7)) << 4);
        *reinterpret_cast<i32x4*>(stage + off) = r.a[i];
        *reinterpret_cast<i32x4*>(stage + TILE_BYTES + off) = r.b[i];
    }
}

// ---- staging: direct global -> LDS (global_load_lds_dwordx4) ----
// wave w, piece i covers LDS bytes [(i*4+w)*1024, +1024) of each operand tile = 8 rows; lane l lands at
// +l*16, i.e. (row = (i*4+w)*8 + (l>>3), physical slot = l&7) and must fetch logical slot
// (l&7) ^ ((row>>1)&7) of that row.
__device__ __forceinline__ void stage_glds(const GemmParams& p, int kt, int row0_m, int row0_n, int wave, int lane,
                                           char* stage) {
    const char *A, *Bt; int64_t lda, ldb, kb;
    seg_of(p, kt, A, Bt, lda, ldb, kb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int piece = i * 4 + wave;
        int row = piece * 8 + (lane >> 3);
        int sslot = (lane & 7) ^ ((row >> 1) & 7);
        const char* ga = A + (int64_t)(row0_m + row) * lda + kb + sslot * 16;
        const char* gb = Bt + (int64_t)(row0_n + row) * ldb + kb + sslot * 16;
        char* la = stage + piece * 1024;
        char* lb = stage + TILE_BYTES + piece * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ga,
                                         (__attribute__((address_space(3))) void*)la, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gb,
                                         (__attribute__((address_space(3))) void*)lb, 16, 0, 0);
    }
}

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// One K tile of MFMA work for a wave.  All 16 fragment reads (ds_read_b128, 64 VGPRs) are issued back to back and
// the four MFMA groups wait with COUNTED lgkmcnt (12/8/4/0): the first MFMAs start as soon as their fragments land
// and the LDS latency of the rest hides behind them.  rocprofv3 showed ~50 % of wave time parked in lgkmcnt(0) with
// the compiler's own read->wait(0)->MFMA x4 schedule, and hipcc turns any source-level hoisting back into a full
// wait, so the reads are inline asm (invisible to its scoreboard) with hand-placed waits; each wait is followed by
// sched_barrier(0) because register-only MFMAs may otherwise be hoisted above an asm s_waitcnt (guide 5.4 rule 18).
__device__ __forceinline__ i32x4 lds_read_b128(uint32_t addr) {
    i32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=&v"(v) : "v"(addr));
    return v;
}
__device__ __forceinline__ i32x4 lds_read_b128_off4096(uint32_t addr) {
    i32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:4096" : "=&v"(v) : "v"(addr));
    return v;
}

template <typename T>
__device__ __forceinline__ void compute_stage(const char* stage, int wm, int wn, int lane, f32x16 (&acc)[2][2]) {
    const int r = lane & 31, g = lane >> 5;
    const int swz = (r >> 1) & 7;
    const uint32_t base = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)stage;
    const uint32_t pa = base + (wm * 64 + r) * BKB;
    const uint32_t pb = base + TILE_BYTES + (wn * 64 + r) * BKB;
    i32x4 a[4][2], b[4][2];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const uint32_t so = ((kk * 2 + g) ^ swz) << 4;
        a[kk][0] = lds_read_b128(pa + so);
        a[kk][1] = lds_read_b128_off4096(pa + so);          // + 32 rows * 128 B
        b[kk][0] = lds_read_b128(pb + so);
        b[kk][1] = lds_read_b128_off4096(pb + so);
    }
#define DAE_MMA_GROUP(KK, CNT)                                   \
    asm volatile("s_waitcnt lgkmcnt(" #CNT ")" ::: "memory");    \
    __builtin_amdgcn_sched_barrier(0);                           \
    Mma<T>::run(a[KK][0], b[KK][0], acc[0][0]);                  \
    Mma<T>::run(a[KK][0], b[KK][1], acc[0][1]);                  \
    Mma<T>::run(a[KK][1], b[KK][0], acc[1][0]);                  \
    Mma<T>::run(a[KK][1], b[KK][1], acc[1][1]);
    DAE_MMA_GROUP(0, 12)
    DAE_MMA_GROUP(1, 8)
    DAE_MMA_GROUP(2, 4)
    DAE_MMA_GROUP(3, 0)
#undef DAE_MMA_GROUP
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
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int nk = kt1 - kt0;
    if (nk <= 0) return;

    if constexpr (NST >= 2) {
        // ---- LDS-DMA addressing: this lane's 16-byte chunk of each of its 4 pieces per operand, as a 32-bit byte offset
        //      from a uniform (SGPR) panel pointer that advances by one K tile per stage ----
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
            const int piece = i * 4 + wave;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gA + voA[i]),
                                             (__attribute__((address_space(3))) void*)(slot + piece * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gB + voB[i]),
                                             (__attribute__((address_space(3))) void*)(slot + TILE_BYTES + piece * 1024), 16, 0, 0);
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
        const uint32_t lbase = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)lds;
        const uint32_t offa = (wm * 64 + r) * BKB, offb = TILE_BYTES + (wn * 64 + r) * BKB;
        uint32_t so[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) so[kk] = (uint32_t)(((kk * 2 + g) ^ swz) << 4);
        i32x4 fa[4][2], fb[4][2];
#define DAE_READ_KK(KK, SLOTBASE)                                          \
    fa[KK][0] = lds_read_b128((SLOTBASE) + offa + so[KK]);                 \
    fa[KK][1] = lds_read_b128_off4096((SLOTBASE) + offa + so[KK]);         \
    fb[KK][0] = lds_read_b128((SLOTBASE) + offb + so[KK]);                 \
    fb[KK][1] = lds_read_b128_off4096((SLOTBASE) + offb + so[KK]);
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
            asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
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
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
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
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // drain the stale tail reads before the LDS is reused
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
