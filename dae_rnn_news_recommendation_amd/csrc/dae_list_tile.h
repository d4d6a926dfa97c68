// dae_list_tile.h -- what the kernels that work on ONE LIST'S OWN score tile share (dae_dedup.hip: dae_dedup_lists; dae_mmr.hip:
// dae_mmr_lists).  A row is a list of L <= 128 article indices; its rows of the normalised corpus image are gathered into a buffer
// (dedup_gather_kernel, dae_dedup.hip), and one workgroup per list runs gemm_mainloop<float, 2> with A = Bt = that buffer on tile
// (r, r): the list's 128 x 128 score tile.  The kernels differ in the epilogue alone.  Here: the sizes, the workspace
// (image + gather buffer + validity masks of a chunk of R lists), its carve with the checks every entry makes, and the gather launch.
#pragma once
#include "dae_score_sweep.h"

namespace dae {

constexpr int DEDUP_MAX = 128;                                 // one score tile per list
// The gather buffer of one chunk.  256 MiB is a GUESS, not a measurement: large enough that a chunk fills the chip many times over
// (1024 lists at D = 512), small beside the memory of one device.
constexpr uint64_t DEDUP_GATHER_BYTES = 256ull << 20;
constexpr int DEDUP_TILE_BYTES = BM * BN * 4;

static inline uint64_t dedup_list_bytes(int64_t Dp) { return (uint64_t)DEDUP_MAX * (uint64_t)Dp * 4; }
static inline int64_t dedup_r0(int64_t Dp) {
    const int64_t r = (int64_t)(DEDUP_GATHER_BYTES / dedup_list_bytes(Dp));
    return r < 1 ? 1 : r;
}
// image + gather buffer + validity masks of R lists
static inline uint64_t dedup_bytes(int64_t Nap, int64_t Dp, int64_t R) {
    return al256((uint64_t)Nap * Dp * 4) + (uint64_t)R * dedup_list_bytes(Dp) + al256((uint64_t)R * 16);
}
// what dae_dedup_lists_workspace and dae_mmr_lists_workspace return: the image and min(Nr, R0) lists
static inline uint64_t list_workspace_bytes(int32_t Nr, int32_t Na, int32_t D, int32_t L) {
    if (Nr <= 0 || Na <= 0 || D <= 0 || L <= 0) return 0;
    const int64_t Dp = pad128(D), R0 = dedup_r0(Dp);
    return dedup_bytes(pad128(Na), Dp, Nr < R0 ? Nr : R0);
}

struct ListWorkspace {
    float* image;                 // [Nap x Dp] the normalised corpus
    float* gathered;              // [R * 128 x Dp]
    unsigned long long* valid;    // [R][2]
    int64_t Nap, Dp, R;           // R: lists per chunk
};

// The checks of the image and the workspace (messages prefixed with `who`) and the carve: as many lists per chunk as the
// workspace holds, at most R0 (the K loop addresses the gather buffer with 32-bit byte offsets) and Nr.  No HIP call.
static inline int list_workspace_carve(const char* who, int32_t Na, int32_t D, int32_t Nr, void* workspace, uint64_t workspace_bytes,
                                       ListWorkspace& w) {
    w.Nap = pad128(Na); w.Dp = pad128(D);
    DAE_CHECK_ARG(w.Nap * w.Dp * 4 < (1ll << 32), "%s: the corpus image exceeds 4 GiB", who);
    const uint64_t least = dedup_bytes(w.Nap, w.Dp, 1);
    DAE_CHECK_ARG(workspace_bytes >= least, "%s: workspace too small (%llu < %llu bytes: the corpus image and one list)", who,
                  (unsigned long long)workspace_bytes, (unsigned long long)least);
    DAE_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "%s: workspace must be 256-byte aligned", who);
    int64_t R = (int64_t)((workspace_bytes - al256((uint64_t)w.Nap * w.Dp * 4)) / (dedup_list_bytes(w.Dp) + 16));
    const int64_t R0 = dedup_r0(w.Dp);
    if (R > R0) R = R0;
    if (R > Nr) R = Nr;
    while (R > 1 && dedup_bytes(w.Nap, w.Dp, R) > workspace_bytes) --R;
    w.R = R;
    char* c = (char*)workspace;
    w.image = (float*)c;                    c += al256((uint64_t)w.Nap * w.Dp * 4);
    w.gathered = (float*)c;                 c += (uint64_t)R * dedup_list_bytes(w.Dp);
    w.valid = (unsigned long long*)c;
    return 0;
}

// dedup_gather_kernel (dae_dedup.hip) on n lists: list r's rows of the image into rows 128 r .. 128 r + 127 of `gathered`, an entry
// < 0 or >= Na and the positions >= L as zero rows, and the list's 128-bit mask of the entries in range into valid[2 r .. 2 r + 1]
int launch_list_gather(const float* image, int Dp, int Na, const int32_t* lists, int64_t ldl, int L, int64_t n, float* gathered,
                       unsigned long long* valid, hipStream_t st);

}  // namespace dae
