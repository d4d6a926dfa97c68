// dae_api.hip -- extern "C" surface of libdae_hip.so (declared in include/dae_hip.h): the thin wrappers of the launchers, the plan's lifecycle,
// options and profile, and the data-parallel entry points.  The step driver (dae_train_step, dae_encode_rows) is dae_step.hip.
#include <stdarg.h>
#include <new>

#include "dae_plan.h"

namespace dae {

static thread_local char g_err[1024] = "";
thread_local LaunchTimer g_lt = {nullptr, nullptr, nullptr, 0, 0, false};
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace dae

using namespace dae;

extern "C" int dae_abi_version(void) { return DAE_ABI_VERSION; }
extern "C" const char* dae_last_error(void) { return g_err; }
extern "C" int64_t dae_pad(int64_t n) { return pad128(n); }
extern "C" void dae_set_glds(int32_t nst) { set_use_glds(nst); }
extern "C" int32_t dae_gemm_w8_splits(int32_t dtype, int32_t M, int32_t N, int32_t K) { return gemm_w8_splits(dtype, M, N, K * (dtype == DAE_BF16 ? 2 : 4) / 128); }
extern "C" int32_t dae_decode_tile_n(int32_t dtype) { return decode_tile_n(dtype); }
// 16-bit storage format this library was built for: 0 = bfloat16 (libdae_hip.so), 1 = IEEE fp16 (libdae_hip_f16.so); see dae_common.h
extern "C" int32_t dae_storage_format(void) { return kF16 ? 1 : 0; }

extern "C" int dae_gemm_nt(int32_t dtype, int32_t M, int32_t N, const void* A0, int64_t lda0, const void* Bt0, int64_t ldb0,
                           int32_t K0, const void* A1, int64_t lda1, const void* Bt1, int64_t ldb1, int32_t K1, float* C,
                           int64_t ldc, int32_t splits, int64_t slab_stride, void* stream) {
    return launch_gemm_f32out(dtype, M, N, A0, lda0, Bt0, ldb0, K0, A1, lda1, Bt1, ldb1, K1, C, ldc, splits, slab_stride,
                              (hipStream_t)stream);
}

extern "C" int dae_gemm_nt_n(int32_t dtype, int32_t M, int32_t N, const dae_gemm_seg* segs, int32_t nsegs, float* C, int64_t ldc,
                             int32_t splits, int64_t slab_stride, void* stream) {
    DAE_CHECK_ARG(segs && nsegs >= 1 && nsegs <= 6, "gemm_nt_n: 1..6 K segments");
    GemmSegDesc d[6];
    for (int i = 0; i < nsegs; ++i) d[i] = {segs[i].A, segs[i].lda, segs[i].Bt, segs[i].ldb, segs[i].K};
    return launch_gemm_f32out_n(dtype, M, N, d, nsegs, C, ldc, splits, slab_stride, (hipStream_t)stream);
}

extern "C" int dae_gemm_trace(int32_t dtype, int32_t M, int32_t N, const void* A0, int64_t lda0, const void* Bt0, int64_t ldb0,
                              int32_t K0, const void* A1, int64_t lda1, const void* Bt1, int64_t ldb1, int32_t K1, float* C,
                              int64_t ldc, int32_t splits, int64_t slab_stride, int32_t nst, uint64_t* trace, void* stream) {
    return launch_gemm_trace(dtype, M, N, A0, lda0, Bt0, ldb0, K0, A1, lda1, Bt1, ldb1, K1, C, ldc, splits, slab_stride, nst,
                             (unsigned long long*)trace, (hipStream_t)stream);
}

extern "C" int dae_encode_bits(const uint32_t* xc_bits, int64_t ldw, const void* Wt_lo, int64_t ldwt, int32_t Bp, int32_t Hp, int32_t Fp,
                               float* slabs, int64_t ld_slab, int32_t splits, int64_t slab_stride, void* stream) {
    return launch_encode_bits(Bp, Hp, Fp, xc_bits, ldw, Wt_lo, ldwt, slabs, ld_slab, splits, slab_stride, (hipStream_t)stream);
}

extern "C" int dae_gram(const float* h_f32, int64_t ldh, int32_t Bp, int32_t Hp, float* D_slabs, int32_t splits, void* stream) {
    return launch_gemm_f32out(DAE_F32, Bp, Bp, h_f32, ldh, h_f32, ldh, Hp, nullptr, 0, nullptr, 0, 0, D_slabs, Bp, splits,
                              (int64_t)Bp * Bp, (hipStream_t)stream);
}

extern "C" int dae_decode_loss(int32_t dtype, int32_t B, int32_t F, int32_t H, const void* h_lo, int64_t ldh, const void* W_lo,
                               int64_t ldw, const float* bv, const void* x, int64_t ldx, const float* cw, int32_t dec_act,
                               int32_t loss_func, int32_t cos_pass, const float* cos_stats, float* cos_part,
                               float* rowloss_part, float* tile_part, float* dbv_part, void* delta2, int64_t ldd,
                               void* delta2_t, int64_t lddt, void* stream) {
    DAE_CHECK_ARG(h_lo && W_lo && bv && x && cw, "decode_loss: null input");
    DAE_CHECK_ARG(B > 0 && F > 0 && H > 0, "decode_loss: bad shape");
    DAE_CHECK_ARG(loss_func >= DAE_LOSS_CROSS_ENTROPY && loss_func <= DAE_LOSS_COSINE, "decode_loss: unknown loss %d", loss_func);
    if (loss_func == DAE_LOSS_COSINE) {
        DAE_CHECK_ARG(cos_pass == 1 || cos_pass == 2, "decode_loss: cosine needs cos_pass 1 or 2");
        DAE_CHECK_ARG(cos_stats && (cos_pass != 1 || cos_part), "decode_loss: cosine statistics buffers required");
    } else {
        DAE_CHECK_ARG(cos_pass == 0 && (rowloss_part || tile_part), "decode_loss: rowloss_part or tile_part required");
    }
    DecodeEpi e;
    memset(&e, 0, sizeof(e));
    e.bv = bv; e.x = x; e.ldx = ldx; e.cw = cw; e.cos_stats = cos_stats; e.rowloss_part = rowloss_part; e.tile_part = tile_part; e.dbv_part = dbv_part;
    e.cos_part = cos_part; e.delta2 = delta2; e.ldd = ldd; e.delta2_t = delta2_t; e.lddt = lddt;
    e.B = B; e.F = F; e.Bp = (int)pad128(B); e.Fp = (int)pad128(F); e.dec_act = dec_act; e.loss_func = loss_func;
    e.cos_pass = cos_pass;
    return launch_decode_loss(dtype, e.Bp, e.Fp, (int)pad128(H), h_lo, ldh, W_lo, ldw, e, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// plan: sizes, workspace carving, step driver
// ------------------------------------------------------------------------------------------------
// names of the per-kernel HIP-event timing slots of the step driver (PS_*, dae_plan.h; bench.py's roofline leg)
static const char* const kProfNames[PS_COUNT] = {"memset_xct", "gather", "encode_gemm", "encode_finish", "label_stats", "gram",
                                                 "miner", "triplet_finalize", "sym_scale", "decode_loss", "cos_reduce",
                                                 "step_stats", "dh_gemm", "dh_finish", "dw_gemm", "bias_grads", "opt_step"};

static int auto_splits(int tiles, int ktiles) {
    int s = 384 / (tiles > 0 ? tiles : 1);
    if (s >= 8) s = (s / 8) * 8;
    if (s > 16) s = 16;
    int cap = ktiles / 4;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    return s;
}
// slab count of the Gram matrix: ONE for the 64 x 64-tile kernel over the whole K (gram64_ok), else split-K slices of the 128 x 128 kernel
static int plan_gram_splits(const dae_plan* p) {
    if (p->gram64_ok) return 1;
    const int kt = p->Hp * 4 / 128;
    const int s = p->cfg.gram_splits > 0 ? p->cfg.gram_splits : auto_splits((p->Bpm / 128) * (p->Bpm / 128), kt);
    return s > kt ? kt : s;
}

// split-bf16 mode on dense-ndarray input: slice counts of the 3-segment encode and the 4-5-segment dh contraction (see dae_plan_create)
static void plan_x3_splits(dae_plan* p) {
    const dae_config& c = p->cfg;
    const int kt_f = p->Fp * p->es / 128, kt_b = p->Bpm * p->es / 128;
    p->s_enc3 = p->s_enc; p->s_dh3 = p->s_dh;
    if (!p->x3) return;
    const uint32_t T = p->terms;
    const int n_enc = 1 + ((T & X3T_ENC_WLO) ? 1 : 0) + ((T & X3T_ENC_XLO) ? 1 : 0);
    const int n_dh = 1 + ((T & X3T_DH_WLO) ? 1 : 0) + ((T & X3T_DH_D2LO) ? 1 : 0);
    if (c.encode_splits <= 0) if (const int w = gemm_w8_splits(c.dtype, p->Bpm, p->Hp, n_enc * kt_f)) p->s_enc3 = w;
    if (c.dh_splits <= 0) if (const int w = gemm_w8_splits(c.dtype, p->Bpm, p->Hp, n_dh * kt_f + ((T & X3T_DH_HLO) ? 2 : 1) * kt_b)) p->s_dh3 = w;
}

static uint64_t carve(dae_plan* p, char* base) {
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) -> char* {
        char* r = base ? base + off : nullptr;
        off += (bytes + 255) / 256 * 256;
        return r;
    };
    const uint64_t Bp = p->Bpm, Fp = p->Fp, Hp = p->Hp, es = p->es;
    p->x = take(Bp * Fp * es);
    p->xc = take(Bp * Fp * es);
    p->xct = take(Fp * Bp * es);
    p->xc_bits = (uint32_t*)take(Bp * (Fp / 32) * 4);
    p->x_bits = (uint32_t*)take(Bp * (Fp / 32) * 4);
    p->delta2 = take(Bp * Fp * es);
    p->delta2_t = take(Fp * Bp * es);
    int smax = p->s_enc > p->s_dh ? p->s_enc : p->s_dh;
    if (p->x3) { if (p->s_enc3 > smax) smax = p->s_enc3; if (p->s_dh3 > smax) smax = p->s_dh3; }
    p->slabs = (float*)take((uint64_t)smax * Bp * Hp * 4);
    p->h_f32 = (float*)take(Bp * Hp * 4);
    p->h_lo = take(Bp * Hp * es);
    p->h_t = take(Hp * Bp * es);
    p->delta1_t = take(Hp * Bp * es);
    p->delta1_lo = take(Bp * Hp * es);
    p->dh_extra = (float*)take(Bp * Hp * 4);
    const uint32_t T = p->x3 ? p->terms : 0u;          // lo images exist only for the product terms that read them
    p->W_lo2 = take((T & X3T_DEC_WLO) ? Fp * Hp * 2 : 256);
    p->Wt_lo2 = take(p->x3 ? Hp * Fp * 2 : 256);      // (the split mode's dW epilogue always writes it)
    p->h_t2 = take((T & (X3T_DH_HLO | X3T_DW_HLO)) ? Hp * Bp * 2 : 256);
    p->delta2_2 = take((T & X3T_DH_D2LO) ? Bp * Fp * 2 : 256);
    p->delta2_t2 = take((T & X3T_DW_D2LO) ? Fp * Bp * 2 : 256);
    p->delta1_t2 = take((T & X3T_DW_D1LO) ? Hp * Bp * 2 : 256);
    p->x_2 = take((T & X3T_XV) ? Bp * Fp * 2 : 256);
    p->xct_2 = take((T & X3T_XV) ? Fp * Bp * 2 : 256);
    p->xc_2 = take((T & X3T_ENC_XLO) ? Bp * Fp * 2 : 256);
    p->hcat_a = take(p->gram_split ? Bp * 3 * Hp * 2 : 256);
    p->hcat_b = take(p->gram_split ? Bp * 3 * Hp * 2 : 256);
    p->D_slabs = (float*)take((uint64_t)p->s_gram * Bp * Bp * 4);
    p->G = (float*)take(Bp * Bp * 4);
    p->Gs = take(Bp * Bp * es);
    p->role_cnt = (uint32_t*)take(Bp * Bp * 4);        // pos_triplets_only role counts (probe builds: the miner's timeline stamps)
    const uint64_t dbn = plan_dec_bn(p);                 // tile width of the decode kernel: lays out its partial-sum arrays
    p->rowloss_part = (float*)take((2 * Fp / dbn) * Bp * 4);
    p->dbv_part = (float*)take((2 * Bp / 128) * Fp * 4);
    p->colsum_part = (float*)take(2 * (Bp / 32) * Hp * 4);
    p->cos_part = (float*)take(2 * (2 * Fp / dbn) * Bp * 4);
    p->cos_stats = (float*)take(3 * Bp * 4);
    p->rowsq_scratch = (float*)take((Fp / 64) * Bp * 4);
    p->zbuf = (float*)take(p->cfg.loss_func == DAE_LOSS_COSINE ? Bp * Fp * 4 : 256);     // cosine: the decode's accumulators between its two passes (DecodeEpi::z_io)
    p->tile_part = (float*)take((Bp / 128) * (Fp / dbn) * 4);
    p->cw = (float*)take(Bp * 4);
    p->loss_part = (float*)take(Bp * 4);
    p->dw_f32 = (float*)take(Bp * 4);
    p->cnt_part = (uint32_t*)take(Bp * 4);
    p->dw_i32 = (int32_t*)take(Bp * 4);
    p->n_same = (int32_t*)take(Bp * 4);
    p->dw_i64 = (int64_t*)take(Bp * 8);
    p->nvalid = (int64_t*)take(256);
    p->acc = (uint64_t*)take(256);
    p->tri_scalars = (float*)take(256);
    p->miner_order = (int32_t*)take(Bp * 4);
    p->cls_range = (int32_t*)take((1 + 2 * Bp) * 4);
    return off;
}

extern "C" int dae_plan_create(const dae_config* cfg, dae_plan** out) {
    DAE_CHECK_ARG(cfg && out, "plan_create: null argument");
    DAE_CHECK_ARG(cfg->n_features > 0 && cfg->n_components > 0 && cfg->max_batch > 0, "plan_create: bad sizes");
    DAE_CHECK_ARG(cfg->dtype == DAE_BF16 || cfg->dtype == DAE_F32 || cfg->dtype == DAE_BF16X3, "plan_create: bad dtype");
    DAE_CHECK_ARG(cfg->enc_act >= 0 && cfg->enc_act <= 2 && cfg->dec_act >= 0 && cfg->dec_act <= 2, "plan_create: bad activation");
    DAE_CHECK_ARG(cfg->loss_func >= 0 && cfg->loss_func <= 2, "plan_create: bad loss_func");
    DAE_CHECK_ARG(cfg->opt >= 0 && cfg->opt <= 3, "plan_create: bad optimizer");
    DAE_CHECK_ARG(cfg->triplet >= 0 && cfg->triplet <= 3, "plan_create: bad triplet strategy");
    dae_plan* p = new (std::nothrow) dae_plan();
    DAE_CHECK_ARG(p, "plan_create: out of memory");
    memset(p, 0, sizeof(*p));
    p->cfg = *cfg;
    // split-bf16 mode: bf16 element type and kernels everywhere (cfg.dtype reads DAE_BF16 from here on); x3 adds the lo images, the
    // extra K segments of the three gradient GEMMs and the epilogues that write both parts
    p->x3 = cfg->dtype == DAE_BF16X3;
    if (p->x3) p->cfg.dtype = DAE_BF16;
    cfg = &p->cfg;
    p->F = cfg->n_features; p->H = cfg->n_components; p->Bmax = cfg->max_batch;
    p->Fp = (int)pad128(p->F); p->Hp = (int)pad128(p->H); p->Bpm = (int)pad128(p->Bmax);
    p->es = cfg->dtype == DAE_BF16 ? 2 : 4;
    const int tiles_bh = (p->Bpm / 128) * (p->Hp / 128);
    const int kt_f = p->Fp * p->es / 128;
    p->s_enc = cfg->encode_splits > 0 ? cfg->encode_splits : auto_splits(tiles_bh, kt_f);
    p->s_dh = cfg->dh_splits > 0 ? cfg->dh_splits : auto_splits(tiles_bh, kt_f);
    // large dense-input shapes: the 256 x 256 kernel picks its own slice count (one workgroup per CU)
    if (cfg->encode_splits <= 0) if (const int w = gemm_w8_splits(cfg->dtype, p->Bpm, p->Hp, kt_f)) p->s_enc = w;
    if (cfg->dh_splits <= 0) if (const int w = gemm_w8_splits(cfg->dtype, p->Bpm, p->Hp, kt_f + p->Bpm * p->es / 128)) p->s_dh = w;
    if (p->s_enc > kt_f) p->s_enc = kt_f;
    if (p->s_dh > kt_f) p->s_dh = kt_f;
    // split-bf16 mode on dense-ndarray input: the encode contraction has 3 K segments and dh 5; the 256 x 256 kernel is taken exactly when the
    // launch is handed ITS slice count for the real K-tile total, so these are planned with the segment lists' totals
    p->terms = kF16 ? (uint32_t)X3T_F16_DEFAULT : (uint32_t)X3T_ALL;
    // fp16 storage: op_scale = the largest power of two <= 16 * max_batch (capped at 2^14).  Bounds that keep the scaled images finite: |delta2| <= cw_i
    // (<= ~8 / B typically, <= 1 always) for a sigmoid decoder, |Gs| <= 2 alpha B / N_valid; the stores saturate at +-65504 beyond that (sat16)
    p->op_scale = 1.f;
    if (kF16 && p->es == 2) { float sc = 1.f; while (sc * 2.f <= 16.f * (float)p->Bmax && sc < 16384.f) sc *= 2.f; p->op_scale = sc; }
    p->dw_pair_ok = true;
    plan_x3_splits(p);
    p->gram_split = (cfg->dtype == DAE_BF16) && (p->x3 || cfg->triplet == DAE_TRIPLET_BATCH_ALL || cfg->triplet == DAE_TRIPLET_BATCH_HARD);   // x3: hcat_a also holds the row-major h_lo
    p->dw_tr_mode = -1;
    p->gram64_ok = p->gram_split && cfg->gram_splits <= 0;        // (an explicit split count keeps the 128 x 128 split-K form)
    p->s_gram = plan_gram_splits(p);
    p->ws_bytes = carve(p, nullptr);
    // code-path choices below are plan state (dae_plan_set_option), never read from the environment
    p->fuse_opt_ok = true;
    p->tail_ok = true;
    p->label_enc_ok = true;
    p->ce_literal = false;
    p->xbits_ok = cfg->dtype == DAE_BF16;
    p->xct_clean = false; p->xct2_clean = false;
    p->enc_w32_ok = cfg->dtype == DAE_BF16;
    p->w32_cols = 128;                                 // measured: 128-column fp32 slices (5.2 MB, served by the MALL) beat 64-column ones
    // binary CSR + bf16: x~ goes to the encode GEMM as a bit image whenever the 8-wave bit kernel can run the shape
    p->bits_ok = cfg->dtype == DAE_BF16 && encode_bits_fits(p->Bpm, p->Hp, p->Fp, p->s_enc);
    p->sparse_ok = true;
    p->miner_order_ok = true; p->sym_ride_ok = true; p->miner_ranges_ok = true;
    p->cos_zstore_ok = true;
    *out = p;
    return 0;
}

extern "C" void dae_plan_destroy(dae_plan* p) {
    if (!p) return;
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    for (int i = 0; i < dae_plan::PROF_POOL; ++i) if (p->pev[i]) (void)hipEventDestroy(p->pev[i]);
    if (p->ev_dw) (void)hipEventDestroy(p->ev_dw);
    delete p;
}

// the options that change the workspace layout (and what of it, for the error message); NULL for every other name
static const char* relayout_reason(const char* name) {
    if (!strcmp(name, "x3_dec_wlo") || !strcmp(name, "x3_dh_hlo") || !strcmp(name, "x3_terms")) return "split-K plan (workspace layout)";
    if (!strcmp(name, "gram64")) return "workspace layout (slab count)";
    if (!strcmp(name, "decode_bn") || !strcmp(name, "gram_fp32")) return "workspace layout";
    return nullptr;
}

// Code-path choices of a plan (A/B measurements and equivalence tests).  Every option selects between implementations of
// the SAME arithmetic; nothing here is read from the environment, so a stray variable can never change a training run.
extern "C" int dae_plan_set_option(dae_plan* p, const char* name, int32_t value) {
    DAE_CHECK_ARG(p && name, "plan_set_option: null argument");
    const bool on = value != 0;
    if (!strcmp(name, "encode_sparse")) p->sparse_ok = on;
    else if (!strcmp(name, "encode_bits")) p->bits_ok = on && p->cfg.dtype == DAE_BF16 && encode_bits_fits(p->Bpm, p->Hp, p->Fp, p->s_enc);
    else if (!strcmp(name, "x_bits")) p->xbits_ok = on && p->cfg.dtype == DAE_BF16;
    else if (!strcmp(name, "fused_opt")) p->fuse_opt_ok = on;
    else if (!strcmp(name, "dw_pair")) p->dw_pair_ok = on;
    else if (!strcmp(name, "dw_tr")) { DAE_CHECK_ARG(value >= -1 && value <= 1, "plan_set_option: dw_tr is -1 (auto), 0 or 1"); p->dw_tr_mode = value; p->xct_clean = false; }
    else if (!strcmp(name, "encode_w32")) p->enc_w32_ok = on && p->cfg.dtype == DAE_BF16;
    else if (!strcmp(name, "encode_w32_cols")) { DAE_CHECK_ARG(value == 64 || value == 128, "plan_set_option: encode_w32_cols is 64 or 128"); p->w32_cols = value; }
    else if (!strcmp(name, "tail")) p->tail_ok = on;
    else if (!strcmp(name, "label_with_encode")) p->label_enc_ok = on;
    else if (!strcmp(name, "ce_literal")) p->ce_literal = on;
    else if (!strcmp(name, "gather_tile")) set_gather_tile(value);        // process-wide: tile shape of the dense gather (A/B measurements)
    else if (!strcmp(name, "dw_rounds")) { DAE_CHECK_ARG(value >= 1 && value <= 64, "plan_set_option: dw_rounds in 1..64"); set_use_glds(-100 - value); }   // process-wide, like miner_pack
    else if (!strcmp(name, "cos_zstore")) p->cos_zstore_ok = on;
    else if (!strcmp(name, "gram_fused")) set_use_glds(on ? -20 : -19);    // process-wide: the split Gram's three products per K tile in one LDS stage (gram64f_kernel; default on), 0 = the K-concatenated walk (gram64_kernel)
    else if (!strcmp(name, "decode_x3")) set_use_glds(on ? -18 : -17);     // process-wide: the split modes' decode on the K loops that keep the hi stage's fragments in registers (mainloop_n64_x3 / _c2; default on, binary input)
    else if (!strcmp(name, "pad_skip")) set_use_glds(on ? -12 : -11);      // process-wide: 0 = multiply / evaluate the all-padding 32-row blocks of the last batch tile too (A/B)
    else if (!strcmp(name, "decode_bm")) {                                  // tile height of the decode kernel: 0 auto (batch_route), 128, 160 (gemm_decode_loss_160)
        DAE_CHECK_ARG(value == 0 || value == 128 || value == 160, "plan_set_option: decode_bm is 0 (auto), 128 or 160");
        DAE_CHECK_ARG(value != 160 || plan_dec_bm160_form(p, p->xbits_ok),
                      "plan_set_option: decode_bm = 160 needs the three-term 16-bit decode with a bit image of x (f16x2h on a binary CSR train set; no cosine loss, no lo images of delta2 / x, decode_bn 64)");
        p->dec_bm = value;
    }
    else if (!strcmp(name, "miner_order")) p->miner_order_ok = on;
    else if (!strcmp(name, "miner_ranges")) p->miner_ranges_ok = on;
    else if (!strcmp(name, "miner_pack")) set_miner_pack(on);        // process-wide (the launcher's choice), like dae_set_glds
    else if (!strcmp(name, "miner_tile")) set_miner_tile(on);        // process-wide: 0 = the former wave-per-positive batch_all kernel
    else if (!strcmp(name, "sym_in_decode")) p->sym_ride_ok = on;
    else if (!strcmp(name, "op_scale_log2")) {
        DAE_CHECK_ARG(value >= 0 && value <= 20, "plan_set_option: op_scale_log2 in 0..20");
        DAE_CHECK_ARG(p->es == 2, "plan_set_option: op_scale_log2 applies to the 16-bit modes");
        p->op_scale = (float)(1u << value);
    }
    else if (const char* why = relayout_reason(name)) {      // the options that change the workspace layout: before dae_plan_bind only, then re-plan and re-carve
        DAE_CHECK_ARG(!p->bound, "plan_set_option: %s changes the %s, set it before dae_plan_bind", name, why);
        if (!strcmp(name, "x3_terms")) {
            DAE_CHECK_ARG(value >= 0 && (uint32_t)value <= X3T_ALL, "plan_set_option: x3_terms is a mask of the X3T_* bits (0..%u)", (unsigned)X3T_ALL);
            p->terms = (uint32_t)value;
        } else if (name[0] == 'x') {                         // the legacy options flip their bit of the mask
            const uint32_t bit = !strcmp(name, "x3_dec_wlo") ? X3T_DEC_WLO : X3T_DH_HLO;
            p->terms = on ? (p->terms | bit) : (p->terms & ~bit);
        } else if (!strcmp(name, "decode_bn")) {
            DAE_CHECK_ARG(value == 0 || value == 64 || value == 128, "plan_set_option: decode_bn is 0 (auto), 64 or 128");
            p->dec_bn = value;
        } else if (!strcmp(name, "gram64")) {
            p->gram64_ok = on && p->gram_split;
        } else {                                             // gram_fp32; the exact-fp32 Gram runs on the 128 x 128 split-K kernel
            DAE_CHECK_ARG(!p->x3, "plan_set_option: gram_fp32 is not available in split-bf16 mode (its Gram operands double as the row-major h images)");
            p->gram_split = !on && p->cfg.dtype == DAE_BF16 && (p->cfg.triplet == DAE_TRIPLET_BATCH_ALL || p->cfg.triplet == DAE_TRIPLET_BATCH_HARD);
            if (!p->gram_split) p->gram64_ok = false;
        }
        plan_x3_splits(p);
        p->s_gram = plan_gram_splits(p);
        p->ws_bytes = carve(p, nullptr);
    } else {
        set_error("plan_set_option: unknown option '%s'", name);
        return 1;
    }
    return 0;
}

extern "C" int dae_plan_profile(dae_plan* p, int32_t enable) {
    DAE_CHECK_ARG(p, "plan_profile: null plan");
    if (enable && !p->ev0) {
        DAE_CHECK_HIP(hipEventCreate(&p->ev0));
        DAE_CHECK_HIP(hipEventCreate(&p->ev1));
    }
    const int rf = p->pev_used ? plan_prof_flush(p) : 0;     // pairs still queued belong to the mode being left; a failed read is reported, the switch still happens
    if ((enable == 2 || enable == 3) && !p->pev[0])
        for (int i = 0; i < dae_plan::PROF_POOL; ++i) DAE_CHECK_HIP(hipEventCreate(&p->pev[i]));
    if (enable) { memset(p->prof_ms, 0, sizeof(p->prof_ms)); memset(p->prof_n, 0, sizeof(p->prof_n)); }
    p->prof = enable != 0;
    p->prof_queued = enable == 2 || enable == 3;
    p->prof_stamps = enable == 3;
    p->pev_used = 0;
    return rf;
}

extern "C" int dae_plan_profile_read(const dae_plan* p, int32_t max_slots, double* ms_total, int32_t* counts) {
    DAE_CHECK_ARG(p && ms_total && counts, "plan_profile_read: null argument");
    if (int rf = plan_prof_flush(const_cast<dae_plan*>(p))) return rf;
    for (int i = 0; i < PS_COUNT && i < max_slots; ++i) { ms_total[i] = p->prof_ms[i]; counts[i] = p->prof_n[i]; }
    return PS_COUNT <= max_slots ? 0 : 1;
}

extern "C" int32_t dae_plan_profile_slots(void) { return PS_COUNT; }
extern "C" const char* dae_plan_profile_name(int32_t slot) { return (slot >= 0 && slot < PS_COUNT) ? kProfNames[slot] : ""; }
extern "C" uint64_t dae_plan_workspace_bytes(const dae_plan* p) { return p ? p->ws_bytes : 0; }

extern "C" int dae_plan_bind(dae_plan* p, const dae_buffers* bufs) {
    DAE_CHECK_ARG(p && bufs, "plan_bind: null argument");
    DAE_CHECK_ARG(bufs->W && bufs->bh && bufs->bv && bufs->grad && bufs->W_lo && bufs->Wt_lo, "plan_bind: null parameter buffer");
    DAE_CHECK_ARG(bufs->workspace && bufs->workspace_bytes >= p->ws_bytes, "plan_bind: workspace too small (%llu < %llu)",
                  (unsigned long long)bufs->workspace_bytes, (unsigned long long)p->ws_bytes);
    DAE_CHECK_ARG(((uintptr_t)bufs->workspace % 256) == 0, "plan_bind: workspace must be 256-byte aligned");
    DAE_CHECK_ARG((bufs->indptr != nullptr) != (bufs->dense != nullptr) || (!bufs->indptr && !bufs->dense),
                  "plan_bind: give either a CSR or a dense train set");
    DAE_CHECK_ARG(p->cfg.opt == DAE_OPT_SGD || bufs->opt_s1, "plan_bind: optimizer slot buffer required");
    DAE_CHECK_ARG(p->cfg.opt != DAE_OPT_ADAM || bufs->opt_s2, "plan_bind: second optimizer slot buffer required");
    p->b = *bufs;
    carve(p, (char*)bufs->workspace);
    p->bound = true;
    p->xct_clean = false;            // a (re)bound workspace has not been cleared: the next backward step memsets x~^T once
    p->xct2_clean = false;
    return 0;
}

extern "C" int dae_plan_sync_shadows(dae_plan* p, void* stream) {
    DAE_CHECK_ARG(p && p->bound, "plan_sync_shadows: plan not bound");
    return plan_opt_step(p, 0.f, 1.f, /*apply=*/0, stream);
}

extern "C" void* dae_plan_buffer(dae_plan* p, const char* name) {
    if (!p || !p->bound || !name) return nullptr;
#define DAE_BUF(n) if (!strcmp(name, #n)) return (void*)p->n;
    DAE_BUF(hcat_a) DAE_BUF(hcat_b) DAE_BUF(x) DAE_BUF(xc) DAE_BUF(xct) DAE_BUF(h_lo) DAE_BUF(h_t) DAE_BUF(Gs) DAE_BUF(delta2) DAE_BUF(delta2_t) DAE_BUF(delta1_t)
    DAE_BUF(delta1_lo) DAE_BUF(W_lo2) DAE_BUF(Wt_lo2) DAE_BUF(h_t2) DAE_BUF(delta2_2) DAE_BUF(delta2_t2) DAE_BUF(delta1_t2) DAE_BUF(x_2) DAE_BUF(xct_2) DAE_BUF(xc_2)
    DAE_BUF(slabs) DAE_BUF(h_f32) DAE_BUF(D_slabs) DAE_BUF(G) DAE_BUF(rowloss_part) DAE_BUF(dbv_part) DAE_BUF(colsum_part)
    DAE_BUF(cos_part) DAE_BUF(cos_stats) DAE_BUF(cw) DAE_BUF(loss_part) DAE_BUF(dw_f32) DAE_BUF(tri_scalars) DAE_BUF(dh_extra)
    DAE_BUF(tile_part) DAE_BUF(cnt_part) DAE_BUF(role_cnt) DAE_BUF(dw_i32) DAE_BUF(n_same) DAE_BUF(nvalid) DAE_BUF(dw_i64)
#undef DAE_BUF
    return nullptr;
}

extern "C" int dae_plan_info(const dae_plan* p, int32_t* out8) {
    DAE_CHECK_ARG(p && out8, "plan_info: null");
    out8[0] = p->Fp; out8[1] = p->Hp; out8[2] = p->Bpm; out8[3] = p->s_enc; out8[4] = p->s_dh; out8[5] = p->s_gram;
    out8[6] = p->es; out8[7] = p->x3 ? (int32_t)(1u | (p->terms << 1) | ((uint32_t)ilogbf(p->op_scale) << 16)) : (int32_t)((uint32_t)ilogbf(p->op_scale) << 16);   // bit 0: split mode; bits 1..11: its lo terms; bits 16..: log2 op_scale
    return 0;
}

// queued profile mode: wait for the step's last pair, then add every pair to its slot
int plan_prof_flush(dae_plan* p) {
    if (!p->prof_queued || p->pev_used == 0) return 0;
    const int used = p->pev_used;
    p->pev_used = 0;                                    // (also on the error paths below: a failed read must not poison the next profile call)
    DAE_CHECK_HIP(hipEventSynchronize(p->pev[used - 1]));
    for (int i = 0; i < used; i += 2) {
        float ms = 0.f;
        DAE_CHECK_HIP(hipEventElapsedTime(&ms, p->pev[i], p->pev[i + 1]));
        const int sl = p->pev_slot[i / 2] & 0xff;          // bit 8: the first launch of its PROF call (a call with several launches counts once)
        p->prof_ms[sl] += ms; p->prof_n[sl] += (p->pev_slot[i / 2] >> 8) & 1;
    }
    return 0;
}

extern "C" int dae_plan_apply(dae_plan* p, int32_t adam_t, float grad_scale, void* stream) {
    DAE_CHECK_ARG(p && p->bound, "plan_apply: plan not bound");
    return plan_opt_step(p, plan_lr(p, adam_t), grad_scale, /*apply=*/1, stream);
}

// The same on the row band [f0, f1) of W (multiples of 64) -- dp.AllReduceExchange with buckets: the flat gradient is all-reduced band by band and every
// band is applied as soon as its sum has arrived, while the next band is still on the wire.  The band that ends at Fp also updates the biases (their
// gradients sit behind the W part of the flat buffer, i.e. in the last bucket).  Bands applied in any order give the weights of one dae_plan_apply.
extern "C" int dae_plan_apply_band(dae_plan* p, int32_t adam_t, float grad_scale, int32_t f0, int32_t f1, void* stream) {
    DAE_CHECK_ARG(p && p->bound, "plan_apply_band: plan not bound");
    return plan_opt_step(p, plan_lr(p, adam_t), grad_scale, /*apply=*/1, stream, f0, f1);
}

// ---- the exchange itself, on the step's stream (dae_comm.hip holds the communicator; reference step: autoencoder.py:206-246) ----
namespace dae {
int comm_allreduce_sum(dae_comm* c, float* buf, int64_t n, hipStream_t st);
hipStream_t comm_wire(dae_comm* c);
hipEvent_t comm_ev_ready(dae_comm* c);
hipEvent_t comm_ev_band(dae_comm* c, int k);
}  // namespace dae

// In-place all-reduce(sum) of the plan's flat fp32 gradient [dW (Fp x Hp) | dbh (Hp) | dbv (Fp)] over the communicator, enqueued on `stream` --
// the stream the step's kernels run on, so it starts when the gradient is complete and dae_plan_apply behind it needs no cross-stream wait.
extern "C" int dae_allreduce_grads(dae_plan* p, dae_comm* c, void* stream) {
    DAE_CHECK_ARG(p && p->bound && c, "allreduce_grads: plan not bound / null communicator");
    DAE_CHECK_ARG(!p->b.grad_lo, "allreduce_grads: the plan writes a 16-bit exchange image (grad_lo); the flat fp32 gradient would be stale");
    return comm_allreduce_sum(c, p->b.grad, (int64_t)p->Fp * p->Hp + p->Hp + p->Fp, (hipStream_t)stream);
}

// The whole second half of a data-parallel step after dae_train_step(phase = 1): all-reduce of the flat gradient + the optimizer on every rank.
//   buckets <= 1: ncclAllReduce and dae_plan_apply back to back on `stream`.
//   buckets  > 1: the flat buffer is cut into row bands of W (dae_dp_bands).  The collectives run on the communicator's wire stream: the bands
//     that hold W rows only start behind the dW GEMM (the plan's ev_dw, i.e. beside the step's tail kernel), the last band -- it carries the bias
//     gradients the tail writes -- behind the tail.  `stream` applies band k (dae_plan_apply_band) as soon as band k has been reduced, while band
//     k + 1 is still on the wire.  Element-wise the same sums and the same update as one bucket.
// Costs per step on the host: 2 event records + (buckets + 2) stream waits -- microseconds, where torch.distributed took ~25 us per collective.
extern "C" int dae_dp_exchange(dae_plan* p, dae_comm* c, int32_t adam_t, float grad_scale, int32_t buckets, void* stream) {
    DAE_CHECK_ARG(p && p->bound && c, "dp_exchange: plan not bound / null communicator");
    DAE_CHECK_ARG(!p->b.grad_lo, "dp_exchange: the plan writes a 16-bit exchange image (grad_lo); the flat fp32 gradient would be stale");
    hipStream_t st = (hipStream_t)stream;
    const int Fp = p->Fp, Hp = p->Hp;
    const int64_t n_flat = (int64_t)Fp * Hp + Hp + Fp;
    int32_t bounds[DAE_COMM_MAX_BUCKETS + 1];
    const int nb = dae_dp_bands(Fp, buckets, bounds);
    if (nb == 1) {
        RC(comm_allreduce_sum(c, p->b.grad, n_flat, st));
        return dae_plan_apply(p, adam_t, grad_scale, stream);
    }
    hipStream_t wire = comm_wire(c);
    if (!p->ev_dw) DAE_CHECK_HIP(hipEventCreateWithFlags(&p->ev_dw, hipEventDisableTiming));      // recorded by the steps enqueued from now on
    if (p->ev_dw_live) {
        DAE_CHECK_HIP(hipStreamWaitEvent(wire, p->ev_dw, 0));                 // W gradient complete: bands 0 .. nb-2 run beside the step's tail
    } else {
        DAE_CHECK_HIP(hipEventRecord(comm_ev_ready(c), st));
        DAE_CHECK_HIP(hipStreamWaitEvent(wire, comm_ev_ready(c), 0));
    }
    for (int k = 0; k < nb; ++k) {
        const int64_t lo = (int64_t)bounds[k] * Hp, hi = k + 1 < nb ? (int64_t)bounds[k + 1] * Hp : n_flat;
        if (k == nb - 1 && p->ev_dw_live) {                                   // the bias gradients sit behind the W part: wait for the tail too
            DAE_CHECK_HIP(hipEventRecord(comm_ev_ready(c), st));
            DAE_CHECK_HIP(hipStreamWaitEvent(wire, comm_ev_ready(c), 0));
        }
        RC(comm_allreduce_sum(c, p->b.grad + lo, hi - lo, wire));
        DAE_CHECK_HIP(hipEventRecord(comm_ev_band(c, k), wire));
    }
    for (int k = 0; k < nb; ++k) {
        DAE_CHECK_HIP(hipStreamWaitEvent(st, comm_ev_band(c, k), 0));
        RC(dae_plan_apply_band(p, adam_t, grad_scale, bounds[k], bounds[k + 1], stream));
    }
    return 0;
}

// Data-parallel second half with a SHARDED optimizer: this rank owns rows [f0, f1) of W.  grad_rows holds the
// rank-summed gradient of those rows (fp32 [f1-f0 x Hp], the output of the reduce-scatter); biases are updated on every rank
// from the all-reduced bias part of the plan's flat gradient when update_bias != 0.  Afterwards the ranks all-gather W_lo and
// call dae_plan_refresh_wt.
extern "C" int dae_plan_apply_rows(dae_plan* p, int32_t adam_t, float grad_scale, const float* grad_rows, int32_t f0, int32_t f1,
                                   int32_t update_bias, void* stream) {
    // split-bf16 mode: only the fp32 master rows (and their hi image) are current afterwards; the caller all-gathers the MASTER rows and
    // rebuilds all four shadows with dae_plan_sync_shadows (dp.ShardedExchange)
    DAE_CHECK_ARG(p && p->bound && grad_rows, "plan_apply_rows: plan not bound / null gradient");
    DAE_CHECK_ARG(f0 >= 0 && f0 <= f1 && f1 <= p->Fp && f0 % 64 == 0 && f1 % 64 == 0, "plan_apply_rows: rows [%d, %d) outside [0, %d] or not multiples of 64", f0, f1, p->Fp);
    const float lr = plan_lr(p, adam_t);
    RC(dae_opt_step_rows(p->cfg.opt, lr, p->cfg.momentum, grad_scale, p->b.W, grad_rows, p->b.opt_s1, p->b.opt_s2, p->Hp, f0, f1, p->cfg.dtype,
                         p->b.W_lo, stream));
    if (update_bias) {
        const int64_t off = (int64_t)p->Fp * p->Hp;
        dim3 grid((p->Hp + p->Fp + 255) / 256), block(256);
        RC(dae_opt_bias(p->cfg.opt, lr, p->cfg.momentum, grad_scale, p->b.bh, p->b.bv, p->b.grad + off, plan_bias_slot(p, p->b.opt_s1),
                        plan_bias_slot(p, p->b.opt_s2), p->Hp, p->Fp, stream));
    }
    return 0;
}

// Data parallel: make `stream` wait until the W gradient of the LAST enqueued dae_train_step is complete (the event sits between the dW
// GEMM and the step's tail kernel).  The first call creates the event; steps enqueued before it are not covered (returns DAE_WAIT_DW_CREATED then;
// 0 = the wait was enqueued; any other value is an error, text in dae_last_error).
extern "C" int dae_plan_stream_wait_dw(dae_plan* p, void* stream) {
    DAE_CHECK_ARG(p && p->bound, "plan_stream_wait_dw: plan not bound");
    if (!p->ev_dw) {
        DAE_CHECK_HIP(hipEventCreateWithFlags(&p->ev_dw, hipEventDisableTiming));
        return DAE_WAIT_DW_CREATED;      // not an error (dae_last_error untouched): the event covers the steps enqueued from now on
    }
    DAE_CHECK_HIP(hipStreamWaitEvent((hipStream_t)stream, p->ev_dw, 0));
    return 0;
}

// Packed form of the sharded second half (dp.ShardedExchange): the low-precision rows of [f0, f1) go straight into the all-gather SEND
// buffer (row f at send + (f - f0) * Hp * es) and this rank's bias gradients are copied behind them (bias_off_bytes) -- the biases ride on
// the all-gather instead of their own all-reduce, and no copy of the updated rows is needed.  Biases are NOT updated here.
extern "C" int dae_plan_apply_rows_packed(dae_plan* p, int32_t adam_t, float grad_scale, const float* grad_rows, int32_t f0, int32_t f1,
                                          void* send, int64_t bias_off_bytes, void* stream) {
    DAE_CHECK_ARG(!p || !p->x3, "plan_apply_rows_packed: split-bf16 mode has no data-parallel path yet");
    DAE_CHECK_ARG(p && p->bound && grad_rows && send, "plan_apply_rows_packed: plan not bound / null buffer");
    DAE_CHECK_ARG(f0 >= 0 && f0 <= f1 && f1 <= p->Fp && f0 % 64 == 0 && f1 % 64 == 0, "plan_apply_rows_packed: rows [%d, %d) outside [0, %d] or not multiples of 64", f0, f1, p->Fp);
    const float lr = plan_lr(p, adam_t);
    char* lo_base = (char*)send - (int64_t)f0 * p->Hp * p->es;                 // dae_opt_step_rows writes row f at base + f * Hp * es
    RC(dae_opt_step_rows(p->cfg.opt, lr, p->cfg.momentum, grad_scale, p->b.W, grad_rows, p->b.opt_s1, p->b.opt_s2, p->Hp, f0, f1, p->cfg.dtype,
                         lo_base, stream));
    DAE_CHECK_HIP(hipMemcpyAsync((char*)send + bias_off_bytes, p->b.grad + (int64_t)p->Fp * p->Hp, (size_t)(p->Hp + p->Fp) * sizeof(float),
                                 hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// After the all-gather of the packed chunks: W_lo, Wt_lo and the biases of this rank (see dp_unpack_kernel).
extern "C" int dae_plan_dp_unpack(dae_plan* p, const void* recv, int32_t world, int32_t chunk_rows, int64_t chunk_stride_bytes,
                                  int64_t bias_off_bytes, int32_t adam_t, float grad_scale, void* stream) {
    DAE_CHECK_ARG(!p || !p->x3, "plan_dp_unpack: split-bf16 mode has no data-parallel path yet");
    DAE_CHECK_ARG(p && p->bound && recv, "plan_dp_unpack: plan not bound / null buffer");
    const int64_t off = (int64_t)p->Fp * p->Hp;
    return dae_dp_unpack(recv, world, chunk_rows, chunk_stride_bytes, bias_off_bytes, p->Fp, p->Hp, p->cfg.dtype, p->b.W_lo, p->b.Wt_lo, p->cfg.opt,
                         plan_lr(p, adam_t), p->cfg.momentum, grad_scale, p->b.bh, p->b.bv, plan_bias_slot(p, p->b.opt_s1),
                         plan_bias_slot(p, p->b.opt_s2), p->b.grad + off, stream);
}

extern "C" int dae_plan_refresh_wt(dae_plan* p, void* stream) {
    DAE_CHECK_ARG(!p || !p->x3, "plan_refresh_wt: split-bf16 mode has no data-parallel path yet");
    DAE_CHECK_ARG(p && p->bound, "plan_refresh_wt: plan not bound");
    return dae_transpose_shadow(p->b.W_lo, p->Fp, p->Hp, p->cfg.dtype, p->b.Wt_lo, stream);
}
