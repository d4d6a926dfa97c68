// dae_step.hip -- the whole-step driver: dae_train_step enqueues one DAE training step (DenoisingAutoencoder._run_train_step's per-batch body,
// autoencoder.py:223-245) as a fixed sequence of HIP kernels on one stream, with no host sync.  step_route decides ONCE which launches the step
// takes (StepRoute, dae_plan.h); the stages below issue them and decide nothing.  dae_encode_rows runs the step's encode stage alone.
#include "dae_plan.h"

// ------------------------------------------------------------------------------------------------
// the route
// ------------------------------------------------------------------------------------------------
// Encode path of a batch.  csr / dense: form of the rows to encode; bits_src: they are rows of a binary CSR matrix that is not corrupted beforehand.
static EncodeRoute encode_route(const dae_plan& p, bool csr, bool dense, bool bits_src, float scale) {
    EncodeRoute e;
    e.w32 = p.enc_w32_ok && p.cfg.dtype == DAE_BF16;
    if (csr && p.sparse_ok) e.path = ENC_SPARSE;
    else if (p.x3 && dense) e.path = ENC_X3_GEMM;
    else if (p.bits_ok && bits_src && scale == 1.0f) e.path = ENC_BITS_GEMM;
    else e.path = ENC_GEMM;
    e.splits = e.path == ENC_X3_GEMM ? p.s_enc3 : p.s_enc;
    return e;
}

// the three things of dae_step::phase that decisions outside the phase part may depend on; phases 4 and 5 have the same class
struct PhaseClass { bool backward, apply_now, ext_mine; };
static PhaseClass phase_class(int phase) { return {phase != 2, phase == 0 || phase == 3, phase == 4 || phase == 5}; }

// Everything decided from plan state, shapes, inputs and the phase class alone, so that the phase-4 / phase-5 halves of an externally mined step agree.
static BatchRoute batch_route(const dae_plan& p, const PhaseClass& k, int B, const int64_t* c_indptr, const float* c_values, float scale) {
    const dae_config& c = p.cfg;
    const int Fp = p.Fp, Hp = p.Hp, dt = c.dtype;
    BatchRoute r;
    memset(&r, 0, sizeof(r));
    r.B = B; r.Bp = (int)pad128(B); r.Bk = (B + 63) / 64 * 64;
    r.copy_in = c_indptr != nullptr;
    r.csr_in = c_indptr || p.b.indptr;
    r.dense_in = !r.csr_in && p.b.dense;
    r.src_binary = c_indptr ? !c_values : (p.b.indptr && !p.b.values);
    r.enc = encode_route(p, r.csr_in, r.dense_in, !c_indptr && p.b.indptr && !p.b.values, scale);
    const bool use_sparse = r.enc.path == ENC_SPARSE;
    r.use_xbits = p.xbits_ok && p.b.indptr && !p.b.values;
    r.own_clean = use_sparse && !c_indptr && r.use_xbits && encode_csr_lds_bytes(dt, r.enc.w32, p.w32_cols, Fp / 32) <= 64 * 1024;
    r.x3 = p.x3;
    r.T = p.x3 ? p.terms : 0u;
    r.x2_clean = p.x3 && (r.T & X3T_XV) && !r.use_xbits && (p.b.values || p.b.dense);
    if (p.x3) {
        uint32_t u; memcpy(&u, &scale, 4);
        r.x3_vals = (r.T & X3T_XV) && (!r.src_binary || (u & 0xffffu) != 0u || (p.b.indptr && p.b.values) || r.dense_in);
    }
    r.osc = p.es == 2 ? p.op_scale : 1.f; r.oinv = 1.f / r.osc;
    // label statistics: on the encode GEMM's launch when that grid leaves a CU free (else on the CSR gather's, else their own)
    r.explicit3 = c.triplet == 3;
    const bool label_with_encode = p.tail_ok && !r.explicit3 && !k.ext_mine && r.Bp <= 1024 && p.label_enc_ok;
    const bool label_in_gather = p.tail_ok && !label_with_encode && !r.explicit3 && !k.ext_mine && !c_indptr && p.b.indptr && r.Bp <= 1024;
    r.label = k.ext_mine ? LABEL_CALLER : r.explicit3 ? LABEL_EXPLICIT : label_with_encode ? LABEL_ENCODE : (label_in_gather && !use_sparse) ? LABEL_GATHER : LABEL_OWN;
    r.mined = !k.ext_mine && (c.triplet == DAE_TRIPLET_BATCH_ALL || c.triplet == DAE_TRIPLET_BATCH_HARD);
    r.fold_finalize = (c.triplet == DAE_TRIPLET_BATCH_ALL && !c.pos_triplets_only) && !k.ext_mine;
    r.sym_ride = r.mined && k.backward && p.sym_ride_ok;
    r.dbn = plan_dec_bn(&p);
    // 160 x 128 tiles: forced by option "decode_bm" (the launcher refuses where the form does not exist), or where the form exists and the grid is one
    // resident round that the 128 x 64 grid is not (B = 800: 474 tiles on 512 slots instead of 1106 on 768)
    r.dbm = (p.dec_bm == 160 || (p.dec_bm == 0 && plan_dec_bm160_form(&p, r.use_xbits) && decode_bm160_one_round(r.Bp, Fp))) ? 160 : 128;
    r.is_cos = c.loss_func == DAE_LOSS_COSINE;
    r.zstore = r.is_cos && k.backward && p.cos_zstore_ok && p.zbuf;
    r.s_dh = (p.x3 && r.dense_in) ? p.s_dh3 : p.s_dh;
    // split-bf16 mode: the fused dW + optimizer kernel exists for shapes of at most one 160 x 128 tile per CU; larger shapes (and the
    // data-parallel gradient-only phases) take the N-segment dW GEMM to memory + the optimizer kernel that writes all four shadows
    const bool fuse_opt = k.backward && k.apply_now && dt == DAE_BF16 && p.fuse_opt_ok && (!p.x3 || dw_x3_fits(Fp, Hp, r.Bp));
    const bool dw_pc_grad = k.backward && !k.apply_now && dt == DAE_BF16 && p.fuse_opt_ok && (p.x3 ? dw_x3_fits(Fp, Hp, r.Bp) : dw_grad_fits(Fp, Hp, r.Bp));
    r.dw = fuse_opt ? DW_FUSED_OPT : dw_pc_grad ? DW_PC_GRAD : DW_GEMM;
    const bool dw_plain2 = !p.x3 || !(r.T & (X3T_DW_D1LO | X3T_DW_HLO | X3T_DW_D2LO | X3T_XV));
    r.dw_tr = (p.dw_tr_mode == 1 || (p.dw_tr_mode < 0 && r.dense_in)) && dt == DAE_BF16 && k.backward && (fuse_opt || dw_pc_grad) && dw_plain2 &&
              (use_sparse || r.dense_in) && (p.x3 || dw_pc_taken(Fp, Hp, r.Bk, r.Bk, !fuse_opt));
    r.tail = p.tail_ok;
    r.stats_in_tail = k.backward && r.tail;
    r.fuse_bias = k.apply_now;
    return r;
}

// The route of one step.  No HIP call, nothing written to the plan.  One quantity stays a stage result: whether the encode launch actually carried
// the label block (LABEL_ENCODE is an offer; the launcher reports at launch time whether its grid left a CU free, see stage_encode).
static StepRoute step_route(const dae_plan& p, const dae_step& s) {
    const PhaseClass k = phase_class(s.phase);
    StepRoute r;
    memset(&r, 0, sizeof(r));
    static_cast<BatchRoute&>(r) = batch_route(p, k, s.B, s.c_indptr, s.c_values, s.scale);
    r.backward = k.backward; r.apply_now = k.apply_now; r.ext_mine = k.ext_mine;
    r.h_only = s.phase == 4; r.resume = s.phase == 5;
    r.grad_out = s.phase != 3;
    r.own_opt = !(s.phase == 1 || s.phase == 5 || r.dw == DW_FUSED_OPT);
    if (r.resume) r.enc.path = ENC_RESUME;
    const bool clear = !r.resume && r.backward && r.csr_in;
    r.clear_xct = clear && !(r.tail && p.xct_clean);
    r.clear_xct2 = clear && r.x3_vals && !(r.tail && p.xct2_clean);
    return r;
}

// ------------------------------------------------------------------------------------------------
// input images and encode (shared by the training step and dae_encode_rows)
// ------------------------------------------------------------------------------------------------
static int memset_async(void* ptr, size_t bytes, hipStream_t st) {
    DAE_CHECK_HIP(hipMemsetAsync(ptr, 0, bytes, st));
    return 0;
}
struct RowSrc {                  // a CSR matrix or a dense one, and the rows of it that make the batch
    const int64_t* indptr; const int32_t* indices; const float* values; const float* dense; int64_t ld_dense; const int32_t* row_idx;
};
// how a gather corrupts and scales the rows it reads (dae_step: corr_mode, keep_bits, seed, rng_stream, corr_frac, scale)
struct Corrupt { int mode; const uint32_t* keep_bits; uint64_t seed; uint32_t rng_stream; float frac, scale; };
static const Corrupt kNoCorrupt = {DAE_CORR_NONE, nullptr, 0, 0, 0.f, 1.f};

static int gather_batch(dae_plan* p, const RowSrc& r, int B, void* x, void* xc, void* xct, float* rowsq, const Corrupt& k, void* stream,
                        uint32_t* xc_bits = nullptr, const LabelJob* label_job = nullptr, uint32_t* x_bits = nullptr, void* x2 = nullptr) {
    if (r.indptr)
        return launch_gather_csr(r.indptr, r.indices, r.values, r.row_idx, B, p->F, p->cfg.dtype, x, xc, p->Fp, xct, p->Bpm, rowsq, k.mode,
                                 k.keep_bits, k.seed, k.rng_stream, k.frac, k.scale, xc_bits, p->Fp / 32, label_job, (hipStream_t)stream, x_bits, x2);
    DAE_CHECK_ARG(r.dense, "step: no train set bound");
    return dae_gather_dense(r.dense, r.ld_dense, r.row_idx, B, p->F, p->cfg.dtype, x, xc, p->Fp, xct, p->Bpm, rowsq, p->rowsq_scratch,
                            k.mode, k.keep_bits, k.seed, k.rng_stream, k.frac, k.scale, stream);
}
// split-bf16 mode, dense input: the lo images of x / x~ / x~^T (a second pass over the fp32 rows with the same keep decisions)
static int gather_dense_lo(dae_plan* p, const RowSrc& r, int B, void* x2, void* xc2, void* xct2, const Corrupt& k, void* stream) {
    return launch_gather_dense(r.dense, r.ld_dense, r.row_idx, B, p->F, p->cfg.dtype, x2, xc2, p->Fp, xct2, p->Bpm, nullptr, nullptr, k.mode, k.keep_bits,
                               k.seed, k.rng_stream, k.frac, k.scale, stream, 1);
}

// One encode: the rows, how they are corrupted, and the images wanted besides h_f32 (NULL = not written).
struct EncodeJob {
    RowSrc src;                  // the rows to encode
    const RowSrc* clean;         // src is an explicitly corrupted copy: the train set rows the clean images are gathered from (NULL: from src itself)
    int B;
    Corrupt corr;                // corruption and scale of src
    void *h_lo, *h_t, *hcat_a, *hcat_b, *h_t2;           // images of h (hcat_*: the Gram operands)
    void* x; uint32_t* x_bits; void* x_2; float* rowsq;  // the clean rows for the decode epilogue: dense or as a bit image, lo image, row squares
    void *xct, *xct_2; int64_t ldt; int xct_rm;          // x~^T and its lo image for dW (xct_rm: row-major x~ instead, EncCsrLaunch::xct_rm)
    const LabelJob* label_enc;   // label statistics offered to the encode launch ...
    const LabelJob* label_gather;   // ... or riding on the gather launch (at most one of the two)
    bool own_clean;              // ENC_SPARSE: the encode launch itself writes x_bits / rowsq
    bool timed;                  // charge the launches to the plan's profile slots
};

// ENC_SPARSE.  The clean rows reach the decode epilogue as a bit image written by the same launch (binary data) or as a dense tile from
// the gather kernel (valued data / explicitly corrupted copy).
template <class Run>
static int encode_sparse(dae_plan* p, const EncodeRoute& er, const EncodeJob& j, hipStream_t st, Run&& run) {
    const RowSrc& cs = j.clean ? *j.clean : j.src;
    if (!j.own_clean && (j.x || j.x_bits))
        RC(run(PS_GATHER, [&] { return gather_batch(p, cs, j.B, j.x, nullptr, nullptr, j.rowsq, kNoCorrupt, st, nullptr, nullptr, j.x_bits, cs.values ? j.x_2 : nullptr); }));
    // a DENSE train set with an explicitly corrupted CSR copy (salt-and-pepper): the clean rows' lo image comes from the dense rows
    if (!j.own_clean && j.x_2 && cs.dense && !cs.indptr)
        RC(run(PS_GATHER, [&] { return gather_dense_lo(p, cs, j.B, j.x_2, nullptr, nullptr, kNoCorrupt, st); }));
    EncCsrLaunch q;
    memset(&q, 0, sizeof(q));
    q.indptr = j.src.indptr; q.indices = j.src.indices; q.values = j.src.values; q.row_idx = j.src.row_idx; q.B = j.B; q.F = p->F; q.H = p->H; q.dtype = p->cfg.dtype;
    q.W = er.w32 ? (const void*)p->b.W : (const void*)p->b.W_lo; q.w_f32 = er.w32 ? 1 : 0; q.w32_cols = p->w32_cols; q.ldw = p->Hp; q.bh = p->b.bh; q.enc_act = p->cfg.enc_act;
    q.corr_mode = j.corr.mode; q.keep_bits = j.corr.keep_bits; q.seed = j.corr.seed; q.rng_stream = j.corr.rng_stream;
    q.corr_frac = j.corr.frac; q.scale = j.corr.scale;
    q.h_f32 = p->h_f32; q.h_lo = j.h_lo; q.ldh = p->Hp; q.h_t = j.h_t; q.ldht = j.h_t ? p->Bpm : 0;
    q.hcat_a = j.hcat_a; q.hcat_b = j.hcat_b;
    q.x_bits = j.own_clean ? j.x_bits : nullptr; q.ldxb = (j.x || j.x_bits) ? p->Fp / 32 : 0; q.xct = j.xct; q.ldt = j.ldt;
    q.xct_rm = j.xct_rm;
    q.rowsq = j.own_clean ? j.rowsq : nullptr;
    q.h_t2 = j.h_t2;
    q.xct2 = j.xct_2;
    q.label_job = j.label_enc;
    return run(PS_ENC_GEMM, [&] { return launch_encode_csr(q, st); });
}

// The GEMM paths: gather x~ (and the clean rows), the encode GEMM into split-K slabs, encode_finish.  *enc_label_done: the GEMM launch carried j.label_enc.
template <class Run>
static int encode_gemm(dae_plan* p, const EncodeRoute& er, const EncodeJob& j, hipStream_t st, int* enc_label_done, Run&& run) {
    const int Bp = (int)pad128(j.B), Fp = p->Fp, Hp = p->Hp, dt = p->cfg.dtype;
    const uint32_t T = p->x3 ? p->terms : 0u;
    const bool use_bits = er.path == ENC_BITS_GEMM;
    if (j.clean) {               // the clean rows from the train set, x~ from the copy (corrupted already: its scale alone applies)
        const Corrupt scale_only = {DAE_CORR_NONE, nullptr, 0, 0, 0.f, j.corr.scale};
        RC(run(PS_GATHER, [&] { return gather_batch(p, *j.clean, j.B, j.x, nullptr, nullptr, j.rowsq, kNoCorrupt, st, nullptr, nullptr, j.x_bits); }));
        RC(run(PS_GATHER, [&] { return gather_batch(p, j.src, j.B, nullptr, p->xc, j.xct, nullptr, scale_only, st); }));
    } else {
        RC(run(PS_GATHER, [&] { return gather_batch(p, j.src, j.B, j.x, use_bits ? nullptr : p->xc, j.xct_rm ? nullptr : j.xct, j.rowsq, j.corr, st,
                                                    use_bits ? p->xc_bits : nullptr, j.label_gather, j.x_bits); }));
    }
    void* xc_2 = (er.path == ENC_X3_GEMM && (T & X3T_ENC_XLO)) ? p->xc_2 : nullptr;
    if (er.path == ENC_X3_GEMM && (j.x_2 || xc_2))
        RC(run(PS_GATHER, [&] { return gather_dense_lo(p, j.src, j.B, j.x_2, xc_2, j.xct_2, j.corr, st); }));
    const int64_t slab = (int64_t)Bp * Hp;
    int* done = j.label_enc ? enc_label_done : nullptr;
    if (er.path == ENC_X3_GEMM) {
        const GemmSegDesc es3[3] = {{p->xc, Fp, p->b.Wt_lo, Fp, Fp}, {p->xc, Fp, p->Wt_lo2, Fp, (T & X3T_ENC_WLO) ? Fp : 0},
                                    {p->xc_2, Fp, p->b.Wt_lo, Fp, (T & X3T_ENC_XLO) ? Fp : 0}};
        RC(run(PS_ENC_GEMM, [&] { return launch_gemm_f32out_n(dt, Bp, Hp, es3, 3, p->slabs, Hp, er.splits, slab, st, GEMM_ROLE_ENCODE, j.label_enc, done); }));
    } else if (use_bits) {
        RC(run(PS_ENC_GEMM, [&] { return launch_encode_bits(Bp, Hp, Fp, p->xc_bits, Fp / 32, p->b.Wt_lo, Fp, p->slabs, Hp, er.splits, slab, st, j.label_enc, done); }));
    } else {
        RC(run(PS_ENC_GEMM, [&] { return launch_gemm_f32out(dt, Bp, Hp, p->xc, Fp, p->b.Wt_lo, Fp, Fp, nullptr, 0, nullptr, 0, 0, p->slabs, Hp, er.splits, slab, st,
                                                            GEMM_ROLE_ENCODE, j.label_enc, done); }));
    }
    return run(PS_ENC_FIN, [&] { return launch_encode_finish(p->slabs, er.splits, slab, Hp, p->b.bh, j.B, p->H, p->cfg.enc_act, dt, p->h_f32, j.h_lo, Hp,
                                                             j.h_t, j.h_t ? p->Bpm : 0, j.hcat_a, j.hcat_b, j.h_t2, st); });
}

// h_f32 (and the images the job names) of the batch.  *label_done: a launch of this stage carried the job's label statistics.
static int stage_encode(dae_plan* p, const EncodeRoute& er, const EncodeJob& j, hipStream_t st, bool* label_done) {
    auto run = [&](int slot, auto&& call) { return j.timed ? prof(p, slot, st, call) : call(); };
    int enc_label_done = 0;
    if (er.path == ENC_SPARSE) {
        RC(encode_sparse(p, er, j, st, run));
        *label_done = j.label_enc != nullptr;          // the fused launch always has room for the label block
    } else {
        RC(encode_gemm(p, er, j, st, &enc_label_done, run));
        *label_done = j.label_gather || enc_label_done;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the stages of a training step: each issues the launches its part of the route names
// ------------------------------------------------------------------------------------------------
#define PROF(slot, expr) RC(prof(p, (slot), st, [&] { return (expr); }))

static LabelJob label_job(const dae_plan* p, const dae_step* s, const StepRoute& r) {
    return LabelJob{s->labels, r.B, r.Bp, p->cfg.triplet, p->nvalid, p->dw_i64, p->cw, p->cfg.alpha, p->tri_scalars, p->miner_order_ok ? p->miner_order : nullptr,
                    p->miner_ranges_ok ? p->cls_range : nullptr};
}

// 1-4. corrupt + gather + encode (K0-K2)
static int stage_input_encode(dae_plan* p, const dae_step* s, const StepRoute& r, hipStream_t st, bool* labels_done) {
    if (r.clear_xct) PROF(PS_MEMSET, memset_async(p->xct, (size_t)p->Fp * p->Bpm * p->es, st));
    if (r.clear_xct2) PROF(PS_MEMSET, memset_async(p->xct_2, (size_t)p->Fp * p->Bpm * 2, st));
    if (r.backward) { p->xct_clean = false; if (r.x3_vals) p->xct2_clean = false; }
    *labels_done = r.label == LABEL_CALLER;          // produced by the caller
    if (r.resume) return 0;
    const LabelJob lj = label_job(p, s, r);
    const RowSrc train = {p->b.indptr, p->b.indices, p->b.values, p->b.dense, p->b.ld_dense, s->row_idx};
    const RowSrc copy = {s->c_indptr, s->c_indices, s->c_values, nullptr, 0, s->c_row_idx ? s->c_row_idx : s->row_idx};
    const bool have_ht2 = r.T & (X3T_DH_HLO | X3T_DW_HLO);
    EncodeJob j;
    memset(&j, 0, sizeof(j));
    j.src = r.copy_in ? copy : train; j.clean = r.copy_in ? &train : nullptr; j.B = r.B;
    j.corr = Corrupt{r.copy_in ? DAE_CORR_NONE : s->corr_mode, s->keep_bits, s->seed, s->rng_stream, s->corr_frac, s->scale};
    j.h_lo = p->h_lo; j.h_t = p->h_t; j.hcat_a = p->gram_split ? p->hcat_a : nullptr; j.hcat_b = p->gram_split ? p->hcat_b : nullptr;
    j.h_t2 = have_ht2 ? p->h_t2 : nullptr;
    j.x = r.use_xbits ? nullptr : p->x; j.x_bits = r.use_xbits ? p->x_bits : nullptr; j.x_2 = r.x2_clean ? p->x_2 : nullptr;
    j.rowsq = r.is_cos ? p->cos_stats : nullptr;
    j.xct = r.backward ? p->xct : nullptr; j.xct_2 = (r.x3_vals && r.backward) ? p->xct_2 : nullptr;
    j.ldt = r.dw_tr ? p->Fp : p->Bpm; j.xct_rm = r.dw_tr ? 1 : 0;
    j.label_enc = r.label == LABEL_ENCODE ? &lj : nullptr; j.label_gather = r.label == LABEL_GATHER ? &lj : nullptr;
    j.own_clean = r.own_clean; j.timed = true;
    return stage_encode(p, r.enc, j, st, labels_done);
}

// 5-6. miners (K5-K7).  K5: D = h h^T (triplet_loss_utils.py:93,219).  fp32 mode: exact-fp32 MFMA.  bf16 mode: split-bf16 (h = hi + lo,
// three bf16 MFMA products concatenated along K = 3*Hp), ~2^-17 relative error, 16x the MFMA rate.
static int launch_gram(dae_plan* p, int Bp, int Hp, int64_t dslab, hipStream_t st) {
    if (p->gram_split && p->gram64_ok && p->s_gram == 1) return launch_gram64(p->hcat_a, p->hcat_b, Bp, Hp, p->D_slabs, st);
    if (p->gram_split)
        return launch_gemm_f32out(DAE_BF16, Bp, Bp, p->hcat_a, 3 * Hp, p->hcat_b, 3 * Hp, 3 * Hp, nullptr, 0, nullptr, 0, 0, p->D_slabs, Bp,
                                  p->s_gram, dslab, st, GEMM_ROLE_GRAM);
    return launch_gemm_f32out(DAE_F32, Bp, Bp, p->h_f32, Hp, p->h_f32, Hp, Hp, nullptr, 0, nullptr, 0, 0, p->D_slabs, Bp, p->s_gram, dslab, st,
                              GEMM_ROLE_GRAM);
}
static int stage_miners(dae_plan* p, const dae_step* s, const StepRoute& r, hipStream_t st, bool labels_done) {
    const dae_config& c = p->cfg;
    const int B = r.B, Bp = r.Bp, dt = c.dtype;
    void* stream = st;
    if (r.label == LABEL_EXPLICIT) {
        const int Bt = B / 3;
        PROF(PS_LABEL, dae_label_stats(nullptr, Bt, Bp, DAE_TRIPLET_NONE, nullptr, nullptr, nullptr, nullptr, p->cw, 0.f, nullptr, stream));
        DAE_CHECK_HIP(hipMemcpyAsync(p->cw + Bt, p->cw, (size_t)Bt * 4, hipMemcpyDeviceToDevice, st));
        DAE_CHECK_HIP(hipMemcpyAsync(p->cw + 2 * Bt, p->cw, (size_t)Bt * 4, hipMemcpyDeviceToDevice, st));
        PROF(PS_MINER, dae_explicit_triplet(p->h_f32, p->Hp, Bt, p->H, c.alpha, p->dh_extra, p->loss_part, p->tri_scalars, stream));
    } else if (!labels_done) {
        PROF(PS_LABEL, dae_label_stats(s->labels, B, Bp, c.triplet, p->n_same, p->acc, p->nvalid, p->dw_i64, p->cw, c.alpha, p->tri_scalars, stream));
    }
    if (!r.mined) return 0;
    const int64_t dslab = (int64_t)Bp * Bp;
    // the label block of this step's encode launch also ranked the anchors by sweep cost (only then is the buffer current)
    const int32_t* order = (labels_done && p->miner_order_ok && c.triplet == DAE_TRIPLET_BATCH_ALL) ? p->miner_order : nullptr;
    const int32_t* cls = (labels_done && p->miner_ranges_ok && c.triplet == DAE_TRIPLET_BATCH_ALL) ? p->cls_range : nullptr;
    PROF(PS_GRAM, launch_gram(p, Bp, p->Hp, dslab, st));
    if (c.triplet == DAE_TRIPLET_BATCH_ALL)
        PROF(PS_MINER, launch_batch_all(p->D_slabs, p->s_gram, dslab, Bp, s->labels, B, Bp, 0, B,
                                 (c.pos_triplets_only ? DAE_MINER_POS_ONLY : 0) | (dt == DAE_BF16 ? DAE_MINER_FAST : 0), p->loss_part,
                                 p->cnt_part, p->G, p->role_cnt, order, st, cls));
    else
        PROF(PS_MINER, dae_triplet_batch_hard(p->D_slabs, p->s_gram, dslab, Bp, s->labels, B, Bp, p->loss_part, p->cnt_part, p->dw_i32, p->G,
                                  stream));
    if (!r.fold_finalize)
        PROF(PS_TRI_FIN, dae_triplet_finalize(c.triplet, c.pos_triplets_only, B, Bp, c.alpha, p->loss_part, p->cnt_part, p->nvalid,
                                p->dw_i32, p->role_cnt, p->dw_f32, p->cw, p->tri_scalars, stream));
    if (r.backward && !r.sym_ride) PROF(PS_SYM, launch_sym_scale(p->G, B, Bp, p->tri_scalars, dt, p->Gs, r.osc, st));
    return 0;
}

// 7. decode + reconstruction loss + d cost/d z2   (K3/K4); `sym_ride`: the launch also scales G + G^T (sym_scale)
static int stage_decode(dae_plan* p, const dae_step*, const StepRoute& r, hipStream_t st) {
    const dae_config& c = p->cfg;
    const int B = r.B, Bp = r.Bp, Fp = p->Fp, Hp = p->Hp, dt = c.dtype;
    const uint32_t T = r.T;
    const bool backward = r.backward;
    DecodeEpi e;
    memset(&e, 0, sizeof(e));
    e.bv = p->b.bv; e.x = p->x; e.ldx = Fp; e.x_bits = r.use_xbits ? p->x_bits : nullptr; e.ldxb = Fp / 32; e.cw = p->cw; e.cos_stats = r.is_cos ? p->cos_stats : nullptr;
    e.rowloss_part = r.is_cos ? p->rowloss_part : nullptr; e.tile_part = r.is_cos ? nullptr : p->tile_part;
    e.dbv_part = backward ? p->dbv_part : nullptr; e.cos_part = p->cos_part;
    e.delta2 = backward ? p->delta2 : nullptr; e.ldd = Fp; e.delta2_t = (backward && !r.dw_tr) ? p->delta2_t : nullptr; e.lddt = p->Bpm;
    e.B = B; e.F = p->F; e.Bp = Bp; e.Fp = Fp; e.dec_act = c.dec_act; e.loss_func = c.loss_func; e.ce_literal = p->ce_literal ? 1 : 0;
    e.op_scale = r.osc; e.bn = r.dbn; e.bm = r.dbm;
    if (r.sym_ride) { e.sym_G = p->G; e.sym_scalars = p->tri_scalars; e.sym_Gs = p->Gs; e.sym_B = B; e.sym_Bp = Bp; }
    // z2 = h W^T: one K segment, or -- split-bf16 -- (h_hi, W_hi) (h_hi, W_lo) (h_lo, W_hi); the row-major h_hi / h_lo are the first and
    // third block of the Gram operand hcat_a = [hi | hi | lo] (leading dimension 3 Hp)
    GemmSegDesc dsegs[3] = {{p->h_lo, Hp, p->b.W_lo, Hp, Hp}, {nullptr, 0, nullptr, 0, 0}, {nullptr, 0, nullptr, 0, 0}};
    int ndseg = 1;
    if (r.x3) {
        dsegs[0] = {p->hcat_a, 3 * (int64_t)Hp, p->b.W_lo, Hp, Hp};
        dsegs[1] = {p->hcat_a, 3 * (int64_t)Hp, p->W_lo2, Hp, (T & X3T_DEC_WLO) ? Hp : 0};      // K = 0: the term is dropped
        dsegs[2] = {p->hcat_a + (size_t)2 * Hp * 2, 3 * (int64_t)Hp, p->b.W_lo, Hp, (T & X3T_DEC_HLO) ? Hp : 0};
        ndseg = 3;
        if (backward) { e.delta2_2 = (T & X3T_DH_D2LO) ? p->delta2_2 : nullptr; e.delta2_t2 = (T & X3T_DW_D2LO) ? p->delta2_t2 : nullptr; }
        if (r.x2_clean) e.x2 = p->x_2;    // valued clean rows: x = hi + lo (RES instantiations)
    }
    if (!r.is_cos) {
        e.cos_pass = 0;
        PROF(PS_DECODE, launch_decode_loss_n(dt, Bp, Fp, dsegs, ndseg, e, st));
        return 0;
    }
    e.cos_pass = 1;
    if (r.zstore) { e.z_io = p->zbuf; e.ldz = Fp; e.z_mode = 1; }
    PROF(PS_DECODE, launch_decode_loss_n(dt, Bp, Fp, dsegs, ndseg, e, st));
    if (r.zstore) e.z_mode = 2;
    PROF(PS_COS_REDUCE, dae_cos_reduce(p->cos_part, 2 * Fp / r.dbn, B, Bp, p->cos_stats, p->rowloss_part, (void*)st));
    e.sym_G = nullptr;                                 // the first pass carried the rider
    if (backward) { e.cos_pass = 2; PROF(PS_DECODE, launch_decode_loss_n(dt, Bp, Fp, dsegs, ndseg, e, st)); }
    return 0;
}

// 8. statistics of this step (autoencoder.py:233 fetch list): their own launch, or a rider of the step tail
static StatsArgs stats_args(const dae_plan* p, const dae_step* s, const StepRoute& r) {
    const dae_config& c = p->cfg;
    return StatsArgs{r.is_cos ? p->rowloss_part : nullptr, 1, r.is_cos ? nullptr : p->tile_part, r.dbm == 160 ? ((r.Bp + 159) / 160) * (p->Fp / 128) : (r.Bp / 128) * (p->Fp / r.dbn), p->cw, r.B, r.Bp,
                     c.triplet == 3 ? DAE_TRIPLET_BATCH_HARD : c.triplet, c.alpha, p->tri_scalars,
                     (c.triplet == DAE_TRIPLET_BATCH_ALL && !r.ext_mine) ? p->nvalid : nullptr, s->stats, r.fold_finalize ? p->loss_part : nullptr,
                     r.fold_finalize ? p->cnt_part : nullptr};
}
static int stage_stats(dae_plan* p, const dae_step* s, const StepRoute& r, hipStream_t st) {
    const StatsArgs sa = stats_args(p, s, r);
    PROF(PS_STATS, dae_step_stats(sa.rowloss_part, sa.n_col_waves, sa.tile_part, sa.n_tiles, sa.cw, r.B, r.Bp, sa.triplet, sa.alpha, sa.tri_scalars,
                                  sa.nvalid, sa.loss_part, sa.cnt_part, s->stats, (void*)st));
    return 0;
}

// 9-10. dL/dh = delta2 W + alpha (G+G^T) h ; delta1                     (K8)
static int stage_dh(dae_plan* p, const dae_step*, const StepRoute& r, hipStream_t st) {
    const int B = r.B, Bp = r.Bp, Fp = p->Fp, Hp = p->Hp, ldB = p->Bpm, dt = p->cfg.dtype, Bk = r.Bk;
    const uint32_t T = r.T;
    const bool mined = r.mined;
    const int64_t slab = (int64_t)Bp * Hp;
    if (r.x3) {     // (d2_hi, Wt_hi) (d2_hi, Wt_lo) (d2_lo, Wt_hi) + Gs.h_hi (+ Gs.h_lo with option x3_dh_hlo): Gs itself stays bf16 (tools/precision_study.py)
        const GemmSegDesc hs[5] = {{p->delta2, Fp, p->b.Wt_lo, Fp, Fp}, {p->delta2, Fp, p->Wt_lo2, Fp, (T & X3T_DH_WLO) ? Fp : 0},
                                   {p->delta2_2, Fp, p->b.Wt_lo, Fp, (T & X3T_DH_D2LO) ? Fp : 0},
                                   {p->Gs, Bp, p->h_t, ldB, mined ? Bk : 0}, {p->Gs, Bp, p->h_t2, ldB, (mined && (T & X3T_DH_HLO)) ? Bk : 0}};
        PROF(PS_DH_GEMM, launch_gemm_f32out_n(dt, Bp, Hp, hs, 5, p->slabs, Hp, r.s_dh, slab, st, GEMM_ROLE_DH, nullptr, nullptr, 1.f, B));
    } else {
        PROF(PS_DH_GEMM, launch_gemm_f32out(dt, Bp, Hp, p->delta2, Fp, p->b.Wt_lo, Fp, Fp, mined ? p->Gs : nullptr, Bp, mined ? p->h_t : nullptr, ldB,
                              mined ? Bk : 0, p->slabs, Hp, r.s_dh, slab, st, GEMM_ROLE_DH, nullptr, nullptr, B));
    }
    PROF(PS_DH_FIN, launch_dh_finish(p->slabs, r.s_dh, slab, Hp, (r.explicit3 || r.ext_mine) ? p->dh_extra : nullptr, p->h_f32, Hp, p->b.bh, B, p->H, p->cfg.enc_act, dt,
                     p->delta1_t, ldB, p->colsum_part, nullptr, nullptr, st, (T & X3T_DW_D1LO) ? p->delta1_t2 : nullptr, r.oinv, r.osc));
    return 0;
}

// 11. dW = x~^T delta1 + delta2^T h                                      (K8, tied weights)
static int stage_dw(dae_plan* p, const dae_step* s, const StepRoute& r, hipStream_t st) {
    const dae_config& c = p->cfg;
    const int Fp = p->Fp, Hp = p->Hp, ldB = p->Bpm, dt = c.dtype, Bk = r.Bk;
    const uint32_t T = r.T;
    // the segment table (K = 0 segments are skipped; the launches without lo images take segments 0 and 3): the third one exists only when x~^T has a lo image
    // (dw_tr: the A operands are the row-major images -- x~ from the CSR scatter (p->xct used as [Bp x Fp]) or the dense gather (p->xc), and delta2)
    const void* a_x = r.dw_tr ? (const void*)(r.dense_in ? p->xc : p->xct) : (const void*)p->xct;
    const void* a_d2 = r.dw_tr ? (const void*)p->delta2 : (const void*)p->delta2_t;
    const int64_t lda_w = r.dw_tr ? Fp : ldB;
    const GemmSegDesc ws[6] = {{a_x, lda_w, p->delta1_t, ldB, Bk}, {p->xct, ldB, p->delta1_t2, ldB, (T & X3T_DW_D1LO) ? Bk : 0},
                               {p->xct_2, ldB, p->delta1_t, ldB, r.x3_vals ? Bk : 0},
                               {a_d2, lda_w, p->h_t, ldB, Bk}, {p->delta2_t, ldB, p->h_t2, ldB, (T & X3T_DW_HLO) ? Bk : 0},
                               {p->delta2_t2, ldB, p->h_t, ldB, (T & X3T_DW_D2LO) ? Bk : 0}};
    if (r.dw != DW_GEMM) {
        OptEpi oe;
        memset(&oe, 0, sizeof(oe));
        oe.ldw = Hp; oe.ldwt = Fp; oe.gin = r.oinv;
        if (r.dw == DW_FUSED_OPT) {
            oe.W = p->b.W; oe.grad = r.grad_out ? p->b.grad : nullptr; oe.s1 = p->b.opt_s1; oe.s2 = p->b.opt_s2;
            oe.W_lo = p->b.W_lo; oe.Wt_lo = p->b.Wt_lo; oe.opt = c.opt; oe.lr = plan_lr(p, s->adam_t);
            oe.mom = c.momentum; oe.gscale = s->grad_scale;
        } else {                                     // data parallel: gradient to memory (fp32 flat buffer, or the bf16 exchange image)
            oe.opt = DW_OPT_GRAD_ONLY; oe.grad = p->b.grad_lo ? nullptr : p->b.grad; oe.grad_lo = p->b.grad_lo;
        }
        if (r.x3) {   // x~^T.(d1_hi + d1_lo) + (d2^T_hi, h^T_hi) (d2^T_hi, h^T_lo) (d2^T_lo, h^T_hi); the epilogue writes both parts of both shadows
            oe.W_lo2 = (T & X3T_DEC_WLO) ? p->W_lo2 : nullptr; oe.Wt_lo2 = p->Wt_lo2;     // W_lo2 feeds the decode's (h_hi, W_lo) term only
            PROF(PS_DW_GEMM, launch_dw_opt_n(Fp, Hp, ws, 6, oe, st, p->dw_pair_ok, r.dw_tr));
        } else {
            PROF(PS_DW_GEMM, launch_dw_opt(Fp, Hp, ws[0].A, ws[0].lda, ws[0].Bt, ws[0].ldb, Bk, ws[3].A, ws[3].lda, ws[3].Bt, ws[3].ldb, Bk, oe, st, r.dw_tr));
        }
    } else if (r.x3) {
        PROF(PS_DW_GEMM, launch_gemm_f32out_n(dt, Fp, Hp, ws, 6, p->b.grad, Hp, 1, 0, st, GEMM_ROLE_DW, nullptr, nullptr, r.oinv));
    } else {
        const GemmSegDesc ws2[2] = {ws[0], ws[3]};
        PROF(PS_DW_GEMM, launch_gemm_f32out_n(dt, Fp, Hp, ws2, 2, p->b.grad, Hp, 1, 0, st, GEMM_ROLE_DW, nullptr, nullptr, r.oinv));
        // data parallel with a bf16 exchange image: the shape did not fit the kernel that writes it directly
        if (!r.apply_now && dt == DAE_BF16 && p->b.grad_lo) RC(launch_cast_bf16(p->b.grad, p->b.grad_lo, (int64_t)Fp * Hp, st));
    }
    p->ev_dw_live = false;
    if (p->ev_dw) { DAE_CHECK_HIP(hipEventRecord(p->ev_dw, st)); p->ev_dw_live = true; }      // the W gradient (grad / grad_lo) is complete from here on
    return 0;
}

// 12-13. bias gradients (with the statistics and the x~^T un-scatter when the step has a tail), then the optimizer (K9): W (+ shadows); the bias
// kernel updated the biases
static int stage_tail(dae_plan* p, const dae_step* s, const StepRoute& r, hipStream_t st) {
    const dae_config& c = p->cfg;
    const int B = r.B, Bp = r.Bp, F = p->F, H = p->H, Fp = p->Fp, Hp = p->Hp;
    float* g_bh = p->b.grad + (int64_t)Fp * Hp;
    const BiasArgs ba{p->dbv_part, r.dbm == 160 ? (Bp + 159) / 160 : 2 * Bp / 128, p->colsum_part, Bp / 32, p->b.bh, H, Hp, F, Fp, c.enc_act, g_bh, g_bh + Hp,
                      r.fuse_bias ? 1 : 0, c.opt, plan_lr(p, s->adam_t), c.momentum, s->grad_scale, p->b.bv,
                      plan_bias_slot(p, p->b.opt_s1), plan_bias_slot(p, p->b.opt_s2)};
    if (r.tail) {
        const StatsArgs sa = stats_args(p, s, r);
        const ClearArgs ca{s->c_indptr ? s->c_indptr : p->b.indptr, s->c_indptr ? s->c_indices : p->b.indices,
                           (s->c_indptr && s->c_row_idx) ? s->c_row_idx : s->row_idx, B, F, p->xct, r.dw_tr ? (int64_t)Fp : (int64_t)p->Bpm, p->es,
                           r.x3_vals ? p->xct_2 : nullptr, r.dw_tr ? 1 : 0};
        PROF(PS_BIAS, launch_step_tail(ba, &sa, r.csr_in ? &ca : nullptr, st));
        if (r.csr_in) { p->xct_clean = true; if (r.x3_vals) p->xct2_clean = true; }
    } else {
        PROF(PS_BIAS, dae_bias_grads(ba.dbv_part, ba.n_row_waves, ba.colsum_part, ba.n_row_blocks, ba.bh, ba.H, ba.Hp, ba.F, ba.Fp, ba.enc_act, ba.dbh, ba.dbv,
                                     ba.apply, ba.opt, ba.lr, ba.mom, ba.gscale, ba.bv, ba.s1b, ba.s2b, (void*)st));
    }
    if (r.own_opt) PROF(PS_OPT, plan_opt_step(p, plan_lr(p, s->adam_t), s->grad_scale, /*apply=*/2, (void*)st));
    return 0;
}

static int train_step_body(dae_plan* p, const dae_step* s, void* stream) {
    DAE_CHECK_ARG(p && p->bound && s, "train_step: plan not bound / null step");
    DAE_CHECK_ARG(s->row_idx && s->B > 0 && s->B <= p->Bmax, "train_step: batch %d outside (0, %d]", s ? s->B : -1, p->Bmax);
    const dae_config& c = p->cfg;
    const bool explicit3 = (c.triplet == 3);
    DAE_CHECK_ARG(c.triplet == DAE_TRIPLET_NONE || explicit3 || s->labels, "train_step: labels required for triplet mining");
    DAE_CHECK_ARG(!explicit3 || s->B % 3 == 0, "train_step: explicit-triplet batch must stack org/pos/neg (B %% 3 == 0)");
    DAE_CHECK_ARG(s->stats, "train_step: stats pointer required");
    const StepRoute r = step_route(*p, *s);
    if (r.x3) {
        // split-bf16 mode: CSR input encoded from the fp32 master weights (h is fp32-accurate and its hi / lo images come from the same
        // launch); x~ must be exact in bf16 (binary data, or values with <= 8 significant bits).  Every phase: the data-parallel
        // exchange of this mode moves fp32 gradients and fp32 master rows (dp.ShardedExchange), so the master is current on every rank
        // (h from the 16-bit hi image of W alone was measured in round 6, profiles/r06_ab_measurements.txt: the same 26.8 us -- the kernel is not bound by its
        //  W-row bytes -- and the triplet leg of c2 leaves the gate at step 5 (1.5e-3): refused, not offered)
        DAE_CHECK_ARG((r.csr_in && p->sparse_ok && p->enc_w32_ok) || r.dense_in, "train_step: split-bf16 mode needs the fp32-master sparse encode (CSR input) or a dense train set");
        DAE_CHECK_ARG(!p->b.grad_lo, "train_step: split-bf16 mode exchanges fp32 gradients (no bf16 gradient image)");
    }
    hipStream_t st = (hipStream_t)stream;
    bool labels_done = false;        // label statistics already produced by a workgroup of an earlier launch (or by the caller)
    RC(stage_input_encode(p, s, r, st, &labels_done));
    if (r.h_only) return 0;
    if (!r.ext_mine) RC(stage_miners(p, s, r, st, labels_done));
    RC(stage_decode(p, s, r, st));
    if (!r.stats_in_tail) RC(stage_stats(p, s, r, st));
    if (!r.backward) return 0;
    RC(stage_dh(p, s, r, st));
    RC(stage_dw(p, s, r, st));
    return stage_tail(p, s, r, st);
}
#undef PROF

extern "C" int dae_train_step(dae_plan* p, const dae_step* s, void* stream) {
    const int rc = train_step_body(p, s, stream);
    if (p && p->prof_queued && p->pev_used + dae_plan::PROF_STEP_MAX > dae_plan::PROF_POOL) { const int rf = plan_prof_flush(p); return rc ? rc : rf; }
    return rc;
}

extern "C" int dae_encode_rows(dae_plan* p, const int32_t* row_idx, int32_t B, float scale, const int64_t* indptr,
                               const int32_t* indices, const float* values, const float* dense, int64_t ld_dense, float* out,
                               int64_t ld_out, void* stream) {
    DAE_CHECK_ARG(p && p->bound && row_idx && out, "encode_rows: bad arguments");
    DAE_CHECK_ARG(B > 0 && B <= p->Bmax, "encode_rows: batch %d outside (0, %d]", B, p->Bmax);
    DAE_CHECK_ARG((indptr != nullptr) != (dense != nullptr), "encode_rows: give either a CSR or a dense matrix");
    hipStream_t st = (hipStream_t)stream;
    // only h_f32 is wanted: no image of h, of the clean rows or of x~^T, no label job, no corruption, nothing charged to the profile slots
    EncodeJob j;
    memset(&j, 0, sizeof(j));
    j.src = RowSrc{indptr, indices, values, dense, ld_dense, row_idx}; j.B = B;
    j.corr = Corrupt{DAE_CORR_NONE, nullptr, 0, 0, 0.f, scale};
    bool label_done = false;
    RC(stage_encode(p, encode_route(*p, indptr != nullptr, dense != nullptr, indptr && !values, scale), j, st, &label_done));
    DAE_CHECK_HIP(hipMemcpy2DAsync(out, (size_t)ld_out * 4, p->h_f32, (size_t)p->Hp * 4, (size_t)p->H * 4, B, hipMemcpyDeviceToDevice, st));
    return 0;
}
