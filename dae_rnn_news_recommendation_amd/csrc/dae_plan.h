// dae_plan.h -- the training plan (struct dae_plan), its small helpers, the profile-slot timer and the route of one training step (StepRoute):
// what dae_api.hip (plan lifecycle, options, profile, data-parallel entry points) and dae_step.hip (the step driver) share.  Host code only.
#pragma once
#include "dae_kernels.h"

using namespace dae;

// per-kernel HIP-event timing slots of the step driver (bench.py's roofline leg)
enum { PS_MEMSET = 0, PS_GATHER, PS_ENC_GEMM, PS_ENC_FIN, PS_LABEL, PS_GRAM, PS_MINER, PS_TRI_FIN, PS_SYM, PS_DECODE,
       PS_COS_REDUCE, PS_STATS, PS_DH_GEMM, PS_DH_FIN, PS_DW_GEMM, PS_BIAS, PS_OPT, PS_COUNT };

struct dae_plan {
    bool prof;
    hipEvent_t ev0, ev1;
    // profile mode 2 (queued): one event pair per launch taken from this pool, the host never waits between launches; the pairs are read
    // when the pool cannot hold another step and by dae_plan_profile_read -- kernels and steps run back to back as they do un-profiled
    enum { PROF_POOL = 256, PROF_STEP_MAX = 48 };
    bool prof_queued;
    bool prof_stamps;                 // profile mode 3: the pairs carry the dispatches' own begin / end timestamps (DAE_LAUNCH, dae_common.h)
    int pev_used;
    hipEvent_t pev[PROF_POOL];
    int pev_slot[PROF_POOL / 2];
    bool ev_dw_live;                  // ev_dw was recorded by the last dae_train_step (an event that never was recorded does not hold a waiter back)
    hipEvent_t ev_dw;                 // recorded right behind the kernel that completes the W gradient (dae_plan_dw_event): a data-parallel
                                      // caller starts its reduce-scatter from here, beside the step's tail kernel
    bool sym_ride_ok;                 // Gs = a/Nv (G + G^T) computed by rider workgroups of the decode launch instead of its own launch
    bool miner_order_ok;              // dispatch the batch_all workgroups by descending sweep cost (LabelJob::order)
    int32_t* miner_order;
    int32_t* cls_range;               // [1 + 2 Bpm]: sortedness flag + class range of every row (LabelJob::cls), the miner's range fast path
    bool miner_ranges_ok;             // option "miner_ranges" = 0: always compact positives / negatives by ballots
    double prof_ms[PS_COUNT];
    int prof_n[PS_COUNT];
    dae_config cfg;
    dae_buffers b;
    bool bound;
    int F, H, Fp, Hp, Bmax, Bpm;     // Bpm = padded max batch (leading dimension of every [.. x batch] image)
    int es;
    int s_enc, s_dh, s_gram;
    uint64_t ws_bytes;
    // carved pointers
    char *x, *xc, *xct, *h_lo, *h_t, *Gs, *delta2, *delta2_t, *delta1_t, *delta1_lo, *hcat_a, *hcat_b;
    // split-bf16 mode (dae_config.dtype = DAE_BF16X3): every stored operand x of the gradient GEMMs is hi + lo, both bf16; the *_2 images are the lo parts
    bool x3;
    char *W_lo2, *Wt_lo2, *h_t2, *delta2_2, *delta2_t2, *delta1_t2;
    char *x_2, *xct_2, *xc_2;         // ... and of the clean rows x / of x~^T / of x~ (dense input), used when the input values (or the corruption scale) are not exact in bf16
    int s_enc3, s_dh3;               // split-K slice counts of the dense-input encode / dh GEMMs in split-bf16 mode (3 resp. 4-5 K segments)
    // split-bf16 mode, the two lo product terms a CPU replay of the 20-step curve called droppable (tools/precision_study.py --per-term: cost 2.5e-5,
    // triplet 4.4e-5).  Measured on the GPU against the frozen reference curve, dropping them leaves the gate: cost 7.0e-5, triplet 1.56e-4
    // (profiles/r04_precision_terms.txt) -- so both stay ON; the options exist for that measurement (decode 57.9 -> 48.3 us without its term)
    // -> generalised to one bit per lo product term (X3T_* in dae_kernels.h, option "x3_terms"; the legacy options "x3_dec_wlo" / "x3_dh_hlo" flip their bit).
    // bf16 storage: all terms on.  fp16 storage (libdae_hip_f16.so): the two W terms alone (decode (h, W_lo), dh (delta2, W^T_lo)) -- no lo image of
    // delta2 / delta2^T / h / delta1 is written or read (CPU replay of the 20-step curve: cost 1.4e-5, triplet 6.5e-5; profiles/r04_precision_fp16_study.txt)
    uint32_t terms;
    // 16-bit images of the back-propagated operands (delta2, delta2^T, Gs, delta1^T) hold op_scale * value, a power of two the consuming epilogues
    // divide out (dh_finish: 1 / op_scale; the dW epilogue: OptEpi::gin): fp16's normal range ends at 6.1e-5 and delta2 ~ (y - x) / B, Gs ~ 1e-6 sit
    // below it.  1 for bf16 storage and fp32.  Option "op_scale_log2".
    float op_scale;
    int dec_bn;                      // tile width of the decode kernel: decode_tile_n(dtype), or 128 in the 16-bit modes when the 64-column tiles would be more than
                                     // DEC_WIDE_ROUNDS rounds of the chip's 768 slots (option "decode_bn" = 64 | 128 | 0 auto; before dae_plan_bind)
    int dec_bm;                      // option "decode_bm": tile height of the decode kernel, 0 = auto (batch_route: 160 where the 160 x 128 form exists and fits one resident
                                     // round that the 128 x 64 grid does not), 128, 160 (an error where the form does not exist for the plan's mode / loss)
    bool dw_pair_ok;                 // option "dw_pair": split-bf16 dW kernel streams x~^T resp. delta2^T_hi ONCE for the hi and lo image of delta1^T resp. h^T
    bool xct2_clean;
    bool enc_w32_ok;                 // option "encode_w32": bf16 mode encodes from the fp32 MASTER weights (h fp32-accurate); 0 = from W_lo
    int w32_cols;                    // option "encode_w32_cols": 128 (default) or 64 H columns per workgroup of that kernel
    bool gram_split;                 // Gram matrix as a 3-term split-bf16 MFMA GEMM (bf16 mode) instead of exact-fp32 MFMA
    int dw_tr_mode;                  // option "dw_tr": the dW kernel reads x~ and delta2 ROW-MAJOR through transposing LDS reads (gemm_dw_pc<TRA>) -- the decode stores
                                     // delta2 once (no delta2^T), the gathers write x~ instead of x~^T.  1 on, 0 off, -1 (default) = on for DENSE train sets only:
                                     // measured (profiles/r05_ab_measurements.txt) -38 us per step at F = 50000 (the gather and the decode each write 90 MB less),
                                     // but +3..5 us at the CSR shape of c2 (11 fragment-read instructions per k step instead of 6; its decode does not get faster)
    bool gram64_ok;                  // option "gram64" (default 1): the split Gram on 64 x 64 tiles over the whole K, ONE slab (gram64_kernel); 0: 128 x 128 tiles, split-K
    float *slabs, *h_f32, *D_slabs, *G, *rowloss_part, *dbv_part, *colsum_part, *cos_part, *cos_stats, *cw, *loss_part,
        *dw_f32, *tri_scalars, *dh_extra, *rowsq_scratch, *tile_part, *zbuf;
    bool cos_zstore_ok;               // option "cos_zstore" (default 1): the cosine decode's second pass reads the first pass's accumulators back instead of recomputing the GEMM
    uint32_t *cnt_part, *role_cnt, *xc_bits, *x_bits;
    bool xbits_ok;                   // binary CSR + bf16: the decode epilogue reads x as a bit image (option "x_bits" = 0 disables)
    bool xct_clean;                  // x~^T holds only zeros (every step un-scatters what it wrote; see step_tail_kernel)
    bool tail_ok;                    // option "tail" = 0: separate bias_grads / step_stats launches and a full memset per step (A/B)
    bool fuse_opt_ok;                // option "fused_opt" = 0 keeps the separate optimizer kernel (A/B, equivalence tests)
    bool label_enc_ok;               // option "label_with_encode" = 0: label statistics ride on the gather launch / their own
    bool ce_literal;                 // option "ce_literal" = 1: cross_entropy always by the reference-literal formula
    bool sparse_ok;                  // CSR input: fused corrupt + gather + encode on the stored entries (option "encode_sparse" = 0: dense MFMA GEMM)
    bool bits_ok;                    // binary CSR + bf16: x~ handed to the encode GEMM as a bit image (dae_plan_set_option("encode_bits", 0) disables)
    int32_t *dw_i32, *n_same;
    int64_t *nvalid, *dw_i64;
    uint64_t* acc;
};

// lo image of the row-major shadow: exists (and is kept current by every kernel that updates W) only while the decode's (h, W_lo) term is on
static void* plan_w_lo2(const dae_plan* p) { return (p->x3 && (p->terms & X3T_DEC_WLO)) ? (void*)p->W_lo2 : nullptr; }

// tile width the decode launch of this plan uses (see dae_plan::dec_bn); lo images of delta2 / valued x keep the 64-column kernel
static int plan_dec_bn(const dae_plan* p) {
    const int def = decode_tile_n(p->cfg.dtype);
    if (p->es != 2) return def;
    const bool res = p->x3 && (p->terms & (X3T_DH_D2LO | X3T_DW_D2LO | X3T_XV));
    if (res) return def;
    if (p->dec_bn == 64 || p->dec_bn == 128) return p->dec_bn;
    const int64_t tiles64 = (int64_t)(p->Bpm / 128) * (p->Fp / 64);
    return tiles64 > 4 * 768 ? 128 : def;             // F = 50000: 5474 tiles of 128 x 64 = 7.1 rounds of 768 slots -> 2737 wide tiles
}

// does the 160 x 128 decode kernel exist for this plan's mode, terms and loss (x_bits: the clean rows reach the decode as a bit image)?
static bool plan_dec_bm160_form(const dae_plan* p, bool x_bits) {
    const uint32_t T = p->x3 ? p->terms : 0u;
    return decode_bm160_form(p->cfg.dtype, plan_dec_bn(p), x_bits, (T & X3T_DEC_WLO) && (T & X3T_DEC_HLO), (T & (X3T_DH_D2LO | X3T_DW_D2LO | X3T_XV)) != 0,
                             p->cfg.loss_func, p->Fp);
}

#define RC(expr) do { if (int rc__ = (expr)) return rc__; } while (0)

// learning rate handed to the optimizer kernels (Adam: lr_t = lr * sqrt(1-b2^t)/(1-b1^t), TF AdamOptimizer)
static inline float plan_lr(const dae_plan* p, int adam_t) {
    float lr = p->cfg.learning_rate;
    if (p->cfg.opt == DAE_OPT_ADAM) {
        const double t = adam_t < 1 ? 1 : adam_t;
        lr = (float)((double)lr * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
    }
    return lr;
}
// the bias part of an optimizer slot buffer (opt_s1 / opt_s2: laid out like the flat gradient, biases behind the Fp x Hp weights); NULL slot stays NULL
static inline float* plan_bias_slot(const dae_plan* p, float* slot) { return slot ? slot + (int64_t)p->Fp * p->Hp : nullptr; }
// K9 on W (+ biases) with every shadow the plan keeps.  apply: 0 = refresh the shadows only, 1 = apply the flat gradient (biases too), 2 = W alone (the
// step's bias kernel updated the biases); [f0, f1) = a row band of W (default: all of it)
static inline int plan_opt_step(dae_plan* p, float lr, float grad_scale, int apply, void* stream, int f0 = 0, int f1 = -1) {
    return launch_opt_step(p->cfg.opt, lr, apply ? p->cfg.momentum : 0.f, grad_scale, p->b.W, p->b.bh, p->b.bv, p->b.grad, p->b.opt_s1, p->b.opt_s2, p->Fp, p->Hp,
                           p->cfg.dtype, p->b.W_lo, p->b.Wt_lo, plan_w_lo2(p), p->x3 ? p->Wt_lo2 : nullptr, apply, stream, f0, f1);
}

// queued profile modes: wait for the last pair, then add every pair to its slot (dae_api.hip)
int plan_prof_flush(dae_plan* p);
// prof(p, slot, st, call): in profile mode time `call` (a callable that enqueues launches on `st` and returns their status) with HIP events ON THE STEP'S
// STREAM and accumulate the elapsed GPU time of that slot (dae_plan_profile, include/dae_hip.h).  Mode 1: an event pair around the call and a host wait
// behind it.  Mode 2 (queued): a pair of the plan's pool around the call, read later by plan_prof_flush.  Mode 3 (stamped): the pool is handed to
// DAE_LAUNCH (dae_common.h) for the duration of the call, every kernel launch inside takes a pair and has it stamped by its own dispatch; memsets
// keep the mode-2 form.
template <class Call>
static int prof(dae_plan* p, int slot, hipStream_t st, Call&& call) {
    const bool queued = p->prof && p->prof_queued && p->pev_used + 2 <= dae_plan::PROF_POOL;
    const bool stamped = queued && p->prof_stamps && slot != PS_MEMSET;
    if (stamped) g_lt = LaunchTimer{p->pev, &p->pev_used, p->pev_slot, dae_plan::PROF_POOL, slot, true};
    else if (queued) DAE_CHECK_HIP(hipEventRecord(p->pev[p->pev_used], st));
    else if (p->prof) DAE_CHECK_HIP(hipEventRecord(p->ev0, st));
    const int rc = call();
    if (stamped) g_lt.pool = nullptr;
    if (rc || stamped) return rc;                       // stamped: the launches took their pairs
    if (queued) {
        DAE_CHECK_HIP(hipEventRecord(p->pev[p->pev_used + 1], st));
        p->pev_slot[p->pev_used / 2] = slot | 0x100; p->pev_used += 2;
    } else if (p->prof) {
        DAE_CHECK_HIP(hipEventRecord(p->ev1, st));
        DAE_CHECK_HIP(hipEventSynchronize(p->ev1));
        float ms = 0.f;
        DAE_CHECK_HIP(hipEventElapsedTime(&ms, p->ev0, p->ev1));
        p->prof_ms[slot] += ms; p->prof_n[slot] += 1;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// route of one training step: every decision the driver makes before its first launch (dae_step.hip: step_route)
// ------------------------------------------------------------------------------------------------
enum EncPath {
    ENC_RESUME,       // phase 5: h and the side images are those of the preceding phase-4 call
    ENC_SPARSE,       // CSR input: corrupt + gather + encode in one launch on the stored entries (tf.sparse.matmul, autoencoder.py:377,389); the dense x~ image
                      // is never formed
    ENC_X3_GEMM,      // split mode, dense input: z1 = x~ W as (x~_hi, W^T_hi) (x~_hi, W^T_lo) (x~_lo, W^T_hi), three K segments
    ENC_BITS_GEMM,    // binary CSR, unit scale, bf16: the corrupted batch goes to the encode GEMM as a BIT image (1.1 MB, not 18 MB of bf16)
    ENC_GEMM          // gather x~, one dense MFMA GEMM
};
// how the rows of one batch are encoded: decided by encode_route for the training step and for dae_encode_rows alike
struct EncodeRoute {
    EncPath path;
    bool w32;         // ENC_SPARSE reads the fp32 MASTER weights (a sharded-optimizer exchange turns the option off: only W_lo is current on every rank)
    int splits;       // split-K slice count of the encode GEMM (ENC_X3_GEMM: the 3-segment plan's)
};
// where the label statistics (cw, N_valid, data weights) of the step are produced: they depend on the labels alone
enum LabelPath {
    LABEL_CALLER,     // externally mined step: the caller wrote them
    LABEL_EXPLICIT,   // explicit triplets: every one of the 3*Bt stacked rows carries weight 1/(Bt + 1e-16), three unweighted row means (:303-305)
    LABEL_ENCODE,     // offered to the encode launch, which carries them when its grid leaves a CU free (else their own launch)
    LABEL_GATHER,     // ride on the CSR gather launch
    LABEL_OWN         // their own launch
};
enum DwForm {
    DW_FUSED_OPT,     // phase 0 / 3 in bf16 mode: the optimizer runs in the dW GEMM's epilogue (phase 3 does not materialise the W gradient)
    DW_PC_GRAD,       // phase 1 / 5 (data parallel) in bf16 mode: the same kernel in its gradient-only form when the shape fits it
                      // (split-bf16 mode: the gradient-only form of the same N-segment kernel, fp32 gradient to the flat buffer)
    DW_GEMM           // the segment GEMM writes the fp32 gradient to the flat buffer, the optimizer is its own launch
};
// What the two halves of an externally mined step (phases 4 and 5) must decide alike: computed by batch_route from the plan, the shapes, the inputs
// and the phase CLASS (backward / apply_now / ext_mine, equal for 4 and 5) -- batch_route never sees dae_step::phase.
struct BatchRoute {
    int B, Bp;
    int Bk;                     // contractions over the BATCH (dW's K, the Gs.h segment of dh) stop at the last 64-deep K tile that holds a real row: the
                                // images are zero beyond B, and B = 800 pads to 896 = 14 K tiles of which 13 hold data
    // ---- input
    bool csr_in;                // the rows to encode are CSR (the train set or an explicitly corrupted copy)
    bool dense_in;              // ... a dense train set
    bool copy_in;               // an explicitly corrupted CSR copy of the train set (salt&pepper, host-side noise): dae_step::c_indptr
    bool src_binary;
    // ---- encode path (of the half that encodes)
    EncodeRoute enc;
    // ---- clean rows: how they reach the decode epilogue
    bool use_xbits;             // binary CSR train set in bf16 mode: as a bit image (1.1 MB, not 18 MB)
    bool own_clean;             // the encode launch also emits the clean-row images, unless their LDS rows do not fit (e.g. 50000 features)
    bool x2_clean;              // the clean rows get a lo image (valued CSR / dense train set)
    // ---- label statistics
    LabelPath label;
    // ---- split-mode terms
    bool x3;
    uint32_t T;                 // lo product terms that are multiplied (X3T_*)
    bool x3_vals;               // split-bf16 mode with VALUED input (tf-idf, salt-and-pepper copies, decay noise's scale factor): x~ = scale * v is not exact in
                                // bf16, so x~^T and the clean rows x get lo images too (xct_2, x_2) and the dW contraction walks 6 segments; binary data with
                                // a bf16-exact scale (masking noise: 1.0) needs neither
    float osc, oinv;            // operand scale of the 16-bit delta images (a power of two) and its inverse
    // ---- mining
    bool explicit3;
    bool mined;                 // batch_all / batch_hard mined by this library (Gram, miner, Gs)
    bool fold_finalize;         // batch_all over all valid triplets: scale comes from label_stats, sums from step_stats (no triplet_finalize launch)
    bool sym_ride;              // the decode launch also scales G + G^T (sym_scale)
    // ---- decode
    int dbn;                    // tile width
    int dbm;                    // tile height: 128, or 160 (gemm_decode_loss_160; lays out dbv_part / tile_part, see DecodeEpi::bm)
    bool is_cos;
    bool zstore;                // cosine: the second pass reads the first pass's accumulators back
    // ---- dh
    int s_dh;                   // its slice count
    // ---- dW
    DwForm dw;
    bool dw_tr;                 // Transposed-A dW (gemm_dw_pc<TRA>): x~ and delta2 are consumed ROW-MAJOR [batch x feature], so delta2^T is never stored and the
                                // gathers write x~ (the CSR scatter lands in one 20 KB row per batch row instead of one line per entry).  Needs the 160 x 128
                                // kernel and the two plain K segments (16-bit modes without lo images of x~ / delta2 / delta1 / h in dW: f16x2, bf16, f16)
    // ---- tail
    bool tail;                  // bias gradients + statistics + x~^T un-scatter in one launch
    bool stats_in_tail;         // the step statistics ride on the step-tail launch after the dW GEMM
    bool fuse_bias;             // single-GPU step: the bias update rides on the bias-gradient kernel
};
struct StepRoute : BatchRoute {
    // ---- phase.  Phases 4 / 5 split the step around an EXTERNAL miner (data parallel with global-batch mining, dp.GlobalMiner): phase 4
    // stops after the encode (h_f32 / h_lo / h_t and the side images stay in the workspace); the caller mines over the
    // all-gathered batch and writes the row weights (cw), the triplet scalars and d(triplet)/dh (dh_extra) into the plan's
    // buffers; phase 5 resumes at the decode and ends like phase 1 (gradients in the flat buffer).
    bool backward, apply_now, ext_mine;   // the phase class
    bool h_only, resume;                  // which half of an externally mined step
    bool grad_out;                        // the fused dW + optimizer kernel also stores the W gradient (phase 3 does not materialise it)
    bool own_opt;                         // the optimizer is its own launch behind the tail (K9): neither a gradient-only phase nor fused into dW
    // x~^T: the CSR gather only scatters kept entries, so the image must be zero beforehand.  The step tail un-scatters
    // exactly what was written, so the 18 MB memset runs once (or after a failed / foreign step); the dense gather
    // overwrites whole tiles and never needs it.  (dae_plan::xct_clean / xct2_clean, read here; the input stage and the tail update them)
    bool clear_xct, clear_xct2;
};
