/*
 * dae_hip.h -- C ABI of libdae_hip.so: the MI355X (gfx950) implementation of the DAE
 * article-embedding training hot path of louislung/DAE_RNN_News_Recommendation.
 *
 * The reference has NO native/FFI boundary (100 % Python on TensorFlow 1.12): the hot path is
 * whatever `tf_session.run([train_step, ...])` executes per mini-batch.  This header therefore
 * defines the boundary a maintainer would bind with ctypes from the reference's own Python
 * (see INTEGRATION.md).  Each entry point cites the reference code it replaces; paths are
 * relative to the reference repo root.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - every function returns 0 on success, non-zero on error (message via dae_last_error());
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *     stream-ordered, nothing synchronises the host;
 *   - dense activations use one element type per call: DAE_BF16 (MFMA bf16, fp32 accumulate)
 *     or DAE_F32 (exact-fp32 MFMA, the parity mode); parameters / gradients / statistics are fp32;
 *   - "padded" sizes: every dense row/column extent is rounded up to a multiple of DAE_PAD (128)
 *     and the padding is kept EXACTLY ZERO by every kernel (see DESIGN.md "HBM layout").
 */
#ifndef DAE_HIP_H
#define DAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAE_PAD 128
#define DAE_ABI_VERSION 9   /* still 9 with dae_user_pair_loss / dae_user_pair_loss_workspace, dae_user_states and dae_topk_similarity_ex / dae_topk_similarity_ex_workspace: they are new symbols only (no struct or signature of version 9 changed), which a caller detects by symbol lookup (dlsym); 9: dae_pair_hist / dae_pair_hist_workspace / dae_pair_hist_max_bins (label AUROC and pair statistics from fused per-class score histograms); 8: dae_threshold_pairs / dae_threshold_pairs_workspace (near-duplicate search: all pairs over a threshold); 7: dae_topk_similarity / dae_topk_similarity_workspace (fused similarity + top-k retrieval); 6:dae_comm_* / dae_allreduce_grads / dae_dp_exchange / dae_dp_bands (the data-parallel collective in the C ABI, RCCL on the step's stream); 5: dae_storage_format (the fp16 build libdae_hip_f16.so), options x3_terms / op_scale_log2, DAE_WAIT_DW_CREATED = 100; 4: DAE_BF16X3 (split-bf16 mode), dae_gemm_nt_n; 3: dae_buffers.grad_lo, option encode_w32 (and one since removed); 2: dae_step.c_row_idx, plan options, phases 4/5, sharded apply */

enum { DAE_BF16 = 0, DAE_F32 = 1,
       DAE_BF16X3 = 2 /* dae_config.dtype only: bf16 storage and MFMA, but every stored operand of the three gradient GEMMs is kept as
                         hi + lo (both bf16) and multiplied as (hi,hi) + (hi,lo) + (lo,hi) -- 2^-16 operands at ~3x the bf16 GEMM work;
                         every input kind and phase.  In the fp16 build of the library (dae_storage_format() == 1) the same dtype keeps only the
                         lo terms of plan option "x3_terms" -- by default the two W terms -- i.e. TWO products per gradient GEMM: the product's
                         precision='f16x2' */ };
enum { DAE_ACT_NONE = 0, DAE_ACT_SIGMOID = 1, DAE_ACT_TANH = 2 };
enum { DAE_LOSS_CROSS_ENTROPY = 0, DAE_LOSS_MEAN_SQUARED = 1, DAE_LOSS_COSINE = 2 };
enum { DAE_OPT_SGD = 0, DAE_OPT_ADAGRAD = 1, DAE_OPT_MOMENTUM = 2, DAE_OPT_ADAM = 3 };
enum { DAE_TRIPLET_NONE = 0, DAE_TRIPLET_BATCH_ALL = 1, DAE_TRIPLET_BATCH_HARD = 2,
       DAE_TRIPLET_EXPLICIT = 3 /* DenoisingAutoencoderTriplet: rows stacked [org; pos; neg] */ };
enum { DAE_CORR_NONE = 0, DAE_CORR_KEEPBITS = 1, DAE_CORR_PHILOX_MASK = 2 };
/* `mode` bits of dae_triplet_batch_all */
enum { DAE_MINER_POS_ONLY = 1, DAE_MINER_FAST = 2 };

/* slots of the per-step statistics record (float[DAE_STATS_STRIDE]) -- the values the reference
 * fetches at autoencoder.py:233 and averages per epoch at :283-294 */
enum { DAE_STAT_COST = 0, DAE_STAT_AE = 1, DAE_STAT_TRIPLET = 2, DAE_STAT_FRACTION = 3,
       DAE_STAT_NUM = 4, DAE_STAT_NVALID = 5, DAE_STATS_STRIDE = 8 };

int         dae_abi_version(void);
const char* dae_last_error(void);
/* padded extent: ceil(n / DAE_PAD) * DAE_PAD */
int64_t     dae_pad(int64_t n);

/* ---------------------------------------------------------------------------------------------
 * K0+K1 (front half): corrupt + CSR-row -> dense tile gather, staged through LDS.
 * Replaces utils.masking_noise (utils.py:94-115), the per-batch CSR fancy-index
 * (utils.py:59-60), get_sparse_ind_val_shape (utils.py:162-180) and tf.sparse.to_dense
 * (triplet_loss_utils.py:264).
 *   rows  i = 0..B-1 take CSR row row_idx[i];  columns are the CSR's (sorted) column ids.
 *   x      [Bp x ldx]  clean rows (target of the reconstruction loss)          (may be NULL)
 *   xc     [Bp x ldx]  corrupted rows  x~ = scale * keep(e) * value(e)         (may be NULL)
 *   xct    [Fp x ldt]  transpose of xc (A operand of the dW GEMM)              (may be NULL;
 *                      must be zero-filled by the caller, only kept entries are written)
 *   rowsq  [Bp] fp32   sum of squares of each clean row (cosine_proximity)     (may be NULL)
 *   corr_mode: DAE_CORR_NONE      -> keep everything
 *              DAE_CORR_KEEPBITS  -> keep entry e iff bit e of keep_bits (reference-exact stream
 *                                    np.random.rand(nnz) >= v, generated on the host)
 *              DAE_CORR_PHILOX_MASK -> keep iff philox_uniform(e; seed, stream) >= corr_frac
 *   values == NULL means a binary matrix (all stored values 1.0; main_autoencoder.py:235).
 * ------------------------------------------------------------------------------------------- */
int dae_gather_csr(const int64_t* indptr, const int32_t* indices, const float* values,
                   const int32_t* row_idx, int32_t B, int32_t F, int32_t dtype,
                   void* x, void* xc, int64_t ldx, void* xct, int64_t ldt, float* rowsq,
                   int32_t corr_mode, const uint32_t* keep_bits, uint64_t seed, uint32_t rng_stream,
                   float corr_frac, float scale, void* stream);

/* Same kernel, additionally emitting the corrupted batch as a BIT image for dae_encode_bits:
 *   xc_bits [Bp x ldw] u32, bit b of word w of row i  <=>  entry (i, 32*w + b) of x~ is kept (value 1.0).
 * Only for binary matrices (values == NULL) with scale == 1; rows >= B and columns >= F are zero.
 * xc may then be NULL (the dense x~ image is not needed by the encode GEMM). */
int dae_gather_csr_bits(const int64_t* indptr, const int32_t* indices, const float* values,
                        const int32_t* row_idx, int32_t B, int32_t F, int32_t dtype,
                        void* x, void* xc, int64_t ldx, void* xct, int64_t ldt, float* rowsq,
                        int32_t corr_mode, const uint32_t* keep_bits, uint64_t seed, uint32_t rng_stream,
                        float corr_frac, float scale, uint32_t* xc_bits, int64_t ldw, void* stream);

/* K1 for binary inputs: fused corrupt+encode GEMM  slab[s] = bits(x~) . Wt_lo^T  over K range s
 * (autoencoder.py:389 tf.sparse.matmul(sparse x~, W); the reference multiplies the 0/1 CSR directly).
 * The A operand is the bit image and is expanded to bf16 MFMA fragments inside LDS; only W^T is streamed.
 * bf16 only.  Bp, Hp multiples of 128; Fp multiple of 64; slabs as for dae_gemm_nt. */
int dae_encode_bits(const uint32_t* xc_bits, int64_t ldw, const void* Wt_lo, int64_t ldwt,
                    int32_t Bp, int32_t Hp, int32_t Fp, float* slabs, int64_t ld_slab,
                    int32_t splits, int64_t slab_stride, void* stream);

/* K0+K1+K2 for CSR inputs in ONE launch: corrupt + gather + encode on the stored entries -- the reference's own
 * formulation, tf.sparse.matmul(x~, W) + b_h -> activation -> - act(b_h) (autoencoder.py:377,389):
 *     h[i,:] = act( sum_{e in row_idx[i], kept(e)} scale * v_e * W_lo[col_e, :] + bh ) - act(bh)
 * The dense x~ image is never formed (a row holds ~2 % of the features): the kernel reads ~140 W rows per batch row and is
 * bound by L2 -> register bandwidth, not by MFMA.  W_lo: [Fp x ldw] row-major in `dtype` (the bf16 shadow, or fp32 in parity
 * mode); fp32 accumulation in stored-entry order.  Outputs (any may be NULL): h_f32 / h_lo [Bp x ldh], h_t [Hp x ldht],
 * hcat_a / hcat_b split-bf16 Gram operands [Bp x 3Hp]; side images of the batch: x_bits [Bp x ldxb] (bit image of the CLEAN
 * rows, binary data only), xct [Fp x ldt] (kept entries scattered into the pre-zeroed x~^T), rowsq [Bp] (sum of squares of
 * the clean row).  Corruption arguments as for dae_gather_csr. */
int dae_encode_csr(const int64_t* indptr, const int32_t* indices, const float* values, const int32_t* row_idx,
                   int32_t B, int32_t F, int32_t H, int32_t dtype, const void* W_lo, int64_t ldw, const float* bh,
                   int32_t enc_act, int32_t corr_mode, const uint32_t* keep_bits, uint64_t seed, uint32_t rng_stream,
                   float corr_frac, float scale, float* h_f32, void* h_lo, int64_t ldh, void* h_t, int64_t ldht,
                   void* hcat_a, void* hcat_b, uint32_t* x_bits, int64_t ldxb, void* xct, int64_t ldt, float* rowsq,
                   void* stream);

/* Salt-and-pepper corruption of a mini-batch ON THE DEVICE (utils.salt_and_pepper_noise, utils.py:118-144, with a counter
 * RNG instead of the host stream): for batch row i (train-set row row_idx[i]) `v` column ids are drawn with replacement,
 * col_t = floor(u * F), and each is set to `lo` (coin < 0.5) or `hi`; later draws win.  (u, coin) = the first two words of
 * Philox4x32-10 at counter (row_idx[i], t, rng_stream, 1), key = seed -- restated by oracle.salt_and_pepper_philox.
 * Output: a batch-local CSR with a fixed row capacity `cap` (>= longest row + v): row i occupies out_indices / out_values
 * [i*cap, i*cap + len_i), sorted by column, zeros dropped; out_span[2i], out_span[2i+1] = its start and end, so the arrays
 * serve as (c_indptr = out_span, c_row_idx[i] = 2i) of dae_train_step. */
int dae_salt_pepper_batch(const int64_t* indptr, const int32_t* indices, const float* values, const int32_t* row_idx,
                          int32_t B, int32_t F, int32_t v, float lo, float hi, uint64_t seed, uint32_t rng_stream,
                          int64_t* out_span, int32_t* out_indices, float* out_values, int32_t cap, void* stream);

/* Reference-exact masking noise on the HOST, continuing NumPy's legacy global stream natively (autoencoder/utils.py:111
 * `np.random.rand(nnz) >= v`; dense input utils.py:108 `np.random.choice([0,1], size, p=[v,1-v])` consumes the same doubles):
 * key[624] / *pos are the ('MT19937', key, pos, ...) fields of np.random.get_state(); n doubles are drawn (2 words each, a>>5
 * and b>>6 as randomkit does) and bit e of bits_out (little-endian uint32 words, (n+31)/32 of them) = (double_e >= corr_frac),
 * decided by an exact integer comparison.  key / *pos come back advanced: np.random.set_state with them continues the stream as
 * if NumPy had drawn the n doubles.  HOST pointers; no stream; thread-safe for distinct states.  Returns 0, or 1 on bad input. */
int dae_host_mt19937_keep_bits(uint32_t* key, int32_t* pos, int64_t n, double corr_frac, uint32_t* bits_out);

/* Dense-ndarray input (autoencoder.py:143 sparse_input=False; utils.py:107-109 dense masking):
 * gathers fp32 rows data[row_idx[i], :] into x / xc / xct (ldx, ldt multiples of 128; x / xc / xct 16-byte aligned) with the
 * keep decision from keep_bits (DAE_CORR_KEEPBITS) or from Philox (DAE_CORR_PHILOX_MASK): element (row, f) is kept iff word
 * f & 3 of Philox4x32-10 at counter (f >> 2, row, rng_stream, 2), key = seed, scaled to [0, 1) by (w >> 8) * 2^-24, is
 * >= corr_frac -- one draw per four neighbouring features (restated by oracle.philox_uniform_dense). */
int dae_gather_dense(const float* data, int64_t ld_data, const int32_t* row_idx, int32_t B, int32_t F,
                     int32_t dtype, void* x, void* xc, int64_t ldx, void* xct, int64_t ldt, float* rowsq,
                     float* rowsq_scratch /* [(Fp/64) x Bp], needed iff rowsq */,
                     int32_t corr_mode, const uint32_t* keep_bits /* bit index = row*F + f */,
                     uint64_t seed, uint32_t rng_stream, float corr_frac, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Generic NT GEMM on MFMA tiles:  C[M x N] (+)= sum_seg A_seg[M x K_seg] * Bt_seg[N x K_seg]^T
 * fp32 accumulate, fp32 output; up to two K segments (tied-weight gradient, triplet term).
 * M, N multiples of 128, K_seg multiples of 64 (bf16) / 32 (fp32); lda/ldb/ldc in ELEMENTS.
 * splits > 1 writes `splits` partial slabs C + s*slab_stride (consumer sums them).
 * This is tf.matmul / tf.sparse.matmul of the reference graph (autoencoder.py:389,411;
 * triplet_loss_utils.py:93,219) and of its autodiff (autoencoder.py:452-472).
 * ------------------------------------------------------------------------------------------- */
int dae_gemm_nt(int32_t dtype, int32_t M, int32_t N,
                const void* A0, int64_t lda0, const void* Bt0, int64_t ldb0, int32_t K0,
                const void* A1, int64_t lda1, const void* Bt1, int64_t ldb1, int32_t K1,
                float* C, int64_t ldc, int32_t splits, int64_t slab_stride, void* stream);

/* The same contraction over 1..5 K segments: C = sum_s A_s[M x K_s] . Bt_s[N x K_s]^T.  Split-bf16 operands (x = hi + lo, both bf16)
 * multiply as (hi,hi) + (hi,lo) + (lo,hi): three segments per product, the lo.lo term (2^-16 of a 2^-8 term) is dropped.  Segments with
 * K = 0 are skipped.  Same tiles, split-K slabs and kernels as dae_gemm_nt. */
typedef struct dae_gemm_seg { const void* A; int64_t lda; const void* Bt; int64_t ldb; int32_t K; } dae_gemm_seg;
int dae_gemm_nt_n(int32_t dtype, int32_t M, int32_t N, const dae_gemm_seg* segs, int32_t nsegs, float* C, int64_t ldc,
                  int32_t splits, int64_t slab_stride, void* stream);

/* Diagnostic twin of dae_gemm_nt (bf16, LDS-DMA ring depth nst = 2 or 3): same arithmetic, and every wave also writes
 * shader-clock sums of its K-loop phases to trace[(block*4 + wave)*8 + k]:
 *   k=0 first MFMA half (+DMA issue)  1 waits (vmcnt/lgkmcnt)  2 barrier  3 reads + second MFMA half + DMA issue  4 K iterations
 *   5 whole K loop  6 epilogue stores  7 s_memtime at entry.    Used by tools/gemm_trace.py; not on the training path. */
int dae_gemm_trace(int32_t dtype, int32_t M, int32_t N, const void* A0, int64_t lda0, const void* Bt0, int64_t ldb0,
                   int32_t K0, const void* A1, int64_t lda1, const void* Bt1, int64_t ldb1, int32_t K1, float* C,
                   int64_t ldc, int32_t splits, int64_t slab_stride, int32_t nst, uint64_t* trace, void* stream);

/* K2: encode epilogue  h = act(sum_s slab_s + bh) - act(bh)   (autoencoder.py:389)
 * writes h fp32 [Bp x ldh], h in `dtype` [Bp x ldh] and h^T in `dtype` [Hp x ldht]; rows >= B
 * and columns >= H are written as zero.  Any output pointer may be NULL.
 * hcat_a / hcat_b (both or neither): bf16 [Bp x 3*Hp] = [hi|hi|lo] and [hi|lo|hi] with h = hi + lo, the
 * operands of the split-bf16 Gram matrix  D ~= hcat_a . hcat_b^T  (one dae_gemm_nt call with K = 3*Hp). */
int dae_encode_finish(const float* slabs, int32_t splits, int64_t slab_stride, int64_t ld_slab,
                      const float* bh, int32_t B, int32_t H, int32_t enc_act, int32_t dtype,
                      float* h_f32, void* h_lo, int64_t ldh, void* h_t, int64_t ldht,
                      void* hcat_a, void* hcat_b, void* stream);

/* K3+K4 (+ seeds of K8): decode GEMM fused with bias, activation, per-row reconstruction loss
 * and d cost / d z2   (autoencoder.py:411; triplet_loss_utils.py:262-277 weighted_loss).
 *   y = act(h W^T + bv);  rowloss_i = sum_f loss(x_if, y_if);
 *   delta2_if = cw_i * dloss/dy * act'(z2)      with cw_i = w_i / (sum w + 1e-16)
 * outputs: rowloss_part [n_col_waves x Bp] partial row sums (n_col_waves = 2*Fp/dae_decode_tile_n(dtype); may be NULL),
 *          tile_part [(Bp/128)*(Fp/dae_decode_tile_n(dtype))] each tile's share of sum_i cw_i * rowloss_i (may be NULL),
 *          dbv_part [n_row_waves x Fp] partial column sums of delta2 (n_row_waves = 2*Bp/128),
 *          delta2 [Bp x ldd] and delta2^T [Fp x lddt] in `dtype` (any of these may be NULL).
 * cosine_proximity needs whole-row statistics and runs as two passes over the same GEMM:
 *   cos_pass 1: cos_stats[0..Bp) = sum x^2 (from the gather) is read, cos_part
 *               [2 x n_col_waves x Bp] receives partial {sum y^2, sum xhat.y};
 *   dae_cos_reduce folds them into cos_stats[Bp..3Bp) and the row loss;
 *   cos_pass 2: produces delta2 / delta2^T / dbv_part.   Other losses: cos_pass = 0. */
int dae_decode_loss(int32_t dtype, int32_t B, int32_t F, int32_t H,
                    const void* h_lo, int64_t ldh, const void* W_lo, int64_t ldw,
                    const float* bv, const void* x, int64_t ldx, const float* cw,
                    int32_t dec_act, int32_t loss_func, int32_t cos_pass, const float* cos_stats,
                    float* cos_part, float* rowloss_part, float* tile_part, float* dbv_part,
                    void* delta2, int64_t ldd, void* delta2_t, int64_t lddt, void* stream);
/* columns of y per workgroup of dae_decode_loss for `dtype` (64 for DAE_BF16, 128 for DAE_F32): rowloss_part / cos_part hold
 * 2 * Fp / width partial rows, tile_part (Bp/128) * (Fp/width) entries */
int32_t dae_decode_tile_n(int32_t dtype);

int dae_cos_reduce(const float* cos_part, int32_t n_col_waves, int32_t B, int32_t Bp,
                   float* cos_stats, float* rowloss, void* stream);

/* K5: Gram matrix D = h h^T in exact fp32 MFMA (triplet_loss_utils.py:93,219).
 * D_slabs: `splits` slabs of [Bp x Bp] (consumers sum them). */
int dae_gram(const float* h_f32, int64_t ldh, int32_t Bp, int32_t Hp, float* D_slabs, int32_t splits,
             void* stream);

/* Label statistics (triplet_loss_utils.py:47-76,110-111,129): integer-exact N_valid and batch_all
 * data_weight from label multiplicities, and cw_i = w_i/(sum w + 1e-16) (zero beyond B).
 *   labels int32[B]; n_same_scratch int32[B]; acc_scratch uint64[2]; nvalid_out int64[1];
 *   dw_out int64[B] (may be NULL); cw float[Bp].
 * DAE_TRIPLET_NONE writes cw_i = 1/(B + 1e-16) (weighted_loss's default weight ones, :266) and
 * needs no labels/scratch; DAE_TRIPLET_BATCH_HARD only fills nvalid/dw (cw comes from the miner). */
int dae_label_stats(const int32_t* labels, int32_t B, int32_t Bp, int32_t triplet,
                    int32_t* n_same_scratch, uint64_t* acc_scratch,
                    int64_t* nvalid_out, int64_t* dw_out, float* cw,
                    float alpha, float* tri_scalars /* may be NULL; batch_all: [0] = alpha/(N_valid+1e-16) */,
                    void* stream);

/* K6: batch_all online miner, one fused sweep per anchor (triplet_loss_utils.py:79-131).
 *   loss_part[a] = sum_{p,n valid} softplus(D[a,n]-D[a,p])   (only positive triplets if pos_only)
 *   npos_part[a] = #{valid (p,n): D[a,n]-D[a,p] > 1e-16}
 *   G[a,:]       = d(sum softplus)/dD[a,:]   (un-normalised, [Bp x Bp], row stride Bp)
 *   role_cnt[a,:] (pos_only): per-column positive-triplet counts (NULL otherwise)
 * D is given as `d_splits` slabs (stride slab_stride) that are summed on load.
 * mode: DAE_MINER_POS_ONLY (the reference's pos_triplets_only=True) | DAE_MINER_FAST (bf16 training mode: sigmoid as
 *       1 - 1/(1+e) and log(fl(1+e)) without the log1p correction -- per-anchor error bound 2e-6 relative, enforced by an
 *       in-kernel fallback to the exact form; counts stay bit-exact). */
int dae_triplet_batch_all(const float* D_slabs, int32_t d_splits, int64_t slab_stride, int64_t ldd,
                          const int32_t* labels, int32_t B, int32_t Bp, int32_t mode,
                          float* loss_part, uint32_t* npos_part, float* G, uint32_t* role_cnt,
                          void* stream);

/* The same miner for the anchors [a0, a0 + n_anchors) of the batch only: row r of D_slabs / G / loss_part / npos_part belongs
 * to batch element a0 + r, D is [n_anchors x ldd] (its columns are the WHOLE batch of B rows, labels[B] likewise).  This is what
 * a data-parallel rank runs on ITS rows against the all-gathered embeddings (global-batch mining, SURVEY 8e mode i). */
int dae_triplet_batch_all_rows(const float* D_slabs, int32_t d_splits, int64_t slab_stride, int64_t ldd,
                               const int32_t* labels, int32_t B, int32_t Bp, int32_t a0, int32_t n_anchors, int32_t mode,
                               float* loss_part, uint32_t* npos_part, float* G, uint32_t* role_cnt, void* stream);

/* K7: batch_hard online miner (triplet_loss_utils.py:202-259) incl. its quirks.
 *   dist_a = max(hn_a - hp_a, 0); cnt_a = dist_a > 0;
 *   loss_part[a] = softplus(dist_a)*cnt_a;  cnt_part[a] = cnt_a;
 *   dw[j] += cnt_a*([D[a,j]==hp_a] + [D[a,j]==hn_a] + [j==a])     (int32 atomics; zeroed here)
 *   G[a,:] = d(sum_a softplus(dist_a) cnt_a)/dD[a,:]  (un-normalised; ties split equally) */
int dae_triplet_batch_hard(const float* D_slabs, int32_t d_splits, int64_t slab_stride, int64_t ldd,
                           const int32_t* labels, int32_t B, int32_t Bp,
                           float* loss_part, uint32_t* cnt_part, int32_t* dw, float* G, void* stream);

/* batch_hard for the anchors [a0, a0 + n_anchors) only (see dae_triplet_batch_all_rows).  dw[B] is zeroed by EVERY call and then
 * receives the contributions of this call's anchors: callers that split a batch over several calls / ranks sum the dw vectors. */
int dae_triplet_batch_hard_rows(const float* D_slabs, int32_t d_splits, int64_t slab_stride, int64_t ldd,
                                const int32_t* labels, int32_t B, int32_t Bp, int32_t a0, int32_t n_anchors,
                                float* loss_part, uint32_t* cnt_part, int32_t* dw, float* G, void* stream);

/* Reduce miner partials into the normalisers / statistics:
 *   tri_scalars[0] = alpha / (N + 1e-16)  (N = N_valid | N_pos | sum cnt) -> scale of (G+G^T)
 *   tri_scalars[1] = triplet loss, [2] = fraction, [3] = num
 * For batch_hard (and pos_only) also converts the integer data_weight into dw_f32_out and cw. */
int dae_triplet_finalize(int32_t triplet, int32_t pos_only, int32_t B, int32_t Bp, float alpha,
                         const float* loss_part, const uint32_t* cnt_part, const int64_t* nvalid,
                         const int32_t* dw_i32, const uint32_t* role_cnt, float* dw_f32_out,
                         float* cw, float* tri_scalars, void* stream);

/* Gs = tri_scalars[0] * (G + G^T) on [0,B)^2 (zero elsewhere) in `dtype` [Bp x Bp] -- the A operand
 * of the triplet term of dL/dh = delta2 W + alpha (G + G^T) h (autodiff of triplet_loss_utils.py:93). */
int dae_sym_scale(const float* G, int32_t B, int32_t Bp, const float* tri_scalars, int32_t dtype,
                  void* Gs, void* stream);

/* K8 (middle): dh = sum_s slab_s (+ dh_extra);  delta1 = dh * act'(z1);  delta1^T in `dtype`
 * [Hp x ldt]; partial column sums for db_h = sum_i delta1 - act'(bh) * sum_i dh (the -act(bh) term
 * of autoencoder.py:389).  colsum_part: [2 x (Bp/32) x Hp].  delta1_f32 optional [Bp x ldh]. */
int dae_dh_finish(const float* slabs, int32_t splits, int64_t slab_stride, int64_t ld_slab,
                  const float* dh_extra, const float* h_f32, int64_t ldh, const float* bh,
                  int32_t B, int32_t H, int32_t enc_act, int32_t dtype, void* delta1_t, int64_t ldt,
                  float* colsum_part, float* delta1_f32, void* stream);

/* Reduce the bias-gradient partials into the flat gradient buffer [dW | dbh | dbv]. */
int dae_bias_grads(const float* dbv_part, int32_t n_row_waves, const float* colsum_part, int32_t n_row_blocks,
                   float* bh, int32_t H, int32_t Hp, int32_t F, int32_t Fp, int32_t enc_act,
                   float* dbh, float* dbv,
                   /* apply != 0: also run the optimizer update of bh / bv here (slots laid out [bh | bv]) */
                   int32_t apply, int32_t opt, float lr, float momentum, float grad_scale, float* bv,
                   float* s1_bias, float* s2_bias, void* stream);

/* K9: optimizer step on the padded flat parameter vector [W (Fp*Hp) | bh (Hp) | bv (Fp)] (grad, s1,
 * s2 share that layout), refreshing the low-precision shadows W_lo [Fp x Hp] and W^T_lo [Hp x Fp]
 * (autoencoder.py:444-477; tf.train.* semantics: Adagrad accumulator starts at 0.1, Momentum without
 * Nesterov, Adam with lr = lr_t precomputed by the caller).  grad_scale multiplies the gradient first
 * (1/world_size for data parallel).  apply: 0 only refreshes the shadows, 1 updates W and the biases,
 * 2 updates W only (the biases were updated by dae_bias_grads). */
int dae_opt_step(int32_t opt, float lr, float momentum, float grad_scale,
                 float* W, float* bh, float* bv, const float* grad, float* s1, float* s2,
                 int32_t Fp, int32_t Hp, int32_t dtype, void* W_lo, void* Wt_lo, int32_t apply, void* stream);

/* Final per-step statistics (autoencoder.py:233 fetch list):
 * ae = sum_i cw_i * rowloss_i (from rowloss_part + cw, or from the decode kernel's tile_part if given);
 * cost = ae + alpha * triplet.  stats: float[DAE_STATS_STRIDE]. */
/* Pieces of the data-parallel (sharded-optimizer) second half, see dae_plan_apply_rows: the optimizer on rows [f0, f1) of W
 * (W_lo rows refreshed, Wt_lo untouched), the bias update alone, and Wt_lo = W_lo^T. */
int dae_opt_step_rows(int32_t opt, float lr, float momentum, float grad_scale, float* W, const float* grad_rows, float* s1,
                      float* s2, int32_t Hp, int32_t f0, int32_t f1, int32_t dtype, void* W_lo, void* stream);
int dae_opt_bias(int32_t opt, float lr, float momentum, float grad_scale, float* bh, float* bv, const float* grad_b, float* s1b,
                 float* s2b, int32_t Hp, int32_t Fp, void* stream);
int dae_transpose_shadow(const void* W_lo, int32_t Fp, int32_t Hp, int32_t dtype, void* Wt_lo, void* stream);

int dae_step_stats(const float* rowloss_part, int32_t n_col_waves, const float* tile_part, int32_t n_tiles,
                   const float* cw, int32_t B, int32_t Bp, int32_t triplet, float alpha,
                   float* tri_scalars, const int64_t* nvalid,
                   /* optional batch_all miner partials: reduces them here instead of dae_triplet_finalize */
                   const float* loss_part, const uint32_t* cnt_part, float* stats, void* stream);

/* Explicit (anchor,pos,neg) triplet term of DenoisingAutoencoderTriplet
 * (autoencoder_triplet.py:308-311): t_i = h_i.hneg_i - h_i.hpos_i; loss = mean softplus(t).
 * h3 = [org; pos; neg] stacked compactly (3*B rows, stride ldh); writes alpha * dloss/dh3 into dh3
 * (same layout), loss_part[B] and tri_scalars[1] = loss. */
int dae_explicit_triplet(const float* h3, int64_t ldh, int32_t B, int32_t H, float alpha,
                         float* dh3, float* loss_part, float* tri_scalars, void* stream);

/* Stand-alone per-row reconstruction loss of a given decode (triplet_loss_utils.py:268-273) for the
 * function-level weighted_loss() API: x, y fp32 [B x F]; rowloss[B].  The weighted mean
 * sum(row*w)/(sum w + 1e-16) (:275) is then taken by dae_step_stats with n_col_waves = 1. */
int dae_weighted_loss_rows(const float* x, int64_t ldx, const float* y, int64_t ldy, int32_t B, int32_t F,
                           int32_t loss_func, float* rowloss, void* stream);

/* A/B switch for the plain GEMM's staging: 0 = register staging (2 LDS buffers), 2/3/4 = depth of the
 * global_load_lds ring with counted vmcnt waits (default 2); -1 / -2 = 4-wave kernel for every grid / 8-wave
 * producer-consumer kernel for grids of at most one workgroup per CU (default); -3 / -4 / -5 = dW + optimizer on the 4-wave
 * 128 x 128 kernel / on the 8-wave 160 x 128 kernel when its grid fills one round of the chip (default) / whenever it fits. */
void dae_set_glds(int32_t nst);

/* K slices with which dae_gemm_nt runs a bf16 shape on the 256 x 256-tile kernel (8 MFMA waves, one workgroup per CU; the large
 * split-K contractions of the dense-input configs: x~[B x F].W and delta2.W with F = 50 000) -- calling dae_gemm_nt with exactly this
 * `splits` selects it; 0 = the shape stays on the 128 x 128 kernels.  dae_set_glds(-6) / (-7) turn the kernel off / on (A/B). */
int32_t dae_gemm_w8_splits(int32_t dtype, int32_t M, int32_t N, int32_t K);

/* ---------------------------------------------------------------------------------------------
 * Whole-step driver: what DenoisingAutoencoder._run_train_step (autoencoder.py:206-246) does per
 * mini-batch, as one host call that enqueues every kernel above on `stream`.
 * ------------------------------------------------------------------------------------------- */
typedef struct dae_plan dae_plan;

typedef struct {
    int32_t n_features, n_components, max_batch;
    int32_t dtype, enc_act, dec_act, loss_func, opt, triplet;
    int32_t pos_triplets_only;
    int32_t encode_splits, dh_splits, gram_splits;   /* 0 = pick automatically */
    float   learning_rate, momentum, alpha;
} dae_config;

typedef struct {
    /* train set, CSR (sorted column ids) or dense fp32; exactly one of indptr / dense non-NULL */
    const int64_t* indptr; const int32_t* indices; const float* values;
    const float* dense; int64_t ld_dense;
    int64_t n_rows, nnz;
    /* parameters, padded: W [Fp x Hp], bh [Hp], bv [Fp]; flat gradient [Fp*Hp + Hp + Fp];
     * optimizer slots (same length as the gradient; may be NULL for SGD) */
    float* W; float* bh; float* bv; float* grad; float* opt_s1; float* opt_s2;
    /* low-precision shadows W_lo [Fp x Hp], Wt_lo [Hp x Fp] in cfg.dtype */
    void* W_lo; void* Wt_lo;
    void* workspace; uint64_t workspace_bytes;
    /* optional (may be NULL): bf16 image [Fp x Hp] of the W gradient.  When set, phase 1 / 5 steps in bf16 mode write the W part of the
     * gradient THERE instead of into `grad` (the bias parts stay in `grad`): the operand of a bf16 reduce-scatter, produced by the dW
     * kernel's epilogue instead of a separate cast pass. */
    void* grad_lo;
} dae_buffers;

typedef struct {
    const int32_t* row_idx;      /* device int32[B]: rows of the train set in this batch */
    const int32_t* labels;       /* device int32[B] (NULL for triplet none) */
    int32_t B;
    int32_t corr_mode; const uint32_t* keep_bits; uint64_t seed; uint32_t rng_stream;
    float corr_frac, scale;
    /* optional second CSR holding an already-corrupted copy of the train set (salt&pepper etc.) */
    const int64_t* c_indptr; const int32_t* c_indices; const float* c_values;
    const int32_t* c_row_idx;    /* rows of the corrupted CSR to take (NULL: the same row_idx as the clean set) */
    float* stats;                /* device float[DAE_STATS_STRIDE] for this step */
    int32_t phase;               /* 0 = forward+backward+update, 1 = forward+backward only (DP:
                                    caller all-reduces `grad` then calls dae_plan_apply), 2 = forward only,
                                    3 = as 0 but the W part of `grad` is not materialised (bf16: the optimizer
                                    runs in the dW GEMM's epilogue and nothing reads the gradient image),
                                    4 / 5 = the step split around an EXTERNAL miner (data parallel, global-batch mining):
                                    4 stops after the encode (h_f32, h_lo, h_t and the side images stay in the workspace);
                                    the caller mines over the all-gathered batch and writes the plan buffers `cw` (row
                                    weights), `tri_scalars`[1..3] (triplet loss, fraction, num) and `dh_extra`
                                    (d alpha*triplet / dh of its rows); 5 resumes at the decode with the same row_idx
                                    and ends like 1 */
    int32_t adam_t; float grad_scale;
} dae_step;

/* -------------------------------------------------------------------------------------------------
 * Evaluation step after the training path: N x N similarity of row vectors.
 * Replaces helpers.pairwise_similarity (helpers.py:11-50; called by main_autoencoder.py:307-317):
 *   [sklearn.preprocessing.normalize(X, norm)]  ->  cosine_similarity | linear_kernel  ->  fill_diagonal(0).
 *   X [N x ldx] fp32 (device), norm: 0 none / 1 'l1' / 2 'l2' / 3 'max', metric: 0 'cosine' / 1 'linear kernel'
 *   (any other metric is rejected, as the reference's assert does), zero_diagonal as set_diagonal_zero.
 *   out: fp32 image [dae_pad(N) x ldo], ldo >= dae_pad(N); rows / columns >= N are zero.
 *   workspace: dae_pairwise_similarity_workspace(N, D) bytes, 16-byte aligned (the normalised operand image).
 * Exact-fp32 MFMA product, fp32 accumulation.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_pairwise_similarity_workspace(int32_t N, int32_t D);
int dae_pairwise_similarity(const float* X, int64_t ldx, int32_t N, int32_t D, int32_t norm, int32_t metric,
                            int32_t zero_diagonal, float* out, int64_t ldo, void* workspace,
                            uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Retrieval: the k most similar corpus rows of every query row, without an N x N matrix (the top-k that
 * helpers.pairwise_similarity + a sort would give; helpers.most_similar).
 *   Q [Nq x ldq] fp32 queries; C [Nc x ldc] fp32 corpus, or C == NULL: the corpus is Q itself (pass Nc == Nq).
 *   norm, metric: exactly as dae_pairwise_similarity (0 none / 1 'l1' / 2 'l2' / 3 'max'; 0 'cosine' / 1 'linear kernel').
 *   Score of (i, j): the exact-fp32 MFMA dot product of the two normalised rows -- the value dae_pairwise_similarity writes.
 *   Output, per query row i: idx[i * ldk + r] (int32 corpus row) and score[i * ldk + r] (fp32), r < k, ldk >= k, ordered by
 *   score descending, then index ascending (a total order: the result is bit-identical run to run and independent of the
 *   grid).  When fewer than k candidates exist the tail is idx = -1, score = -inf.
 *   exclude_self (only with C == NULL) drops the pair j == i.  Unlike the reference's set_diagonal_zero, which keeps
 *   the self pair at score 0 in the matrix, the self pair is removed from the candidates altogether.
 *   1 <= k <= 128.  Non-finite inputs are out of scope (their order is undefined).
 *   workspace: dae_topk_similarity_workspace(Nq, Nc, D, k) bytes, 256-byte aligned: the two normalised operand images
 *   plus per-row partial lists, O(Nq * splits * k) -- no N x N buffer.  Each operand image must stay below 4 GiB.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_topk_similarity_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t k);
int dae_topk_similarity(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc,
                        int32_t D, int32_t norm, int32_t metric, int32_t k, int32_t exclude_self,
                        int32_t* idx, float* score, int64_t ldk, void* workspace, uint64_t workspace_bytes,
                        void* stream);

/* -------------------------------------------------------------------------------------------------
 * Seen-aware retrieval: dae_topk_similarity with a list of excluded corpus rows per query row (the articles a user has
 * already read; helpers.most_similar(exclude=...), helpers.recommend).
 *   Every argument of dae_topk_similarity, and the same scores, order and workspace size, plus an exclusion CSR on the
 *   device: excl_indptr int64[Nq + 1], excl_items int32[excl_indptr[Nq]]; row i's items are corpus indices, sorted
 *   ascending and unique (a precondition: the lookup is a binary search).  Candidate j is skipped for query row i when j
 *   is in row i's list -- before it can take one of the k slots, so a row still gets k results whenever k admissible
 *   candidates exist (admissible: j < Nc, not excluded, and not i itself with exclude_self); otherwise the tail is
 *   idx = -1, score = -inf.  Membership is tested only for the candidates that beat the row's current k-th score.
 *   Both pointers NULL: exactly dae_topk_similarity (which forwards here), bit for bit; exactly one NULL is an argument error.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_topk_similarity_ex_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t k);
int dae_topk_similarity_ex(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc,
                           int32_t D, int32_t norm, int32_t metric, int32_t k, int32_t exclude_self,
                           const int64_t* excl_indptr, const int32_t* excl_items, int32_t* idx, float* score,
                           int64_t ldk, void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Full-rank evaluation: the position of one target corpus row per query row among ALL corpus rows, without an Nq x Nc
 * matrix (AUC, mean / median rank, untruncated MRR / nDCG; helpers.target_ranks, helpers.recommend_ranks).
 *   Q, ldq, Nq, C, ldc, Nc, D, norm, metric, exclude_self, excl_indptr, excl_items: exactly as dae_topk_similarity_ex, and
 *   the same scores and order (score descending, then index ascending, -0 == +0); there is no k.  Both excl pointers NULL:
 *   no lists; exactly one NULL is an argument error.
 *   targets int32[Nq] (device): the corpus row whose rank is asked for, per query row; a negative value means "no target".
 *   Output (device, Nq entries each), for a row i with t = targets[i] >= 0:
 *       rank[i] = 1 + #{ j in [0, Nc) : j != t, j not in row i's list, not (exclude_self and j == i), (S[i, j], j) before (S[i, t], t) }
 *       target_score[i] = S[i, t]
 *   i.e. rank[i] is the position (from 1) the target takes in dae_topk_similarity_ex with the same arguments for every
 *   k >= rank[i], and target_score[i] is that call's score bit for bit.  The list removes competitors only: a target that is
 *   in its own row's list (or is the row itself under exclude_self) is still ranked among the admissible candidates;
 *   whether it counts is the caller's decision.  Rows without a target get rank 0, target_score -inf.  Zero-padded rows
 *   and columns are never counted.  Integer counts: bit-identical run to run, independent of the grid and the corpus split.
 *   The exclusion work is one step per list item; it does not grow with the rank.
 *   Precondition: every targets[i] < Nc.  It is not reported: an index outside is read as the last corpus row.
 *   workspace: dae_rank_similarity_workspace(Nq, Nc, D) bytes, 256-byte aligned: the two normalised operand images, the
 *   targets' rows gathered into a third image of the queries' size, and 8 bytes per query row -- no Nq x Nc term.  Each
 *   operand image must stay below 4 GiB.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_rank_similarity_workspace(int32_t Nq, int32_t Nc, int32_t D);
int dae_rank_similarity(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                        int32_t norm, int32_t metric, int32_t exclude_self, const int64_t* excl_indptr,
                        const int32_t* excl_items, const int32_t* targets, int32_t* rank, float* target_score,
                        void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Candidate windows: dae_topk_similarity_ex and dae_rank_similarity with one contiguous range of admissible corpus rows
 * per query row (a news feed: the articles that existed when the user clicked, and only the recent ones; with the corpus
 * ordered by publication time that is a column range; helpers.most_similar / recommend / target_ranks(window=...)).
 *   Every argument of the plain call, and the same scores, 64-bit key order, tails, determinism, grid-independence and
 *   workspace size, plus win_lo, win_hi: int32[Nq] on the device.  Candidate j is admissible for query row i only if
 *   win_lo[i] <= j < win_hi[i] -- in addition to j < Nc, not in row i's list, and not i itself under exclude_self.
 *   win_lo[i] >= win_hi[i] is an empty window: the top-k row is idx = -1, score = -inf throughout.  Values are clamped
 *   to [0, Nc] in the kernel.  The workgroups of a 128-row query tile walk only the 128-column corpus tiles that the union
 *   of the tile's non-empty windows touches, so rows with similar windows should be neighbours (the helpers sort them).
 *   dae_rank_similarity_win: the window removes competitors only, exactly as the exclusion list does -- a target outside
 *   its own row's window is still scored and ranked among the admissible candidates; whether it counts is the caller's
 *   decision.  A list item outside the window is neither counted nor taken out again.
 *   Both window pointers NULL: exactly the plain call (which forwards here), bit for bit; exactly one NULL is an argument
 *   error.  All other argument checks are those of the plain calls, with their messages.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_topk_similarity_win_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t k);
int dae_topk_similarity_win(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc,
                            int32_t D, int32_t norm, int32_t metric, int32_t k, int32_t exclude_self,
                            const int64_t* excl_indptr, const int32_t* excl_items, const int32_t* win_lo,
                            const int32_t* win_hi, int32_t* idx, float* score, int64_t ldk, void* workspace,
                            uint64_t workspace_bytes, void* stream);
uint64_t dae_rank_similarity_win_workspace(int32_t Nq, int32_t Nc, int32_t D);
int dae_rank_similarity_win(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                            int32_t norm, int32_t metric, int32_t exclude_self, const int64_t* excl_indptr,
                            const int32_t* excl_items, const int32_t* win_lo, const int32_t* win_hi,
                            const int32_t* targets, int32_t* rank, float* target_score, void* workspace,
                            uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Shared stamped exclusion lists: the windowed calls for query rows that are the successive states of one user (row e = the
 * state after click e, which must skip the articles clicked at positions <= e; helpers.most_similar / target_ranks
 * (exclude_shared=...), recommend_every_click, recommend_ranks_every_click).  Instead of one list per query row there is one
 * list per user, read by all of that user's rows, with a stamp per item: the lists stay the size of the click log.
 *   Every argument of the _win calls but excl_indptr / excl_items, and the same scores, 64-bit key order, tails, exclude_self,
 *   windows, determinism, grid-independence and workspace size, plus (all on the device)
 *     list_indptr int64[n_lists + 1], list_items int32[list_indptr[n_lists]], list_stamps int32[same]: a CSR of n_lists lists;
 *       each list's items are corpus indices, sorted ascending and unique (a precondition, as in dae_topk_similarity_ex), and
 *       every item carries one stamp (for a click log: the position of the item's first click);
 *     row_list int32[Nq]: the list that query row i reads; a value outside [0, n_lists) means "no list" (tested in the kernel:
 *       a wrong value never becomes a stray read);
 *     row_limit int32[Nq]: the row's stamp limit.
 *   Candidate j is barred for query row i iff j == list_items[p] for some p in row i's list with list_stamps[p] <= row_limit[i].
 *   Everything else is exactly the _win call given, per row, the materialised list { list_items[p] : list_stamps[p] <=
 *   row_limit[i] } -- bit for bit: in dae_rank_similarity_seq the list removes competitors only, and a list item outside the
 *   row's window is neither counted nor taken out again.  The top-k lookup (a binary search in the shared list, then the
 *   stamp compare) runs only on the candidates that beat the row's current k-th score; the rank call walks the shared list
 *   once per row, one step per item.
 *   All five list pointers NULL: exactly the _win call without lists, bit for bit; some but not all NULL is an argument
 *   error, and so is a negative n_lists.  All other argument checks are those of the _win calls, with their messages.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_topk_similarity_seq_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t k);
int dae_topk_similarity_seq(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc,
                            int32_t D, int32_t norm, int32_t metric, int32_t k, int32_t exclude_self,
                            const int64_t* list_indptr, const int32_t* list_items, const int32_t* list_stamps,
                            int32_t n_lists, const int32_t* row_list, const int32_t* row_limit, const int32_t* win_lo,
                            const int32_t* win_hi, int32_t* idx, float* score, int64_t ldk, void* workspace,
                            uint64_t workspace_bytes, void* stream);
uint64_t dae_rank_similarity_seq_workspace(int32_t Nq, int32_t Nc, int32_t D);
int dae_rank_similarity_seq(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc, int32_t D,
                            int32_t norm, int32_t metric, int32_t exclude_self, const int64_t* list_indptr,
                            const int32_t* list_items, const int32_t* list_stamps, int32_t n_lists,
                            const int32_t* row_list, const int32_t* row_limit, const int32_t* win_lo,
                            const int32_t* win_hi, const int32_t* targets, int32_t* rank, float* target_score,
                            void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * User states from browsing histories: the decaying model of "Embedding-based News Recommendation for Millions of
 * Users" (KDD'17), a decay-weighted mean of the embeddings of the articles a user has read (helpers.user_states).
 *   E [Na x lde] fp32 article embeddings (device).  History CSR (device): indptr int64[M + 1], items int32[nnz], each
 *   user's events oldest first; an article may occur more than once.  Per user, in this order:
 *       s = 0 (H floats), z = 0;   for every event e:   s = d_e * s + E[items[e]];   z = d_e * z + 1;   state_e = s / z
 *   d_e: decay == NULL: the scalar beta in [0, 1] for every event; else decay float32[nnz] (device), the factor applied
 *   to the running state before event e is added (time-based decay, session resets with 0); values are expected in [0, 1].
 *   A user's first factor is ignored.
 *   all_states == 0: U [M x ldu], row u = the state after u's last event, zeros for an empty history.
 *   all_states != 0: U [nnz x ldu], row e = state_e (the state that predicts event e + 1).
 *   fp32 throughout (one fused multiply-add per step, one IEEE division per output), fixed order, no atomics:
 *   bit-identical run to run and independent of the order of the users; the all_states row of a user's last event
 *   equals its all_states == 0 row bit for bit.
 *   Precondition: every items[e] is in [0, Na).  It is not reported: an index outside is read as the nearest valid row.
 *   No workspace.  lde, ldu >= H; 16-byte aligned E / U with lde, ldu and H multiples of 4 take the vector path.
 * ------------------------------------------------------------------------------------------------- */
int dae_user_states(const float* E, int64_t lde, int32_t Na, int32_t H, const int64_t* indptr, const int32_t* items,
                    int64_t M, int64_t nnz, float beta, const float* decay, int32_t all_states, float* U, int64_t ldu,
                    void* stream);

/* -------------------------------------------------------------------------------------------------
 * Training step of the decay user model: pairwise ranking loss of the relevance R(u, a) = (alpha * u) . a over click
 * histories and its gradients with respect to alpha (one weight per embedding dimension) and the decay beta, in one
 * walk of every history (helpers.user_pair_loss, helpers.fit_user_model).  E is fixed: there is no backward pass, and
 * neither the [events x H] matrix of states nor its derivative is stored.
 *   E, lde, Na, H, indptr, items, M, nnz: as dae_user_states (device memory).  alpha float[H].
 *   Per-event factor f_e and its derivative f'_e = d f_e / d beta:
 *       decay == NULL: f_e = beta, f'_e = 1.   Otherwise decay float[nnz] and ddecay float[nnz]; ddecay == NULL means
 *       f' = 0, and dbeta comes out 0 (ddecay without decay is an argument error).  A user's first event ignores both.
 *   negatives int32[nnz x n_neg], 1 <= n_neg <= 16: the sampled negatives of every event (those of a user's first event
 *   are not read as pairs).
 *   Per user, in event order; the first event starts the chain:
 *       first event:   s = E[item], z = 1, g = 0, zg = 0                               (no pair is scored)
 *       event e after: for each j < n_neg with n = negatives[e, j], n >= 0 and n != items[e]        (a valid pair)
 *                          D_h   = E[items[e], h] - E[n, h]
 *                          x     = (sum_h alpha_h s_h D_h) / z                          one division per pair
 *                          xb    = (sum_h alpha_h g_h D_h) / z - x (zg / z)             = sum_h alpha_h d(s_h / z)/dbeta D_h
 *                          loss += softplus(-x);   c = -sigmoid(-x)
 *                          dalpha_h += c s_h D_h / z;   dbeta += c xb;   n_pairs += 1
 *                          margin[e, j] = x
 *                      then, with the OLD s and z on the right-hand sides:
 *                          g = f_e g + f'_e s;   zg = f_e zg + f'_e z;   s = f_e s + E[item];   z = f_e z + 1
 *   s / z is the all_states row of the previous event of dae_user_states, and the s and z updates are its fused
 *   multiply-adds.  The sums are NOT divided by n_pairs.
 *   Outputs (device memory): *loss, dalpha[H], *dbeta as double, *n_pairs as int64, and, unless NULL, margin
 *   float[nnz x n_neg] (0 where the pair is not valid).
 *   fp32 arithmetic per pair; sums over more than 64 events and all sums across users in fp64; no atomics.  The
 *   result is bit-identical run to run on one device; n_pairs and margin do not depend on the grid, on the order of the
 *   users or on the alignment of E, and a user's margins do not change when other users are added or permuted.
 *   Preconditions, not reported: items in [0, Na); negatives < Na (a negative one marks "no pair").  An index outside is
 *   read as the nearest valid row.
 *   H <= 1024.  workspace: dae_user_pair_loss_workspace(M, H) bytes, 256-byte aligned (one partial per wave).
 *   lde >= H; a 16-byte aligned E with lde and H multiples of 4 is read with 16-byte loads.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_user_pair_loss_workspace(int64_t M, int32_t H);
int dae_user_pair_loss(const float* E, int64_t lde, int32_t Na, int32_t H, const int64_t* indptr, const int32_t* items,
                       int64_t M, int64_t nnz, float beta, const float* decay, const float* ddecay, const float* alpha,
                       const int32_t* negatives, int32_t n_neg, double* loss, double* dalpha, double* dbeta,
                       int64_t* n_pairs, float* margin, void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * GRU user states: the recurrent user model of the same paper, inference only (helpers.gru_user_states).  The state of
 * every user after every click, from weights in the layout of torch.nn.GRU (one layer, gate row blocks r, z, n).
 *   E [Na x lde] fp32 article embeddings, D columns (device).  W_ih [3H x ldwi] (D columns), W_hh [3H x ldwh] (H columns),
 *   b_ih, b_hh float[3H] (device).  History CSR as dae_user_states.  Per user, events oldest first, x = E[items[e]]:
 *       gi = W_ih x + b_ih        gh = W_hh h + b_hh
 *       r = sigmoid(gi_r + gh_r)  z = sigmoid(gi_z + gh_z)  n = tanh(gi_n + r * gh_n)  h' = (1 - z) * n + z * h
 *   h starts at zero (h0 == NULL) or at row u of h0 [M x ldh0] (device, one row per user in the caller's order: the
 *   states of an earlier call, continued without replaying the history).  D != H is allowed.
 *   Schedule (helpers.gru_schedule): the work is time-major, one launch per step over the users still active.
 *       order int32[M] (device): a permutation of the users with history lengths non-increasing.
 *       active_host int64[T] (HOST memory): active_host[t] = number of users with more than t events; non-increasing,
 *       active_host[0] <= M, and their sum at most nnz.  T = the longest history (fewer steps truncate every history).
 *   all_states == 0: U [M x ldu], row u = the state after u's last event; zeros, or its h0 row, for an empty history.
 *   all_states != 0: U [nnz x ldu], row e = the state after event e (the state that predicts event e + 1).
 *   fp32 throughout: the products are exact-fp32 MFMA chains in a fixed k order, the gates use expf / tanhf and IEEE
 *   division; no atomics.  Bit-identical run to run; a user's states do not depend on the other users of the call, on
 *   their order or on all_states, and continuing from a stored state gives the bits of the unsplit history.
 *   Preconditions, not reported: items in [0, Na) (an index outside is read as the nearest valid row); order and
 *   active_host agree with indptr.
 *   workspace: dae_gru_user_states_workspace(Na, D, H, M) bytes, 256-byte aligned: padded images of E, W_ih, W_hh, the
 *   input projection of every article [pad(Na) x 3 pad(H)] and two state buffers [pad(M) x pad(H)] -- no events x H term.
 *   Every image must stay below 4 GiB (split the users into several calls).  M == 0 returns 0 without a launch.
 *   lde, ldwi >= D; ldwh, ldu, ldh0 >= H.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_gru_user_states_workspace(int32_t Na, int32_t D, int32_t H, int64_t M);
int dae_gru_user_states(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t H, const float* W_ih, int64_t ldwi,
                        const float* W_hh, int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr,
                        const int32_t* items, const int32_t* order, int64_t M, int64_t nnz, int32_t T,
                        const int64_t* active_host, const float* h0, int64_t ldh0, int32_t all_states, float* U,
                        int64_t ldu, void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * LSTM and plain-RNN user states: the other two recurrent user models of the same paper, inference
 * (helpers.lstm_user_states, helpers.rnn_user_states), from weights in the layout of torch.nn.LSTM (gate row blocks
 * i, f, g, o: W_ih [4H x ldwi], W_hh [4H x ldwh], b_ih, b_hh float[4H]) and of torch.nn.RNN(nonlinearity='tanh') (one
 * block: W_ih [H x ldwi], W_hh [H x ldwh], b_ih, b_hh float[H]).  Per user, events oldest first, x = E[items[e]]:
 *       LSTM:  i = sigmoid(W_ii x + b_ii + W_hi h + b_hi)   f, o likewise   g = tanh(W_ig x + b_ig + W_hg h + b_hg)
 *              c' = f * c + i * g      h' = o * tanh(c')
 *       RNN:   h' = tanh(W_ih x + b_ih + W_hh h + b_hh)
 *   Every argument dae_rnn_user_states shares with dae_gru_user_states means what it means there: E, the history CSR, the
 *   schedule (order, active_host, T), h0 / ldh0, all_states, U / ldu, workspace, stream.  dae_lstm_user_states adds
 *       c0 [M x ldc0] (device) or NULL: the cell state every user starts from (zero when NULL), with or without h0;
 *       C [M x ldc] (device) or NULL: receives every user's cell state after their last event; for an empty history its
 *       c0 row, or zeros.  (h, c) = (U, C) of a call, handed back as (h0, c0), continue the histories.
 *   fp32 throughout, exact-fp32 MFMA chains in a fixed k order, expf / tanhf and IEEE division in the gates, no atomics:
 *   bit-identical run to run; a user's states do not depend on the other users of the call, on their order or on
 *   all_states, and continuing from stored states gives the bits of the unsplit history.  Without h0 the first step
 *   skips the recurrent product (h = 0) and gives the bits of a call with a zero h0.
 *   Preconditions, not reported: as dae_gru_user_states.
 *   workspace, 256-byte aligned, with pad = round up to 128, al = round up to 256 and G = 4 (LSTM) or 1 (RNN):
 *       al(4 pad(Na) pad(D)) + al(4 G pad(H) pad(D)) + al(4 G pad(H) pad(H)) + al(4 G pad(Na) pad(H)) + S al(4 pad(M) pad(H))
 *   bytes -- the images of E, W_ih and W_hh, the input projection of every article, and S = 2 state buffers (RNN) or
 *   S = 3, two state buffers and the cell buffer (LSTM).  No events x H term; linear in M.  Every image must stay below
 *   4 GiB (split the users into several calls).  M == 0 returns 0 without a launch.  Every argument error is reported
 *   before any HIP call.  lde, ldwi >= D; ldwh, ldu, ldh0, ldc0, ldc >= H.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_lstm_user_states_workspace(int32_t Na, int32_t D, int32_t H, int64_t M);
int dae_lstm_user_states(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t H, const float* W_ih, int64_t ldwi,
                         const float* W_hh, int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr,
                         const int32_t* items, const int32_t* order, int64_t M, int64_t nnz, int32_t T,
                         const int64_t* active_host, const float* h0, int64_t ldh0, const float* c0, int64_t ldc0,
                         int32_t all_states, float* U, int64_t ldu, float* C, int64_t ldc, void* workspace,
                         uint64_t workspace_bytes, void* stream);
uint64_t dae_rnn_user_states_workspace(int32_t Na, int32_t D, int32_t H, int64_t M);
int dae_rnn_user_states(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t H, const float* W_ih, int64_t ldwi,
                        const float* W_hh, int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr,
                        const int32_t* items, const int32_t* order, int64_t M, int64_t nnz, int32_t T,
                        const int64_t* active_host, const float* h0, int64_t ldh0, int32_t all_states, float* U,
                        int64_t ldu, void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Training step of the GRU user model: the pairwise ranking loss of dae_user_pair_loss on the states of
 * dae_gru_user_states, forward and backward through time over one mini-batch of histories, with the gradients of the
 * four weight arrays (helpers.gru_pair_loss, helpers.fit_gru_user_model).  E is fixed and gets no gradient.
 *   E, lde, Na, W_ih, ldwi, W_hh, ldwh, b_ih, b_hh, indptr, items, order, M, nnz, T, active_host: as
 *   dae_gru_user_states, with D = H (the state is scored against the embeddings: W_ih is [3H x H]); h starts at zero.
 *   negatives int32[nnz x n_neg], 1 <= n_neg <= 16 (device): the sampled negatives of every event; those of a user's
 *   first event are not read.
 *   Per user with events e0 .. e1 - 1, h_e the state after event e (the all_states row e of dae_gru_user_states):
 *       for e = e0 + 1 .. e1 - 1, j < n_neg, n = negatives[e, j], n >= 0 and n != items[e]              (a valid pair)
 *           x = h_(e-1) . (E[items[e]] - E[n]);   loss += softplus(-x);   n_pairs += 1;   margin[e, j] = x
 *   and the gradients of `loss` with respect to W_ih, W_hh, b_ih, b_hh by back-propagation through time, per event with
 *   the stored r, z, n, q = W_hn h + b_hn and h_prev (dh = the loss term plus the carry from the next event):
 *       dn = dh (1 - z)      dz = dh (h_prev - n)      da_n = dn (1 - n^2)      da_z = dz z (1 - z)
 *       dq = da_n r          da_r = da_n q r (1 - r)   dgi = [da_r, da_z, da_n]   dgh = [da_r, da_z, dq]
 *       carry to h_prev = dh z + dgh . W_hh
 *       dW_ih += dgi^T x     dW_hh += dgh^T h_prev     db_ih += dgi     db_hh += dgh
 *   The state after a user's last event predicts nothing; the histories are run without it.  The sums are NOT divided
 *   by n_pairs.
 *   Outputs (device memory): *loss as double, *n_pairs as int64, dW_ih [3H x ld_dwi], dW_hh [3H x ld_dwh], db_ih and
 *   db_hh float[3H], and, unless NULL, margin float[nnz x n_neg] (0 where there is no pair).  A call without a pair to
 *   score (M == 0, T <= 1, only histories of one event) writes zero loss, zero pairs and zero gradients.
 *   fp32 arithmetic (exact-fp32 MFMA chains in a fixed k order, expf / tanhf / log1pf, IEEE division); the loss of a
 *   pair is widened to fp64 before any sum across pairs or rows, the pair count is int64.  No atomics of any kind.
 *   Every output is bit-identical run to run on one device.  n_pairs and margin do not depend on the order of the
 *   users or on the alignment or leading dimension of E.  The gradients sum over the users in schedule order: under a
 *   permutation of the users they agree to rounding, not bit for bit.
 *   Preconditions, not reported: items in [0, Na), negatives < Na (an index outside is read as the nearest valid row);
 *   order and active_host agree with indptr.
 *   workspace: dae_gru_pair_loss_workspace(Na, H, M, nnz, T, n_neg) bytes, 256-byte aligned.  Unlike inference it HAS an
 *   events x H term -- the time-major stash of every step's h_prev, h, r, z, n, q, their gradients and the K-contiguous
 *   copies the weight-gradient GEMMs read: at most 13 float arrays of pad128(nnz + 128 T) x pad128(H), beside the images of
 *   dae_gru_user_states, one of W_hh^T, one [pad128(M) x pad128(H)] buffer and 16 split-K slabs [3 pad128(H) x
 *   pad128(H)].  Every image must stay below 4 GiB: 16 pad128(H) (nnz + 128 T) < 2^32 (train in mini-batches of users).
 *   lde, ldwi, ldwh, ld_dwi, ld_dwh >= H.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_gru_pair_loss_workspace(int32_t Na, int32_t H, int64_t M, int64_t nnz, int32_t T, int32_t n_neg);
int dae_gru_pair_loss(const float* E, int64_t lde, int32_t Na, int32_t H, const float* W_ih, int64_t ldwi, const float* W_hh,
                      int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr, const int32_t* items,
                      const int32_t* order, int64_t M, int64_t nnz, int32_t T, const int64_t* active_host,
                      const int32_t* negatives, int32_t n_neg, double* loss, int64_t* n_pairs, float* dW_ih, int64_t ld_dwi,
                      float* dW_hh, int64_t ld_dwh, float* db_ih, float* db_hh, float* margin, void* workspace,
                      uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Training steps of the LSTM and plain-RNN user models: dae_gru_pair_loss for the other two cells, on the states of
 * dae_lstm_user_states / dae_rnn_user_states (helpers.lstm_pair_loss / fit_lstm_user_model, helpers.rnn_pair_loss /
 * fit_rnn_user_model).  The contract is that of dae_gru_pair_loss, argument for argument: D = H, E fixed and without a
 * gradient, h (and the LSTM's c) start at zero, the schedule, the negatives, what a valid pair is, loss / n_pairs /
 * margin, the histories run without their last event, sums NOT divided by n_pairs, the argument checks (every one
 * reported before any HIP call, messages prefixed "lstm_pair_loss: " / "rnn_pair_loss: ") and the call without a pair
 * to score, which needs no workspace and writes zero loss, zero pairs and zero gradients.
 *   Weights and gradients in the layout of torch.nn.LSTM (gate row blocks i, f, g, o: W_ih, dW_ih [4H x ld], W_hh,
 *   dW_hh [4H x ld], b_ih, b_hh, db_ih, db_hh float[4H]) and of torch.nn.RNN(nonlinearity='tanh') ([H x ld], float[H]).
 *   Back-propagation through time, per event with the stored gates and states (dh = the loss term plus the carry from
 *   the next event, x = E[items[e]], h_prev and c_prev the state and cell before the event):
 *     LSTM:  tc = tanh(c')      dc = dh o (1 - tc^2) + carry_c      da_o = dh tc o (1 - o)      da_i = dc g i (1 - i)
 *            da_g = dc i (1 - g^2)      da_f = dc c_prev f (1 - f)      da = [da_i, da_f, da_g, da_o]
 *            carry_c to c_prev = dc f      carry to h_prev = da . W_hh
 *     RNN:   da = dh (1 - h'^2)      carry to h_prev = da . W_hh
 *     both:  dW_ih += da^T x      dW_hh += da^T h_prev      db_ih += da      db_hh += da
 *   Arithmetic and guarantees as dae_gru_pair_loss: fp32 (exact-fp32 MFMA chains in a fixed k order, expf / tanhf /
 *   log1pf, IEEE division), pair losses widened to fp64 before any sum, no atomics of any kind, every output
 *   bit-identical run to run; n_pairs and margin independent of the order of the users, the gradients equal under a
 *   permutation to rounding.  The forward states are the bits of dae_lstm_user_states / dae_rnn_user_states.
 *   workspace, 256-byte aligned, with pad = round up to 128, al = round up to 256, Hp = pad(H), Rb = pad(nnz + 128 T),
 *   G = 4 and I = 13 (LSTM) or G = 1 and I = 6 (RNN):
 *       al(4 pad(Na) Hp) + 3 al(4 G Hp Hp) + al(4 G pad(Na) Hp) + I al(4 Rb Hp) + [LSTM: al(4 pad(M) Hp)]
 *       + 2 al(8 Rb) + al(4 Rb) + al(64 G Hp Hp)
 *   bytes -- the images of E, W_ih, W_hh and W_hh^T, the input projection of every article, the time-major stash (LSTM:
 *   h_prev, h, i, f, g, o, c', the four transposed gate gradients, h_prev^T and x^T; RNN: h_prev, h, its copy, da^T,
 *   h_prev^T, x^T), the LSTM's cell carry, three per-row arrays and 16 split-K slabs [G Hp x Hp].  Every image must stay
 *   below 4 GiB: 4 G Hp Rb < 2^32 (train in mini-batches of users).  lde, ldwi, ldwh, ld_dwi, ld_dwh >= H.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_lstm_pair_loss_workspace(int32_t Na, int32_t H, int64_t M, int64_t nnz, int32_t T, int32_t n_neg);
int dae_lstm_pair_loss(const float* E, int64_t lde, int32_t Na, int32_t H, const float* W_ih, int64_t ldwi, const float* W_hh,
                       int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr, const int32_t* items,
                       const int32_t* order, int64_t M, int64_t nnz, int32_t T, const int64_t* active_host,
                       const int32_t* negatives, int32_t n_neg, double* loss, int64_t* n_pairs, float* dW_ih, int64_t ld_dwi,
                       float* dW_hh, int64_t ld_dwh, float* db_ih, float* db_hh, float* margin, void* workspace,
                       uint64_t workspace_bytes, void* stream);
uint64_t dae_rnn_pair_loss_workspace(int32_t Na, int32_t H, int64_t M, int64_t nnz, int32_t T, int32_t n_neg);
int dae_rnn_pair_loss(const float* E, int64_t lde, int32_t Na, int32_t H, const float* W_ih, int64_t ldwi, const float* W_hh,
                      int64_t ldwh, const float* b_ih, const float* b_hh, const int64_t* indptr, const int32_t* items,
                      const int32_t* order, int64_t M, int64_t nnz, int32_t T, const int64_t* active_host,
                      const int32_t* negatives, int32_t n_neg, double* loss, int64_t* n_pairs, float* dW_ih, int64_t ld_dwi,
                      float* dW_hh, int64_t ld_dwh, float* db_ih, float* db_hh, float* margin, void* workspace,
                      uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Near-duplicate search: every pair (i, j) whose score reaches a threshold, without an N x N matrix (the range query
 * of article de-duplication; helpers.similar_pairs).
 *   Q, ldq, Nq, C, ldc, Nc, D, norm, metric: exactly as dae_topk_similarity, and the same scores.
 *   A pair qualifies when score(i, j) >= threshold, i < Nq, j < Nc and, with C == NULL (the corpus is Q itself), j < i:
 *   the strict lower triangle, i.e. every unordered pair once and never the self pair.  A NaN score never qualifies; a NaN
 *   threshold is an argument error; -inf / +inf thresholds are allowed.  In self mode only the tiles on or below the
 *   diagonal are computed.
 *   *count_host (host memory) receives the exact number of qualifying pairs, whatever the capacity, and the stream is
 *   synchronised before the call returns.  If *count_host <= capacity, rows / cols / scores [0, *count_host) (device
 *   memory, `capacity` entries each) hold the pairs ordered by i ascending, then j ascending -- bit-identical run to run
 *   and independent of the grid.  Otherwise the three arrays are unspecified and the return value is still 0: allocate
 *   *count_host entries and call again.  capacity == 0 with NULL arrays is a pure count.
 *   workspace: dae_threshold_pairs_workspace(Nq, Nc, D, capacity) bytes, 256-byte aligned: the two normalised operand
 *   images, the unsorted records, the sort's scratch and the cursor -- linear in Nq, Nc and capacity, no Nq x Nc term.
 *   Each operand image must stay below 4 GiB.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_threshold_pairs_workspace(int32_t Nq, int32_t Nc, int32_t D, uint64_t capacity);
int dae_threshold_pairs(const float* Q, int64_t ldq, int32_t Nq, const float* C, int64_t ldc, int32_t Nc,
                        int32_t D, int32_t norm, int32_t metric, float threshold, int32_t* rows, int32_t* cols,
                        float* scores, uint64_t capacity, uint64_t* count_host, void* workspace,
                        uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * De-duplication of recommendation lists: the greedy "skip an article too similar to one already selected" pass over every
 * row of a [Nr x L] table of candidate article indices, best first (helpers.dedup_lists; recommend(dedup_threshold=)).
 *   E, lde, Na, D, norm, metric: the article vectors, exactly as the corpus of dae_pairwise_similarity, and the same scores:
 *   s(p, q) of a row is the score dae_pairwise_similarity gives row lists[p] against column lists[q] (the same normalised
 *   image, the same exact-fp32 products over the whole K range -- a score does not depend on where its tile lies).
 *   lists int32 [Nr x ldl], L <= 128 entries per row.  Walking a row front to back, the entry at position p is kept iff no entry
 *   kept at a position q < p has s(p, q) >= threshold (a pair AT the threshold is a duplicate, as in dae_threshold_pairs); the
 *   walk stops after k kept, 1 <= k <= L.  Entries < 0 (the -1 tail of a short row) or >= Na are skipped and never kept.  An
 *   index that occurs twice is compared like any other pair (under cosine: a duplicate of itself).  A NaN score never
 *   qualifies; a NaN threshold is an argument error.
 *   out_idx / out_pos int32 [Nr x ldo], ldo >= k: the kept articles and their positions in the input row, in the row's order;
 *   -1 where fewer than k survive.  counts int32 [Nr x 2]: [2 i] the number kept; [2 i + 1] the number of pairs
 *   q < p < min(k, L) of valid entries with s(p, q) >= threshold -- the duplicate pairs the plain top-k would have shown.
 *   Deterministic: bit-identical run to run, independent of the grid and of the chunking below.
 *   workspace: 256-byte aligned.  It holds the corpus image (below 4 GiB) and the gathered rows of a chunk of lists
 *   (128 x dae_pad(D) x 4 bytes each); dae_dedup_lists_workspace(Nr, Na, D, L) asks for min(Nr, R0) lists, R0 the number whose
 *   rows fill 256 MiB.  Any workspace that holds the image and one list -- dae_dedup_lists_workspace(1, Na, D, L) -- is
 *   accepted: the rows are walked in chunks of as many lists as fit, with the same result.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_dedup_lists_workspace(int32_t Nr, int32_t Na, int32_t D, int32_t L);
int dae_dedup_lists(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t norm, int32_t metric, const int32_t* lists,
                    int64_t ldl, int32_t Nr, int32_t L, int32_t k, float threshold, int32_t* out_idx, int32_t* out_pos,
                    int64_t ldo, int32_t* counts, void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Diversification of recommendation lists: Maximal Marginal Relevance over every row of a [Nr x L] table of candidate article
 * indices, with an optional de-dup threshold and an optional cap on the articles of one label (helpers.diversify_lists,
 * helpers.recommend_diverse).
 *   E, lde, Na, D, norm, metric: the article vectors, exactly as the corpus of dae_pairwise_similarity, and the same scores:
 *   s(q, p) of a row is the score dae_pairwise_similarity gives row lists[q] against column lists[p] (the same normalised image,
 *   the same exact-fp32 products over the whole K range, as in dae_dedup_lists).  The orientation is fixed: row = the selected
 *   article, column = the candidate.
 *   lists int32 [Nr x ldl] and rel fp32 [Nr x ldr], L <= 128 entries per row: the candidates and their relevance, normally what
 *   dae_topk_similarity returned, best first; the rule does not assume that order.  Position p is VALID iff
 *   0 <= lists[p] < Na and rel[p] is finite (NaN and +-inf make it invalid); an invalid position is never selected and never
 *   influences anything.  labels int32 [Na] or NULL; max_per_label >= 0, and > 0 needs labels.
 *   State: m[p] = 0.0f for every position, selected = {}, alive[p] = valid[p].  Each of at most k steps, 1 <= k <= L:
 *     - for every alive p, v[p] = (lambda (x) rel[p]) (-) ((1 (-) lambda) (x) m[p]), (x) and (-) single correctly rounded fp32
 *       operations (no fused multiply-add), 0 <= lambda <= 1;
 *     - the alive p with the largest v[p] is selected, equal values go to the lowest position; val = v[p], near = m[p];
 *       alive[p] = false;
 *     - for every alive p', m[p'] = fmaxf(m[p'], s(p, p')): a NaN score leaves m unchanged, so the penalty is
 *       max(0, max over the selected of s) -- the first pick is the most relevant, a negative similarity earns no bonus;
 *     - threshold finite (+inf: off; NaN is an argument error): every alive p' with s(p, p') >= threshold, an fp32 compare, becomes
 *       not alive -- the rule of dae_dedup_lists as a side condition;
 *     - max_per_label > 0 and c = labels[lists[p]] >= 0: once the number of selected entries with label c equals max_per_label,
 *       every alive p' with that label becomes not alive.  Labels < 0 are never capped;
 *     - stop after k selections or when nothing is alive.
 *   Outputs per row, in selection order, [Nr x ldo], ldo >= k: out_idx (the articles) and out_pos (their positions in the input
 *   row) int32, tail -1; out_val (val) and out_near (near) fp32, tail -inf.  Nothing past column k is written.  counts int32
 *   [Nr x 2]: [2 i] the number selected; [2 i + 1] how many of the selected are NOT among the first k valid positions of the row --
 *   how far the re-rank reached past the plain top-k.
 *   With lambda = 1, no threshold and no cap the result is the stable sort by relevance; with lambda = 1, a threshold T and a
 *   best-first row the selected set is that of dae_dedup_lists.  Deterministic: a row's result depends on its own score tile
 *   alone, bit-identical run to run, independent of the grid and of the chunking below.
 *   workspace: 256-byte aligned; the layout, the size and the chunking of dae_dedup_lists: dae_mmr_lists_workspace(Nr, Na, D, L)
 *   asks for the corpus image (below 4 GiB) and min(Nr, R0) lists, and any workspace that holds the image and one list --
 *   dae_mmr_lists_workspace(1, Na, D, L) -- is accepted, with the same result.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_mmr_lists_workspace(int32_t Nr, int32_t Na, int32_t D, int32_t L);
int dae_mmr_lists(const float* E, int64_t lde, int32_t Na, int32_t D, int32_t norm, int32_t metric, const int32_t* lists,
                  int64_t ldl, const float* rel, int64_t ldr, const int32_t* labels, int32_t max_per_label, int32_t Nr, int32_t L,
                  int32_t k, float lambda, float threshold, int32_t* out_idx, int32_t* out_pos, float* out_val, float* out_near,
                  int64_t ldo, int32_t* counts, void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Label statistics without an N x N matrix: the per-class score histograms of all row pairs (helpers.label_similarity_stats).
 *   Q, ldq, Nq, C, ldc, Nc, D, norm, metric: exactly as dae_threshold_pairs, and the same scores.  labels_q_host int32[Nq] and,
 *   with C, labels_c_host int32[Nc] on the HOST (with C == NULL the corpus and its labels are Q's; labels_c_host is ignored).
 *   A pair (i, j) counts when i < Nq, j < Nc, both labels are >= 0 and, with C == NULL, j < i (the strict lower triangle);
 *   it is "related" when the two labels are equal, "unrelated" otherwise.  In self mode only the tiles on or below the
 *   diagonal are computed.
 *   A score s falls in bin clamp(floor((s - lo) * bins / (hi - lo)), 0, bins - 1), computed in fp32 exactly as written
 *   (IEEE subtract, multiply by (float) bins, divide by the fp32 difference hi - lo); a NaN score is counted in n_nan and in
 *   no bin.  2 <= bins <= dae_pair_hist_max_bins() (2048: the two histograms stay in LDS beside the GEMM's staging ring).
 *   lo >= hi asks for the automatic range, returned in out16: [-1, 1] for cosine; for the linear kernel [-M, M] with
 *   M = (largest row 2-norm of the query image) x (largest row 2-norm of the corpus image), rounded up by one part in 2^20.
 *   lo / hi NaN or infinite are argument errors.
 *   hist_host (host, uint64[2][bins]): related, then unrelated counts -- integers, bit-identical run to run and independent
 *   of the grid.  out16_host (host): [0] n_related, [1] n_unrelated (the histograms' totals), [2] n_nan, [3] sum of the
 *   related scores, [4] of the unrelated ones (fp64, reduced in a fixed shape: bit-identical run to run on one device),
 *   [5] min related, [6] max related, [7] min unrelated, [8] max unrelated (exact fp32 values; NaN, like the sums, where
 *   the class is empty), [9] lo, [10] hi as used, [11] workgroups of the grid, [12] tiles computed, [13..15] NaN.
 *   Synchronises the stream (returns host numbers).
 *   workspace: dae_pair_hist_workspace(Nq, Nc, D, bins) bytes, 256-byte aligned: the two normalised operand images, the
 *   labels, the global histogram and one small record per workgroup -- linear in Nq and Nc, no Nq x Nc term and no
 *   per-pair term.  Each operand image must stay below 4 GiB.
 * ------------------------------------------------------------------------------------------------- */
int32_t dae_pair_hist_max_bins(void);
uint64_t dae_pair_hist_workspace(int32_t Nq, int32_t Nc, int32_t D, int32_t bins);
int dae_pair_hist(const float* Q, int64_t ldq, int32_t Nq, const int32_t* labels_q_host, const float* C, int64_t ldc,
                  int32_t Nc, const int32_t* labels_c_host, int32_t D, int32_t norm, int32_t metric, float lo, float hi,
                  int32_t bins, uint64_t* hist_host, double* out16_host, void* workspace, uint64_t workspace_bytes,
                  void* stream);

/* -------------------------------------------------------------------------------------------------
 * Sparse and chunked operands for top-k and label statistics (helpers.most_similar / label_similarity_stats with chunk_rows=).
 * Every sweep above builds its two normalised, zero-padded fp32 operand images [dae_pad(rows) x dae_pad(D)] inside the call,
 * from dense fp32 rows, and so needs the whole operand dense and below 4 GiB.  The entries here split that: the caller builds
 * the image of a CHUNK of rows -- from dense rows or straight from CSR rows -- and sweeps pairs of images; top-k carries each
 * row's running list from one corpus chunk to the next, the histograms add.  Scores do not depend on the tiling, the top-k
 * order is total and the counts are integers, so the chunked results equal the one-shot ones bit for bit (the fp64 score sums
 * of the label statistics are folded in another order).
 *   dae_sweep_image_bytes(rows, D): the bytes of one image, a multiple of 256.
 *   dae_sweep_image_dense: the image of X [rows x ldx] by the kernel the plain entries use.  dae_sweep_image_csr: the same image,
 *   bit for bit, of CSR rows: indptr int64[rows + 1] points at the chunk's first row and holds offsets into indices int32 / values
 *   fp32 (values NULL: every stored entry is 1); column ids ascending and unique within a row and inside [0, D) (an entry that
 *   is not is dropped, never written).  norm / metric as dae_pairwise_similarity.  image: 256-byte aligned, image_bytes >=
 *   dae_sweep_image_bytes(rows, D), below 4 GiB.  Rows past `rows` are zero.
 *   dae_sweep_image_norm2_max: the largest squared row 2-norm of an image's first `rows` rows in fp64 (host; synchronises).  The
 *   maximum over chunks is the maximum over the operand, so the automatic linear-kernel range of dae_pair_hist can be rebuilt on
 *   the host: M = sqrt(max_q) * sqrt(max_c) * (1 + 2^-20), rounded up to fp32 (1 when that is not positive and finite).
 *   workspace: dae_sweep_image_norm2_max_workspace() bytes, 256-byte aligned.
 *   dae_topk_images: dae_topk_similarity_ex over two prepared images (Ci == NULL: the corpus is Qi, pass Nc == Nq).  Image row i
 *   is query row0 + i and image column j is candidate col0 + j: those global ids are the ones in idx, in the self test
 *   (exclude_self may go with Ci here) and in excl_items; excl_indptr points at the entry of query row0 (offsets into the whole
 *   excl_items).  carry: dae_topk_carry_bytes(Nq, k) bytes, 256-byte aligned -- each row's k sorted keys, then its count; all-zero
 *   bytes are an empty carry.  The call merges the carry with this corpus chunk's candidates, writes the carry back and writes
 *   idx / score from it, so after the last corpus chunk idx / score are those of the one-shot call.  The same k in every call
 *   on one carry.  A full carry's k-th key is the threshold from the first tile on.  Windows and shared lists are not taken.
 *   workspace: dae_topk_images_workspace(Nq, Nc, k) bytes -- NOT monotone in Nq (fewer query tiles get more corpus slices): a caller
 *   that reuses one workspace asks for every block shape it sweeps.
 *   dae_pair_hist_images: dae_pair_hist over two prepared images (Ci == NULL: self mode, the pairs j < i of Qi) with an explicit
 *   range lo < hi; hist_host / out16_host as there.  For the strict lower triangle of a chunked operand: self mode on the
 *   diagonal blocks, Ci = an earlier chunk for the blocks below it.  workspace: dae_pair_hist_images_workspace(Nq, Nc, bins).
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_sweep_image_bytes(int32_t rows, int32_t D);
int dae_sweep_image_dense(const float* X, int64_t ldx, int32_t rows, int32_t D, int32_t norm, int32_t metric, float* image,
                          uint64_t image_bytes, void* stream);
int dae_sweep_image_csr(const int64_t* indptr, const int32_t* indices, const float* values, int32_t rows, int32_t D,
                        int32_t norm, int32_t metric, float* image, uint64_t image_bytes, void* stream);
uint64_t dae_sweep_image_norm2_max_workspace(void);
int dae_sweep_image_norm2_max(const float* image, int32_t rows, int32_t D, double* out_host, void* workspace,
                              uint64_t workspace_bytes, void* stream);
uint64_t dae_topk_carry_bytes(int32_t Nq, int32_t k);
uint64_t dae_topk_images_workspace(int32_t Nq, int32_t Nc, int32_t k);
int dae_topk_images(const float* Qi, int32_t Nq, int32_t row0, const float* Ci, int32_t Nc, int32_t col0, int32_t D, int32_t k,
                    int32_t exclude_self, const int64_t* excl_indptr, const int32_t* excl_items, void* carry, int32_t* idx,
                    float* score, int64_t ldk, void* workspace, uint64_t workspace_bytes, void* stream);
uint64_t dae_pair_hist_images_workspace(int32_t Nq, int32_t Nc, int32_t bins);
int dae_pair_hist_images(const float* Qi, int32_t Nq, const int32_t* labels_q_host, const float* Ci, int32_t Nc,
                         const int32_t* labels_c_host, int32_t D, float lo, float hi, int32_t bins, uint64_t* hist_host,
                         double* out16_host, void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Spherical k-means on the device (helpers.kmeans / kmeans_assign / ClusterIndex): one Lloyd iteration is dae_kmeans_assign
 * followed by dae_kmeans_update.  Both read sweep images the caller built (dae_sweep_image_dense / dae_sweep_image_csr):
 * Xi [dae_pad(N) x dae_pad(D)] of the rows, Ci [dae_pad(K) x dae_pad(D)] of the centroids, 256-byte aligned, each below 4 GiB.
 * Both return host numbers and so synchronise the stream.
 *   dae_kmeans_assign: labels[i] int32 = the centroid j < K with the largest score Xi[i] . Ci[j] (the exact-fp32 products of the
 *   other sweeps), ties to the lower j with -0 and +0 one score (the order of dae_topk_similarity), scores[i] fp32 = that score;
 *   a padded centroid row never wins.  A row whose scores are all -inf or NaN gets label -1, score -inf (dae_topk_similarity
 *   returns a column for -inf and lets a NaN win; on finite scores the two agree bit for bit).  prev_labels int32[N] or NULL.
 *   out_host (host, double[4]): [0] the fp64 sum of scores, folded in a fixed order (a fixed tree per 128 rows, then the tiles
 *   ascending by thread and a fixed tree), [1] the rows whose label differs from prev_labels (N when it is NULL), [2] the grid of
 *   the sweep, [3] its centroid slices per row tile.  Bit-identical from run to run.
 *   workspace: dae_kmeans_assign_workspace(N, K) bytes, 256-byte aligned.
 *   dae_kmeans_update: counts int32[K], offsets int64[K + 1] (the exclusive scan of counts) and order int32[N] -- the row ids
 *   sorted by (label, row id), a stable sort; rows whose label is outside [0, K) take no part and form the tail of order.  For
 *   every cluster with members, s_d = the fp64 sum of its image rows in a fixed order (segments of at most 256 consecutive
 *   members of order, each summed ascending, the segment sums added ascending), n2 = the fp64 sum of s_d^2 in a fixed order, and
 *   centroids[c][d] = fl32(s_d / sqrt(n2)) for d < D (centroids fp32 [K x ldc], ldc >= D).  A cluster without members, or with
 *   n2 == 0, keeps its row.  centroids == NULL: counts / offsets / order alone.  No floating-point atomics: bit-identical from run
 *   to run.  out_host (host, double[4]): [0] rows left out, [1] clusters without members, [2] clusters with members and n2 == 0,
 *   [3] segments.  workspace: dae_kmeans_update_workspace(N, K, D) bytes, 256-byte aligned; the size includes the scratch
 *   rocprim asks for on the current device, so ask on the device that runs the call (0: the query failed, and so will the call).
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_kmeans_assign_workspace(int32_t N, int32_t K);
int dae_kmeans_assign(const float* Xi, int32_t N, const float* Ci, int32_t K, int32_t D, const int32_t* prev_labels,
                      int32_t* labels, float* scores, double* out_host, void* workspace, uint64_t workspace_bytes, void* stream);
uint64_t dae_kmeans_update_workspace(int32_t N, int32_t K, int32_t D);
int dae_kmeans_update(const float* Xi, int32_t N, int32_t D, const int32_t* labels, int32_t K, float* centroids, int64_t ldc,
                      int32_t* counts, int32_t* order, int64_t* offsets, double* out_host, void* workspace,
                      uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Co-visitation, the item-to-item baseline (helpers.covisit_neighbors / CovisitIndex): "readers of this article also read ...",
 * from co-clicks alone -- no embeddings, no Na x Na matrix (emit -> sort -> run-length -> select; csrc/dae_covisit.hip).
 * The log is a history CSR: indptr int64[M + 1], items int32[nnz], oldest click first, over Na articles.
 *   records: for every user and every pair of positions p < q <= p + window of that user's history, a = items[p], b = items[q]:
 *   if a != b the record (a, b), and with both = 1 also (b, a).  Equal items emit nothing; a repeat of an article is an ordinary
 *   click.  (An item outside [0, Na) is no click and pairs with nothing.)  c[a, b] = the number of records (a, b); clicks[a] = the
 *   occurrences of a in items; degree[a] = the number of distinct b with c[a, b] > 0.
 *   similarity, fp32 with one rounding per operation: normalize 0 (none) s = (float) c; normalize 1 (cosine)
 *   s = (float) c / sqrtf((float) clicks[a] * (float) clicks[b]) -- a correctly rounded product, root and quotient, so the table
 *   equals a NumPy float32 restatement bit for bit.
 *   table: row a holds its min(K, degree[a]) best neighbours by (s descending, b ascending) as nbr int32 / sim fp32 / cnt int32
 *   [Na x ld], ld >= K; the tail of a row is -1 / 0 / 0; columns K .. ld are not touched.  1 <= K <= 128, window >= 1.
 *   dae_covisit_record_bound (host only, no GPU): sum over the users and p of min(window, L - 1 - p), doubled for both -- the number
 *   of records when no pair has equal items, and an upper bound otherwise.  0 for M <= 0 or window < 1.
 *   dae_covisit_neighbors: indptr / items on the device, indptr_host a host copy of indptr: the call takes the bound from it and
 *   checks the workspace against it before anything is launched, and a record is stored only below the bound, so the record
 *   buffers cannot be overrun.  degree / clicks int32[Na]; totals int64[2] (device): records emitted, distinct pairs.  All integer
 *   counts (the click counts and the record cursor use integer atomics: exact), every float one fixed chain of roundings: the
 *   outputs are bit-identical from run to run and do not depend on the order of the users or on the workspace size.  Rows are
 *   skewed, so a row of up to 256 distinct neighbours is selected by one wave and a longer one by a whole workgroup in passes.
 *   M == 0, nnz == 0 or a bound of 0 (no history of two clicks): tails and zeros, no workspace needed.  The call synchronises.
 *   memory: dae_covisit_neighbors_workspace(record_bound, Na, K) = 20 bytes per record of the bound (two 8-byte key buffers and
 *   the 4-byte run counts) + 8 (Na + 1) + the scratch rocprim asks for on the current device (0: bound 0, a bad argument or a
 *   failed query); 256-byte aligned.  One call takes a bound below 2^31 records; a larger log has to be built from fewer users
 *   (merging count tables of user batches is not provided).
 *   dae_covisit_recommend: per user u of a query CSR (indptr int64[M + 1], items int32; need not be the log of the table) the
 *   sources are the last min(last, L) clicks, walked oldest first; the source of age j (0: the newest click) with item x adds
 *   __fmul_rn(age_weight[j], sim[x, t]) to the fp32 accumulator of candidate nbr[x, t] for every filled slot t, with __fadd_rn
 *   from 0 in the order of the sources; an article clicked twice among them contributes twice.  A candidate is any article
 *   reached, whatever its sum, that is not in the user's seen list (seen_indptr int64[M + 1], seen_items int32: every row ascending
 *   and unique -- helpers.normalize_exclusions) and, with win_lo / win_hi int32[M] (both or neither), has win_lo[u] <= c <
 *   win_hi[u].  idx int32 / score fp32 [M x ldo], ldo >= k: the k best by (score descending, index ascending), -0 and +0 one
 *   score, tail -1 / -inf (the convention of dae_topk_similarity); columns k .. ldo are not touched.  1 <= last <= 32, 1 <= k <=
 *   128, age_weight fp32[last] on the device.  One workgroup per user, at most last * K <= 4096 entries in 48 KiB of LDS; no
 *   workspace, no synchronisation.  Bit-identical from run to run.
 * Argument errors are reported before any HIP call, with the prefixes "covisit_neighbors: " / "covisit_recommend: ".
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_covisit_record_bound(const int64_t* indptr_host, int32_t M, int32_t window, int32_t both);
uint64_t dae_covisit_neighbors_workspace(uint64_t record_bound, int32_t Na, int32_t K);
int dae_covisit_neighbors(const int64_t* indptr, const int32_t* items, const int64_t* indptr_host, int32_t M, int64_t nnz,
                          int32_t Na, int32_t window, int32_t both, int32_t normalize, int32_t K, int32_t* nbr, float* sim,
                          int32_t* cnt, int64_t ld, int32_t* degree, int32_t* clicks, int64_t* totals, void* workspace,
                          uint64_t workspace_bytes, void* stream);
int dae_covisit_recommend(const int32_t* nbr, const float* sim, int64_t ld, int32_t Na, int32_t K, const int64_t* indptr,
                          const int32_t* items, int32_t M, const int64_t* seen_indptr, const int32_t* seen_items,
                          const int32_t* win_lo, const int32_t* win_hi, const float* age_weight, int32_t last, int32_t k,
                          int32_t* idx, float* score, int64_t ldo, void* stream);

/* -------------------------------------------------------------------------------------------------
 * The word-based user model, the baseline of "Embedding-based News Recommendation for Millions of Users" (section 5.1;
 * helpers.word_profiles / word_recommend / word_ranks; csrc/dae_words.hip).  An article is the set of its words: row a of a CSR
 * matrix [Na x V] (art_indptr int64[Na + 1], art_indices int32[nnz] ascending and unique per row, values fp32[nnz] or NULL: all
 * ones).  A user is the set of the words of the articles clicked; the relevance is a weighted count of the words the two share.
 *   profile: word w is in profile(u) when some article among the last max_events clicks of user u (history CSR hist_indptr
 *   int64[M + 1], hist_items int32[hist_nnz], oldest first; max_events 0: every click) stores column w -- explicit zeros count,
 *   repeated clicks change nothing.  An item outside [0, Na) and a column outside [0, V) are dropped, never written.
 *   bitmaps: word-major per tile of 128 users, uint32 [ceil(M / 128)][V][4]; bit (u & 31) of word (u & 127) >> 5 of cell
 *   (u >> 7, w) says "user u has word w".  dae_word_profiles_bytes(M, V) = ceil(M / 128) * V * 16 bytes; 16-byte aligned.
 *   dae_word_profiles zeroes the bitmaps, sets the bits with integer atomicOr (exact, whatever the schedule) and writes
 *   sizes int32[M], the number of distinct words of every profile, from a bit-counting pass over the bitmaps (no atomics).
 *   entry weights: dae_word_entry_weights writes weights fp32[nnz] once per stored entry p with column c_p and value x_p (1 without
 *   values): e_p = x_p when term_weights is NULL, else __fmul_rn(term_weights[c_p], x_p) (term_weights fp32[V]); +0 for a column
 *   outside [0, V).  dae_word_entry_weights_bytes(nnz) = the size of that array.
 *   score: R(u, a) = s_n with s_0 = +0 and s_i = __fadd_rn(s_{i-1}, c_i in profile(u) ? e_i : +0) over a's entries in storage
 *   order -- the sequential fp32 sum of the co-occurring entry weights, nothing contracted.  With values = term_weights = NULL it
 *   is the co-occurrence count, an exact integer.
 *   dae_word_topk: per user the k best articles by (score descending, index ascending), -0 and +0 one score (the order and the
 *   outputs of dae_topk_similarity: idx int32 / score fp32 [M x ldk], tail -1 / -inf, 1 <= k <= 128).  excl_indptr int64[M + 1] /
 *   excl_items int32 (both or neither; every row ascending and unique): an excluded article never takes one of the k slots.
 *   win_lo / win_hi int32[M] (both or neither): user u admits the articles win_lo[u] <= a < win_hi[u], clamped to [0, Na].
 *   grid = (user tiles) x (corpus slices); per 128-article tile a thread keeps 64 users' partial scores of one article in
 *   registers, the tile's CSR rows are staged through LDS, and every entry costs one 8-byte mask load and 64 select-adds; the
 *   epilogue and the merge are those of dae_topk_similarity.  dae_word_topk_workspace(M, Na, k) = the slices' partial lists.
 *   dae_word_rank: rank[u] = 1 + #{ a < Na, a != t, a not in u's list, a in u's window : key(R(u, a), a) > key(R(u, t), t) } for
 *   t = targets[u] (the definition at the top of csrc/dae_rank.hip on these scores); target_score[u] = R(u, t), bit-equal to the
 *   score dae_word_topk writes for that pair.  t < 0 (or >= Na): rank 0, target_score -inf.  The target is ranked whether or not
 *   the list or the window holds it (the caller decides what such a rank means).  Integer atomics only.
 *   dae_word_rank_workspace(M) = one key per user.
 *   Every row range read from art_indptr / hist_indptr is clamped to [0, nnz] / [0, hist_nnz].  The results are bit-identical
 *   from run to run and independent of the workspace size and of the order of the users.  No call synchronises.
 * Argument errors are reported before any HIP call, with the prefixes "word_profiles: " / "word_entry_weights: " / "word_topk: " /
 * "word_rank: ".
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_word_profiles_bytes(int32_t M, int32_t V);
int dae_word_profiles(const int64_t* hist_indptr, const int32_t* hist_items, int64_t hist_nnz, int32_t M, int32_t max_events,
                      const int64_t* art_indptr, const int32_t* art_indices, int64_t nnz, int32_t Na, int32_t V, void* bitmaps,
                      uint64_t bitmap_bytes, int32_t* sizes, void* stream);
uint64_t dae_word_entry_weights_bytes(int64_t nnz);
int dae_word_entry_weights(const int32_t* art_indices, const float* art_values, int64_t nnz, int32_t V, const float* term_weights,
                           float* weights, void* stream);
uint64_t dae_word_topk_workspace(int32_t M, int32_t Na, int32_t k);
int dae_word_topk(const void* bitmaps, int32_t M, int32_t V, const int64_t* art_indptr, const int32_t* art_indices,
                  const float* weights, int64_t nnz, int32_t Na, int32_t k, const int64_t* excl_indptr, const int32_t* excl_items,
                  const int32_t* win_lo, const int32_t* win_hi, int32_t* idx, float* score, int64_t ldk, void* workspace,
                  uint64_t workspace_bytes, void* stream);
uint64_t dae_word_rank_workspace(int32_t M);
int dae_word_rank(const void* bitmaps, int32_t M, int32_t V, const int64_t* art_indptr, const int32_t* art_indices,
                  const float* weights, int64_t nnz, int32_t Na, const int64_t* excl_indptr, const int32_t* excl_items,
                  const int32_t* win_lo, const int32_t* win_hi, const int32_t* targets, int32_t* rank, float* target_score,
                  void* workspace, uint64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Implicit-feedback matrix factorisation by alternating least squares (helpers.fit_als / ALSModel; Hu, Koren, Volinsky 2008;
 * csrc/dae_als.hip).  r_ui = the number of times user u clicked article i, c_ui = 1 + alpha r_ui, p_ui = [r_ui > 0];
 *   L = sum over ALL u, i of c_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2), X fp32 [M x F], Y fp32 [Na x F], 1 <= F <= 128.
 * One half-sweep holds Y and solves A_u x_u = b_u for every row u of a CSR (ptr int64[R + 1], idx int32, cnt int32):
 *   A_u = G + sum_j alpha cnt_j y_j y_j^T,  G = Y^T Y + lambda I,  b_u = sum_j (1 + alpha cnt_j) y_j,  j over the row's entries,
 * by cg_steps steps of conjugate gradient from the row's current factor; A_u is never formed.  The other half-sweep is the same
 * call on the other orientation with X and Y swapped.
 *   dae_als_interactions: the history CSR (indptr int64[M + 1], items int32[nnz], on the device) as both orientations of the
 *   de-duplicated interaction matrix: user_ptr int64[M + 1], user_idx / user_cnt int32 (per user the distinct articles ascending
 *   and how often each was clicked), item_ptr int64[Na + 1], item_idx / item_cnt (per article its distinct users ascending).
 *   The idx / cnt buffers hold cap >= nnz cells; only the first `distinct pairs` cells are written.  totals int64[2] (device):
 *   events, distinct pairs.  An item outside [0, Na) is no event.  Integer arithmetic only: 64-bit keys, rocprim radix sort over
 *   the bits in use, run-length encode, row offsets by binary search.  nnz < 2^31 per call.  workspace:
 *   dae_als_interactions_workspace(nnz, M, Na) = 24 bytes per event + the scratch rocprim asks for on the current device (0:
 *   nnz 0, a bad argument or a failed query); 256-byte aligned; nnz == 0 needs none.  The call synchronises.
 *   dae_als_gram: G fp32 [F x F] (contiguous) = fl32(Y^T Y + lambda I) of Y fp32 [N x ldy]: fp64 sums over
 *   nb = min(256, ceil(N / 64)) blocks of ceil(N / nb) consecutive rows, each block ascending, the blocks added ascending, lambda
 *   added in fp64, one rounding to fp32.  workspace: dae_als_gram_workspace(N, F) = 8 nb F^2 bytes.
 *   dae_als_solve_rows: X fp32 [R x ldx] updated in place from Y fp32 [N x ldy] (X and Y must differ), ldx, ldy >= F; columns
 *   F .. ld are not touched.  1 <= cg_steps <= 32.  Per row, in fp32 with one rounding per operation (no contraction):
 *     no entries: x = 0 exactly.  Otherwise r = b - A x, p = r, rs = r . r; per step: stop if rs <= 1e-20; Ap = A p; stop unless
 *     p . Ap > 0; a = rs / (p . Ap); x += a p; r -= a Ap; rs' = r . r; p = r + (rs' / rs) p; rs = rs'.
 *   A v = G v + sum_j (alpha cnt_j) (y_j . v) y_j is one sum of scaled rows -- the rows of G ascending, then the entries in stored
 *   order; an entry whose index lies outside [0, N) adds nothing.  The terms are dealt round-robin to Gt groups of lanes, each
 *   group adds its terms in that order, and the group sums are added in a fixed tree.  Gt depends on F and on whether the row has
 *   at most 256 entries (one wave per row) or more (one workgroup of 16 waves per row) -- on the row's length and on nothing else:
 *   not on the row's position, its neighbours in the launch or the workspace.  No floating-point atomics: bit-identical from run
 *   to run and under any permutation of the rows.  workspace: dae_als_solve_rows_workspace(R) = 256 + 4 R bytes (the list of
 *   the long rows).  No synchronisation.
 *   dae_als_loss: *loss (device, double) = L above without the M x Na matrix,
 *     L = <X^T X, Y^T Y> + sum over the stored entries of [c (1 - s)^2 - s^2] + lambda (|X|^2 + |Y|^2),  s = x_u . y_i,
 *   all in fp64: both Grams by the kernels of dae_als_gram, one partial per row of X (its entries and lambda |x_u|^2), one per row
 *   of Y, one per Gram cell, summed in a fixed order (256 chunks, then one).  alpha and lambda are the fp32 numbers the solve and
 *   the Gram were given.  workspace: dae_als_loss_workspace(R, N, F).  No synchronisation.
 * Argument errors are reported before any HIP call, with the prefixes "als_interactions: " / "als_gram: " / "als_solve_rows: " /
 * "als_loss: ".
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_als_interactions_workspace(int64_t nnz, int32_t M, int32_t Na);
int dae_als_interactions(const int64_t* indptr, const int32_t* items, int32_t M, int64_t nnz, int32_t Na, int64_t* user_ptr,
                         int32_t* user_idx, int32_t* user_cnt, int64_t* item_ptr, int32_t* item_idx, int32_t* item_cnt, int64_t cap,
                         int64_t* totals, void* workspace, uint64_t workspace_bytes, void* stream);
uint64_t dae_als_gram_workspace(int32_t N, int32_t F);
int dae_als_gram(const float* Y, int64_t ldy, int32_t N, int32_t F, float lambda, float* G, void* workspace, uint64_t workspace_bytes,
                 void* stream);
uint64_t dae_als_solve_rows_workspace(int32_t R);
int dae_als_solve_rows(const int64_t* ptr, const int32_t* idx, const int32_t* cnt, int32_t R, const float* Y, int64_t ldy, int32_t N,
                       int32_t F, const float* G, float alpha, int32_t cg_steps, float* X, int64_t ldx, void* workspace,
                       uint64_t workspace_bytes, void* stream);
uint64_t dae_als_loss_workspace(int32_t R, int32_t N, int32_t F);
int dae_als_loss(const int64_t* ptr, const int32_t* idx, const int32_t* cnt, int32_t R, const float* X, int64_t ldx, const float* Y,
                 int64_t ldy, int32_t N, int32_t F, float alpha, float lambda, double* loss, void* workspace, uint64_t workspace_bytes,
                 void* stream);

/* -------------------------------------------------------------------------------------------------
 * From a count matrix to the training input (helpers.column_stats / limit_features / select_columns / TfidfTransformer): what
 * sklearn's CountVectorizer._limit_features and TfidfTransformer do to a bag of words, on CSR rows that stay on the device.
 * CSR as dae_sweep_image_csr: indptr int64[rows + 1] points at the chunk's first row and holds offsets into indices int32 /
 * values fp32 (values NULL: every stored entry is 1); column ids ascending and unique within a row.  An entry whose column
 * lies outside [0, F) is dropped and counted.  Every call returns host numbers and so synchronises the stream.
 *   dae_csr_column_stats: df[c] += stored entries of column c (explicit zeros count, as sklearn's _document_frequency counts
 *   them), tf[c] += sum of the column's counts; both int64[F] on the device.  The call ADDS, so a corpus can be passed in row
 *   chunks: zero both before the first.  The counts are added as integers by integer atomics: exact, independent of scheduling.
 *   counts2_host (host, uint64[2]): [0] entries in range whose value is not an integer in [0, 2^24] (nothing is added to tf for
 *   them; df counts them), [1] entries dropped for their column (not looked at further).
 *   workspace: dae_csr_column_stats_workspace() bytes, 256-byte aligned.
 *   dae_csr_select_columns: the rows with the columns renumbered by remap int32[F] (device; -1: the column is dropped; the kept
 *   columns map increasingly, so a row stays ascending): count per row, exclusive scan, fill.  out_indptr int64[rows + 1] is
 *   always written; out_indices int32 / out_values fp32 hold `capacity` entries (out_values may be NULL: the structure alone;
 *   values NULL writes ones).  out2_host (host, int64[2]): [0] the new nnz, [1] entries dropped for their column.  When the
 *   new nnz exceeds capacity the call returns 1 with out2_host set and writes nothing to out_indices / out_values; it never
 *   writes past them.  workspace: dae_csr_select_columns_workspace(rows) bytes, 256-byte aligned.
 *   dae_tfidf_transform: sklearn's TfidfTransformer.transform.  idf fp32[F] on the device (NULL: use_idf=False) -- computed
 *   on the host in fp64 from the integer df and rounded once; sublinear 0 | 1; norm 0 none, 1 l1, 2 l2.  Per entry
 *   v = fl32(t * idf[c]) with t the count, or fl32(1 + log((double) count)) when sublinear; the row norm (sum |v|, or the
 *   square root of the sum of v^2) is summed in fp64 in an order fixed by the row alone; the result is fl32((double) v / norm).
 *   A row whose norm is 0 or not finite keeps its v.  A dropped entry takes no part in the norm and its output is 0.
 *   out_values fp32 (as long as values) may be values.  Bit-identical from run to run.  dropped_host (host, uint64[1]).
 *   workspace: dae_tfidf_transform_workspace() bytes, 256-byte aligned.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dae_csr_column_stats_workspace(void);
int dae_csr_column_stats(const int64_t* indptr, const int32_t* indices, const float* values, int32_t rows, int32_t F, int64_t* df,
                         int64_t* tf, uint64_t* counts2_host, void* workspace, uint64_t workspace_bytes, void* stream);
uint64_t dae_csr_select_columns_workspace(int32_t rows);
int dae_csr_select_columns(const int64_t* indptr, const int32_t* indices, const float* values, int32_t rows, int32_t F,
                           const int32_t* remap, int64_t* out_indptr, int32_t* out_indices, float* out_values, uint64_t capacity,
                           int64_t* out2_host, void* workspace, uint64_t workspace_bytes, void* stream);
uint64_t dae_tfidf_transform_workspace(void);
int dae_tfidf_transform(const int64_t* indptr, const int32_t* indices, const float* values, int32_t rows, int32_t F,
                        const float* idf, int32_t sublinear, int32_t norm, float* out_values, uint64_t* dropped_host,
                        void* workspace, uint64_t workspace_bytes, void* stream);

/* Related / unrelated pair statistics of an N x N similarity matrix: the numbers behind
 * helpers.visualize_pairwise_similarity (helpers.py:79-135) -- AUROC of "same label" vs "different label" over the strict
 * lower triangle (labels < 0 are missing and drop their pairs; ties count half, as sklearn's roc_curve + auc do) and the
 * box-plot statistics of the two score populations.
 *   S [N x lds] fp32 on the device; labels_host int32[N] on the HOST (the class sizes come from its histogram);
 *   out16 (host): [0] auroc, [1] n_related, [2] n_unrelated, [3] mean related, [4] mean unrelated,
 *                 [5..9] related min, q1, median, q3, max, [10..14] unrelated min, q1, median, q3, max (numpy 'linear'
 *                 percentiles); NaN where a population is empty.
 * Synchronises the stream (returns host numbers).  workspace: dae_pair_stats_workspace(N) bytes, 256-byte aligned. */
uint64_t dae_pair_stats_workspace(int32_t N);
int dae_pair_stats(const float* S, int64_t lds, const int32_t* labels_host, int32_t N, double* out16, void* workspace,
                   uint64_t workspace_bytes, void* stream);

int      dae_plan_create(const dae_config* cfg, dae_plan** out);
void     dae_plan_destroy(dae_plan* p);
uint64_t dae_plan_workspace_bytes(const dae_plan* p);
int      dae_plan_bind(dae_plan* p, const dae_buffers* bufs);
/* refresh W_lo / Wt_lo from W (after set_params / checkpoint restore) */
int      dae_plan_sync_shadows(dae_plan* p, void* stream);
/* Code-path choice of a plan, for A/B measurements and equivalence tests (every option selects between implementations of the
 * same arithmetic; the library never reads the environment).  Names: "encode_sparse" (CSR inputs: fused corrupt + gather + encode on the stored
 * entries, dae_encode_csr -- default on; 0 = dense MFMA encode GEMM), "encode_bits" (dense path: x~ as a bit image into the encode
 * GEMM; on by default for binary CSR + bf16), "x_bits" (clean rows as a bit image into the decode epilogue), "fused_opt" (optimizer in the
 * dW GEMM's epilogue), "tail" (bias gradients + statistics + x~^T un-scatter in one launch), "label_with_encode", "ce_literal"
 * (cross_entropy always by the reference-literal formula), "gather_tile" (process-wide: tile of the dense-ndarray gather, bit 0 = 128
 * features instead of 64, bit 1 = 128 rows instead of 64; 0 is the measured best), "miner_tile" (process-wide: 1 = lane-grid batch_all kernel,
 * default), "miner_order" / "miner_ranges" / "sym_in_decode" (side jobs riding on other launches), "gram_fp32" (exact-fp32 Gram
 * matrix in bf16 mode; before dae_plan_bind only), "miner_pack"
 * (batch_all workgroups = one resident round, each walking the anchor list in snake order; 0 = one workgroup per anchor), "encode_w32" (bf16 mode: the
 * sparse encode reads the fp32 master weights, so h -- and with the split-bf16 Gram matrix the triplet leg -- is fp32-accurate; default
 * on; a sharded-optimizer exchange must turn it off because only W_lo is current on every rank), "encode_w32_cols" (128 | 64 columns
 * per workgroup of that kernel), "x3_dec_wlo" / "x3_dh_hlo" (split-bf16 mode, before dae_plan_bind only, default 1: the decode multiplies
 * (h_hi, W_lo) and the dh GEMM (Gs, h^T_lo) too; 0 drops the term -- a CPU replay of the 20-step curve called both droppable, the GPU run against
 * the frozen reference curve then measured cost 7.0e-5 / triplet 1.56e-4, outside the 1e-4 gate, so they stay on: profiles/r04_precision_terms.txt;
 * with x3_dec_wlo = 0 the dW epilogue skips the lo image of the row-major shadow, which only that decode term reads), "dw_pair" (split-bf16 mode: the dW kernel runs the K segments that share their A operand
 * -- x~^T . [delta1^T_hi ; delta1^T_lo], delta2^T_hi . [h^T_hi ; h^T_lo] -- as paired ring stages of one A tile and two B tiles; default 1, 0 = one
 * segment after the other), "x3_terms" (split mode, before dae_plan_bind only: bit mask of the lo product terms that are multiplied -- bit 0 decode
 * (h_hi, W_lo), 1 decode (h_lo, W_hi), 2 dh (delta2_hi, W^T_lo), 3 dh (delta2_lo, W^T_hi), 4 dh (Gs, h^T_lo), 5 dW (x~^T, delta1^T_lo), 6 dW (delta2^T_hi,
 * h^T_lo), 7 dW (delta2^T_lo, h^T_hi), 8 / 9 dense-input encode (x~_hi, W^T_lo) / (x~_lo, W^T_hi), 10 lo images of valued inputs (clean rows, x~^T); default
 * all (bf16 storage) or bits 0 and 2 (fp16 storage); a lo image whose terms are all off is neither written nor allocated), "op_scale_log2" (16-bit modes:
 * the images of delta2, delta2^T, Gs and delta1^T hold 2^value times the quantity and the consuming epilogues divide it out; default 0 for bf16 storage,
 * log2 of the largest power of two <= 16 * max_batch (at most 14) for fp16 storage, whose normal range ends at 6.1e-5), "gram64" (16-bit modes, before
 * dae_plan_bind: the split Gram matrix on 64 x 64 tiles over the whole K, ONE slab -- default 1; 0 = 128 x 128 tiles, split-K slabs summed by the miner),
 * "decode_bn" (16-bit modes, before dae_plan_bind: tile width of the decode kernel, 64 | 128 | 0 = by tile count: 128 once the 64-column tiles are more than
 * four rounds of the chip, i.e. F = 50000), "decode_bm" (tile height of the decode kernel, 0 | 128 | 160: 160 = the 160 x 128 tiles of the three-term 16-bit
 * decode with a bit image of x, an error for a plan whose mode or loss has no such kernel; 0 = 160 where that kernel exists and its grid is one resident
 * round of the chip while the 128 x 64 grid is not, e.g. B = 800 at F = 10000), "dw_tr" (-1 | 0 | 1: the dW kernel reads x~ and delta2 row-major through transposing LDS reads, so that
 * delta2^T / x~^T are never written; -1 = for dense train sets only, where it was measured faster), "dw_rounds" (process-wide: rounds of the chip the fused
 * 160 x 128 dW + optimizer kernel may take, default 16 for the split modes / 1 otherwise), "pad_skip" (process-wide, default 1: the decode epilogue does not
 * evaluate the loss of 32-row blocks that are pure batch padding).  Unknown names are an error. */
int      dae_plan_set_option(dae_plan* p, const char* name, int32_t value);
/* 16-bit storage format the loaded library was built for: 0 = bfloat16 (libdae_hip.so), 1 = IEEE fp16 (libdae_hip_f16.so: the same sources compiled with
 * -DDAE_F16=1; every 16-bit image and the MFMA that multiplies it switch together).  DAE_BF16 / DAE_BF16X3 name "the 16-bit format" in either build. */
int32_t  dae_storage_format(void);
int      dae_train_step(dae_plan* p, const dae_step* step, void* stream);
int      dae_plan_apply(dae_plan* p, int32_t adam_t, float grad_scale, void* stream);
/* dae_plan_apply restricted to the rows [f0, f1) of W (multiples of 64; every low-precision image of those rows is rebuilt): the bucketed form of the
 * data-parallel all-reduce applies band k while band k + 1 is still being reduced.  The band with f1 == Fp also updates the biases. */
int      dae_plan_apply_band(dae_plan* p, int32_t adam_t, float grad_scale, int32_t f0, int32_t f1, void* stream);
/* Data parallel with a SHARDED optimizer: after dae_train_step(phase = 1) the ranks reduce-scatter the W part of the flat gradient
 * by row chunks and all-reduce its (small) bias part; every rank then updates the rows [f0, f1) it owns from grad_rows (fp32
 * [f1-f0 x Hp], rank-summed) and -- update_bias != 0 -- the biases, all-gathers W_lo and rebuilds Wt_lo = W_lo^T locally
 * (dae_plan_refresh_wt).  Per step and rank this moves 1/2 (fp32 gradients) to 1/4 (bf16 gradients) of an fp32 all-reduce. */
int      dae_plan_apply_rows(dae_plan* p, int32_t adam_t, float grad_scale, const float* grad_rows, int32_t f0, int32_t f1,
                             int32_t update_bias, void* stream);
int      dae_plan_refresh_wt(dae_plan* p, void* stream);

/* Packed exchange of the data-parallel step (two collectives per step instead of three, no copy, one rebuild kernel):
 *   dae_plan_apply_rows_packed: the sharded optimizer step of dae_plan_apply_rows, but the low-precision rows of [f0, f1) are written
 *     into the all-gather SEND buffer (row f at send + (f - f0) * Hp * elem) and this rank's LOCAL bias gradients (Hp + Fp floats) are
 *     copied to send + bias_off_bytes; the biases are not updated.
 *   dae_plan_dp_unpack: after all-gathering the send buffers into recv (world chunks of chunk_stride_bytes): W_lo <- the rows,
 *     Wt_lo <- their transpose, and the biases are updated from the rank-ordered sum of the gathered bias gradients (every rank
 *     computes the same sum).  dae_dp_unpack is the plan-free form. */
/* Data parallel: `stream` waits until the W gradient of the last enqueued dae_train_step is complete (an event between the dW GEMM and
 * the step's tail kernel), so that a reduce-scatter issued on `stream` runs beside the tail.  The first call only creates the event and
 * returns DAE_WAIT_DW_CREATED (not an error, dae_last_error untouched; steps enqueued earlier are not covered: wait for the step's
 * stream instead); 0 = the wait was enqueued; any other value is an error. */
#define DAE_WAIT_DW_CREATED 100   /* outside the error codes (1 = bad argument, 2 = HIP failure) */
int dae_plan_stream_wait_dw(dae_plan* plan, void* stream);
int dae_plan_apply_rows_packed(dae_plan* plan, int32_t adam_t, float grad_scale, const float* grad_rows, int32_t f0, int32_t f1,
                               void* send, int64_t bias_off_bytes, void* stream);
int dae_plan_dp_unpack(dae_plan* plan, const void* recv, int32_t world, int32_t chunk_rows, int64_t chunk_stride_bytes,
                       int64_t bias_off_bytes, int32_t adam_t, float grad_scale, void* stream);
int dae_dp_unpack(const void* recv, int32_t world, int32_t chunk_rows, int64_t chunk_stride_bytes, int64_t bias_off_bytes,
                  int32_t Fp, int32_t Hp, int32_t dtype, void* W_lo, void* Wt_lo, int32_t opt, float lr, float momentum,
                  float grad_scale, float* bh, float* bv, float* s1b, float* s2b, float* grad_b, void* stream);
/* -------------------------------------------------------------------------------------------------
 * The data-parallel collective in the C ABI (SURVEY 8(b) proposed `dae_allreduce_grads`; SURVEY 8(e): all-reduce(sum) of the flat gradient
 * [dW | dbh | dbv] over xGMI, then the identical optimizer step on every rank).  Shards the reference's per-mini-batch step,
 * autoencoder/autoencoder.py:206-246 (one session.run), over one process per GPU.
 *
 *   dae_comm_unique_id   rank 0 draws a DAE_COMM_ID_BYTES id (ncclGetUniqueId) and shares it with the other ranks over any out-of-band
 *                        channel the host has (a file, a socket, torch.distributed's store, MPI).
 *   dae_comm_init        every rank, on its own device (the calling thread's current HIP device): ncclCommInitRank.  world = 1 is valid (a
 *                        one-rank communicator: the exchange then equals dae_plan_apply).  RCCL is located with dlopen at this point -- a
 *                        copy already loaded into the process is shared, else librccl.so.1 of the ROCm install -- so single-GPU users of the
 *                        library never load it; a missing RCCL is an error here, not at load time.
 *   dae_allreduce_grads  in-place ncclAllReduce(sum, fp32) of the plan's flat gradient, enqueued on `stream` -- the stream the step's kernels
 *                        run on: no process-group stream, no cross-stream hop, no host synchronisation.
 *   dae_dp_exchange      all-reduce + optimizer, i.e. everything behind dae_train_step(phase = 1).  buckets <= 1: dae_allreduce_grads +
 *                        dae_plan_apply back to back on `stream`.  buckets > 1 (at most DAE_COMM_MAX_BUCKETS): the flat buffer is reduced in
 *                        row bands of W (dae_dp_bands) on the communicator's own wire stream -- the W-only bands start behind the dW GEMM,
 *                        beside the step's tail kernel; the last band (it carries the bias gradients) behind the tail -- and `stream`
 *                        applies band k (dae_plan_apply_band) while band k + 1 is on the wire.  Same sums, same update as one bucket.
 *   dae_dp_bands         the band boundaries (host arithmetic; bounds[0 .. n], bounds[n] = Fp), returns n.
 *   dae_comm_allreduce_f32  the bare collective on a caller buffer (op 0 = sum, 1 = max): loss normalisers, "ranks seen" tokens, timings.
 * Return codes as everywhere (0 ok, 1 bad argument, 2 HIP failure) plus 3 = RCCL failure; text in dae_last_error().
 * ------------------------------------------------------------------------------------------------- */
#define DAE_COMM_ID_BYTES 128
#define DAE_COMM_MAX_BUCKETS 8
typedef struct dae_comm dae_comm;
int         dae_comm_unique_id(void* id_out);
int         dae_comm_init(const void* id, int32_t rank, int32_t world, dae_comm** out);
void        dae_comm_destroy(dae_comm* c);
/* out4 = {rank, world, RCCL version code, DAE_COMM_MAX_BUCKETS} */
int         dae_comm_info(const dae_comm* c, int32_t* out4);
/* which RCCL the library resolved ("" before the first dae_comm_unique_id / dae_comm_init) */
const char* dae_comm_library(void);
int         dae_comm_allreduce_f32(dae_comm* c, float* buf, int64_t n, int32_t op, void* stream);
int32_t     dae_dp_bands(int32_t Fp, int32_t buckets, int32_t* bounds);
int         dae_allreduce_grads(dae_plan* p, dae_comm* c, void* stream);
int         dae_dp_exchange(dae_plan* p, dae_comm* c, int32_t adam_t, float grad_scale, int32_t buckets, void* stream);

/* transform(): out[B x H] fp32 (ld_out) = encode of rows row_idx (autoencoder.py:479-505) */
int      dae_encode_rows(dae_plan* p, const int32_t* row_idx, int32_t B, float scale,
                         const int64_t* indptr, const int32_t* indices, const float* values,
                         const float* dense, int64_t ld_dense, float* out, int64_t ld_out, void* stream);
/* pointers into the workspace for tests / debugging (NULL if name unknown) */
void*    dae_plan_buffer(dae_plan* p, const char* name);
/* Per-kernel timing of dae_train_step with HIP events recorded on the step's own stream (bench.py's
 * roofline leg).  enable = 1: every launch is bracketed by two events and the host waits for it (a launch
 * starts on an idle device).  enable = 2 (queued): every launch of a step has its own event pair, nothing
 * waits between launches or steps, the pairs are read when the pool is full and by dae_plan_profile_read
 * -- the kernels run back to back as they do un-profiled and the averages come within the two markers' cost of rocprofv3's.  Throughput numbers
 * enable = 3 (kernel timestamps): like 2, but the pair of a kernel launch is handed to hipExtLaunchKernelGGL
 * and carries the dispatch's own begin / end times (no marker packets in the stream; a call with several
 * launches adds them up) -- the figure rocprofv3 --kernel-trace reports.  Throughput numbers
 * must be taken with profiling off (enable = 0).  Slot names via dae_plan_profile_name(). */
int         dae_plan_profile(dae_plan* p, int32_t enable);
int         dae_plan_profile_read(const dae_plan* p, int32_t max_slots, double* ms_total, int32_t* counts);
int32_t     dae_plan_profile_slots(void);
const char* dae_plan_profile_name(int32_t slot);
/* out8 = {Fp, Hp, Bp_max, encode_splits, dh_splits, gram_splits, element_size, 0} */
int      dae_plan_info(const dae_plan* p, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif /* DAE_HIP_H */
