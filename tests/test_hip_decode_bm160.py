"""GPU tests of the 160 x 128 decode tile (gemm_decode_loss_160, plan option decode_bm = 160) through dae_train_step: against the 128 x 64 route
(decode_bm = 128) on the same inputs and against the fp64 CPU oracle.

The kernel exists for the three-term 16-bit decode with a bit image of x -- precision 'f16x2h' on a binary CSR train set -- so that is the mode
of every case.  Both routes walk K tile by K tile in the same term order (hi.hi; then per k step hi.lo, lo.hi), so every logit is the same
fp32 sum and delta2 / delta2^T must agree to the last bit; the loss and bias-gradient partial sums are added in another order.

Tolerances against the oracle are those of the register-carry decode tests in test_hip_f16.py (test_decode_register_carry_k_loops_equal_the_segment_walk:
cost 3e-5, dW 2e-3; test_step_f16x2_matches_oracle: bias gradients 1.5e-3, parameters 2e-3; the Gram tests: triplet loss 1e-4)."""
import numpy as np
import pytest
import torch

import oracle as O
from test_hip_step import _mk, _rel, _run_case

pytestmark = pytest.mark.gpu

MODE = "f16x2h"
CE = ("cross_entropy", ("sigmoid", "sigmoid"))
# B, F, H: one tile and one K tile | a second row panel with ONE real row (four padded 32-row blocks), a partial last column tile (72 real columns), two K
# tiles of which the second is zero-padded | eight K tiles (the two-stage ring wraps), 32 real rows in panel 2 | five exact panels
SHAPES = [(160, 128, 64), (161, 200, 96), (192, 256, 500), (800, 256, 64)]


def _pad(n):
    return (n + 127) // 128 * 128


def _step_with(bm, B, F, H, strategy="none", loss=CE, phase=0, seed=3, steps=1, **kw):
    """One _run_case with the decode tile height forced; returns its result and the delta2 / delta2^T / dbv_part images behind the last step."""
    grabbed = {}

    def grab(eng, s):
        Bp, Fp = _pad(B), _pad(F)
        grabbed["op_scale"] = eng.info()["op_scale"]
        grabbed["d2"] = eng.buffer("delta2", (Bp, Fp), torch.float16).cpu().numpy().copy()
        grabbed["d2t"] = eng.buffer("delta2_t", (Fp, eng.info()["Bpm"]), torch.float16).cpu().numpy().copy()

    res = _run_case(MODE, strategy, loss[0], loss[1], "gradient_descent", N=B + 37, F=F, H=H, B=B, steps=steps, seed=seed, phase=phase,
                    options={"decode_bm": bm}, after_step=grab, **kw)
    return res, grabbed


@pytest.mark.parametrize("B,F,H", SHAPES)
def test_decode_160_row_tile_equals_128_row_tile_and_oracle(B, F, H):
    (oa, _, pa), ga = _step_with(160, B, F, H)
    (ob, _, pb), gb = _step_with(128, B, F, H)
    # delta2 and delta2^T: the same bits, padding included (rows >= B and columns >= F are zero on both routes)
    assert np.array_equal(ga["d2"].view(np.uint16), gb["d2"].view(np.uint16))
    assert np.array_equal(ga["d2t"].view(np.uint16), gb["d2t"].view(np.uint16))
    Bp = _pad(B)
    assert np.array_equal(ga["d2"][:B, :F], ga["d2t"][:F, :B].T) and not ga["d2"][B:].any() and not ga["d2t"][:, B:Bp].any() and not ga["d2"][:, F:].any()
    (r, sa, dWa, dbha, dbva), (_, sb, dWb, dbhb, dbvb) = oa[0], ob[0]
    d2 = ga["d2"][:B, :F].astype(np.float64) / ga["op_scale"]
    print(f"[bm160 {B}x{F}x{H}] delta2 vs oracle {_rel(d2, r['delta2']):.2e}  cost {abs(sa[0] - r['cost']) / abs(r['cost']):.2e}  dbv {_rel(dbva, r['dbv']):.2e}  "
          f"dW {_rel(dWa, r['dW']):.2e}")
    assert _rel(d2, r["delta2"]) < 2e-3                      # (fp16 images: 2^-12 per element, the bound of the gradients they feed)
    # loss, bias gradient, cost statistics: another summation order than the 128-row route, both at the oracle
    assert np.allclose(sa[:3], sb[:3], rtol=3e-6, atol=0), (sa, sb)
    assert np.allclose(dbva, dbvb, rtol=1e-5, atol=1e-9)
    assert np.array_equal(dWa, dWb) and np.array_equal(dbha, dbhb)          # ... and what is computed from delta2 alone: the same bits
    assert abs(sa[0] - r["cost"]) <= 3e-5 * abs(r["cost"]) and abs(sa[1] - r["ae_loss"]) <= 3e-5 * abs(r["ae_loss"]), (sa, r["cost"])
    assert _rel(dWa, r["dW"]) < 2e-3 and _rel(dbva, r["dbv"]) < 1.5e-3 and _rel(dbha, r["dbh"]) < 1.5e-3
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]) and _rel(pa[2], np.asarray(pb[2], np.float64)) < 1e-5      # (b_v: from the re-ordered partial sums)


def test_decode_160_mean_squared_tanh_linear():
    """The literal (non cross-entropy) arm of the epilogue: mean_squared with a linear decoder, binary rows."""
    B, F, H = 161, 200, 96
    m = _mk(np.random.default_rng(7), B + 37, F, True)
    (oa, _, _), ga = _step_with(160, B, F, H, loss=("mean_squared", ("tanh", "none")), m=m)
    (ob, _, _), gb = _step_with(128, B, F, H, loss=("mean_squared", ("tanh", "none")), m=m)
    assert np.array_equal(ga["d2"].view(np.uint16), gb["d2"].view(np.uint16)) and np.array_equal(ga["d2t"].view(np.uint16), gb["d2t"].view(np.uint16))
    (r, sa, dWa, _, dbva), (_, sb, dWb, _, dbvb) = oa[0], ob[0]
    assert abs(sa[0] - r["cost"]) <= 3e-5 * abs(r["cost"]) and _rel(dWa, r["dW"]) < 2e-3 and _rel(dbva, r["dbv"]) < 1.5e-3
    assert np.array_equal(dWa, dWb)


def test_decode_160_saturated_logits_in_the_padded_panel_take_the_literal_path():
    """|z| > 14 in the rows of both panels, the last one (one real row of 160) included: W[:, 0] = 40 and b_h[0] = -30, so hidden unit 0 is ~1 for every row with
    a stored entry, z = 40 + b_v and y rounds to exactly 1 in fp32.  The reference-literal formula gives -log(0 + 1e-16) = 36.84 where x = 0 and a finite
    delta2; the expectation is test_decode_ce_saturation's: the fp32 oracle rows at rtol 1e-4."""
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd.engine import Engine
    B, F, H = 161, 200, 96
    rng = np.random.default_rng(11)
    m = _mk(rng, B, F, True)
    W0 = rng.uniform(-0.05, 0.05, (F, H)).astype(np.float32); W0[:, 0] = 40.0
    bh0 = np.zeros(H, np.float32); bh0[0] = -30.0
    bv0 = (rng.standard_normal(F) * 0.1).astype(np.float32)
    got = {}
    for bm in (160, 128):
        eng = Engine(F, H, B, dtype=MODE, triplet="none", loss_func="cross_entropy", learning_rate=0.05)
        eng.set_option("decode_bm", bm)
        eng.upload_csr(m); eng.set_params(W0, bh0, bv0)
        stats = torch.zeros(8, device="cuda")
        eng.train_step(torch.arange(B, dtype=torch.int32, device="cuda"), None, stats, corr_mode=L.CORR_NONE, phase=0)
        torch.cuda.synchronize()
        d2 = eng.buffer("delta2", (_pad(B), _pad(F)), torch.float16).cpu().numpy()
        got[bm] = (stats.cpu().numpy(), d2.copy())
    st, d2 = got[160]
    x = m.toarray().astype(np.float32)
    h, _ = O.encode(m, W0, bh0, "sigmoid", np.float32)
    y = O.decode(h, W0, bv0, "sigmoid", np.float32)
    assert np.all(h[B - 1] @ W0.T + bv0 > 14.0) and np.all(y[B - 1] == 1.0)          # the one real row of the last panel: saturated in fp32
    want = float(np.mean(O.weighted_loss_rows(x, y, "cross_entropy", np.float32).astype(np.float64)))
    assert np.isfinite(st).all() and np.isfinite(d2).all()
    assert abs(st[1] - want) <= 1e-4 * abs(want), (st, want)
    assert np.allclose(st[:3], got[128][0][:3], rtol=3e-6, atol=0)
    assert np.array_equal(d2.view(np.uint16), got[128][1].view(np.uint16))


def test_whole_step_behind_160_row_tiles_matches_oracle_and_repeats():
    """One train_step at (200, 256, 96), batch_all with labels, the default route but for the forced tile height (at this size the route keeps 128 x 64 by
    itself): the Gs rider workgroups run behind the 160-row grid.  Phase 3 twice -- bit-identical -- and phase 0 for the gradients."""
    kw = dict(strategy="batch_all", seed=13)
    (o3, ref, p3), _ = _step_with(160, 200, 256, 96, phase=3, **kw)
    (o3b, _, p3b), _ = _step_with(160, 200, 256, 96, phase=3, **kw)
    (o0, _, p0), _ = _step_with(160, 200, 256, 96, phase=0, **kw)
    r, st = o3[0][0], o3[0][1]
    assert np.array_equal(st, o3b[0][1])
    for u, v, w in zip(p3, p3b, p0):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    assert abs(st[0] - r["cost"]) <= 3e-5 * abs(r["cost"]) and abs(st[1] - r["ae_loss"]) <= 3e-5 * abs(r["ae_loss"]), (st, r["cost"])
    assert abs(st[2] - r["triplet_loss"]) <= 1e-4 * abs(r["triplet_loss"])
    _, s0, dW, dbh, dbv = o0[0]
    assert np.array_equal(s0[:3], st[:3])
    assert _rel(dW, r["dW"]) < 2e-3 and _rel(dbh, r["dbh"]) < 1.5e-3 and _rel(dbv, r["dbv"]) < 1.5e-3, (_rel(dW, r["dW"]), _rel(dbh, r["dbh"]), _rel(dbv, r["dbv"]))
    for a, b in zip(p3, ref):
        assert _rel(a, b) < 2e-3, _rel(a, b)


@pytest.mark.parametrize("dtype,loss,acts", [("fp32", "cross_entropy", ("sigmoid", "sigmoid")), ("f16x2h", "cosine_proximity", ("sigmoid", "sigmoid")),
                                             ("bf16", "cross_entropy", ("sigmoid", "sigmoid"))])
def test_decode_bm_160_is_refused_where_the_kernel_does_not_exist(dtype, loss, acts):
    from dae_rnn_news_recommendation_amd.engine import Engine
    eng = Engine(256, 64, 160, dtype=dtype, enc_act=acts[0], dec_act=acts[1], loss_func=loss, triplet="none")
    with pytest.raises(Exception, match="decode_bm"):
        eng.set_option("decode_bm", 160)
    eng.set_option("decode_bm", 128); eng.set_option("decode_bm", 0)
    with pytest.raises(Exception, match="decode_bm"):
        eng.set_option("decode_bm", 96)
