"""Kernel-level tests of the CSR front end on rows longer than one 256-entry pass: dae_encode_csr (ops.encode_csr) and, through an
Engine, the weight readers and split-mode images it cannot select, against the per-row float64 reference of tests/csr_cases.py.

The inputs sit on dyadic grids (csr_cases.grid_params, long_row_csr; bound and property pinned in tests/test_csr_cases_cpu.py), so every
fp32 summation order is exact: the pre-activation, h for enc_act = none, the row squares and every derived image are compared BIT FOR
BIT over their whole padded extents.  sigmoid / tanh differ from float64 only by the activation's own evaluation and take the tolerance
test_hip_kernels.py::test_encode_finish uses for the same act_apply."""
import numpy as np
import pytest
import torch

import csr_cases as CC
import oracle as O

pytestmark = pytest.mark.gpu

F, HMAX = 1000, 300
FP = CC.pad(F)
SEED, STREAM, FRAC = 0x1234567890ABCDEF, 5, 0.3


@pytest.fixture(scope="module")
def ops():
    from dae_rnn_news_recommendation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from dae_rnn_news_recommendation_amd import _lib
    _lib.load()
    return _lib


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits_of(t):
    """Integer view of a tensor: equality of bits (a NaN left by an unwritten element differs from every expected value)."""
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits_of(a), bits_of(b))


# ----------------------------------------------------------------------------------------------- #
# shared cases: one matrix per input kind, one weight set, one reference per (input kind, corruption, scale)
# ----------------------------------------------------------------------------------------------- #
_cache = {}


def _matrix(valued, pad_cols=True):
    key = ("m", valued, pad_cols)
    if key not in _cache:
        m, keep = CC.long_row_csr(np.random.default_rng(17 + valued), F, valued, pad_cols=pad_cols)
        _cache[key] = (m, keep, dev(m.indptr.astype(np.int64)), dev(m.indices.astype(np.int32)), dev(m.data) if valued else None)
    return _cache[key]


def _weights():
    if "w" not in _cache:
        _cache["w"] = CC.grid_params(np.random.default_rng(23), F, HMAX)
    return _cache["w"]


def _keep(valued, corr):
    m, keep = _matrix(valued)[:2]
    if corr == "philox":
        keep = O.philox_uniform(np.arange(m.nnz, dtype=np.uint64), SEED, STREAM) >= np.float32(FRAC)
    return keep


def _reference(valued, corr, scale):
    """z, bit image, x~ and row squares of EVERY row of the matrix (H = HMAX; a test slices its rows and columns out)."""
    key = ("ref", valued, corr, scale)
    if key not in _cache:
        m = _matrix(valued)[0]
        W, bh = _weights()
        _cache[key] = CC.encode_csr_reference(m, _keep(valued, corr), np.arange(m.shape[0]), F, W, bh, scale, "none", O.act)
    return _cache[key]


def _row_idx(B):
    n = len(CC.ROWS)
    if B <= n:
        return np.concatenate([np.arange(B - 1), [1]]).astype(np.int32)          # the first rows, and the 700-entry row 1 a second time
    return np.concatenate([np.arange(n), np.random.default_rng(B).integers(0, n, B - n)]).astype(np.int32)


def _device_params(H, td):
    """W [Fp x Hp] and b_h [Hp] with finite GARBAGE in the padding: the kernel masks columns >= H itself and never reads rows >= F."""
    W, bh = _weights()
    Hp = CC.pad(H)
    Wp = torch.full((FP, Hp), 3.0, dtype=torch.float32); Wp[F:] = -2.0
    Wp[:F, :H] = torch.as_tensor(W[:, :H])
    bp = torch.full((Hp,), 0.75, dtype=torch.float32); bp[:H] = torch.as_tensor(bh[:H])
    return Wp.to(td).cuda(), bp.cuda()


def _check_images(out, ref, rows, B, H, td, valued, scale, act):
    """Every image of one launch against the reference (rows: the batch's rows of the matrix)."""
    Bp, Hp = CC.pad(B), CC.pad(H)
    _, bh = _weights()
    z = ref["z"][rows][:, :H]
    b = bh[:H].astype(np.float64)
    want_h = O.act(act, z + b) - O.act(act, b)
    h32 = out["h_f32"]
    got = h32.cpu().numpy()
    if act == "none":
        want = np.zeros((Bp, Hp), np.float32); want[:B, :H] = want_h
        assert np.array_equal(want[:B, :H].astype(np.float64), want_h)               # the reference itself is an fp32 number
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    else:
        assert np.allclose(got[:B, :H], want_h, rtol=1e-5, atol=2e-6), np.abs(got[:B, :H] - want_h).max()
        assert (got[B:] == 0).all() and (got[:, H:] == 0).all()
    # low-precision image, its transpose, the split Gram operands: roundings of the DEVICE's h_f32, over the whole padded extents
    hi = h32.to(td)
    assert same_bits(out["h_lo"], hi)
    assert same_bits(out["h_t"], hi.T.contiguous())
    hb = h32.to(torch.bfloat16)
    lo = (h32 - hb.float()).to(torch.bfloat16)
    assert same_bits(out["hcat_a"], torch.cat([hb, hb, lo], 1)) and same_bits(out["hcat_b"], torch.cat([hb, lo, hb], 1))
    assert bool((lo != 0).any())
    # side images
    if not valued:
        want_bits = np.zeros((Bp, FP // 32), np.uint32); want_bits[:B] = ref["x_bits"][rows]
        assert np.array_equal(out["x_bits"].cpu().numpy().view(np.uint32), want_bits)
    xc = np.zeros((Bp, FP), np.float32); xc[:B, :F] = ref["xc"][rows]
    assert np.array_equal(xc[:B, :F].astype(np.float64), ref["xc"][rows])
    assert same_bits(out["xct"], torch.as_tensor(xc.T.copy()).to(td).cuda())
    want_sq = np.zeros(Bp, np.float32); want_sq[:B] = ref["rowsq"][rows]
    assert np.array_equal(want_sq[:B].astype(np.float64), ref["rowsq"][rows])
    assert np.array_equal(out["rowsq"].cpu().numpy(), want_sq)


@pytest.mark.parametrize("corr", ["keepbits", "philox"])
@pytest.mark.parametrize("valued", [False, True], ids=["binary", "valued"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,H", [(21, 100), (21, 200), (21, 300), (130, 100), (130, 200), (130, 300)])
def test_encode_csr_matches_float64_reference(ops, L, B, H, dtype, valued, corr):
    """dae_encode_csr on rows of 0 .. 700 stored entries (one to three passes, every `u`, full and masked walk trips), one to three
    column slices (three placements of the side tasks), a ragged row tile, a row taken twice, stored columns in [F, Fp): h and all its
    images, the clean bit image, the x~^T scatter and the row squares, for scale 1 and 0.5 and the three activations; two launches on the
    same inputs are bit-equal."""
    m, _, indptr, indices, values = _matrix(valued)
    rows = _row_idx(B)
    dt, td = (L.BF16, torch.bfloat16) if dtype == "bf16" else (L.F32, torch.float32)
    W_dev, bh_dev = _device_params(H, td)
    kw = dict(corr_mode=L.CORR_KEEPBITS, keep_bits=dev(CC.keep_words(_keep(valued, corr)))) if corr == "keepbits" else \
        dict(corr_mode=L.CORR_PHILOX_MASK, seed=SEED, rng_stream=STREAM, corr_frac=FRAC)
    want = dict(want_hcat_a=True, want_hcat_b=True, want_x_bits=not valued, want_rowsq=True)
    rows_dev = dev(rows)
    for scale in (1.0, 0.5):
        ref = _reference(valued, corr, scale)
        for act in ("none", "sigmoid", "tanh"):
            out = ops.encode_csr(indptr, indices, values, rows_dev, B, F, H, dt, W_dev, bh_dev, L.ACT[act], scale=scale, **kw, **want)
            _check_images(out, ref, rows, B, H, td, valued, scale, act)
    again = ops.encode_csr(indptr, indices, values, rows_dev, B, F, H, dt, W_dev, bh_dev, L.ACT[act], scale=scale, **kw, **want)
    for name, t in out.items():
        assert (t is None and again[name] is None) or same_bits(t, again[name]), name


def test_encode_csr_refusals(ops, L):
    """Argument combinations the launcher must refuse (nothing is launched), each with its message."""
    m, keep, indptr, indices, _ = _matrix(False)
    _, _, vptr, vind, values = _matrix(True)
    B, H = 21, 100
    rows = dev(_row_idx(B))
    W_dev, bh_dev = _device_params(H, torch.float32)
    args = (rows, B, F, H, L.F32, W_dev, bh_dev, L.ACT["none"])
    with pytest.raises(RuntimeError, match="keep_bits is null"):
        ops.encode_csr(indptr, indices, None, *args, corr_mode=L.CORR_KEEPBITS, keep_bits=None)
    with pytest.raises(RuntimeError, match="the bit image of x needs binary data"):
        ops.encode_csr(vptr, vind, values, *args, want_x_bits=True)
    with pytest.raises(RuntimeError, match="ldt too small"):
        ops.encode_csr(indptr, indices, None, *args, ldt=CC.pad(B) - 64)
    with pytest.raises(RuntimeError, match="hcat_a/hcat_b must be given together"):
        ops.encode_csr(indptr, indices, None, *args, want_hcat_a=True)
    with pytest.raises(RuntimeError, match="hcat_a/hcat_b must be given together"):
        ops.encode_csr(indptr, indices, None, *args, want_hcat_b=True)
    out = ops.encode_csr(indptr, indices, None, *args, want_x_bits=True)              # ... and the plain call still runs
    assert bool(torch.isfinite(out["h_f32"]).all())


# ----------------------------------------------------------------------------------------------- #
# the kernels dae_encode_csr cannot select: through an Engine on the same long rows
# ----------------------------------------------------------------------------------------------- #
def _engine_case(valued, w_bits=8, w_max=0.25, H=200, seed=31):
    rng = np.random.default_rng(seed)
    m, keep = CC.long_row_csr(rng, F, valued)
    W, bh = CC.grid_params(rng, F, H, w_bits, w_max)
    return m, keep, W, bh


@pytest.mark.parametrize("valued", [False, True], ids=["binary", "valued"])
@pytest.mark.parametrize("cols", [64, 128])
def test_fp32_master_readers_on_long_rows(L, cols, valued):
    """bf16 mode encoding from the fp32 MASTER weights (encode_csr_kernel<float, bf16_t, 64 / 128>: walk trips of 72 resp. 36 kept
    entries), forward-only phase, enc_act none: h_f32 is bit-equal to the float64 reference computed from the fp32 W.  W sits on the
    2^-12 grid, NOT exact in bf16: with encode_w32 = 0 the same launch reads W_lo and h equals the reference from the ROUNDED W instead
    -- and differs from the first."""
    from dae_rnn_news_recommendation_amd.engine import Engine
    H, scale = 200, 0.5
    m, keep, W, bh = _engine_case(valued, 12, 0.125, H)
    assert CC.exact_sum_bits(max(CC.LENGTHS), 12, 0.125) <= 24
    B = m.shape[0]
    rows = np.arange(B)
    W_lo = torch.as_tensor(W).to(torch.bfloat16).float().numpy()
    assert (W_lo != W).mean() > 0.2                 # (|W| >= 2^-4 needs more than 8 significand bits unless its low bits are zero: about a quarter)
    want = {w32: CC.encode_csr_reference(m, keep, rows, F, Wx, bh, scale, "none", O.act)["h"] for w32, Wx in ((1, W), (0, W_lo))}
    got = {}
    for w32 in (1, 0):
        eng = Engine(F, H, B, dtype="bf16", enc_act="none")
        eng.set_option("encode_w32", w32); eng.set_option("encode_w32_cols", cols)
        eng.upload_csr(m); eng.set_params(W, bh)
        stats = torch.zeros(8, device="cuda")
        eng.train_step(dev(rows.astype(np.int32)), None, stats, corr_mode=L.CORR_KEEPBITS, keep_bits=dev(CC.keep_words(keep)), scale=scale, phase=2)
        torch.cuda.synchronize()
        got[w32] = eng.buffer("h_f32", (eng.Bpm, eng.Hp), torch.float32).cpu().numpy()
        full = np.zeros((eng.Bpm, eng.Hp), np.float32); full[:B, :H] = want[w32]
        assert np.array_equal(full[:B, :H].astype(np.float64), want[w32])
        assert np.array_equal(got[w32], full), (w32, np.argwhere(got[w32] != full)[:8])
    assert not np.array_equal(got[1], got[0])


def _scatter_images(m, keep, rows, scale, Bp, td):
    """hi / lo images [Bp x Fp] of x~ = fp32(scale * v) at the kept entries (hi = storage rounding, lo = rounding of the residual)."""
    mc = m.copy(); mc.data = (mc.data * keep).astype(np.float32) * np.float32(scale)
    x = torch.zeros((Bp, FP), dtype=torch.float32)
    x[:len(rows), :F] = torch.as_tensor(mc.toarray()[rows])
    hi = x.to(td)
    return hi.cuda(), (x - hi.float()).to(td).cuda()


def test_split_mode_images_on_long_rows(L):
    """bf16x3 with valued input and a scale that is not exact in bf16: the encode launch also writes h^T's lo image and the lo image of
    the x~^T scatter.  h_t / h_t2 are the rounding and the rounded residual of the device's h_f32; xct / xct_2 hold hi / lo of
    fp32(scale * v) at the kept entries and 0 elsewhere (whole images).  The step tail is switched off (option tail = 0) so that the
    scatter is still in place after the step; the tail's un-scatter has its own tests in test_hip_step.py."""
    from dae_rnn_news_recommendation_amd.engine import Engine
    H, scale = 200, 0.7
    rng = np.random.default_rng(37)
    m, keep = CC.long_row_csr(rng, F, True)
    B = m.shape[0]
    rows = rng.permutation(B)
    W0 = rng.uniform(-0.05, 0.05, (F, H)).astype(np.float32); bh0 = (rng.standard_normal(H) * 0.1).astype(np.float32)
    eng = Engine(F, H, B, dtype="bf16x3", loss_func="mean_squared", learning_rate=0.05)
    eng.set_option("tail", 0)
    eng.upload_csr(m); eng.set_params(W0, bh0)
    stats = torch.zeros(8, device="cuda")
    eng.train_step(dev(rows.astype(np.int32)), None, stats, corr_mode=L.CORR_KEEPBITS, keep_bits=dev(CC.keep_words(keep)), scale=scale, phase=0)
    torch.cuda.synchronize()
    h32 = eng.buffer("h_f32", (eng.Bpm, eng.Hp), torch.float32)
    want, _ = O.encode(m[rows].toarray() * keep_dense(m, keep)[rows] * scale, W0, bh0, "sigmoid", np.float64)
    assert np.abs(h32[:B, :H].cpu().numpy() - want).max() < 1e-5 * np.abs(want).max()           # (test_encode_rows_matches_oracle's bound)
    hi = h32.to(torch.bfloat16)
    lo = (h32 - hi.float()).to(torch.bfloat16)
    assert same_bits(eng.buffer("h_t", (eng.Hp, eng.Bpm), torch.bfloat16), hi.T.contiguous())
    assert same_bits(eng.buffer("h_t2", (eng.Hp, eng.Bpm), torch.bfloat16), lo.T.contiguous()) and bool((lo != 0).any())
    x_hi, x_lo = _scatter_images(m, keep, rows, scale, eng.Bpm, torch.bfloat16)
    assert int((x_lo != 0).sum()) > 1000
    assert same_bits(eng.buffer("xct", (eng.Fp, eng.Bpm), torch.bfloat16), x_hi.T.contiguous())
    assert same_bits(eng.buffer("xct_2", (eng.Fp, eng.Bpm), torch.bfloat16), x_lo.T.contiguous())


def keep_dense(m, keep):
    k = m.copy(); k.data = keep.astype(np.float32)
    return k.toarray()


@pytest.mark.parametrize("dw_tr", [0, 1])
def test_scatter_layouts_on_long_rows(L, dw_tr):
    """bf16 step on the 160 x 128 dW kernel: option dw_tr = 0 scatters the kept entries into the transposed image x~^T [Fp x Bp],
    dw_tr = 1 into the row-major image x~ [Bp x Fp] of the same buffer.  Whole images, read after a step without the tail's
    un-scatter (option tail = 0)."""
    from dae_rnn_news_recommendation_amd.engine import Engine
    H, scale = 200, 0.5
    rng = np.random.default_rng(41)
    m, keep = CC.long_row_csr(rng, F, True)
    B = m.shape[0]
    rows = rng.permutation(B)
    W0 = torch.as_tensor(rng.uniform(-0.05, 0.05, (F, H)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    lib = L.load()
    lib.dae_set_glds(-5)                       # the 160 x 128 kernel for every grid that fits one round: the only one with a row-major A form
    try:
        eng = Engine(F, H, B, dtype="bf16", loss_func="mean_squared", learning_rate=0.05)
        eng.set_option("tail", 0); eng.set_option("dw_tr", dw_tr)
        eng.upload_csr(m); eng.set_params(W0)
        stats = torch.zeros(8, device="cuda")
        eng.train_step(dev(rows.astype(np.int32)), None, stats, corr_mode=L.CORR_KEEPBITS, keep_bits=dev(CC.keep_words(keep)), scale=scale, phase=0)
        torch.cuda.synchronize()
    finally:
        lib.dae_set_glds(-4)
    x_hi, _ = _scatter_images(m, keep, rows, scale, eng.Bpm, torch.bfloat16)
    if dw_tr:
        assert same_bits(eng.buffer("xct", (eng.Bpm, eng.Fp), torch.bfloat16), x_hi)
    else:
        assert same_bits(eng.buffer("xct", (eng.Fp, eng.Bpm), torch.bfloat16), x_hi.T.contiguous())
    mc = m.copy(); mc.data = mc.data * keep * scale
    r = O.forward_backward(W0, np.zeros(H), np.zeros(F), m[rows].toarray(), mc[rows].toarray(), None, loss_func="mean_squared",
                           triplet_strategy="none", dt=np.float64)
    dW = eng.grads()[0]
    assert np.abs(dW - r["dW"]).max() < 2e-2 * np.abs(r["dW"]).max()                             # (the bf16 gradient gate of test_hip_step.py)


# ----------------------------------------------------------------------------------------------- #
# the gather kernel on the same rows (a plain strided row walk: one case per dtype)
# ----------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_gather_csr_on_long_rows(ops, L, dtype):
    """dae_gather_csr / dae_gather_csr_bits on the long-row matrix: x, x~, x~^T, the bit image of x~ and the row squares, all exact."""
    dt, td = (L.BF16, torch.bfloat16) if dtype == "bf16" else (L.F32, torch.float32)
    B = len(CC.ROWS) + 1
    rows = _row_idx(B)
    Bp = CC.pad(B)
    # valued rows
    m, keep, indptr, indices, values = _matrix(True, pad_cols=False)
    x, xc, xct, rowsq = ops.gather_csr(indptr, indices, values, dev(rows), B, F, dt, want_rowsq=True, corr_mode=L.CORR_KEEPBITS,
                                       keep_bits=dev(CC.keep_words(keep)), scale=0.5)
    ref = CC.encode_csr_reference(m, keep, rows, F, np.zeros((F, 1)), np.zeros(1), 0.5, "none", O.act)
    want_x = torch.zeros((Bp, FP)); want_x[:B, :F] = torch.as_tensor(m.toarray()[rows])
    want_xc = torch.zeros((Bp, FP)); want_xc[:B, :F] = torch.as_tensor(ref["xc"].astype(np.float32))
    assert same_bits(x, want_x.to(td).cuda()) and same_bits(xc, want_xc.to(td).cuda()) and same_bits(xct, want_xc.to(td).T.contiguous().cuda())
    want_sq = np.zeros(Bp, np.float32); want_sq[:B] = ref["rowsq"]
    assert np.array_equal(rowsq.cpu().numpy(), want_sq)
    # binary rows, with stored columns in [F, Fp): the bit image of x~
    m, keep, indptr, indices, _ = _matrix(False)
    x, bits, xct = ops.gather_csr_bits(indptr, indices, dev(rows), B, F, dt, corr_mode=L.CORR_KEEPBITS, keep_bits=dev(CC.keep_words(keep)))
    ref = CC.encode_csr_reference(m, keep, rows, F, np.zeros((F, 1)), np.zeros(1), 1.0, "none", O.act)
    want_x = torch.zeros((Bp, FP)); want_x[:B, :F] = torch.as_tensor(m.toarray()[rows][:, :F])
    want_xc = torch.zeros((Bp, FP)); want_xc[:B, :F] = torch.as_tensor(ref["xc"].astype(np.float32))
    assert same_bits(x, want_x.to(td).cuda()) and same_bits(xct, want_xc.to(td).T.contiguous().cuda())
    want_bits = np.packbits(want_xc.numpy() != 0, axis=1, bitorder="little").view(np.uint32)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_bits)
