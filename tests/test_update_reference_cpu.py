"""The update-half reference (tests/update_reference.py) pinned on the CPU: its optimizers against oracle.opt_apply /
oracle.OptState, its receive-buffer builder against its own unpack, and its band helper against the whole-matrix update.
The GPU tests in tests/test_hip_update_kernels.py trust these helpers."""
import numpy as np
import pytest
import torch

import oracle as O
import update_reference as R


@pytest.mark.parametrize("opt", R.OPTS)
def test_optimizers_equal_oracle(opt):
    """Three steps from the fresh-optimizer slot values: parameters and slots equal oracle.opt_apply's, in float64 to rounding
    of the last place and in float32 (same formulas, same operation order) to a few ulp."""
    rng = np.random.default_rng(21)
    for dt, rtol in ((np.float64, 1e-14), (np.float32, 1e-6)):
        p0 = rng.standard_normal((37, 5)).astype(dt)
        want = p0.copy()
        st = O.OptState(opt, [p0.shape], dt)
        p = p0.copy()
        s1, s2 = R.init_slots(opt, p0.shape, dt)
        for t in range(1, 4):
            g = rng.standard_normal(p0.shape).astype(dt)
            O.opt_apply(st, [want], [g], 0.1, 0.5, dt)
            p, s1, s2 = R.opt_update(opt, p, g, s1, s2, 0.1, 0.5, t, dt)
            assert p.dtype == dt
        assert np.allclose(p, want, rtol=rtol, atol=0)
        assert not np.array_equal(p, p0)
        if opt in ("ada_grad", "momentum"):
            assert np.allclose(s1, st.acc[0], rtol=rtol, atol=0)
        if opt == "adam":
            assert st.t == 3
            assert np.allclose(s1, st.m[0], rtol=rtol, atol=0) and np.allclose(s2, st.v[0], rtol=rtol, atol=0)


def test_bf16_bits_equal_torch():
    rng = np.random.default_rng(22)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 10.0 ** rng.integers(-30, 30, 4096),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, np.inf, -np.inf, 3.3895314e38, 1e-40], np.float32)]).astype(np.float32)
    want = torch.as_tensor(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(a), want)                       # ties (1.00390625 -> 1.0, 1.01171875 -> 1.015625), overflow to inf, denormals
    assert np.array_equal(R.bf16_bits(R.bf16_from_bits(want)), want)
    assert np.isnan(R.bf16_from_bits(R.bf16_bits(np.array([np.nan], np.float32)))).all()


@pytest.mark.parametrize("es", [2, 4])
def test_distinct_bits(es):
    for rows, cols in ((64, 64), (192, 128), (128, 320), (640, 128)):
        b = R.distinct_bits(rows, cols, es)
        f = R.bf16_from_bits(b) if es == 2 else b.view(np.float32)
        assert np.isfinite(f).all()
        if es == 4 or rows * cols <= 32639:
            assert len(np.unique(b)) == b.size
        assert len({r.tobytes() for r in b}) == rows and len({c.tobytes() for c in b.T}) == cols


@pytest.mark.parametrize("es", [2, 4])
@pytest.mark.parametrize("case", R.UNPACK_CASES)
def test_build_recv_round_trip(case, es):
    Fp, Hp, world, chunk_rows = case
    rng = np.random.default_rng(Fp + Hp + world)
    rows = R.distinct_bits(Fp, Hp, es)
    gb = rng.standard_normal((world, Hp + Fp)).astype(np.float32)
    buf, stride, bias_off = R.build_recv(rows, gb, world, chunk_rows)
    assert stride % 16 == 0 and bias_off % 4 == 0 and buf.size == world * stride
    assert stride - (bias_off + 4 * (Hp + Fp)) >= 64                  # the stride is larger than the payload
    W, gb2, acc = R.unpack_recv(buf, world, chunk_rows, stride, bias_off, Fp, Hp, es)
    assert np.array_equal(W, rows) and np.array_equal(gb2, gb)
    want = np.zeros(Hp + Fp, np.float32)
    for r in range(world):
        want += gb[r]
    assert np.array_equal(acc, want)
    assert np.abs(acc.astype(np.float64) - gb.astype(np.float64).sum(0)).max() <= 4 * world * 2.0 ** -24 * np.abs(gb).sum(0).max()
    # everything that is neither a real row nor a bias gradient is NaN bytes: count them
    real = Fp * Hp * es + world * 4 * (Hp + Fp)
    mask = np.ones(buf.size, bool)
    for r in range(world):
        n = (min((r + 1) * chunk_rows, Fp) - min(r * chunk_rows, Fp)) * Hp * es
        mask[r * stride:r * stride + n] = False
        mask[r * stride + bias_off:r * stride + bias_off + 4 * (Hp + Fp)] = False
    assert mask.sum() == buf.size - real and (buf[mask] == R.NAN_BYTE).all()
    if world * chunk_rows > Fp:
        assert mask.sum() > world * (stride - bias_off - 4 * (Hp + Fp))       # some chunk rows lie beyond Fp


@pytest.mark.parametrize("opt", R.OPTS)
def test_band_tiling_equals_whole_update(opt):
    rng = np.random.default_rng(23)
    Fp, Hp = 384, 64
    W0 = rng.standard_normal((Fp, Hp))
    s10 = rng.random((Fp, Hp)) + 0.1
    s20 = rng.random((Fp, Hp))
    whole = [W0.copy(), s10.copy(), s20.copy()]
    banded = [W0.copy(), s10.copy(), s20.copy()]
    for t in range(1, 4):
        g = rng.standard_normal((Fp, Hp))
        R.band_update(opt, *whole, g, 0, Fp, 0.1, 0.5, t)
        for f0, f1 in ((128, 320), (320, 384), (0, 128), (64, 64)):
            R.band_update(opt, *banded, g[f0:f1], f0, f1, 0.1, 0.5, t)
    for a, b in zip(whole, banded):
        assert np.array_equal(a, b)
    assert not np.array_equal(whole[0], W0)
    # a band leaves the other rows alone, and reads grad_rows from its row 0
    one = [W0.copy(), s10.copy(), s20.copy()]
    g = rng.standard_normal((Fp, Hp))
    R.band_update(opt, *one, g[64:192], 64, 192, 0.1, 0.5, 1)
    st = O.OptState(opt, [(128, Hp)], np.float64)
    if opt in ("ada_grad", "momentum"):
        st.acc = [s10[64:192].copy()]
    if opt == "adam":
        st.m, st.v = [s10[64:192].copy()], [s20[64:192].copy()]
    want = W0[64:192].copy()
    O.opt_apply(st, [want], [g[64:192]], 0.1, 0.5, np.float64)
    assert np.allclose(one[0][64:192], want, rtol=1e-14, atol=0)
    for a, b in zip(one, (W0, s10, s20)):
        assert np.array_equal(a[:64], b[:64]) and np.array_equal(a[192:], b[192:])


def test_dh_finish_and_stats_reference_shapes():
    """dh_finish: the column sums are the block sums of delta1 / dh and everything outside [0,B) x [0,H) is zero whatever the
    padding of the inputs holds; step_stats: COST = AE + alpha * TRIPLET in all three strategies."""
    rng = np.random.default_rng(24)
    B, H, Bp, Hp, S = 33, 65, 128, 128, 9
    slabs = np.full((S, Bp, Hp), np.nan); slabs[:, :B, :H] = rng.standard_normal((S, B, H))
    h = np.full((Bp, Hp), np.nan); h[:B, :H] = rng.random((B, H)) - 0.5
    bh = np.full(Hp, np.nan); bh[:H] = rng.standard_normal(H) * 0.3
    d1, cs = R.dh_finish(slabs, None, h, bh, B, H, "tanh")
    assert np.isfinite(d1).all() and (d1[B:] == 0).all() and (d1[:, H:] == 0).all()
    dh = slabs[:, :B, :H].sum(0)
    assert np.allclose(d1[:B, :H], dh * (1 - (h[:B, :H] + np.tanh(bh[:H])) ** 2), rtol=1e-13)
    assert cs.shape == (2, Bp // 32, Hp) and np.allclose(cs[0].sum(0), d1.sum(0)) and np.allclose(cs[1].sum(0)[:H], dh.sum(0))
    assert (cs[:, 2:] == 0).all()
    s = R.step_stats(0.7, "none", 2.0)
    assert list(s) == [0.7, 0.7, 0, 0, 0, 0]
    s = R.step_stats(0.7, "batch_hard", 2.0, tri_scalars=[9.0, 0.25, 0.5, 12.0])
    assert list(s) == [1.2, 0.7, 0.25, 0.5, 12.0, 12.0]
    s = R.step_stats(0.7, "batch_all", 2.0, nvalid=40, loss_part=[1.0, 3.0], cnt_part=[4, 6])
    assert np.allclose(s, [0.7 + 2.0 * 0.1, 0.7, 0.1, 0.25, 10.0, 40.0], rtol=1e-15)
