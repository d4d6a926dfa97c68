"""CPU pins of tests/csr_cases.py: the long-row builder holds every length and mask class its GPU users rely on, its dyadic grids
make fp32 sums exact in any order, and its per-row float64 reference agrees with the oracle's dense encode."""
import numpy as np
import pytest

import csr_cases as CC
import oracle as O

F = 1000


@pytest.fixture(scope="module", params=[False, True], ids=["binary", "valued"])
def case(request):
    m, keep = CC.long_row_csr(np.random.default_rng(0), F, request.param, pad_cols=True)
    return m, keep, request.param


def test_builder_holds_every_length_and_mask_class(case):
    m, keep, valued = case
    rows = CC.kept_per_pass(m, keep)
    lengths = [n for n, _ in rows]
    assert set(CC.LENGTHS) <= set(lengths)
    assert m.has_sorted_indices and all((np.diff(m.indices[m.indptr[r]:m.indptr[r + 1]]) > 0).all() for r in range(m.shape[0]))
    assert (m.indices >= F).sum() == 3 * len(CC.PAD_COL_ROWS) and m.indices.max() == CC.pad(F) - 1      # stored columns in [F, Fp)
    # every entry kept / dropped, on rows of more than one pass too
    assert any(n == 700 and sum(k) == 700 for n, k in rows) and any(n == 700 and sum(k) == 0 for n, k in rows)
    for n in CC.LENGTHS:
        assert any(nn == n and sum(k) == n for nn, k in rows), n                                        # each length once with all kept
    # only the last stored entry kept: behind a pass boundary, and as lane 0 / lane 63 of a 64-entry group
    for n in (1, 64, 65, 257, 513, 700):
        s = [r for r, (nn, k) in enumerate(rows) if nn == n and sum(k) == 1 and keep[m.indptr[r + 1] - 1]]
        assert s, n
    # only entries of the second pass on (index >= 256), only of the first pass
    assert any(n > 256 and k[0] == 0 and sum(k[1:]) == n - 256 for n, k in rows)
    assert any(n > 256 and k[0] == 256 and sum(k[1:]) == 0 for n, k in rows)
    # kept counts at the walk's trip boundaries within one pass (36 / 72 entries per trip), and a full list
    per_pass = {c for _, k in rows for c in k}
    assert {36, 37, 72, 73, 256} <= per_pass
    # a random mask on every length
    frac = [sum(k) / n for n, k in rows if n >= 144 and 0.55 < sum(k) / n < 0.85]
    assert len(frac) >= 8
    # the first 8-row workgroup mixes the extremes
    assert {0, 1, 700} <= set(lengths[:8])
    if valued:
        assert ((m.data * 16) % 1 == 0).all() and m.data.min() > 0 and m.data.max() <= 1 and len(np.unique(m.data)) == 16
    else:
        assert (m.data == 1).all()


def test_grids_make_fp32_sums_exact():
    """The bound (bits of the sum's range + fractional bits <= 24) for both W grids, and the property itself: fp32 sums of 700 products in
    three random orders, with and without fused multiply-adds' single rounding, are bit-equal to the float64 sum."""
    assert CC.exact_sum_bits(700, 8, 0.25) <= 24
    assert CC.exact_sum_bits(700, 12, 0.125) <= 24             # the fp32-master legs: W not exact in bf16
    assert CC.exact_sum_bits(700, 12, 0.25) > 24               # (the bound is not vacuous)
    rng = np.random.default_rng(1)
    for w_bits, w_max in ((8, 0.25), (12, 0.125)):
        W, bh = CC.grid_params(rng, 700, 16, w_bits, w_max)
        assert np.abs(W).max() <= w_max and ((W * 2.0 ** w_bits) % 1 == 0).all() and ((bh * 2.0 ** 13) % 1 == 0).all()
        import torch
        exact_bf16 = torch.equal(torch.as_tensor(W).to(torch.bfloat16).float(), torch.as_tensor(W))
        exact_f16 = torch.equal(torch.as_tensor(W).to(torch.float16).float(), torch.as_tensor(W))
        assert exact_bf16 == (w_bits == 8) and (exact_f16 or w_bits != 8)
        for scale in (1.0, 0.5):
            v = (rng.integers(1, 17, 700) / 16.0).astype(np.float32)
            w = v * np.float32(scale)
            want = (w.astype(np.float64)[:, None] * W.astype(np.float64)).sum(0)
            for _ in range(3):
                order = rng.permutation(700)
                acc = np.zeros(16, np.float32)
                for k in order:
                    acc = (acc + w[k] * W[k]).astype(np.float32)           # product and sum each rounded to fp32: both exact here
                assert np.array_equal(acc.astype(np.float64), want)
            z = (want + bh).astype(np.float32)
            assert np.array_equal(z.astype(np.float64), want + bh)
            assert np.array_equal((z - bh).astype(np.float64), want)           # (z + b) - b, the kernel's h for enc_act = none


@pytest.mark.parametrize("act", ["none", "sigmoid", "tanh"])
def test_reference_matches_oracle_encode(case, act):
    m, keep, valued = case
    rng = np.random.default_rng(2)
    H = 24
    W, bh = CC.grid_params(rng, F, H)
    row_idx = np.concatenate([np.arange(m.shape[0]), [1, 1, 7]])
    for scale in (1.0, 0.5):
        ref = CC.encode_csr_reference(m, keep, row_idx, F, W, bh, scale, act, O.act)
        mc = m.copy(); mc.data = mc.data * keep * scale
        dense, dense_c = m.toarray()[row_idx][:, :F].astype(np.float64), mc.toarray()[row_idx][:, :F].astype(np.float64)
        want, _ = O.encode(dense_c, W, bh, act, np.float64)
        assert np.array_equal(ref["xc"], dense_c)
        assert np.array_equal(ref["z"], dense_c @ W.astype(np.float64))            # exact inputs: the dense product has the same bits
        assert np.allclose(ref["h"], want, rtol=1e-14, atol=1e-15)
        assert np.array_equal(ref["rowsq"], (dense ** 2).sum(1))
        bits = np.zeros((len(row_idx), CC.pad(F)), bool); bits[:, :F] = dense != 0
        assert np.array_equal(ref["x_bits"], np.packbits(bits, axis=1, bitorder="little").view(np.uint32))


def test_keep_words_round_trip(case):
    m, keep, _ = case
    w = CC.keep_words(keep).view(np.uint32)
    e = np.arange(m.nnz)
    assert np.array_equal(((w[e >> 5] >> (e & 31).astype(np.uint32)) & 1).astype(bool), keep)
