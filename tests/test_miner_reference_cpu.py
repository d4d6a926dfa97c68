"""The per-anchor miner references (tests/miner_reference.py) pinned to the whole-batch oracle, on the CPU.

The GPU tests of the `_rows` miners (tests/test_hip_miner_rows.py) trust these helpers at batch sizes where the oracle's B^3
evaluation is out of reach; here, at B <= 60, whole batches and anchor ranges of both must agree with oracle/dae_oracle.py:
gradients and losses to float64 rounding, every count and data weight as integers."""
import numpy as np
import pytest

import oracle as O
from miner_reference import anchor_sets, batch_all_rows_reference, batch_hard_rows_reference


def _case(name):
    """(labels, float32 D) of a named small batch."""
    rng = np.random.default_rng(sum(map(ord, name)))
    B, H = {"signed": (60, 12), "unsigned": (47, 9), "one_class": (23, 7), "singleton": (31, 8), "duplicates": (40, 10)}[name]
    signed = name != "unsigned"
    h = (rng.random((B, H)) - (0.5 if signed else 0.0)) * 2.0
    lab = rng.integers(0, 4, B)
    if name == "one_class":
        lab[:] = 3
    if name == "singleton":
        lab[lab == 2] = 1
        lab[11] = 2                                     # a class of one member: no positives for it, a negative for everyone else
    if name == "duplicates":
        h[5] = h[3]; h[17] = h[3]; h[30] = h[29]        # duplicated rows, same and different labels among them
        lab[5] = lab[3]; lab[17] = (lab[3] + 1) % 4; lab[30] = lab[29]
    D = (h @ h.T).astype(np.float32)
    if name == "duplicates":                            # make the ties exact whatever the matmul's summation order
        for dst, src in ((5, 3), (17, 3), (30, 29)):
            D[:, dst] = D[:, src]
        for dst, src in ((5, 3), (17, 3), (30, 29)):
            D[dst, :] = D[src, :]
    return lab, D


EPS = 1e-16          # the reference's normaliser epsilon (triplet_loss_utils.py:127)
CASES = ["signed", "unsigned", "one_class", "singleton", "duplicates"]


@pytest.mark.parametrize("pos_only", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_batch_all_reference_equals_oracle(name, pos_only):
    lab, D = _case(name)
    B = len(lab)
    ref = batch_all_rows_reference(D, lab, 0, pos_only)
    h_unused = np.zeros((B, 1))
    lo, dwo, fro, numo, Go = O.batch_all_triplet_loss(lab, h_unused, pos_only, np.float64, return_grad=True, D=D.astype(np.float64))
    _, dw32, _, num32 = O.batch_all_triplet_loss(lab, h_unused, pos_only, np.float32, D=D)
    nv, dw_closed = O.batch_all_closed_form(lab)
    num_pos = int(ref["npos_part"].sum())
    assert num_pos == int(num32) == int(numo)
    assert int(ref["nvalid_part"].sum()) == nv
    norm = float(num_pos if pos_only else nv) + EPS
    assert np.allclose(ref["G"] / norm, Go, rtol=1e-12, atol=1e-15 * max(1.0, np.abs(Go).max()))
    assert np.isclose(ref["loss_part"].sum(), float(lo) * norm, rtol=1e-12, atol=1e-300)
    assert (ref["G"][np.arange(B), np.arange(B)] == 0).all()
    if pos_only:
        dw = ref["npos_part"] + ref["role_cnt"].sum(axis=0)             # anchor role + positive and negative roles
        assert np.array_equal(dw, dw32.astype(np.int64)) and np.array_equal(dw, dwo.astype(np.int64))
        assert dw.sum() == 3 * num_pos
    else:
        assert ref["role_cnt"] is None
        assert np.array_equal(dwo.astype(np.int64), dw_closed)
    if name == "duplicates":
        assert ref["nzero_part"].sum() > 0                                  # exact column ties: T == 0 is not a positive triplet
    if name == "one_class":
        assert nv == 0 and not ref["G"].any() and not ref["loss_part"].any()
    if name == "singleton":
        P, N = anchor_sets(lab, 11)
        assert len(P) == 0 and len(N) == B - 1 and not ref["G"][11].any() and ref["npos_part"][11] == 0


@pytest.mark.parametrize("name", CASES)
def test_batch_hard_reference_equals_oracle(name):
    lab, D = _case(name)
    B = len(lab)
    ref = batch_hard_rows_reference(D, lab, 0)
    h_unused = np.zeros((B, 1))
    lo32, dw32, fr32, num32, G32 = O.batch_hard_triplet_loss(lab, h_unused, np.float32, return_grad=True, D=D)
    lo64, dw64, fr64, num64, G64 = O.batch_hard_triplet_loss(lab, h_unused, np.float64, return_grad=True, D=D.astype(np.float64))
    ncnt = int(ref["cnt_part"].sum())
    assert ncnt == int(num32)
    assert np.array_equal(ref["dw"], dw32.astype(np.int64))
    norm = float(ncnt) + EPS
    # the float32 oracle rounds dist, its loss and its gradient to float32
    assert np.allclose(ref["G"] / norm, G32, rtol=1e-6, atol=1e-7 * max(1e-30, np.abs(G32).max()))
    assert np.isclose(ref["loss_part"].sum(), float(lo32) * norm, rtol=1e-6)
    # the float64 oracle takes the same decisions on these batches (asserted), and then agrees to rounding
    assert int(num64) == ncnt and np.array_equal(dw64.astype(np.int64), ref["dw"])
    assert np.allclose(ref["G"] / norm, G64, rtol=1e-12, atol=1e-15 * max(1e-30, np.abs(G64).max()))
    assert np.isclose(ref["loss_part"].sum(), float(lo64) * norm, rtol=1e-12)
    if name == "duplicates":                                            # tied columns share the gradient equally
        rows = [r for r in range(B) if r not in (3, 5, 17, 29, 30)]
        assert np.array_equal(ref["G"][rows, 30], ref["G"][rows, 29])


@pytest.mark.parametrize("name", ["signed", "duplicates"])
def test_anchor_ranges_are_slices_of_the_whole_batch(name):
    """A row subset with a0 > 0 gives the whole batch's rows; batch_hard's dw of disjoint ranges adds up to the whole batch's."""
    lab, D = _case(name)
    B = len(lab)
    pad = np.full((B, 5), np.nan, np.float32)
    Dw = np.concatenate([D, pad], axis=1)                               # columns beyond B are never read
    whole = batch_all_rows_reference(D, lab, 0, True)
    hard = batch_hard_rows_reference(D, lab, 0)
    dw = np.zeros(B, np.int64)
    for a0, a1 in ((0, 1), (1, B - 13), (B - 13, B)):
        part = batch_all_rows_reference(Dw[a0:a1], lab, a0, True)
        for k in ("loss_part", "npos_part", "G", "role_cnt", "nvalid_part", "row_range", "nzero_part"):
            assert np.array_equal(part[k], whole[k][a0:a1]), k
        ph = batch_hard_rows_reference(Dw[a0:a1], lab, a0)
        for k in ("loss_part", "cnt_part", "G"):
            assert np.array_equal(ph[k], hard[k][a0:a1]), k
        dw += ph["dw"]
    assert np.array_equal(dw, hard["dw"])
