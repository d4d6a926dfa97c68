"""The triplet miners' anchor-range entry points (dae_triplet_batch_all_rows / dae_triplet_batch_hard_rows) and the
pos_triplets_only mode, kernel level, against the per-anchor float64 reference of tests/miner_reference.py (pinned to the oracle
on the CPU by tests/test_miner_reference_cpu.py).

D is built on the host and uploaded (no Gram kernel), so exact column ties, ldd > Bp and NaN padding can be constructed: every
case fills D's padding columns [B, ldd) and a spare row with NaN and every output buffer with a sentinel, and asserts that the
kernel writes exactly the rows [0, n_anchors) x columns [0, Bp) -- zeros in [B, Bp) and at the anchor's own column -- and never
propagates the padding.  A row subset costs n_anchors rows of D, so batches up to the advertised limits (4096 for batch_all,
3072 with pos_triplets_only, 16384 for batch_hard) are a few rows, and the reference costs nP * nN per anchor.

Tolerances are the project's own from test_hip_kernels.py::test_miners_gradients, applied per anchor: counts, role counts and
data weights exact; loss_part rtol 2e-5 (batch_hard 1e-5), atol 1e-7; every row of G within 5e-5 of the reference row's largest
entry (1e-4 in the FAST mode of the bf16 steps).  No tolerance had to be measured or widened.

One fix came with these tests, found by reading and never run un-fixed: dae_triplet_batch_hard_rows launched its kernel with
Bp * 4 + 64 bytes of dynamic LDS -- 65 600 B at Bp = 16384, above the 64 KiB a kernel gets without raising
hipFuncAttributeMaxDynamicSharedMemorySize -- and did not raise it; the launcher now does, once per process.  The cases
test_batch_hard_rows[16300-...] and [16384-...] (both Bp = 16384) are the ones that need it.  Nothing else was wrong: every other
case passed on its first run.
"""
import functools

import numpy as np
import pytest
import torch

from miner_reference import anchor_sets, batch_all_rows_reference, batch_hard_rows_reference

pytestmark = pytest.mark.gpu

F_SENT, I_SENT = -7.5, 0x5A5A5A5A          # what every output buffer holds before a call
H = 40


@pytest.fixture(scope="module")
def ops():
    from dae_rnn_news_recommendation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from dae_rnn_news_recommendation_amd import _lib
    _lib.load()
    return _lib


def _pad(n):
    return (n + 127) // 128 * 128


@functools.lru_cache(maxsize=None)
def _inputs(B, classes, scale, a0, n):
    """(labels[B], float32 D rows [n x B]) of the anchors [a0, a0 + n): D = float32(h h^T), h uniform in +-scale / 2."""
    rng = np.random.default_rng(B)
    h = (rng.random((B, H)) - 0.5) * scale
    lab = rng.integers(0, classes, B)
    D = (h[a0:a0 + n] @ h.T).astype(np.float32)
    D.setflags(write=False); lab.setflags(write=False)
    return lab, D


@functools.lru_cache(maxsize=None)
def _ref_all(B, classes, scale, a0, n, pos_only):
    lab, D = _inputs(B, classes, scale, a0, n)
    return batch_all_rows_reference(D, lab, a0, pos_only)


def _three_slabs(D):
    """Three float32 slabs whose float32 sum IN SLAB ORDER is D exactly (asserted): the half-precision head of D, the
    half-precision head of the rest, and what is left."""
    with np.errstate(over="ignore"):
        s0 = D.astype(np.float16).astype(np.float32)
        s0 = np.where(np.isfinite(s0), s0, np.float32(0))
        s1 = (D - s0).astype(np.float16).astype(np.float32)
    s2 = D - (s0 + s1)
    assert np.array_equal((s0 + s1) + s2, D) and s1.any() and s2.any()
    return np.stack([s0, s1, s2])


def _upload_D(D, B, splits, ldd):
    """[splits x (n + 1) x ldd] on the device: the anchors' rows in columns [0, B), NaN everywhere else (padding columns, spare row)."""
    n = D.shape[0]
    slabs = _three_slabs(D) if splits == 3 else D[None]
    assert slabs.shape[0] == splits
    host = np.full((splits, n + 1, ldd), np.nan, np.float32)
    host[:, :n, :B] = slabs
    return torch.from_numpy(host).cuda()[:, :n]


def _sentinel_out_all(n, Bp, pos_only, spare=2):
    return (torch.full((n + spare,), F_SENT, dtype=torch.float32, device="cuda"),
            torch.full((n + spare,), I_SENT, dtype=torch.int32, device="cuda"),
            torch.full((n + spare, Bp), F_SENT, dtype=torch.float32, device="cuda"),
            torch.full((n + spare, Bp), I_SENT, dtype=torch.int32, device="cuda") if pos_only else None)


def _check_footprint(out, n, B, Bp, a0):
    """Rows [0, n) written, everything else untouched; zeros in the padding columns and at the anchor's own column; all finite."""
    host = [None if t is None else t.cpu().numpy() for t in out]
    for k, t in enumerate(host):
        if t is None:
            continue
        sent = I_SENT if t.dtype == np.int32 else np.float32(F_SENT)
        assert (t[n:] == sent).all(), f"output {k}: rows beyond n_anchors were written"
        if t.ndim == 2:
            assert t.shape[1] == Bp and (t[:n, B:] == 0).all(), f"output {k}: padding columns not zero"
            assert (t[np.arange(n), a0 + np.arange(n)] == 0).all(), f"output {k}: the anchor's own column is not zero"
        if t.dtype == np.float32:
            assert np.isfinite(t).all(), f"output {k}: NaN / inf (the D padding leaked)"
    return host


def _check_rows(G, G_ref, tol):
    """Per row: max |err| <= tol * max |reference row|; an all-zero reference row must be exactly zero."""
    err = np.abs(G.astype(np.float64) - G_ref).max(axis=1)
    mx = np.abs(G_ref).max(axis=1)
    bad = np.flatnonzero(err > tol * mx)
    assert bad.size == 0, (bad[:8], err[bad[:8]], mx[bad[:8]])


def _check_all(host, ref, n, B, pos_only, fast):
    loss, npos, G, role = host
    assert np.array_equal(npos[:n].astype(np.int64), ref["npos_part"])
    if pos_only:
        assert np.array_equal(role[:n, :B].astype(np.int64), ref["role_cnt"])
    assert np.allclose(loss[:n], ref["loss_part"], rtol=2e-5, atol=1e-7), np.abs(loss[:n] / np.maximum(ref["loss_part"], 1e-30) - 1).max()
    _check_rows(G[:n, :B], ref["G"], 1e-4 if fast else 5e-5)


# ----------------------------------------------------------------------------------------------- #
# batch_all: anchor ranges and pos_triplets_only
# ----------------------------------------------------------------------------------------------- #
# (B, classes, scale, a0, n_anchors, splits, ldd - Bp, row-range class, modes)
ALL_CASES = [
    (300, 3, 2.0, 137, 60, 3, 64, "le40", ("all", "fast")),       # lane-grid kernel, pair sweeps, a range across arbitrary labels
    (257, 1, 2.0, 0, 257, 1, 0, "le40", ("all", "pos")),          # one class: no negatives, G exactly zero
    (257, 50, 2.0, 0, 257, 1, 0, "le40", ("all", "pos")),         # classes of one member (nP = 0)
    (800, 4, 2.2, 700, 100, 3, 0, "le40", ("pos",)),              # ~600 negatives: two chunks (6 registers, then <= 4), factorised
    (800, 4, 4.0, 700, 100, 3, 0, "mid", ("pos",)),               # range in (40, 80]: still factorised
    (800, 4, 12.0, 700, 100, 3, 0, "gt80", ("pos",)),             # range > 80: the direct sweep
    (1100, 5, 1.0, 1000, 100, 1, 128, "le40", ("all", "fast", "pos")),   # B > 1024: the strip-loop compaction with a0 > 0
    (4096, 6, 1.0, 4000, 16, 1, 0, "le40", ("all",)),             # Bp = 4096: 16 strips, one workgroup per CU
    (3072, 6, 1.0, 1500, 16, 1, 0, "le40", ("pos",)),             # the largest pos_triplets_only batch the LDS admits
]
ALL_PARAMS = [pytest.param(*c[:8], m, id=f"{c[0]}-{c[1]}-{c[2]}-{m}") for c in ALL_CASES for m in c[8]]


@pytest.mark.parametrize("B,classes,scale,a0,n,splits,ldd_extra,range_class,mode", ALL_PARAMS)
def test_batch_all_rows(ops, B, classes, scale, a0, n, splits, ldd_extra, range_class, mode):
    """Every path of the two batch_all kernels for an anchor range (a0 > 0 wherever the table has one) and for pos_triplets_only,
    per anchor against the float64 reference.  Conditions on the inputs are asserted on the reference, not assumed: the anchors'
    row range is in the class the case names, B = 800 gives every anchor two chunks of negatives, and in every pos-only case that
    has valid triplets at all (the one-class batch has none) between 10 % and 90 % of them are positive."""
    pos_only, fast = mode == "pos", mode == "fast"
    lab, D = _inputs(B, classes, scale, a0, n)
    ref = _ref_all(B, classes, scale, a0, n, pos_only)
    # the inputs are where the table says, so that the case cannot silently test another branch
    rr = ref["row_range"][ref["nvalid_part"] > 0]
    if rr.size:
        assert {"le40": rr.max() <= 40, "mid": rr.min() > 40 and rr.max() <= 80, "gt80": rr.min() > 80}[range_class], (rr.min(), rr.max())
    if classes == 1:
        assert ref["nvalid_part"].sum() == 0
    elif classes == 50:
        assert (np.array([len(anchor_sets(lab, a)[0]) for a in range(B)]) == 0).any()
    if B == 800:
        assert all(384 < len(anchor_sets(lab, a)[1]) <= 640 for a in range(a0, a0 + n))
    if pos_only and classes > 1:
        share = ref["npos_part"].sum() / ref["nvalid_part"].sum()
        assert 0.1 <= share <= 0.9, share
    Bp = _pad(B)
    Dd = _upload_D(D, B, splits, Bp + ldd_extra)
    labels = torch.from_numpy(lab.astype(np.int32)).cuda()
    out = _sentinel_out_all(n, Bp, pos_only)
    ops.triplet_batch_all_rows(Dd, labels, B, a0, n, pos_only, fast, out=out)
    torch.cuda.synchronize()
    host = _check_footprint(out, n, B, Bp, a0)
    _check_all(host, ref, n, B, pos_only, fast)
    if ref["nvalid_part"].sum() == 0:
        assert not host[2][:n].any() and not host[0][:n].any()


@pytest.mark.parametrize("mode", ["all", "pos"])
def test_batch_all_rows_column_ties(ops, mode):
    """Copied D columns -- a positive's onto a negative's, that negative's onto another negative's -- make T exactly 0 for those
    triplets: they are no positive triplets, so they are not counted and do not enter the pos-only loss, G or role counts."""
    B, classes, scale, a0, n = 300, 3, 2.0, 137, 60
    lab, D0 = _inputs(B, classes, scale, a0, n)
    D = D0.copy()
    j0, j1, j2 = (int(np.flatnonzero(lab == c)[3]) for c in range(3))       # one column of each class, none of them an anchor's own
    assert not any(a0 <= j < a0 + n for j in (j0, j1, j2))
    D[:, j1] = D[:, j0]
    D[:, j2] = D[:, j1]
    pos_only = mode == "pos"
    ref = batch_all_rows_reference(D, lab, a0, pos_only)
    assert (ref["nzero_part"] >= 2).all()                                    # every anchor has exact ties among its valid triplets
    Bp = _pad(B)
    Dd = _upload_D(D, B, 3, Bp + 64)
    labels = torch.from_numpy(lab.astype(np.int32)).cuda()
    out = _sentinel_out_all(n, Bp, pos_only)
    ops.triplet_batch_all_rows(Dd, labels, B, a0, n, pos_only, False, out=out)
    torch.cuda.synchronize()
    host = _check_footprint(out, n, B, Bp, a0)
    _check_all(host, ref, n, B, pos_only, False)


@functools.lru_cache(maxsize=None)
def _whole_batch(B, classes, scale, pos_only):
    """One whole-batch call through the _rows entry (a0 = 0, n_anchors = B) on a [B x Bp] D; buffers Bp rows tall, zero-filled."""
    from dae_rnn_news_recommendation_amd import ops
    lab, D = _inputs(B, classes, scale, 0, B)
    Bp = _pad(B)
    Dd = _upload_D(D, B, 1, Bp)
    labels = torch.from_numpy(lab.astype(np.int32)).cuda()
    out = (torch.zeros(Bp, dtype=torch.float32, device="cuda"), torch.zeros(Bp, dtype=torch.int32, device="cuda"),
           torch.zeros((Bp, Bp), dtype=torch.float32, device="cuda"),
           torch.zeros((Bp, Bp), dtype=torch.int32, device="cuda") if pos_only else None)
    ops.triplet_batch_all_rows(Dd, labels, B, 0, B, pos_only, False, out=out)
    torch.cuda.synchronize()
    return Dd, labels, out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("B,classes,scale,mode", [(800, 4, 2.2, "pos"), (1100, 5, 1.0, "all"), (1100, 5, 1.0, "pos")])
def test_batch_all_rows_parts_equal_the_whole(ops, B, classes, scale, mode):
    """Every anchor is swept by one workgroup alone, whatever the grid: three calls over the ragged ranges [0, 1), [1, B - 129),
    [B - 129, B) give the bits of the whole-batch call (which exceeds the resident slots: snake packing, here also pos-only)."""
    pos_only = mode == "pos"
    Dd, labels, whole = _whole_batch(B, classes, scale, pos_only)
    Bp = _pad(B)
    for a0, a1 in ((0, 1), (1, B - 129), (B - 129, B)):
        n = a1 - a0
        out = _sentinel_out_all(n, Bp, pos_only)
        ops.triplet_batch_all_rows(Dd[:, a0:a1], labels, B, a0, n, pos_only, False, out=out)
        torch.cuda.synchronize()
        _check_footprint(out, n, B, Bp, a0)
        for k, (part, full) in enumerate(zip(out, whole)):
            if part is not None:
                assert torch.equal(_bits(part[:n]), _bits(full[a0:a1])), (k, a0, a1)


def test_triplet_finalize_pos_only_at_800(ops, L):
    """dae_triplet_finalize's O(B^2) role-count fold at a real batch size: normalisers, data weights and cw of the pos-only miner."""
    B, classes, scale, alpha = 800, 4, 2.2, 0.5
    lab, D = _inputs(B, classes, scale, 0, B)
    ref = batch_all_rows_reference(D, lab, 0, True, want_grad=False)
    Dd, labels, (lp, npos, G, role) = _whole_batch(B, classes, scale, True)
    Bp = _pad(B)
    nvalid, _, cw = ops.label_stats(labels, B, L.TRIPLET["batch_all"])
    tri, dwf = ops.triplet_finalize(L.TRIPLET["batch_all"], True, B, alpha, lp, npos, nvalid, None, role, cw)
    tri, dwf, cw = tri.cpu().numpy(), dwf.cpu().numpy(), cw.cpu().numpy()
    num, nv = int(ref["npos_part"].sum()), int(ref["nvalid_part"].sum())
    assert int(nvalid.item()) == nv and 0.1 <= num / nv <= 0.9
    assert tri[3] == np.float32(num)
    assert np.isclose(tri[0], alpha / num, rtol=1e-6) and np.isclose(tri[2], num / nv, rtol=1e-6)
    assert np.isclose(tri[1], ref["loss_part"].sum() / num, rtol=2e-5)
    dw = ref["npos_part"] + ref["role_cnt"].sum(axis=0)
    assert dw.max() < 2 ** 24 and np.array_equal(dwf[:B], dw.astype(np.float32)) and (dwf[B:] == 0).all()
    assert np.allclose(cw[:B], dw / (dw.sum() + 1e-16), rtol=1e-6) and (cw[B:] == 0).all()


def test_batch_all_rows_refusals(ops, L):
    """Argument checks: nothing is launched, the buffers keep their sentinel."""
    def refused(B, a0, n, pos_only, match):
        Bp = _pad(B)
        Dd = torch.zeros((1, max(n, 1), Bp), dtype=torch.float32, device="cuda")
        labels = torch.zeros(B, dtype=torch.int32, device="cuda")
        out = _sentinel_out_all(max(n, 1), Bp, True, spare=0)
        with pytest.raises(RuntimeError, match=match):
            ops.triplet_batch_all_rows(Dd, labels, B, a0, n, pos_only, False, out=out)
        torch.cuda.synchronize()
        for t in out:
            sent = I_SENT if t.dtype == torch.int32 else F_SENT
            assert bool((t == sent).all())
    refused(3073, 0, 4, True, r"needs \d+ B of LDS")          # Bp = 3200: 52 B per column no longer fit 160 KiB
    refused(300, 290, 11, False, "outside the batch")
    refused(300, 0, 0, False, "outside the batch")
    refused(4097, 0, 4, False, "exceeds the supported 4096")
    out = _sentinel_out_all(4, _pad(3073), False, spare=0)     # the same batch is accepted without pos_triplets_only
    ops.triplet_batch_all_rows(torch.zeros((1, 4, 3200), dtype=torch.float32, device="cuda"),
                               torch.zeros(3073, dtype=torch.int32, device="cuda"), 3073, 0, 4, False, False, out=out)
    torch.cuda.synchronize()
    assert not bool(out[2].any())                              # one class: zero gradient rows


# ----------------------------------------------------------------------------------------------- #
# batch_hard: anchor ranges up to the advertised Bp = 16384
# ----------------------------------------------------------------------------------------------- #
def _sentinel_out_hard(n, Bp, spare=2):
    return (torch.full((n + spare,), F_SENT, dtype=torch.float32, device="cuda"),
            torch.full((n + spare,), I_SENT, dtype=torch.int32, device="cuda"),
            torch.full((Bp,), I_SENT, dtype=torch.int32, device="cuda"),
            torch.full((n + spare, Bp), F_SENT, dtype=torch.float32, device="cuda"))


def _run_hard(ops, D, lab, B, a0, n, splits, ldd_extra):
    Bp = _pad(B)
    Dd = _upload_D(D, B, splits, Bp + ldd_extra)
    labels = torch.from_numpy(lab.astype(np.int32)).cuda()
    out = _sentinel_out_hard(n, Bp)
    ops.triplet_batch_hard_rows(Dd, labels, B, a0, n, out=out)
    torch.cuda.synchronize()
    loss, cnt, dw, G = (t.cpu().numpy() for t in out)
    assert (loss[n:] == np.float32(F_SENT)).all() and (cnt[n:] == I_SENT).all() and (G[n:] == np.float32(F_SENT)).all()
    assert (G[:n, B:] == 0).all() and np.isfinite(G[:n]).all() and np.isfinite(loss[:n]).all()
    assert (dw[B:] == 0).all()                                  # dw[Bp] is zeroed by every call
    return loss[:n], cnt[:n], dw[:B], G[:n, :B], out


def _check_hard(got, ref):
    loss, cnt, dw, G = got[:4]
    assert np.array_equal(cnt.astype(np.int64), ref["cnt_part"])
    assert np.array_equal(dw.astype(np.int64), ref["dw"])
    assert np.allclose(loss, ref["loss_part"], rtol=1e-5, atol=1e-7)
    _check_rows(G, ref["G"], 5e-5)


@pytest.mark.parametrize("B,classes,a0,n,splits,ldd_extra", [(333, 7, 100, 133, 3, 64), (5000, 5, 4990, 10, 1, 0),
                                                              (16300, 5, 16290, 10, 1, 0), (16384, 5, 0, 4, 1, 0)])
def test_batch_hard_rows(ops, B, classes, a0, n, splits, ldd_extra):
    lab, D = _inputs(B, classes, 2.0, a0, n)
    ref = batch_hard_rows_reference(D, lab, a0)
    assert ref["cnt_part"].sum() > 0
    _check_hard(_run_hard(ops, D, lab, B, a0, n, splits, ldd_extra), ref)


def test_batch_hard_rows_ties(ops):
    """Duplicated D entries tie the hardest positive, the hardest negative and the row maximum; an anchor without positives sends its
    positive-side gradient through the row-max shift.  The gradient splits equally among the tied columns."""
    B, classes, a0, n = 333, 7, 100, 133
    lab0, D0 = _inputs(B, classes, 2.0, a0, n)
    lab, D = lab0.copy(), D0.copy()
    lab[a0 + 5] = classes                                       # a class of one member inside the range
    tied = []
    for r in range(n):
        P, N = anchor_sets(lab, a0 + r)
        d = D[r]
        if len(P) >= 2:
            jp = P[np.argmin(d[P])]; jp2 = P[0] if P[0] != jp else P[1]
            d[jp2] = d[jp]
        else:
            jp = jp2 = None
        jn = N[np.argmax(d[N])]; jn2 = N[0] if N[0] != jn else N[1]
        d[jn2] = d[jn]
        jm = N[2] if N[2] not in (jn, jn2) else N[3]
        if r % 2 == 0 or jp is None:                            # the row maximum (the anchor's own column) tied with a negative's
            assert d[a0 + r] == d.max()
            d[jm] = d[a0 + r]
            jn, jn2 = a0 + r, jm                                # ... which thereby becomes the hardest negative; its partner is the anchor's column
        tied.append((jp, jp2, jn, jn2))
    ref = batch_hard_rows_reference(D, lab, a0)
    assert ref["cnt_part"].all()
    got = _run_hard(ops, D, lab, B, a0, n, 1, 64)
    _check_hard(got, ref)
    G = got[3]
    for r, (jp, jp2, jn, jn2) in enumerate(tied):
        if jp is not None:
            assert G[r, jp] == G[r, jp2] and ref["G"][r, jp] == ref["G"][r, jp2] != 0
        if jn != a0 + r:
            assert G[r, jn] == G[r, jn2] and ref["G"][r, jn] == ref["G"][r, jn2] != 0
    r = 5                                                       # no positives: hp is a shifted invalid entry, its gradient lands on the tied row maxima
    assert tied[r][0] is None and ref["G"][r, a0 + r] != 0 and G[r, a0 + r] != 0


def test_batch_hard_rows_self_column_is_excluded_by_index(ops):
    """On a Gram matrix the anchor's own column is the row maximum and never the hardest positive, so a kernel that excluded
    column `row` instead of column `a0 + row` would go unnoticed.  Here D is edited so that only the INDEX tells: every anchor's
    own column holds the smallest value of its row, and column `row` -- a different batch element, a positive of the anchor
    wherever the labels agree -- is made the hardest positive of those anchors."""
    B, classes, a0, n = 333, 7, 100, 133
    lab, D0 = _inputs(B, classes, 2.0, a0, n)
    D = D0.copy()
    hardest = 0
    for r in range(n):
        a = a0 + r
        D[r, a] = D[r].min() - np.float32(1.0)
        P, _ = anchor_sets(lab, a)
        if lab[r] == lab[a]:
            D[r, r] = D[r, P].min() - np.float32(0.5)
            hardest += 1
    assert hardest >= 10
    ref = batch_hard_rows_reference(D, lab, a0)
    assert ref["cnt_part"].sum() >= n // 2 and all(ref["G"][r, r] < 0 for r in range(n) if lab[r] == lab[a0 + r] and ref["cnt_part"][r])
    _check_hard(_run_hard(ops, D, lab, B, a0, n, 1, 0), ref)


def test_batch_hard_rows_parts_equal_the_whole(ops):
    B, classes = 333, 7
    lab, D = _inputs(B, classes, 2.0, 0, B)
    whole = _run_hard(ops, D, lab, B, 0, B, 1, 0)
    _check_hard(whole, batch_hard_rows_reference(D, lab, 0))
    dw = np.zeros(B, np.int64)
    for a0, a1 in ((0, 1), (1, B - 129), (B - 129, B)):
        part = _run_hard(ops, D[a0:a1], lab, B, a0, a1 - a0, 1, 0)
        dw += part[2]
        assert np.array_equal(part[3].view(np.int32), whole[3][a0:a1].view(np.int32))
        assert np.array_equal(part[0].view(np.int32), whole[0][a0:a1].view(np.int32)) and np.array_equal(part[1], whole[1][a0:a1])
    assert np.array_equal(dw, whole[2].astype(np.int64))


def test_batch_hard_rows_refusals(ops):
    B = 16385                                                   # Bp = 16512
    Bp = _pad(B)
    out = _sentinel_out_hard(2, Bp, spare=0)
    with pytest.raises(RuntimeError, match="too large"):
        ops.triplet_batch_hard_rows(torch.zeros((1, 2, Bp), dtype=torch.float32, device="cuda"),
                                    torch.zeros(B, dtype=torch.int32, device="cuda"), B, 0, 2, out=out)
    with pytest.raises(RuntimeError, match="outside the batch"):
        ops.triplet_batch_hard_rows(torch.zeros((1, 2, 384), dtype=torch.float32, device="cuda"),
                                    torch.zeros(300, dtype=torch.int32, device="cuda"), 300, 299, 2, out=out)
    torch.cuda.synchronize()
    for t in out:
        assert bool((t == (I_SENT if t.dtype == torch.int32 else F_SENT)).all())
