"""CPU checks of the near-duplicate search entry points: argument errors are reported before any HIP call (so on a machine
without a GPU), the workspace has no N x N term and is linear in the capacity, and the host helpers duplicate_groups /
duplicate_pair_precision on worked examples."""
import ctypes

import numpy as np
import pytest


def _lib():
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load()


P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first


def _call(lib, Nq=100, C=None, Nc=100, D=50, ldq=None, ldc=None, norm=0, metric=0, threshold=0.5, capacity=1000, ws=P, ws_bytes=None,
          out=P):
    if ws_bytes is None:
        ws_bytes = lib.dae_threshold_pairs_workspace(Nq, Nc, D, capacity)
    count = ctypes.c_uint64(12345)
    rc = lib.dae_threshold_pairs(P, D if ldq is None else ldq, Nq, C, D if ldc is None else ldc, Nc, D, norm, metric, threshold,
                                 out, out, out, capacity, ctypes.byref(count), ws, ws_bytes, None)
    return rc


@pytest.mark.parametrize("kw, msg", [
    (dict(norm=4), b"norm must be"),
    (dict(norm=-1), b"norm must be"),
    (dict(metric=2), b"metric must be 0 (cosine) or 1 (linear kernel)"),
    (dict(threshold=float("nan")), b"threshold is NaN"),
    (dict(ldq=49), b"ldq"),
    (dict(Nc=99), b"bad corpus"),
    (dict(C=P, Nc=0), b"bad corpus"),
    (dict(C=P, Nc=300, ldc=49), b"bad corpus"),
    (dict(Nq=2 ** 21, Nc=2 ** 21, D=512, capacity=0, ws_bytes=1 << 40), b"operand image exceeds 4 GiB"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
    (dict(out=None), b"rows / cols / scores are NULL"),
])
def test_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _call(lib, **kw) != 0
    assert msg in lib.dae_last_error(), lib.dae_last_error()


def test_workspace_has_no_quadratic_term_and_is_linear_in_capacity():
    lib = _lib()
    ws = lib.dae_threshold_pairs_workspace
    big = ws(10 ** 6, 10 ** 6, 500, 10 ** 7)
    assert 0 < big < 10 ** 12 * 4 // 100                     # the N x N fp32 matrix would be 4e12 bytes
    # equal steps of the capacity give equal growth, up to the 256-byte alignment of the pieces
    a, b, c = (ws(10 ** 6, 10 ** 6, 500, n * 10 ** 7) for n in (1, 2, 3))
    assert abs((c - b) - (b - a)) <= 4096 and b - a >= 20 * 10 ** 7      # 8 + 4 + 8 bytes per record at the least
    assert b - a < 200 * 10 ** 7
    # and equal steps of the row counts
    a, b, c = (ws(n * 128 * 1024, n * 128 * 1024, 500, 10 ** 6) for n in (2, 4, 6))
    assert abs((c - b) - (b - a)) <= 4096 and b > a
    # a pure count needs the operand images and the cursor only
    assert ws(1000, 1000, 64, 0) <= 2 * 1024 * 128 * 4 + 1024
    assert ws(0, 10, 10, 10) == 0 and ws(10, 0, 10, 10) == 0 and ws(10, 10, 0, 10) == 0


def test_duplicate_groups_worked_example():
    from dae_rnn_news_recommendation_amd.helpers import duplicate_groups
    # a chain 0-3, 3-5 (as the lower-triangle pairs similar_pairs returns) and the pair 6-2; items 1 and 4 have no partner
    group, keep = duplicate_groups(np.array([3, 5, 6]), np.array([0, 3, 2]), 7)
    assert group.dtype == np.int64 and keep.dtype == bool
    assert group.tolist() == [0, 1, 2, 0, 4, 0, 2]
    assert keep.tolist() == [True, True, True, False, True, False, False]
    # the orientation and the order of the pairs do not matter, a repeated pair neither
    g2, k2 = duplicate_groups([0, 2, 3, 5], [3, 6, 5, 3], 7)
    assert np.array_equal(g2, group) and np.array_equal(k2, keep)
    # no pair: the identity
    group, keep = duplicate_groups(np.zeros(0, np.int64), np.zeros(0, np.int64), 4)
    assert group.tolist() == [0, 1, 2, 3] and keep.all() and keep.shape == (4,)
    group, keep = duplicate_groups([], [], 0)
    assert group.shape == (0,) and keep.shape == (0,)
    with pytest.raises(ValueError):
        duplicate_groups([7], [0], 7)


def test_duplicate_pair_precision_worked_example():
    from dae_rnn_news_recommendation_amd.helpers import duplicate_pair_precision
    labels = np.array([0, 0, 1, 1, -1, np.nan, 0])
    rows = np.array([1, 2, 3, 4, 5, 6, 6])
    cols = np.array([0, 0, 2, 0, 1, 0, 2])
    # 1-0 equal, 2-0 differ, 3-2 equal, 4-0 and 5-1 skipped (missing label), 6-0 equal, 6-2 differ
    p, n = duplicate_pair_precision(rows, cols, labels)
    assert n == 5 and p == pytest.approx(3 / 5)
    p, n = duplicate_pair_precision([4, 5], [0, 1], labels)
    assert np.isnan(p) and n == 0
    p, n = duplicate_pair_precision([], [], labels)
    assert np.isnan(p) and n == 0
    # queries against a corpus with its own labels (strings work too)
    p, n = duplicate_pair_precision([0, 1, 1], [0, 0, 1], np.array(["a", "b"]), candidate_labels=np.array(["a", "b"]))
    assert (p, n) == (pytest.approx(2 / 3), 3)
