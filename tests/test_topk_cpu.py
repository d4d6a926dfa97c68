"""CPU checks of the top-k retrieval entry points: argument errors are reported before any HIP call (so on a machine without a
GPU), the workspace has no N x N term, and helpers.label_precision_at_k on a worked example."""
import ctypes

import numpy as np
import pytest


def _lib():
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load()


P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first


def _call(lib, Nq=100, C=None, Nc=100, D=50, norm=0, metric=0, k=10, exclude_self=0, ldk=None, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_topk_similarity_workspace(Nq, Nc, D, max(k, 1))
    return lib.dae_topk_similarity(P, D, Nq, C, D, Nc, D, norm, metric, k, exclude_self, P, P, k if ldk is None else ldk, P, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(k=0), b"k must be in 1..128"),
    (dict(k=129), b"k must be in 1..128"),
    (dict(C=P, Nc=300, exclude_self=1), b"exclude_self needs C == NULL"),
    (dict(norm=4), b"norm must be"),
    (dict(norm=-1), b"norm must be"),
    (dict(metric=2), b"metric must be 0 (cosine) or 1 (linear kernel)"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(k=10, ldk=5), b"ldk"),
    (dict(Nc=99), b"bad corpus"),
])
def test_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _call(lib, **kw) != 0
    assert msg in lib.dae_last_error(), lib.dae_last_error()


def test_workspace_has_no_quadratic_term():
    lib = _lib()
    ws = lib.dae_topk_similarity_workspace
    big = ws(10 ** 6, 10 ** 6, 500, 100)
    assert 0 < big < 10 ** 12 * 4 // 100                     # the N x N fp32 matrix would be 4e12 bytes
    # linear in Nq (large Nq: one corpus slice): equal steps give equal growth, up to the 256-byte alignment of the pieces
    a, b, c = (ws(n * 128 * 1024, 10 ** 6, 500, 100) for n in (2, 4, 6))
    assert abs((c - b) - (b - a)) <= 1024 and b > a
    assert ws(1000, 1000, 64, 10) < 1000 * 1000 * 4          # a small query set: the partial lists of its slices, still no N x N
    assert ws(0, 10, 10, 10) == 0 and ws(10, 10, 10, 0) == 0


def test_label_precision_at_k_worked_example():
    from dae_rnn_news_recommendation_amd.helpers import label_precision_at_k
    labels = np.array([0, 0, 1, 1, -1, np.nan, 0])
    idx = np.array([[1, 6, 2],       # 0 -> labels 0, 0, 1      : 2/3
                    [0, 2, -1],      # 0 -> 0, 1, miss          : 1/3
                    [3, 4, 5],       # 1 -> 1, missing, missing : 1/3
                    [2, 0, 1],       # 1 -> 1, 0, 0             : 1/3
                    [0, 1, 2],       # label -1: skipped
                    [0, 1, 2],       # label NaN: skipped
                    [-1, -1, -1]])   # 0 -> nothing             : 0
    p, n = label_precision_at_k(idx, labels)
    assert n == 5
    assert p == pytest.approx((2 / 3 + 1 / 3 + 1 / 3 + 1 / 3 + 0) / 5)
    # queries against a corpus with its own labels (strings work too)
    p, n = label_precision_at_k(np.array([[0, 1], [1, -1]]), np.array(["a", "b"]), candidate_labels=np.array(["a", "b"]))
    assert (p, n) == (pytest.approx(0.5 * (0.5 + 0.5)), 2)
    p, n = label_precision_at_k(np.array([[0]]), np.array([-3]))
    assert np.isnan(p) and n == 0
