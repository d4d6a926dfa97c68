"""CPU checks of the user-state and seen-aware retrieval entry points (dae_user_states, dae_topk_similarity_ex) and of the host
code around them: both builds export the symbols under an unchanged ABI version, argument errors are reported before any HIP
call (so on a machine without a GPU), the workspace has no Nq x Nc term, and the host helpers -- next_click_metrics,
synthetic_sessions, decay_factors, normalize_exclusions, popularity_recommend -- on hand-made cases."""
import ctypes
import math

import numpy as np
import pytest

P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_new_symbols_are_exported_and_the_abi_version_stays(fmt):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load(fmt)
    for name in ("dae_user_states", "dae_topk_similarity_ex", "dae_topk_similarity_ex_workspace"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.dae_abi_version() == _lib.ABI_VERSION == 9


def _user(lib, E=P, lde=64, Na=100, H=64, indptr=P, items=P, M=10, nnz=50, beta=0.9, decay=None, all_states=0, U=P, ldu=64):
    return lib.dae_user_states(E, lde, Na, H, indptr, items, M, nnz, beta, decay, all_states, U, ldu, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(E=None), b"E / indptr are NULL"),
    (dict(indptr=None), b"E / indptr are NULL"),
    (dict(items=None), b"items is NULL"),
    (dict(U=None), b"U is NULL"),
    (dict(U=None, all_states=1), b"U is NULL"),
    (dict(H=0), b"H must be positive"),
    (dict(H=-3), b"H must be positive"),
    (dict(Na=0), b"Na must be positive"),
    (dict(M=-1), b"negative count"),
    (dict(nnz=-1), b"negative count"),
    (dict(lde=63), b"must be >= H"),
    (dict(ldu=10), b"must be >= H"),
    (dict(beta=-0.1), b"beta must be in [0, 1]"),
    (dict(beta=1.5), b"beta must be in [0, 1]"),
    (dict(beta=float("nan")), b"beta must be in [0, 1]"),
])
def test_user_states_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _user(lib, **kw) != 0
    assert msg in lib.dae_last_error(), lib.dae_last_error()


def test_user_states_of_no_users_is_a_no_op():
    lib = _lib()
    assert _user(lib, M=0, nnz=0, items=None, U=None) == 0              # nothing to launch: returns before any HIP call


def _topk_ex(lib, xp=P, xi=P, Nq=100, Nc=100, D=50, k=10, ws=P, ws_bytes=None, norm=0, exclude_self=1):
    if ws_bytes is None:
        ws_bytes = lib.dae_topk_similarity_ex_workspace(Nq, Nc, D, k)
    return lib.dae_topk_similarity_ex(P, D, Nq, None, 0, Nc, D, norm, 0, k, exclude_self, xp, xi, P, P, k, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(xp=None), b"excl_indptr and excl_items go together"),
    (dict(xi=None), b"excl_indptr and excl_items go together"),
    (dict(k=0), b"k must be in 1..128"),
    (dict(k=129), b"k must be in 1..128"),
    (dict(norm=4), b"norm must be"),
    (dict(Nc=99), b"bad corpus"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
])
def test_topk_ex_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _topk_ex(lib, **kw) != 0
    assert msg in lib.dae_last_error(), lib.dae_last_error()


def test_workspace_has_no_quadratic_term():
    lib = _lib()
    ws = lib.dae_topk_similarity_ex_workspace
    big = ws(10 ** 6, 10 ** 6, 500, 128)
    assert 0 < big < 10 ** 12 * 4 // 100                     # the Nq x Nc fp32 matrix would be 4e12 bytes
    # equal steps of the row counts give equal growth, up to the 256-byte alignment of the pieces
    a, b, c = (ws(n * 128 * 1024, n * 128 * 1024, 500, 10) for n in (2, 4, 6))
    assert abs((c - b) - (b - a)) <= 4096 and b > a
    a, b, c = (ws(n * 100000, 50000, 500, 10) for n in (1, 2, 3))
    assert abs((c - b) - (b - a)) <= 4096 and b > a
    # the exclusion lists are read in place: the same bytes as the plain call, whatever the shape
    for shape in ((1000, 1000, 64, 10), (129, 5000, 500, 128), (10 ** 5, 8000, 500, 100)):
        assert ws(*shape) == lib.dae_topk_similarity_workspace(*shape) > 0
    assert ws(0, 10, 10, 16) == 0 and ws(10, 0, 10, 16) == 0 and ws(10, 10, 0, 16) == 0 and ws(10, 10, 10, 0) == 0
    # dae_user_states takes no workspace at all: its signature has none (14 arguments, the last is the stream)
    from dae_rnn_news_recommendation_amd import _lib as L
    assert len(L.SIGNATURES["dae_user_states"][1]) == 14


def test_next_click_metrics_on_hand_made_lists():
    from dae_rnn_news_recommendation_amd.helpers import next_click_metrics
    idx = np.array([[7, 3, 9, 1],        # hit at rank 1
                    [4, 5, 6, 2],        # hit at rank k = 4
                    [4, 5, 6, 2],        # miss
                    [8, -1, -1, -1],     # short list; the target is not in it and -1 matches nothing
                    [8, -1, -1, -1]])    # not counted: no target
    m = next_click_metrics(idx, [7, 2, 0, 3, -1])
    assert m["n"] == 4
    assert m["hit"] == pytest.approx(2 / 4)
    assert m["mrr"] == pytest.approx((1 + 1 / 4) / 4)
    assert m["ndcg"] == pytest.approx((1 + 1 / math.log2(5)) / 4)
    m = next_click_metrics(np.array([[-1, -1]]), [-1])
    assert m["n"] == 0 and math.isnan(m["hit"]) and math.isnan(m["mrr"]) and math.isnan(m["ndcg"])
    m = next_click_metrics(np.array([[5, 6]]), [6])
    assert m == {"hit": 1.0, "mrr": 0.5, "ndcg": pytest.approx(1 / math.log2(3)), "n": 1}
    with pytest.raises(ValueError):
        next_click_metrics(np.array([1, 2, 3]), [1, 2, 3])
    with pytest.raises(ValueError):
        next_click_metrics(np.array([[1, 2]]), [1, 2])


def test_synthetic_sessions_is_deterministic_per_seed():
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
    labels = np.repeat(np.arange(50), 20)
    a = synthetic_sessions(500, labels, mean_len=12, seed=3)
    b = synthetic_sessions(500, labels, mean_len=12, seed=3)
    c = synthetic_sessions(500, labels, mean_len=12, seed=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not (np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]))
    indptr, items = a
    assert indptr.dtype == np.int64 and items.dtype == np.int32 and indptr[0] == 0 and indptr[-1] == items.size
    lens = np.diff(indptr)
    assert lens.min() >= 1 and 9 < lens.mean() < 15
    assert items.min() >= 0 and items.max() < labels.size
    # a user reads mostly from two classes: the two commonest classes of a long history hold most of its clicks
    share = [np.sort(np.bincount(labels[items[indptr[u]:indptr[u + 1]]]))[-2:].sum() / lens[u] for u in range(500) if lens[u] >= 20]
    assert len(share) > 30 and np.mean(share) > 0.8


def test_decay_factors_from_timestamps():
    from dae_rnn_news_recommendation_amd.helpers import decay_factors
    indptr = np.array([0, 3, 3, 5])
    t = np.array([10.0, 12.0, 12.0, 100.0, 103.0])
    d = decay_factors(indptr, t, 0.5, time_unit=2.0)
    assert d.dtype == np.float32
    want = np.array([1.0, 0.5 ** 1.0, 1.0, 1.0, 0.5 ** 1.5], dtype=np.float64).astype(np.float32)
    assert np.array_equal(d, want)                                       # float64 power, rounded once
    assert np.array_equal(decay_factors(indptr, t, 0.0), np.array([1, 0, 1, 1, 0], np.float32))      # beta 0: a gap resets, none keeps
    assert np.array_equal(decay_factors(indptr, t, 1.0), np.ones(5, np.float32))
    assert np.array_equal(decay_factors(indptr, t, 0.9), (0.9 ** np.array([0, 2.0, 0, 0, 3.0])).astype(np.float32))   # unit 1
    with pytest.raises(ValueError, match="decrease within a user"):
        decay_factors(indptr, np.array([10.0, 9.0, 12.0, 100.0, 103.0]), 0.5)
    decay_factors(indptr, np.array([10.0, 11.0, 12.0, 1.0, 3.0]), 0.5)   # a new user may start earlier than the last one ended
    with pytest.raises(ValueError, match="timestamps for"):
        decay_factors(indptr, t[:4], 0.5)
    with pytest.raises(ValueError, match="time_unit"):
        decay_factors(indptr, t, 0.5, time_unit=0.0)
    with pytest.raises(ValueError, match="beta"):
        decay_factors(indptr, t, 1.5)


def test_normalize_exclusions_sorts_dedups_and_drops_out_of_range():
    from dae_rnn_news_recommendation_amd.helpers import normalize_exclusions
    xp, xi = normalize_exclusions([[5, 1, 5, 3], [], [99, -1, 100, 0, 7, 7], [2]], 4, 100)
    assert xp.dtype == np.int64 and xi.dtype == np.int32
    assert xp.tolist() == [0, 3, 3, 6, 7] and xi.tolist() == [1, 3, 5, 0, 7, 99, 2]
    # the (indptr, items) tuple form gives the same
    xp2, xi2 = normalize_exclusions((np.array([0, 4, 4, 10, 11]), np.array([5, 1, 5, 3, 99, -1, 100, 0, 7, 7, 2])), 4, 100)
    assert np.array_equal(xp, xp2) and np.array_equal(xi, xi2)
    xp, xi = normalize_exclusions([[], []], 2, 10)
    assert xp.tolist() == [0, 0, 0] and xi.size == 0
    with pytest.raises(ValueError, match="rows for"):
        normalize_exclusions([[1]], 2, 10)
    with pytest.raises(ValueError, match="integer"):
        normalize_exclusions([[1.5]], 1, 10)
    with pytest.raises(ValueError, match="indptr"):
        normalize_exclusions((np.array([0, 3]), np.array([1, 2])), 1, 10)


def test_popularity_recommend_skips_what_the_user_has_seen():
    from dae_rnn_news_recommendation_amd.helpers import popularity_recommend
    hist = [[0, 0, 1], [0, 2, 2], [3]]                                   # clicks: article 0: 3, 2: 2, 1: 1, 3: 1, 4: 0
    out = popularity_recommend(hist, 5, 3)
    assert out.tolist() == [[2, 3, 4], [1, 3, 4], [0, 2, 1]]
    assert popularity_recommend(hist, 5, 3, seen=[[0, 1, 2, 3], [], []]).tolist() == [[4, -1, -1], [0, 2, 1], [0, 2, 1]]
