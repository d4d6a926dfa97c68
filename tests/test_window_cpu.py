"""CPU checks of the candidate windows (dae_topk_similarity_win, dae_rank_similarity_win) and of the host code around them: both
builds export the symbols under an unchanged ABI version, argument errors are reported before any HIP call (so on a machine
without a GPU), the workspaces equal those of the plain calls, and candidate_windows, the window= validation, the windowed
popularity baselines and synthetic_timed_sessions on hand-made data."""
import ctypes

import numpy as np
import pytest

P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first
NAMES = ("dae_topk_similarity_win", "dae_topk_similarity_win_workspace", "dae_rank_similarity_win", "dae_rank_similarity_win_workspace")


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_window_symbols_are_exported_and_the_abi_version_stays(fmt):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load(fmt)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.dae_abi_version() == _lib.ABI_VERSION == 9


def _topk(lib, Q=P, Nq=100, C=None, ldc=0, Nc=100, D=50, k=10, exclude_self=1, xp=P, xi=P, lo=P, hi=P, idx=P, score=P, ws=P,
          ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_topk_similarity_win_workspace(Nq, Nc, D, k)
    return lib.dae_topk_similarity_win(Q, D, Nq, C, ldc, Nc, D, 0, 0, k, exclude_self, xp, xi, lo, hi, idx, score, k, ws, ws_bytes, None)


def _rank(lib, Q=P, Nq=100, C=None, ldc=0, Nc=100, D=50, exclude_self=1, xp=P, xi=P, lo=P, hi=P, targets=P, rank=P, score=P, ws=P,
          ws_bytes=None, k=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_rank_similarity_win_workspace(Nq, Nc, D)
    return lib.dae_rank_similarity_win(Q, D, Nq, C, ldc, Nc, D, 0, 0, exclude_self, xp, xi, lo, hi, targets, rank, score, ws, ws_bytes,
                                       None)


@pytest.mark.parametrize("call, prefix", [(_topk, b"topk_similarity"), (_rank, b"rank_similarity")])
@pytest.mark.parametrize("kw, msg", [
    (dict(lo=None), b"win_lo and win_hi go together"),
    (dict(hi=None), b"win_lo and win_hi go together"),
    (dict(xp=None), b"excl_indptr and excl_items go together"),
    (dict(xi=None, lo=None, hi=None), b"excl_indptr and excl_items go together"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
    (dict(Q=None), b"bad input"),
    (dict(C=P, ldc=50, exclude_self=1), b"exclude_self needs C == NULL"),
])
def test_window_argument_errors_without_a_gpu(call, prefix, kw, msg):
    lib = _lib()
    assert call(lib, **kw) != 0
    err = lib.dae_last_error()
    assert err.startswith(prefix + b":") and msg in err, err
    if b"win_lo" in msg:
        assert b"win_lo" in err and b"win_hi" in err


def test_window_topk_k_out_of_range_without_a_gpu():
    lib = _lib()
    assert _topk(lib, k=129) != 0
    assert b"topk_similarity: k must be in 1..128 (got 129)" in lib.dae_last_error()


@pytest.mark.parametrize("shape", [(1, 1, 1), (100, 100, 50), (300, 700, 70), (100000, 64000, 500), (129, 4097, 513)])
def test_window_workspaces_equal_the_plain_ones(shape):
    lib = _lib()
    Nq, Nc, D = shape
    for k in (1, 10, 128):
        assert lib.dae_topk_similarity_win_workspace(Nq, Nc, D, k) == lib.dae_topk_similarity_workspace(Nq, Nc, D, k) > 0
    assert lib.dae_rank_similarity_win_workspace(Nq, Nc, D) == lib.dae_rank_similarity_workspace(Nq, Nc, D) > 0
    assert lib.dae_topk_similarity_win_workspace(0, Nc, D, 10) == 0 and lib.dae_rank_similarity_win_workspace(Nq, 0, D) == 0


def test_candidate_windows_on_hand_made_times():
    from dae_rnn_news_recommendation_amd.helpers import candidate_windows
    pub = np.array([1.0, 2.0, 2.0, 5.0, 9.0])
    t = np.array([0.5, 1.0, 2.0, 4.9, 5.0, 9.0, 100.0])
    lo, hi = candidate_windows(t, pub)
    assert lo.dtype == np.int32 and hi.dtype == np.int32
    assert lo.tolist() == [0] * 7 and hi.tolist() == [0, 1, 3, 3, 4, 5, 5]           # publish <= t; before the first: empty
    lo, hi = candidate_windows(t, pub, max_age=float("inf"))
    assert lo.tolist() == [0] * 7 and hi.tolist() == [0, 1, 3, 3, 4, 5, 5]
    lo, hi = candidate_windows(t, pub, max_age=3.0)                                  # t - 3 < publish <= t: ties at both ends
    assert hi.tolist() == [0, 1, 3, 3, 4, 5, 5]
    assert lo.tolist() == [0, 0, 0, 1, 3, 4, 5]                                      # t = 5: publish 2 is exactly 3 old -> outside
    lo, hi = candidate_windows(t, pub, max_age=0)                                    # t < publish <= t: nothing
    assert np.array_equal(lo, hi)
    assert (candidate_windows([], pub)[0].shape, candidate_windows([3.0], [])[1].tolist()) == ((0,), [0])


def test_candidate_windows_errors():
    from dae_rnn_news_recommendation_amd.helpers import candidate_windows
    with pytest.raises(ValueError, match=r"np\.argsort\(publish_times, kind='stable'\)"):
        candidate_windows([1.0], [1.0, 3.0, 2.0])
    with pytest.raises(ValueError, match="finite"):
        candidate_windows([np.nan], [1.0, 2.0])
    with pytest.raises(ValueError, match="finite"):
        candidate_windows([1.0], [1.0, np.inf])
    with pytest.raises(ValueError, match="max_age"):
        candidate_windows([1.0], [1.0, 2.0], max_age=-1.0)


@pytest.mark.parametrize("window, msg", [
    ((np.zeros(9, int), np.full(9, 5)), "entries for 10 queries"),
    ((np.zeros(10, int), np.full(11, 5)), "entries for 10 queries"),
    ((np.full(10, 4), np.full(10, 3)), "lo must not exceed hi"),
    ((np.zeros(10, int), np.full(10, 21)), "hi must not exceed the 20 candidates"),
    ((np.full(10, -1), np.full(10, 5)), "lo must not be negative"),
    ((np.zeros(10), np.full(10, 5.0)), "integer"),
    ((np.zeros(10, int),), "pair"),
])
def test_window_validation_raises_before_the_library_is_touched(window, msg, monkeypatch):
    from dae_rnn_news_recommendation_amd import _lib, helpers

    def no_load(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    Q, C = np.zeros((10, 4), np.float32), np.zeros((20, 4), np.float32)
    for call in (lambda: helpers.most_similar(Q, k=3, candidates=C, window=window),
                 lambda: helpers.recommend(Q, C, k=3, window=window),
                 lambda: helpers.target_ranks(Q, np.zeros(10, int), candidates=C, window=window),
                 lambda: helpers.recommend_ranks(Q, C, np.zeros(10, int), window=window),
                 lambda: helpers.popularity_recommend([[0]] * 10, 20, 3, window=window),
                 lambda: helpers.popularity_ranks([[0]] * 10, 20, np.zeros(10, int), window=window)):
        with pytest.raises(ValueError, match=msg):
            call()
    with pytest.raises(ValueError, match="hi must not exceed the 10 candidates"):      # the corpus is in_df itself
        helpers.most_similar(Q, k=3, window=(np.zeros(10, int), np.full(10, 11)))


def test_windowed_popularity_baselines():
    from dae_rnn_news_recommendation_amd.helpers import popularity_ranks, popularity_recommend
    hist = [[0, 0, 1], [0, 2, 2], [3], []]                               # clicks: article 0: 3, 2: 2, 1: 1, 3: 1, 4: 0
    tgt = np.array([4, 1, 3, 2])
    win = (np.array([1, 0, 0, 3]), np.array([5, 2, 5, 5]))              # orders: [2, 3, 4], [1], [0, 2, 1, 4] (3 seen), [3, 4]
    assert popularity_recommend(hist, 5, 3, window=win).tolist() == [[2, 3, 4], [1, -1, -1], [0, 2, 1], [3, 4, -1]]
    rank, ncand = popularity_ranks(hist, 5, tgt, window=win)
    assert rank.tolist() == [3, 1, 0, 0] and ncand.tolist() == [3, 1, 5, 2]           # seen target; target outside its window
    rng = np.random.default_rng(1)
    hist = [rng.integers(0, 40, rng.integers(0, 12)) for _ in range(60)]
    tgt = rng.integers(-1, 40, 60)
    lo = rng.integers(0, 41, 60)
    hi = np.minimum(lo + rng.integers(0, 30, 60), 40)
    rank, ncand = popularity_ranks(hist, 40, tgt, window=(lo, hi))
    lists = popularity_recommend(hist, 40, 40, window=(lo, hi))
    for u in range(60):
        got = lists[u][lists[u] >= 0]
        assert ((got >= lo[u]) & (got < hi[u])).all() and not np.isin(got, hist[u]).any(), u
        pos = np.nonzero(lists[u] == tgt[u])[0] if tgt[u] >= 0 else []
        assert rank[u] == (pos[0] + 1 if len(pos) else 0), u
        seen_t = tgt[u] >= 0 and tgt[u] in hist[u] and lo[u] <= tgt[u] < hi[u]
        assert ncand[u] == got.size + int(seen_t), u
    # the whole corpus as the window is no window
    full = (np.zeros(60, int), np.full(60, 40))
    assert np.array_equal(popularity_recommend(hist, 40, 7, window=full), popularity_recommend(hist, 40, 7))
    a, b = popularity_ranks(hist, 40, tgt, window=full), popularity_ranks(hist, 40, tgt)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_synthetic_timed_sessions():
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions, synthetic_timed_sessions
    labels = np.random.default_rng(0).integers(0, 7, 500)
    indptr, items, t, pub = synthetic_timed_sessions(300, labels, mean_len=9, seed=3, span_hours=100.0, mean_delay_hours=2.0)
    assert indptr.dtype == np.int64 and indptr.shape == (301,) and indptr[0] == 0 and indptr[-1] == items.size == t.size
    assert pub.shape == (500,) and (np.diff(pub) >= 0).all() and pub.min() >= 0 and pub.max() <= 100.0      # articles in time order
    assert items.min() >= 0 and items.max() < 500
    first = np.zeros(t.size, dtype=bool)
    first[indptr[:-1][np.diff(indptr) > 0]] = True
    assert (np.diff(t)[~first[1:]] >= 0).all()                                       # within a user, time does not run backwards
    assert (t >= pub[items]).all()                                                   # no click before publication
    assert np.median(t - pub[items]) < 3 * 2.0                                       # most clicks soon after it
    again = synthetic_timed_sessions(300, labels, mean_len=9, seed=3, span_hours=100.0, mean_delay_hours=2.0)
    for x, y in zip((indptr, items, t, pub), again):
        assert np.array_equal(x, y)
    other = synthetic_timed_sessions(300, labels, mean_len=9, seed=4, span_hours=100.0, mean_delay_hours=2.0)
    assert not np.array_equal(other[3], pub)
    # the same sessions as synthetic_sessions, each user's clicks put in publication order
    p0, i0 = synthetic_sessions(300, labels, mean_len=9, seed=3)
    assert np.array_equal(p0, indptr)
    assert all(np.array_equal(np.sort(i0[a:b]), items[a:b]) for a, b in zip(indptr[:-1], indptr[1:]))


def test_cli_max_age_needs_synthetic_sessions_and_recommend():
    import main_autoencoder as cli
    with pytest.raises(AssertionError, match="--max_age needs --sessions synthetic --recommend"):
        cli.main(["--model_name", "x", "--max_age", "24"])
    with pytest.raises(AssertionError, match="--max_age needs --sessions synthetic --recommend"):
        cli.main(["--model_name", "x", "--max_age", "24", "--sessions", "synthetic"])
