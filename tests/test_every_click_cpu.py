"""CPU checks of the shared stamped exclusion lists (dae_topk_similarity_seq, dae_rank_similarity_seq) and of the host code of the
every-click protocol: both builds export the symbols under an unchanged ABI version, a partly-NULL set of list pointers is
reported before any HIP call (so on a machine without a GPU), and click_prefix_lists, every_click_rows, the n_candidates / barred
bookkeeping, rank_metrics_by_position and popularity_ranks_every_click against brute-force loops."""
import ctypes

import numpy as np
import pytest

P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first
NAMES = ("dae_topk_similarity_seq", "dae_topk_similarity_seq_workspace", "dae_rank_similarity_seq", "dae_rank_similarity_seq_workspace")
LIST_ARGS = ("lp", "li", "ls", "rl", "rm")


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_seq_symbols_are_exported_and_the_abi_version_stays(fmt):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load(fmt)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.dae_abi_version() == _lib.ABI_VERSION == 9


def _topk(lib, Q=P, Nq=100, C=None, ldc=0, Nc=100, D=50, k=10, exclude_self=1, lp=P, li=P, ls=P, n_lists=7, rl=P, rm=P, lo=P, hi=P, idx=P,
          score=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_topk_similarity_seq_workspace(Nq, Nc, D, k)
    return lib.dae_topk_similarity_seq(Q, D, Nq, C, ldc, Nc, D, 0, 0, k, exclude_self, lp, li, ls, n_lists, rl, rm, lo, hi, idx, score, k, ws,
                                       ws_bytes, None)


def _rank(lib, Q=P, Nq=100, C=None, ldc=0, Nc=100, D=50, exclude_self=1, lp=P, li=P, ls=P, n_lists=7, rl=P, rm=P, lo=P, hi=P, targets=P,
          rank=P, score=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_rank_similarity_seq_workspace(Nq, Nc, D)
    return lib.dae_rank_similarity_seq(Q, D, Nq, C, ldc, Nc, D, 0, 0, exclude_self, lp, li, ls, n_lists, rl, rm, lo, hi, targets, rank, score,
                                       ws, ws_bytes, None)


PARTLY_NULL = [dict.fromkeys(s) for s in (("lp",), ("li",), ("ls",), ("rl",), ("rm",), ("lp", "li"), ("rl", "rm"), ("lp", "li", "ls"),
                                           ("li", "ls", "rl", "rm"), ("lp", "li", "ls", "rl"))]


@pytest.mark.parametrize("call, prefix", [(_topk, b"topk_similarity"), (_rank, b"rank_similarity")])
@pytest.mark.parametrize("kw", PARTLY_NULL, ids=lambda kw: "null_" + "_".join(kw))
def test_partly_null_list_pointers_are_an_argument_error_without_a_gpu(call, prefix, kw):
    lib = _lib()
    assert call(lib, **kw) != 0
    err = lib.dae_last_error()
    assert err.startswith(prefix + b":") and b"go together" in err, err
    for name in (b"list_indptr", b"list_items", b"list_stamps", b"row_list", b"row_limit"):
        assert name in err, err
    assert b"(%d of the 5 are NULL)" % len(kw) in err


@pytest.mark.parametrize("call, prefix", [(_topk, b"topk_similarity"), (_rank, b"rank_similarity")])
@pytest.mark.parametrize("kw, msg", [
    (dict(n_lists=-1), b"n_lists must not be negative"),
    (dict(lo=None), b"win_lo and win_hi go together"),
    (dict(dict.fromkeys(LIST_ARGS), hi=None), b"win_lo and win_hi go together"),      # no lists at all: the _win call's checks
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
    (dict(Q=None), b"bad input"),
    (dict(dict.fromkeys(LIST_ARGS), Q=None), b"bad input"),
    (dict(C=P, ldc=50, exclude_self=1), b"exclude_self needs C == NULL"),
])
def test_seq_keeps_the_argument_errors_of_the_windowed_calls(call, prefix, kw, msg):
    lib = _lib()
    assert call(lib, **kw) != 0
    err = lib.dae_last_error()
    assert err.startswith(prefix + b":") and msg in err, err


def test_seq_topk_k_out_of_range_without_a_gpu():
    lib = _lib()
    assert _topk(lib, k=129) != 0
    assert b"topk_similarity: k must be in 1..128 (got 129)" in lib.dae_last_error()


@pytest.mark.parametrize("shape", [(1, 1, 1), (244, 300, 24), (100000, 64000, 500), (129, 4097, 513)])
def test_seq_workspaces_equal_the_windowed_ones(shape):
    lib = _lib()
    Nq, Nc, D = shape
    for k in (1, 10, 128):
        assert lib.dae_topk_similarity_seq_workspace(Nq, Nc, D, k) == lib.dae_topk_similarity_win_workspace(Nq, Nc, D, k) > 0
    assert lib.dae_rank_similarity_seq_workspace(Nq, Nc, D) == lib.dae_rank_similarity_win_workspace(Nq, Nc, D) > 0
    assert lib.dae_topk_similarity_seq_workspace(0, Nc, D, 10) == 0 and lib.dae_rank_similarity_seq_workspace(Nq, 0, D) == 0


def _histories(seed=3, users=40, n_articles=60, max_len=25):
    """Histories with repeated clicks (a small pool of articles per user) and users of length 0, 1 and 2."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, users)
    lens[:3] = [0, 1, 2]
    return [rng.choice(rng.choice(n_articles, 12, replace=False), n) for n in lens], n_articles


def test_click_prefix_lists_against_a_loop():
    from dae_rnn_news_recommendation_amd.helpers import click_prefix_lists
    hist, _ = _histories()
    indptr, items, stamps = click_prefix_lists(hist)
    assert indptr.dtype == np.int64 and items.dtype == np.int32 and stamps.dtype == np.int32 and indptr.shape == (len(hist) + 1,)
    repeats = 0
    for u, h in enumerate(hist):
        first = {}
        for pos, a in enumerate(h.tolist()):
            first.setdefault(a, pos)
        repeats += len(h) - len(first)
        want = sorted(first.items())
        assert items[indptr[u]:indptr[u + 1]].tolist() == [a for a, _ in want], u
        assert stamps[indptr[u]:indptr[u + 1]].tolist() == [p for _, p in want], u
    assert repeats > 50                                                              # stamp = FIRST occurrence is exercised
    assert indptr[-1] == items.size == stamps.size <= sum(len(h) for h in hist)     # never larger than the click log
    csr = (np.concatenate([[0], np.cumsum([len(h) for h in hist])]), np.concatenate(hist))
    for x, y in zip(click_prefix_lists(csr), (indptr, items, stamps)):
        assert np.array_equal(x, y)
    e = click_prefix_lists([[], []])
    assert e[0].tolist() == [0, 0, 0] and e[1].size == 0 and e[2].size == 0
    with pytest.raises(ValueError, match="negative"):
        click_prefix_lists([[1, -1]])
    with pytest.raises(ValueError, match="integer"):
        click_prefix_lists([[1.5]])


def test_every_click_rows_against_a_loop():
    from dae_rnn_news_recommendation_amd.helpers import every_click_rows
    hist, _ = _histories(seed=4)
    t = [np.sort(np.random.default_rng(u).random(len(h)) * 100) for u, h in enumerate(hist)]
    rows = every_click_rows(hist, timestamps=np.concatenate(t))
    want = dict(targets=[], row_list=[], row_limit=[], positions=[], query_times=[])
    for u, h in enumerate(hist):
        for e in range(len(h)):
            lastone = e == len(h) - 1
            want["targets"].append(-1 if lastone else int(h[e + 1]))
            want["row_list"].append(u)
            want["row_limit"].append(e)
            want["positions"].append(e + 1)
            want["query_times"].append(t[u][e] if lastone else t[u][e + 1])
    assert sorted(rows) == sorted(want)
    for name, v in want.items():
        assert np.array_equal(rows[name], np.asarray(v)), name
    assert rows["targets"].dtype == np.int64 and rows["row_list"].dtype == np.int32 and rows["row_limit"].dtype == np.int32
    assert "query_times" not in every_click_rows(hist)
    assert all(v.size == 0 for v in every_click_rows([[], []], timestamps=[]).values())
    with pytest.raises(ValueError, match="timestamps"):
        every_click_rows([[1, 2]], timestamps=[0.0])


def _generic_rows(rng, n_rows, n_lists, max_stamp):
    row_list = rng.integers(0, n_lists, n_rows)
    row_list[rng.random(n_rows) < 0.1] = -1
    row_list[rng.random(n_rows) < 0.05] = n_lists + 3                               # outside on the other side: no list either
    row_limit = rng.integers(-1, max_stamp + 2, n_rows)
    row_limit[0] = np.iinfo(np.int32).max
    return row_list, row_limit


@pytest.mark.parametrize("windows", [False, True])
@pytest.mark.parametrize("exclude_self", [False, True])
def test_shared_bookkeeping_against_loops_and_against_the_per_row_lists(windows, exclude_self):
    from dae_rnn_news_recommendation_amd import helpers
    hist, Nc = _histories(seed=5)
    rng = np.random.default_rng(6)
    lp, li, ls = helpers.click_prefix_lists(hist)
    Nq = Nc if exclude_self else 150
    row_list, row_limit = _generic_rows(rng, Nq, len(hist), 25)
    tgt = rng.integers(-1, Nc, Nq)
    for i in range(0, Nq, 4):                                                      # plenty of targets from the row's own list
        if 0 <= row_list[i] < len(hist) and lp[row_list[i] + 1] > lp[row_list[i]]:
            tgt[i] = li[rng.integers(lp[row_list[i]], lp[row_list[i] + 1])]
    if exclude_self:
        tgt[5:9] = np.arange(5, 9)
    window = None
    if windows:
        lo = rng.integers(0, Nc, Nq)
        near = (rng.random(Nq) < 0.7) & (tgt >= 0)                                  # most targets inside their window
        lo[near] = np.maximum(tgt[near] - rng.integers(0, 20, Nq)[near], 0)
        window = (lo, np.minimum(lo + np.where(near, 20, 0) + rng.integers(0, 40, Nq), Nc))
    shared = helpers.normalize_shared_exclusions(((lp, li), ls, row_list, row_limit), Nq, Nc)
    n_cand, barred = helpers._competitors(tgt, Nq, Nc, exclude_self, None, None, window, shared)
    lists = []
    for i in range(Nq):                                                            # the brute force
        u = row_list[i]
        mine = [int(a) for a, s in zip(li[lp[u]:lp[u + 1]], ls[lp[u]:lp[u + 1]]) if s <= row_limit[i]] if 0 <= u < len(hist) else []
        lists.append(mine)
        lo_i, hi_i = (0, Nc) if window is None else (int(window[0][i]), int(window[1][i]))
        ok = np.zeros(Nc, dtype=bool)
        ok[lo_i:hi_i] = True
        ok[mine] = False
        if exclude_self:
            ok[i] = False
        t = int(tgt[i])
        cannot = t >= 0 and not ok[t]
        if t >= 0 and lo_i <= t < hi_i:
            ok[t] = True                                                           # the target competes even where it is barred
        assert n_cand[i] == ok.sum(), i
        assert barred[i] == cannot, i
    assert barred.sum() >= 10 and (~barred & (tgt >= 0)).sum() >= 10
    xp, xi = helpers.normalize_exclusions(lists, Nq, Nc)
    a, b = helpers._competitors(tgt, Nq, Nc, exclude_self, xp, xi, window)
    assert np.array_equal(a, n_cand) and np.array_equal(b, barred)


def test_shared_exclusions_are_validated_before_the_library_is_touched(monkeypatch):
    from dae_rnn_news_recommendation_amd import _lib, helpers

    def no_load(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    Q, C = np.zeros((4, 3), np.float32), np.zeros((9, 3), np.float32)
    ok = ([[1, 5], [0]], [0, 1, 0], [0, 1, 0, -1], [0, 0, 1, 2])
    bad = [(([[5, 1], [0]],) + ok[1:], "ascending and unique"), (([[1, 1], [0]],) + ok[1:], "ascending and unique"),
           (([[1, 9], [0]],) + ok[1:], "items must be in 0..8"), ((ok[0], [0, 1]) + ok[2:], "2 stamps for 3 list items"),
           (ok[:2] + ([0, 1, 0], ok[3]), "row_list has 3 entries for 4 queries"), (ok[:3] + ([0.5, 0, 1, 2],), "row_limit must hold integers"),
           (ok[:3], "lists, stamps, row_list, row_limit")]
    for shared, msg in bad:
        for call in (lambda: helpers.most_similar(Q, k=2, candidates=C, exclude_shared=shared),
                     lambda: helpers.target_ranks(Q, np.zeros(4, int), candidates=C, exclude_shared=shared)):
            with pytest.raises(ValueError, match=msg):
                call()
    for call in (lambda: helpers.most_similar(Q, k=2, candidates=C, exclude_shared=ok, exclude=[[0]] * 4),
                 lambda: helpers.target_ranks(Q, np.zeros(4, int), candidates=C, exclude_shared=ok, exclude=[[0]] * 4)):
        with pytest.raises(ValueError, match="exclude and exclude_shared do not go together"):
            call()
    lp, li, ls, rl, rm = helpers.normalize_shared_exclusions(ok, 4, 9)                # [1, 5] | [0]: a step down between two lists is fine
    assert (lp.tolist(), li.tolist(), ls.tolist(), rl.tolist(), rm.tolist()) == ([0, 2, 3], [1, 5, 0], [0, 1, 0], [0, 1, 0, -1], [0, 0, 1, 2])
    with pytest.raises(ValueError, match="state rows for 3 events"):
        helpers.recommend_ranks_every_click(Q, C, [[1, 2, 3]])
    with pytest.raises(ValueError, match="keep_best needs validation"):
        helpers.fit_gru_user_model([[1, 2]], C, keep_best=True)
    with pytest.raises(ValueError, match="validation_every"):
        helpers.fit_gru_user_model([[1, 2]], C, validation=[[1, 2]], validation_every=0)


def test_rank_metrics_by_position_partitions_the_rows_and_pools_to_rank_metrics():
    from dae_rnn_news_recommendation_amd.helpers import rank_metrics, rank_metrics_by_position
    rng = np.random.default_rng(8)
    n = 3000
    pos = rng.integers(1, 80, n)
    tgt = rng.integers(-1, 50, n)
    ncand = rng.integers(1, 400, n)
    rank = np.where(rng.random(n) < 0.15, 0, rng.integers(1, 400, n) % ncand + 1)
    ks = (1, 10, 100)
    by = rank_metrics_by_position(rank, ncand, tgt, pos, ks=ks)
    bounds = [(1, 2), (2, 3), (3, 5), (5, 10), (10, 20), (20, 50), (50, None)]
    assert [(b["lo"], b["hi"]) for b in by] == bounds
    member = np.zeros(n, dtype=int)
    for b in by:
        m = (pos >= b["lo"]) & (pos < (b["hi"] if b["hi"] is not None else 1 << 40))
        member += m
        want = rank_metrics(rank[m], ncand[m], tgt[m], ks=ks)
        assert {k: v for k, v in b.items() if k not in ("lo", "hi")} == want
    assert (member == 1).all()                                                     # a partition
    whole = rank_metrics(rank, ncand, tgt, ks=ks)
    assert sum(b["n"] for b in by) == whole["n"] and sum(b["n_ranked"] for b in by) == whole["n_ranked"]
    for key in ("mrr", "ndcg", "hit@1", "hit@10", "mrr@10", "ndcg@100"):           # means over n pool by n
        assert sum(b[key] * b["n"] for b in by) / whole["n"] == pytest.approx(whole[key], rel=1e-12)
    assert sum(b["mean_rank"] * b["n_ranked"] for b in by) / whole["n_ranked"] == pytest.approx(whole["mean_rank"], rel=1e-12)
    # rows below the first edge get a bucket of their own; an empty bucket is all NaN with n = 0
    by = rank_metrics_by_position(rank, ncand, tgt, pos, edges=(5, 1000), ks=ks)
    assert [(b["lo"], b["hi"]) for b in by] == [(None, 5), (5, 1000), (1000, None)] and by[2]["n"] == 0 and np.isnan(by[2]["mrr"])
    assert by[0]["n"] + by[1]["n"] == whole["n"]
    with pytest.raises(ValueError, match="increasing"):
        rank_metrics_by_position(rank, ncand, tgt, pos, edges=(3, 3))
    with pytest.raises(ValueError, match="positions"):
        rank_metrics_by_position(rank, ncand, tgt, pos[:-1])


@pytest.mark.parametrize("windows", [False, True])
def test_popularity_ranks_every_click_against_a_loop(windows):
    from dae_rnn_news_recommendation_amd import helpers
    hist, Na = _histories(seed=9)
    rng = np.random.default_rng(10)
    nnz = sum(len(h) for h in hist)
    window = None
    if windows:
        lo = rng.integers(0, Na, nnz)
        nxt = helpers.every_click_rows(hist)["targets"]
        near = (rng.random(nnz) < 0.7) & (nxt >= 0)                                 # most targets inside their window
        lo[near] = np.maximum(nxt[near] - rng.integers(0, 20, nnz)[near], 0)
        window = (lo, np.minimum(lo + np.where(near, 20, 0) + rng.integers(0, 30, nnz), Na))
    rank, ncand, tgt = helpers.popularity_ranks_every_click(hist, Na, window=window)
    assert rank.shape == ncand.shape == tgt.shape == (nnz,) and np.array_equal(tgt, helpers.every_click_rows(hist)["targets"])
    count = np.bincount(np.concatenate(hist), minlength=Na)
    order = sorted(range(Na), key=lambda a: (-count[a], a))                        # popularity_ranks' order
    e = n_seen_targets = 0
    for h in hist:
        for p in range(len(h)):
            lo_e, hi_e = (0, Na) if window is None else (int(window[0][e]), int(window[1][e]))
            seen = set(h[:p + 1].tolist())
            cands = [a for a in order if lo_e <= a < hi_e and a not in seen]
            t = int(tgt[e])
            assert rank[e] == (cands.index(t) + 1 if t in cands else 0), e
            seen_t = t >= 0 and t in seen and lo_e <= t < hi_e
            n_seen_targets += seen_t
            assert ncand[e] == len(cands) + int(seen_t), e
            e += 1
    assert n_seen_targets >= 20 and (rank > 0).sum() >= 100
    # the row of a user's second-to-last event is the last-click protocol's row
    users = [u for u, h in enumerate(hist) if len(h) >= 2]
    ends = np.cumsum([len(h) for h in hist])
    cut = [h[:-1] for h in hist]
    if not windows:
        # popularity_ranks counts the clicks of the histories it is given: hand it the same counts through `seen`
        r0, c0 = helpers.popularity_ranks(hist, Na, [h[-1] if len(h) >= 2 else -1 for h in hist], seen=cut)
        assert np.array_equal(rank[ends[users] - 2], r0[users]) and np.array_equal(ncand[ends[users] - 2], c0[users])


def test_cli_flags_need_their_companions():
    import main_autoencoder as cli
    with pytest.raises(AssertionError, match="--every_click needs --recommend K"):
        cli.main(["--model_name", "x", "--every_click"])
    with pytest.raises(AssertionError, match="--gru_validation needs --fit_gru"):
        cli.main(["--model_name", "x", "--gru_validation", "0.2"])
