"""Candidate windows on the GPU (dae_topk_similarity_win, dae_rank_similarity_win; helpers.most_similar / target_ranks /
recommend(window=...)).  The reference of every case is fp64 NumPy or the existing unwindowed path on the sliced corpus
C[lo:hi] -- whose results depend only on the operand rows and the K order, not on a row's position -- never the windowed path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NQ, NC, D = 300, 700, 70          # three query tiles, six corpus tiles (the last one ragged): six slices per query tile
# inside one tile; on tile edges; one column; three tiles; hi = Nc; empty (twice); five columns; everything; the ragged tile;
# across one edge; the first tile
WINDOWS = [(10, 100), (128, 256), (300, 301), (200, 500), (450, 700), (350, 350), (0, 0), (695, 700), (0, 700), (640, 700), (255, 257),
           (0, 128)]


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(21)
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    C = rng.standard_normal((NC, D)).astype(np.float32)
    C[400:430] = C[100:130]                                                        # duplicates: score ties across tiles
    which = rng.integers(0, len(WINDOWS), NQ)
    which[:len(WINDOWS)] = np.arange(len(WINDOWS))                                 # every window is used
    which = rng.permutation(which)
    lo = np.array([WINDOWS[w][0] for w in which])
    hi = np.array([WINDOWS[w][1] for w in which])
    seen = [rng.choice(NC, rng.integers(0, 40), replace=False) for _ in range(NQ)]
    tgt = rng.integers(0, NC, NQ)
    inside = rng.random(NQ) < 0.6                                                  # most targets inside their window
    tgt = np.where(inside & (hi > lo), lo + (tgt % np.maximum(hi - lo, 1)), tgt)
    tgt[rng.random(NQ) < 0.1] = -1
    for i in range(0, NQ, 7):                                                      # some targets are seen
        if tgt[i] >= 0:
            seen[i] = np.append(seen[i], tgt[i])
    return dict(Q=Q, C=C, which=which, lo=lo, hi=hi, seen=seen, tgt=tgt)


def _masked(S, lo, hi, exclude=None, exclude_self=False):
    """S with -inf wherever row i may not return column j."""
    R = S.astype(np.float64).copy()
    cols = np.arange(S.shape[1])[None, :]
    R[(cols < lo[:, None]) | (cols >= hi[:, None])] = -np.inf
    if exclude is not None:
        for i, x in enumerate(exclude):
            R[i, np.asarray(x, dtype=np.int64)] = -np.inf
    if exclude_self:
        np.fill_diagonal(R, -np.inf)
    return R


def _check_masked(idx, sc, R, k, tol_rel=1e-5):
    """The checks of test_hip_topk._check against a score matrix whose inadmissible entries are -inf."""
    Nq = R.shape[0]
    assert idx.shape == (Nq, k) and sc.shape == (Nq, k) and idx.dtype == np.int64 and sc.dtype == np.float32
    tol = tol_rel * np.abs(R[np.isfinite(R)]).max()
    for i in range(Nq):
        row = R[i]
        kk = min(k, int(np.isfinite(row).sum()))
        assert (idx[i, kk:] == -1).all() and np.isneginf(sc[i, kk:]).all(), i
        if kk == 0:
            continue
        got, gs = idx[i, :kk], sc[i, :kk]
        assert (got >= 0).all() and (got < R.shape[1]).all() and len(set(got.tolist())) == kk, i
        assert np.isfinite(row[got]).all(), i                                      # only admissible candidates
        assert np.abs(gs - row[got]).max() <= tol, i                               # score check
        sk = np.sort(row)[::-1][kk - 1]
        assert (row[got] >= sk - tol).all(), i                                     # near-tie rule
        assert np.isin(np.nonzero(row > sk + tol)[0], got).all(), i
        d = np.diff(gs)                                                            # order
        assert (d <= 0).all() and (np.diff(got)[d == 0] > 0).all(), i


def _equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_u32(a[1]), _u32(b[1]))


def test_full_window_is_the_old_call(data):
    from dae_rnn_news_recommendation_amd import helpers
    Q, C, seen, tgt = data["Q"], data["C"], data["seen"], data["tgt"]
    full = (np.zeros(NQ, dtype=np.int64), np.full(NQ, NC))
    for kw in (dict(candidates=C), dict(candidates=C, exclude=seen), dict(metric="linear kernel", candidates=C, exclude=seen)):
        for k in (1, 10, 128):
            assert _equal(helpers.most_similar(Q, k=k, window=full, **kw), helpers.most_similar(Q, k=k, **kw)), (kw.keys(), k)
        a, b = helpers.target_ranks(Q, tgt, window=full, **kw), helpers.target_ranks(Q, tgt, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(_u32(a[1]), _u32(b[1])) and np.array_equal(a[2], b[2]), kw.keys()
    X = np.vstack([Q, C[:NC - NQ]])                                                # the corpus is in_df itself: exclude_self
    full = (np.zeros(NC, dtype=np.int64), np.full(NC, NC))
    xs = [np.asarray(s) for s in seen] + [np.zeros(0, dtype=np.int64)] * (NC - NQ)
    t = np.concatenate([tgt, np.full(NC - NQ, 3)])
    for kw in (dict(), dict(exclude=xs), dict(exclude_self=False), dict(exclude_self=False, exclude=xs)):
        assert _equal(helpers.most_similar(X, k=10, window=full, **kw), helpers.most_similar(X, k=10, **kw)), kw
        a, b = helpers.target_ranks(X, t, window=full, **kw), helpers.target_ranks(X, t, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(_u32(a[1]), _u32(b[1])) and np.array_equal(a[2], b[2]), kw


def _sliced_topk(helpers, Q, C, lo, hi, k, **kw):
    """Row by row what the windows admit, from the unwindowed path on the sliced corpus."""
    idx = np.full((Q.shape[0], k), -1, dtype=np.int64)
    sc = np.full((Q.shape[0], k), -np.inf, dtype=np.float32)
    for a, b in sorted(set(zip(lo.tolist(), hi.tolist()))):
        rows = np.nonzero((lo == a) & (hi == b))[0]
        if a >= b:
            continue
        ri, rs = helpers.most_similar(Q[rows], k=k, candidates=C[a:b], **kw)
        idx[rows], sc[rows] = np.where(ri >= 0, ri + a, -1), rs
    return idx, sc


@pytest.mark.parametrize("k", [1, 10, 128])
def test_windows_equal_the_sliced_corpus(data, k):
    from dae_rnn_news_recommendation_amd import helpers
    Q, C, lo, hi = data["Q"], data["C"], data["lo"], data["hi"]
    want = _sliced_topk(helpers, Q, C, lo, hi, k)
    got = helpers.most_similar(Q, k=k, candidates=C, window=(lo, hi))
    assert _equal(got, want)
    empty = lo >= hi
    assert empty.sum() >= 2 and (got[0][empty] == -1).all() and np.isneginf(got[1][empty]).all()
    if k == 128:                                                                   # the five-column window: a -1 / -inf tail
        five = (lo == 695)
        assert (got[0][five][:, :5] >= 695).all() and (got[0][five][:, 5:] == -1).all() and np.isneginf(got[1][five][:, 5:]).all()
    t = helpers.most_similar(torch.from_numpy(Q).cuda(), k=k, candidates=torch.from_numpy(C).cuda(),
                             window=(torch.from_numpy(lo), torch.from_numpy(hi)), return_tensor=True)
    assert t[0].is_cuda and t[0].dtype == torch.int64 and _equal((t[0].cpu().numpy(), t[1].cpu().numpy()), want)


def test_exact_ties_match_stable_argsort_inside_windows():
    """The integer-valued construction of test_hip_topk.test_exact_ties_match_stable_argsort: every score is exact in fp32, so
    indices and scores equal NumPy's stable argsort of the fp64 matrix with -inf outside each row's window, bit for bit."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(5)
    base = rng.integers(-2, 3, (40, 24)).astype(np.float32)
    X = base[rng.integers(0, 40, 700)]                                             # ~17 copies of every row
    S = X.astype(np.float64) @ X.T.astype(np.float64)
    lo = rng.integers(0, 700, 700)
    hi = np.minimum(lo + rng.integers(0, 400, 700), 700)
    for k, kw in ((1, dict()), (37, dict()), (128, dict()), (50, dict(exclude_self=False)), (128, dict(candidates=X))):
        idx, sc = helpers.most_similar(X, k=k, metric="linear kernel", window=(lo, hi), **kw)
        R = _masked(S, lo, hi, exclude_self=not kw)
        want = np.argsort(-R, axis=1, kind="stable")[:, :k]
        ws = np.take_along_axis(R, want, 1)
        assert np.array_equal(idx, np.where(np.isneginf(ws), -1, want)), (k, kw.keys())
        assert np.array_equal(sc, ws.astype(np.float32)), (k, kw.keys())              # exact values (-0 == +0, as in the key)


@pytest.fixture(scope="module")
def selfdata():
    """The corpus is in_df itself (700 rows): windows, lists with items inside and outside them, exclude_self."""
    rng = np.random.default_rng(33)
    X = rng.standard_normal((NC, D)).astype(np.float32)
    lo = rng.integers(0, NC, NC)
    hi = np.minimum(lo + rng.integers(0, 300, NC), NC)
    lo[:5], hi[:5] = [0, 128, 699, 640, 0], [700, 256, 700, 700, 0]
    seen = [rng.choice(NC, rng.integers(0, 60), replace=False) for _ in range(NC)]
    seen[7] = np.arange(lo[7], hi[7])                                              # the whole window is seen
    tgt = np.where(rng.random(NC) < 0.7, lo + rng.integers(0, 300, NC) % np.maximum(hi - lo, 1), rng.integers(0, NC, NC))
    tgt[rng.random(NC) < 0.1] = -1
    tgt[20:30] = np.arange(20, 30)                                                 # the row itself
    for i in range(0, NC, 9):
        if tgt[i] >= 0:
            seen[i] = np.append(seen[i], tgt[i])
    import oracle as O
    return dict(X=X, lo=lo, hi=hi, seen=seen, tgt=tgt,
                S={m: O.pairwise_similarity(X, norm="", metric=m, set_diagonal_zero=False) for m in ("cosine", "linear kernel")})


@pytest.mark.parametrize("metric", ["cosine", "linear kernel"])
def test_windows_with_exclusion_lists_and_exclude_self(selfdata, metric):
    from dae_rnn_news_recommendation_amd import helpers
    X, lo, hi, seen = (selfdata[n] for n in ("X", "lo", "hi", "seen"))
    for k, excl_self, lists in ((10, True, seen), (128, True, seen), (10, False, seen), (10, True, None)):
        idx, sc = helpers.most_similar(X, k=k, metric=metric, exclude_self=excl_self, exclude=lists, window=(lo, hi))
        _check_masked(idx, sc, _masked(selfdata["S"][metric], lo, hi, lists, excl_self), k)


def _tile_windows():
    """700 rows handed to the kernel as they are (the corpus is in_df itself): query tile 0 has every window inside corpus tile 4
    -- five of its six workgroups have nothing to do --, query tile 1 mixes windows in corpus tile 0 with windows in tile 5 -- the
    union is everything and every row masks the rest --, the other tiles draw from WINDOWS."""
    rng = np.random.default_rng(44)
    X = rng.standard_normal((NC, D)).astype(np.float32)
    X[520:540] = X[5:25]
    w4, w05 = [(512, 640), (520, 600), (600, 639)], [(5, 60), (650, 700)]
    win = [w4[i % 3] for i in range(128)] + [w05[i % 2] for i in range(128)] + [WINDOWS[i] for i in rng.integers(0, len(WINDOWS), NC - 256)]
    return X, np.array([w[0] for w in win]), np.array([w[1] for w in win])


def test_empty_slices_and_wide_unions():
    from dae_rnn_news_recommendation_amd import helpers
    X, lo, hi = _tile_windows()
    tgt = np.random.default_rng(45).integers(0, NC, NC)
    for k in (10, 128):
        want = _sliced_topk(helpers, X, X, lo, hi, k)
        a = helpers.most_similar(X, k=k, exclude_self=False, window=(lo, hi))      # the layout above, as it is
        b = helpers.most_similar(X, k=k, exclude_self=False, window=(lo, hi))
        c = helpers.most_similar(X, k=k, candidates=X, window=(lo, hi))            # the rows ordered by their windows
        perm = np.random.default_rng(46).permutation(NC)
        d = helpers.most_similar(X[perm], k=k, candidates=X, window=(lo[perm], hi[perm]))      # shuffled rows
        assert _equal(a, want) and _equal(b, want) and _equal(c, want)
        assert _equal((d[0][np.argsort(perm)], d[1][np.argsort(perm)]), want)
    r = [helpers.target_ranks(X, tgt, exclude_self=False, window=(lo, hi)), helpers.target_ranks(X, tgt, exclude_self=False, window=(lo, hi)),
         helpers.target_ranks(X, tgt, candidates=X, window=(lo, hi))]
    dr = helpers.target_ranks(X[perm], tgt[perm], candidates=X, window=(lo[perm], hi[perm]))
    r.append(tuple(x[np.argsort(perm)] for x in dr))
    for x in r[1:]:
        assert np.array_equal(x[0], r[0][0]) and np.array_equal(_u32(x[1]), _u32(r[0][1])) and np.array_equal(x[2], r[0][2])
    top = helpers.most_similar(X, k=128, exclude_self=False, window=(lo, hi))[0]
    _check_rank_against_topk(r[0][0], r[0][1], top, None, tgt, lo, hi)


def _check_rank_against_topk(rank, score, top, top_sc, tgt, lo, hi):
    """rank = position + 1 wherever the target is in the windowed top-128 row, and nowhere else is 0 < rank <= 128."""
    n_in = 0
    for i in range(len(tgt)):
        pos = np.nonzero(top[i] == tgt[i])[0] if tgt[i] >= 0 else []
        if len(pos):
            n_in += 1
            assert rank[i] == pos[0] + 1, i
            if top_sc is not None:
                assert _u32(score[i:i + 1])[0] == _u32(top_sc[i, pos[0]:pos[0] + 1])[0], i
        else:
            assert rank[i] == 0 or rank[i] > top.shape[1], i
        if tgt[i] >= 0 and not lo[i] <= tgt[i] < hi[i]:
            assert rank[i] == 0, i
        if tgt[i] < 0:
            assert rank[i] == 0 and np.isneginf(score[i]), i
    assert n_in >= 20


def _n_candidates(n_cols, lo, hi, tgt, exclude=None, exclude_self=False):
    out = np.zeros(len(lo), dtype=np.int64)
    for i in range(len(lo)):
        ok = np.zeros(n_cols, dtype=bool)
        ok[lo[i]:hi[i]] = True
        if exclude is not None:
            ok[np.asarray(exclude[i], dtype=np.int64)] = False
        if exclude_self:
            ok[i] = False
        if tgt[i] >= 0 and lo[i] <= tgt[i] < hi[i]:
            ok[tgt[i]] = True                                                      # the target competes even where it is barred
        out[i] = ok.sum()
    return out


@pytest.mark.parametrize("lists", [False, True])
def test_rank_queries_against_a_corpus(data, lists):
    from dae_rnn_news_recommendation_amd import helpers
    Q, C, lo, hi, tgt = (data[n] for n in ("Q", "C", "lo", "hi", "tgt"))
    seen = data["seen"] if lists else None
    rank, score, ncand = helpers.target_ranks(Q, tgt, candidates=C, exclude=seen, window=(lo, hi))
    assert rank.dtype == np.int64 and score.dtype == np.float32 and rank.shape == score.shape == ncand.shape == (NQ,)
    top, top_sc = helpers.most_similar(Q, k=128, candidates=C, exclude=seen, window=(lo, hi))
    _check_rank_against_topk(rank, score, top, top_sc, tgt, lo, hi)
    assert np.array_equal(ncand, _n_candidates(NC, lo, hi, tgt, seen))
    # every row against the unwindowed path on its slice of the corpus (the lists shifted and cut with it)
    n_ranked = 0
    for a, b in sorted(set(zip(lo.tolist(), hi.tolist()))):
        rows = np.nonzero((lo == a) & (hi == b))[0]
        inside = (tgt[rows] >= a) & (tgt[rows] < b)
        assert (rank[rows[~inside]] == 0).all()
        rows = rows[inside]
        if rows.size == 0:
            continue
        sl = None if seen is None else [np.asarray(seen[i])[(np.asarray(seen[i]) >= a) & (np.asarray(seen[i]) < b)] - a for i in rows]
        wr, wsc, wn = helpers.target_ranks(Q[rows], tgt[rows] - a, candidates=C[a:b], exclude=sl)
        assert np.array_equal(rank[rows], wr) and np.array_equal(_u32(score[rows]), _u32(wsc)) and np.array_equal(ncand[rows], wn), (a, b)
        n_ranked += int((wr > 0).sum())
    assert n_ranked >= 100
    if lists:
        barred = np.array([tgt[i] >= 0 and tgt[i] in seen[i] for i in range(NQ)])
        assert barred.sum() >= 10 and (rank[barred] == 0).all()


def test_rank_with_exclusion_lists_and_exclude_self(selfdata):
    from dae_rnn_news_recommendation_amd import helpers
    X, lo, hi, seen, tgt = (selfdata[n] for n in ("X", "lo", "hi", "seen", "tgt"))
    for excl_self, lists in ((True, seen), (False, seen), (True, None)):
        rank, score, ncand = helpers.target_ranks(X, tgt, exclude_self=excl_self, exclude=lists, window=(lo, hi))
        top, top_sc = helpers.most_similar(X, k=128, exclude_self=excl_self, exclude=lists, window=(lo, hi))
        _check_rank_against_topk(rank, score, top, top_sc, tgt, lo, hi)
        assert np.array_equal(ncand, _n_candidates(NC, lo, hi, tgt, lists, excl_self))
        # the count itself, in fp64 NumPy, where no other score is within the tolerance of the target's
        R = _masked(selfdata["S"]["cosine"], lo, hi, lists, excl_self)
        checked = 0
        for i in np.nonzero(rank > 0)[0]:
            s = selfdata["S"]["cosine"][i, tgt[i]]
            row = np.delete(R[i], tgt[i])
            if (np.abs(row[np.isfinite(row)] - s) > 1e-5).all():
                assert rank[i] == 1 + (row > s).sum(), i
                checked += 1
        assert checked >= 100
        if excl_self:
            assert (rank[20:30] == 0).all()                                        # the row itself is never returned
        if lists is not None:
            barred = np.array([tgt[i] >= 0 and tgt[i] in lists[i] for i in range(NC)])
            assert barred.sum() >= 10 and (rank[barred] == 0).all()


def test_no_nq_by_nc_buffer():
    from dae_rnn_news_recommendation_amd import helpers
    Nq, Nc, Dd = 3000, 4000, 64
    g = torch.Generator(device="cuda").manual_seed(1)
    Q = torch.randn((Nq, Dd), device="cuda", generator=g)
    C = torch.randn((Nc, Dd), device="cuda", generator=g)
    rng = np.random.default_rng(2)
    lo = rng.integers(0, Nc - 250, Nq)
    hi = lo + 250
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    idx, sc = helpers.most_similar(Q, k=1, candidates=C, window=(lo, hi), return_tensor=True)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    assert grow < Nq * Nc * 4 // 8, grow
    idx = idx.cpu().numpy()[:, 0]
    assert ((idx >= lo) & (idx < hi)).all() and torch.isfinite(sc).all()


def test_cli_max_age(tmp_path, monkeypatch, capsys):
    import re

    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_timed_sessions
    monkeypatch.chdir(tmp_path)
    model = cli.main(["--model_name", "win", "--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4",
                      "--sessions", "synthetic", "--recommend", "5", "--rank_metrics", "--max_age", "48", "--similarity", "False"])
    out = capsys.readouterr().out
    d = model.data_dir
    import os
    assert not os.path.exists(d + "article_encoded_recommend5.npz") and not os.path.exists(d + "article_encoded_ranks.npz")
    rec, rk = np.load(d + "article_encoded_recommend5_window.npz"), np.load(d + "article_encoded_ranks_window.npz")
    users = 200
    assert rec["indices"].shape == (users, 5) and rk["rank"].shape == (users,) and float(rec["max_age"]) == 48.0 == float(rk["max_age"])
    lo, hi = rec["window_lo"], rec["window_hi"]
    assert np.array_equal(lo, rk["window_lo"]) and np.array_equal(hi, rk["window_hi"]) and np.array_equal(rec["targets"], rk["targets"])
    assert float(rec["mean_window"]) == pytest.approx((hi - lo).mean()) and 0 < float(rec["mean_window"]) < 400
    assert "max age 48 h" in out and ("mean window %.1f of 400" % float(rec["mean_window"])) in out
    labels = helpers.read_file(d + "article_label_category_publish_name.pkl", data_type="pandas_series").to_numpy()
    indptr, items, t, pub = synthetic_timed_sessions(users, np.unique(np.asarray(labels), return_inverse=True)[1], mean_len=12, seed=4)
    last = np.maximum(indptr[1:] - 1, 0)
    wl, wh = helpers.candidate_windows(t[last], pub, 48.0)
    assert np.array_equal(wl, lo) and np.array_equal(wh, hi)
    for u in range(users):                                                          # inside the window, outside the history
        got = rec["indices"][u][rec["indices"][u] >= 0]
        assert ((got >= lo[u]) & (got < hi[u])).all() and not np.isin(got, items[indptr[u]:max(indptr[u + 1] - 1, indptr[u])]).any(), u
    m = helpers.rank_metrics(rk["rank"], rk["n_candidates"], rk["targets"], ks=(1, 5, 10, 100))
    line = re.search(r"ranks decayed user state\s+AUC ([0-9.]+|nan)\s+MRR ([0-9.]+)\s+mean rank ([0-9.]+)\s+median rank ([0-9.]+)\s+"
                     r"hit@1 ([0-9.]+)\s+hit@10 ([0-9.]+)\s+hit@100 ([0-9.]+)", out)
    assert [line.group(i) for i in range(1, 8)] == ["%.4f" % m["auc"], "%.4f" % m["mrr"], "%.1f" % m["mean_rank"], "%.1f" % m["median_rank"],
                                                     "%.4f" % m["hit@1"], "%.4f" % m["hit@10"], "%.4f" % m["hit@100"]]
    topk = re.search(r"hit@5 decayed user state\s+([0-9.]+)", out).group(1)
    assert topk == "%.4f" % m["hit@5"] == "%.4f" % helpers.next_click_metrics(rec["indices"], rec["targets"])["hit"]
    assert out.count("most clicked unseen") == 2
