"""GPU checks of full-rank evaluation (dae_rank_similarity through helpers.target_ranks / recommend_ranks): exact counts on
integer data (every dot product is exact, so NumPy's integer matrix with the key order -- score descending, index ascending --
is the truth), exclusion lists, consistency with most_similar on real data (position and bit-equal score), an fp64 bracket,
determinism and order independence, the end-to-end recommender metrics and the CLI's --rank_metrics.

Shapes: Nq = 130 (two query tiles, the second ragged), Nc = 300 (three corpus tiles, the last ragged, three slices) and
Nc = 100 (one tile, one slice), D = 70 (a ragged K tile)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NQ, NC, NC1, D = 130, 300, 100, 70


def _ref_ranks(S, targets, lists=None, exclude_self=False):
    """1 + the admissible columns before the target in the key order; 0 without a target.  The list never removes the target."""
    Nq, Nc = S.shape
    cols = np.arange(Nc)
    out = np.zeros(Nq, dtype=np.int64)
    for i, t in enumerate(targets):
        if t < 0:
            continue
        ok = np.ones(Nc, dtype=bool)
        if lists is not None:
            l = np.asarray(lists[i], dtype=np.int64)
            ok[l[(l >= 0) & (l < Nc)]] = False
        if exclude_self:
            ok[i] = False
        ok[t] = False
        before = (S[i] > S[i, t]) | ((S[i] == S[i, t]) & (cols < t))
        out[i] = 1 + int((before & ok).sum())
    return out


def _ref_barred(targets, lists=None, exclude_self=False):
    """Rows whose target can never be returned: it is in the row's own list, or is the row itself under exclude_self."""
    bar = np.zeros(len(targets), dtype=bool)
    for i, t in enumerate(targets):
        if t >= 0 and lists is not None and t in np.asarray(lists[i]).tolist():
            bar[i] = True
        if t >= 0 and exclude_self and t == i:
            bar[i] = True
    return bar


def _ref_ncand(Nc, targets, lists=None, exclude_self=False):
    out = np.zeros(len(targets), dtype=np.int64)
    for i, t in enumerate(targets):
        gone = set()
        if lists is not None:
            gone |= {int(x) for x in np.asarray(lists[i]).tolist() if 0 <= x < Nc}
        if exclude_self:
            gone.add(i)
        gone.discard(int(t))
        out[i] = Nc - len(gone)
    return out


@pytest.fixture(scope="module")
def ints():
    rng = np.random.default_rng(3)
    Q = rng.integers(-3, 4, (NQ, D)).astype(np.float32)
    C = rng.integers(-3, 4, (NC, D)).astype(np.float32)
    S = Q.astype(np.int64) @ C.astype(np.int64).T
    t = rng.integers(0, NC, NQ)
    t[[5, 77, 129]] = -1
    return Q, C, S, t


def test_exact_counts_on_integer_data(ints):
    from dae_rnn_news_recommendation_amd.helpers import target_ranks
    Q, C, S, t = ints
    want = _ref_ranks(S, t)
    has = t >= 0
    # the data exercises what it is meant to: index tie-breaks, and negative targets that a zero-padded column would beat
    tied = sum(int((S[i] == S[i, t[i]]).sum() > 1) for i in np.nonzero(has)[0])
    assert tied > NQ // 2 and int((S[np.nonzero(has)[0], t[has]] < 0).sum()) > NQ // 4
    rank, score, ncand = target_ranks(Q, t, metric="linear kernel", candidates=C)
    assert rank.dtype == np.int64 and score.dtype == np.float32 and ncand.dtype == np.int64
    assert np.array_equal(rank, want)
    assert np.array_equal(score[has], S[np.nonzero(has)[0], t[has]].astype(np.float32)) and np.isneginf(score[~has]).all()
    assert (rank[~has] == 0).all() and (ncand == NC).all()
    # one tile, one slice
    t1 = np.where(has, t % NC1, -1)
    rank, score, _ = target_ranks(Q, t1, metric="linear kernel", candidates=C[:NC1])
    assert np.array_equal(rank, _ref_ranks(S[:, :NC1], t1))
    assert np.array_equal(score[has], S[np.nonzero(has)[0], t1[has]].astype(np.float32))
    # the corpus is Q itself, with and without the self pair
    Sq = Q.astype(np.int64) @ Q.astype(np.int64).T
    tq = np.where(has, t % NQ, -1)
    tq[3] = 3                                                            # a target that is the row itself
    for ex in (True, False):
        rank, score, ncand = target_ranks(Q, tq, metric="linear kernel", exclude_self=ex)
        want = np.where(_ref_barred(tq, None, ex), 0, _ref_ranks(Sq, tq, None, ex))
        assert np.array_equal(rank, want), ex
        assert np.array_equal(score[has], Sq[np.nonzero(has)[0], tq[has]].astype(np.float32)), ex
        assert np.array_equal(ncand, _ref_ncand(NQ, tq, None, ex)), ex
        assert (rank[3] == 0) == ex
    with pytest.raises(ValueError, match="targets must be below"):
        target_ranks(Q, np.full(NQ, NC1), metric="linear kernel", candidates=C[:NC1])
    with pytest.raises(ValueError, match="targets for"):
        target_ranks(Q, t[:-1], metric="linear kernel", candidates=C)


def _lists(rng, S, t):
    Nq, Nc = S.shape
    order = np.argsort(-S, axis=1, kind="stable")
    lists = [[],                                                         # empty
             [int(t[1]), 4, 200],                                        # contains the target
             [j for j in range(Nc) if j != t[2]],                        # every candidate but the target: rank 1 of 1
             list(range(128, 256)),                                      # all 128 columns of the middle tile
             list(range(256, 300)),                                      # only columns of the ragged tile
             [1, 2, 3],                                                  # (row 5 has no target)
             [int(j) for j in order[6, :51] if j != t[6]][:50]]          # the would-be top 50
    for i in range(7, Nq):
        n = int(rng.integers(0, 60))
        lists.append(rng.permutation(np.concatenate([order[i, :n // 2], rng.integers(-3, Nc + 3, n - n // 2), order[i, :n // 4]])).tolist())
    return lists


def test_exclusion_lists_on_integer_data(ints):
    from dae_rnn_news_recommendation_amd.helpers import target_ranks
    Q, C, S, t = ints
    lists = _lists(np.random.default_rng(5), S, t)
    assert len(lists) == NQ and t[1] >= 0 and t[2] >= 0 and t[6] >= 0
    rank, score, ncand = target_ranks(Q, t, metric="linear kernel", candidates=C, exclude=lists)
    bar = _ref_barred(t, lists)
    want = np.where(bar, 0, _ref_ranks(S, t, lists))
    assert bar[1] and bar.sum() >= 1
    assert np.array_equal(rank, want)
    assert np.array_equal(ncand, _ref_ncand(NC, t, lists))
    assert rank[2] == 1 and ncand[2] == 1
    has = t >= 0
    assert np.array_equal(score[has], S[np.nonzero(has)[0], t[has]].astype(np.float32))      # a seen target keeps its score
    # the same lists as a CSR tuple, and with the self pair excluded on top (corpus = Q)
    Sq = Q.astype(np.int64) @ Q.astype(np.int64).T
    tq = np.where(has, t % NQ, -1)
    lq = [[x for x in l if x < NQ + 3] for l in lists]
    indptr = np.concatenate([[0], np.cumsum([len(l) for l in lq])]).astype(np.int64)
    items = np.concatenate([np.asarray(l, dtype=np.int64) for l in lq])
    for ex in (True, False):
        rank, _, ncand = target_ranks(Q, tq, metric="linear kernel", exclude_self=ex, exclude=(indptr, items))
        assert np.array_equal(rank, np.where(_ref_barred(tq, lq, ex), 0, _ref_ranks(Sq, tq, lq, ex))), ex
        assert np.array_equal(ncand, _ref_ncand(NQ, tq, lq, ex)), ex


@pytest.fixture(scope="module")
def reals():
    rng = np.random.default_rng(0)
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    C = rng.standard_normal((NC, D)).astype(np.float32)
    t = rng.integers(0, NC, NQ)
    t[[0, 64]] = -1
    S = Q.astype(np.float64) @ C.astype(np.float64).T
    order = np.argsort(-S, axis=1, kind="stable")
    lists = []
    for i in range(NQ):
        n = int(rng.integers(0, 80))
        l = np.concatenate([order[i, :n // 2], rng.integers(0, NC, n - n // 2)])
        lists.append(l[l != t[i]].tolist() if i % 9 else l.tolist())     # every ninth list may hold the target
    return Q, C, t, lists


@pytest.mark.parametrize("norm, metric", [("l2", "cosine"), ("", "linear kernel")])
@pytest.mark.parametrize("with_lists", [False, True])
def test_rank_is_the_position_in_most_similar(reals, norm, metric, with_lists):
    from dae_rnn_news_recommendation_amd.helpers import most_similar, target_ranks
    Q, C, t, lists = reals
    ex = lists if with_lists else None
    rank, score, _ = target_ranks(Q, t, norm=norm, metric=metric, candidates=C, exclude=ex)
    idx, sc = most_similar(Q, k=128, norm=norm, metric=metric, candidates=C, exclude=ex)
    inside = outside = 0
    for i in range(NQ):
        if t[i] < 0:
            assert rank[i] == 0 and np.isneginf(score[i])
            continue
        if 0 < rank[i] <= 128:
            inside += 1
            assert idx[i, rank[i] - 1] == t[i], i
            assert sc[i, rank[i] - 1:rank[i]].view(np.uint32)[0] == score[i:i + 1].view(np.uint32)[0], i       # bit-equal
        else:
            outside += 1
            assert t[i] not in idx[i], i
    assert inside >= 10 and outside >= 10


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rank_lies_in_the_fp64_bracket(seed):
    from dae_rnn_news_recommendation_amd.helpers import target_ranks
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    C = rng.standard_normal((NC, D)).astype(np.float32)
    t = rng.integers(0, NC, NQ)
    rank, _, _ = target_ranks(Q, t, metric="linear kernel", candidates=C)
    lo, hi = _bracket(Q, C, t)
    print("rows with an open bracket:", int((hi > lo).sum()), "widths:", (hi - lo)[hi > lo].tolist())
    assert (lo <= rank).all() and (rank <= hi).all()
    assert (hi > lo).sum() <= 0.05 * NQ                                 # the test cannot pass vacuously


def _bracket(Q, C, t, lists=None):
    """Lowest and highest rank the fp32 scores may give: eps_ij = 2 D 2^-24 sum_k |q_ik c_jk|, the first-order bound on the fp32
    dot product's error, doubled."""
    Q64, C64 = Q.astype(np.float64), C.astype(np.float64)
    S = Q64 @ C64.T
    eps = 2.0 * Q.shape[1] * 2.0 ** -24 * (np.abs(Q64) @ np.abs(C64).T)
    lo, hi = np.zeros(len(t), dtype=np.int64), np.zeros(len(t), dtype=np.int64)
    for i, ti in enumerate(t):
        if ti < 0:
            continue
        ok = np.ones(S.shape[1], dtype=bool)
        if lists is not None:
            ok[np.asarray(lists[i], dtype=np.int64)] = False
        ok[ti] = False
        e = eps[i] + eps[i, ti]
        lo[i] = 1 + int(((S[i] > S[i, ti] + e) & ok).sum())
        hi[i] = 1 + int(((S[i] >= S[i, ti] - e) & ok).sum())
    return lo, hi


def _raw_rank(Q, C, t, lists=None):
    """dae_rank_similarity on the tensors as they are (a strided Q is read in place), linear kernel."""
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd.helpers import normalize_exclusions
    lib = L.load()
    Nq, Dd, Nc = int(Q.shape[0]), int(Q.shape[1]), int(C.shape[0])
    rank = torch.full((Nq,), -7, dtype=torch.int32, device="cuda")
    score = torch.full((Nq,), 7.0, dtype=torch.float32, device="cuda")
    nbytes = int(lib.dae_rank_similarity_workspace(Nq, Nc, Dd))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    off = (-ws.data_ptr()) % 256
    t_d = torch.from_numpy(np.asarray(t, dtype=np.int32)).cuda()
    xp_d = xi_d = None
    if lists is not None:
        xp, xi = normalize_exclusions(lists, Nq, Nc)
        xp_d, xi_d = torch.from_numpy(xp).cuda(), torch.from_numpy(xi if xi.size else np.zeros(1, np.int32)).cuda()
    L.call("dae_rank_similarity", L.ptr(Q), Q.stride(0), Nq, L.ptr(C), C.stride(0), Nc, Dd, 0, 1, 0, L.ptr(xp_d), L.ptr(xi_d), L.ptr(t_d),
           L.ptr(rank), L.ptr(score), ctypes.c_void_p(ws.data_ptr() + off), nbytes, L.current_stream())
    torch.cuda.synchronize()
    return rank.cpu().numpy(), score.cpu().numpy()


def test_determinism_and_order_independence(reals):
    Q, C, t, lists = reals
    Qd, Cd = torch.from_numpy(Q).cuda(), torch.from_numpy(C).cuda()
    r0, s0 = _raw_rank(Qd, Cd, t, lists)
    r1, s1 = _raw_rank(Qd, Cd, t, lists)
    assert r0.tobytes() == r1.tobytes() and s0.tobytes() == s1.tobytes()
    assert (r0[t >= 0] >= 1).all() and (r0[t < 0] == 0).all()
    perm = np.random.default_rng(9).permutation(NQ)
    rp, sp = _raw_rank(Qd[torch.from_numpy(perm).cuda()].contiguous(), Cd, t[perm], [lists[i] for i in perm])
    assert np.array_equal(rp, r0[perm]) and sp.tobytes() == s0[perm].tobytes()
    wide = torch.zeros((NQ, D + 58), dtype=torch.float32, device="cuda")
    wide[:, 21:21 + D] = Qd
    wide[:, :21] = 1e3                                                   # the neighbours of the slice must not leak in
    wide[:, 21 + D:] = -1e3
    view = wide[:, 21:21 + D]
    assert view.stride(0) == D + 58 and not view.is_contiguous()
    rv, sv = _raw_rank(view, Cd, t, lists)
    assert np.array_equal(rv, r0) and sv.tobytes() == s0.tobytes()


def test_recommender_metrics_end_to_end():
    from dae_rnn_news_recommendation_amd import helpers
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
    rng = np.random.default_rng(0)
    labels = np.repeat(np.arange(20), 20)                                # 400 articles
    E = (rng.standard_normal((20, 32))[labels] + 0.5 * rng.standard_normal((400, 32))).astype(np.float32)
    users = 200
    indptr, items = synthetic_sessions(users, labels, mean_len=12, seed=1)
    L = np.diff(indptr)
    targets = np.where(L >= 2, items[np.maximum(indptr[1:] - 1, 0)], -1).astype(np.int64)
    hist = [items[indptr[u]:indptr[u + 1] - 1] for u in range(users)]
    states = helpers.user_states(hist, E, 0.9)
    rank, score, ncand = helpers.recommend_ranks(states, E, targets, seen=hist)
    idx, sc = helpers.recommend(states, E, k=10, seen=hist)
    m = helpers.rank_metrics(rank, ncand, targets)
    want = helpers.next_click_metrics(idx, targets)
    assert m["n"] == want["n"] > 100
    assert m["hit@10"] == want["hit"] and m["mrr@10"] == want["mrr"] and m["ndcg@10"] == want["ndcg"]
    assert 0 < m["hit@10"] < 1
    seen_t = np.array([targets[u] >= 0 and targets[u] in hist[u] for u in range(users)])
    assert np.array_equal(rank == 0, (targets < 0) | seen_t) and seen_t.any()
    assert np.array_equal(ncand, _ref_ncand(400, targets, hist))
    # AUC against fp64: between the values of the bracket's two ends
    lo, hi = _bracket(states, E, np.where(seen_t, -1, targets), hist)
    a = (rank > 0) & (ncand > 1)
    auc_hi = ((ncand[a] - lo[a]) / (ncand[a] - 1.0)).mean()
    auc_lo = ((ncand[a] - hi[a]) / (ncand[a] - 1.0)).mean()
    print("auc", m["auc"], "fp64 bracket", auc_lo, auc_hi, "open rows", int((hi > lo)[a].sum()))
    assert auc_lo - 1e-12 <= m["auc"] <= auc_hi + 1e-12
    assert auc_hi - auc_lo <= 0.05 and m["auc"] > 0.6                   # the user model beats chance by far on these sessions


def test_cli_rank_metrics(tmp_path, monkeypatch, capsys):
    import re

    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    monkeypatch.chdir(tmp_path)
    argv = ["--model_name", "rec", "--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4",
            "--sessions", "synthetic", "--recommend", "10", "--similarity", "False"]
    model = cli.main(argv)
    out0 = capsys.readouterr().out
    import os
    assert not os.path.exists(model.data_dir + "article_encoded_ranks.npz") and "rank metrics" not in out0
    model = cli.main(argv + ["--rank_metrics"])
    out = capsys.readouterr().out
    r = np.load(model.data_dir + "article_encoded_ranks.npz")
    assert sorted(r.files) == ["n_candidates", "rank", "score", "targets"]
    assert r["rank"].shape == r["score"].shape == r["n_candidates"].shape == r["targets"].shape == (200,)
    assert r["rank"].dtype == np.int64 and r["score"].dtype == np.float32
    rec = np.load(model.data_dir + "article_encoded_recommend10.npz")
    assert np.array_equal(rec["targets"], r["targets"])
    for name in ("decayed user state", "most clicked unseen"):
        topk = re.search(r"hit@10 " + name + r"\s+([0-9.]+)", out).group(1)
        full = re.search(r"ranks " + name + r".*hit@10 ([0-9.]+)", out).group(1)
        assert topk == full, (name, topk, full)
    assert "AUC" in out and "median rank" in out and "hit@100" in out
    m = helpers.rank_metrics(r["rank"], r["n_candidates"], r["targets"], ks=(10,))
    assert m["hit@10"] == helpers.next_click_metrics(rec["indices"], rec["targets"])["hit"]
    with pytest.raises(AssertionError, match="--rank_metrics needs --recommend"):
        cli.main(["--model_name", "x", "--rank_metrics"])
