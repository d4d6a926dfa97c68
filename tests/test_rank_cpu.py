"""CPU checks of full-rank evaluation (dae_rank_similarity) and of the host code around it: both builds export the symbols under
an unchanged ABI version, argument errors are reported before any HIP call (so on a machine without a GPU), the workspace has
no Nq x Nc term, and rank_metrics / popularity_ranks on hand-made ranks, against next_click_metrics where the two overlap."""
import ctypes
import math

import numpy as np
import pytest

P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_rank_symbols_are_exported_and_the_abi_version_stays(fmt):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load(fmt)
    for name in ("dae_rank_similarity", "dae_rank_similarity_workspace"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.dae_abi_version() == _lib.ABI_VERSION == 9


def _rank(lib, Q=P, ldq=None, Nq=100, C=None, ldc=0, Nc=100, D=50, norm=0, metric=0, exclude_self=1, xp=P, xi=P, targets=P, rank=P,
          score=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_rank_similarity_workspace(Nq, Nc, D)
    return lib.dae_rank_similarity(Q, D if ldq is None else ldq, Nq, C, ldc, Nc, D, norm, metric, exclude_self, xp, xi, targets, rank,
                                   score, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(xp=None), b"excl_indptr and excl_items go together"),
    (dict(xi=None), b"excl_indptr and excl_items go together"),
    (dict(Q=None), b"bad input"),
    (dict(ws=None), b"bad input"),
    (dict(ldq=49), b"bad input"),
    (dict(targets=None), b"targets / rank / target_score are NULL"),
    (dict(rank=None), b"targets / rank / target_score are NULL"),
    (dict(score=None), b"targets / rank / target_score are NULL"),
    (dict(Nc=99), b"bad corpus"),
    (dict(C=P, ldc=10, exclude_self=0), b"bad corpus"),
    (dict(norm=4), b"norm must be"),
    (dict(norm=-1), b"norm must be"),
    (dict(metric=2), b"metric must be"),
    (dict(C=P, ldc=50, exclude_self=1), b"exclude_self needs C == NULL"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
    (dict(Nq=3 * 10 ** 6, Nc=3 * 10 ** 6, D=500), b"exceeds 4 GiB"),
])
def test_rank_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _rank(lib, **kw) != 0
    assert b"rank_similarity" in lib.dae_last_error() and msg in lib.dae_last_error(), lib.dae_last_error()


def test_rank_workspace_has_no_quadratic_term():
    lib = _lib()
    ws = lib.dae_rank_similarity_workspace
    Nqp, Ncp, Dp = lib.dae_pad(100000), lib.dae_pad(64000), lib.dae_pad(500)
    got = ws(100000, 64000, 500)
    assert 0 < got < 2 * (Nqp + Ncp) * Dp * 4 + 64 * Nqp                # the users x articles fp32 matrix would be 25.6 GB
    assert got < 100000 * 64000 * 4 // 40
    # equal steps of the row counts give equal growth, up to the 256-byte alignment of the pieces
    a, b, c = (ws(n * 100000, 50000, 500) for n in (1, 2, 3))
    assert abs((c - b) - (b - a)) <= 4096 and b > a
    a, b, c = (ws(50000, n * 100000, 500) for n in (1, 2, 3))
    assert abs((c - b) - (b - a)) <= 4096 and b > a
    assert ws(0, 10, 10) == 0 and ws(10, 0, 10) == 0 and ws(10, 10, 0) == 0


def _lists_from_ranks(rank, targets, k):
    """A k-list per query in which the target sits at position rank - 1 (when 0 < rank <= k) among fillers that match nothing."""
    idx = np.full((len(rank), k), 10 ** 6, dtype=np.int64)
    for i, (r, t) in enumerate(zip(rank, targets)):
        if t >= 0 and 0 < r <= k:
            idx[i, r - 1] = t
    return idx


def test_rank_metrics_on_hand_made_ranks():
    from dae_rnn_news_recommendation_amd.helpers import next_click_metrics, rank_metrics
    #                 hit@1  hit@5  miss@10..  seen target  single candidate  no target
    rank = np.array([1, 4, 60, 0, 1, 0])
    ncand = np.array([100, 100, 101, 90, 1, 100])
    tgt = np.array([7, 3, 9, 5, 2, -1])
    m = rank_metrics(rank, ncand, tgt, ks=(1, 5, 10, 50, 100))
    assert m["n"] == 5 and m["n_ranked"] == 4
    assert m["hit@1"] == pytest.approx(2 / 5) and m["hit@5"] == pytest.approx(3 / 5) and m["hit@50"] == pytest.approx(3 / 5)
    assert m["hit@100"] == pytest.approx(4 / 5)
    assert m["mrr@5"] == pytest.approx((1 + 1 / 4 + 1) / 5) and m["mrr"] == pytest.approx((1 + 1 / 4 + 1 / 60 + 0 + 1) / 5)
    assert m["ndcg@5"] == pytest.approx((1 + 1 / math.log2(5) + 1) / 5)
    assert m["ndcg"] == pytest.approx((1 + 1 / math.log2(5) + 1 / math.log2(61) + 1) / 5)
    assert m["mean_rank"] == pytest.approx((1 + 4 + 60 + 1) / 4) and m["median_rank"] == pytest.approx(2.5)
    assert m["auc"] == pytest.approx((99 / 99 + 96 / 99 + 41 / 100) / 3)      # the single-candidate row is skipped, the seen one unranked
    # truncated metrics equal next_click_metrics on lists built from the same ranks, exactly
    for k in (1, 5, 10, 50, 100):
        want = next_click_metrics(_lists_from_ranks(rank, tgt, k), tgt)
        assert want["n"] == m["n"]
        assert m[f"hit@{k}"] == want["hit"] and m[f"mrr@{k}"] == want["mrr"] and m[f"ndcg@{k}"] == want["ndcg"], k
    rng = np.random.default_rng(0)
    rank = rng.integers(0, 300, 500)
    tgt = np.where(rng.random(500) < 0.1, -1, rng.integers(0, 1000, 500))
    m = rank_metrics(rank, np.full(500, 1000), tgt, ks=(3, 128))
    for k in (3, 128):
        want = next_click_metrics(_lists_from_ranks(rank, tgt, k), tgt)
        assert m[f"hit@{k}"] == want["hit"] and m[f"mrr@{k}"] == want["mrr"] and m[f"ndcg@{k}"] == want["ndcg"], k


def test_rank_metrics_where_nothing_counts():
    from dae_rnn_news_recommendation_amd.helpers import rank_metrics
    m = rank_metrics([0, 0], [10, 10], [-1, -1], ks=(1, 10))
    assert m["n"] == 0 and m["n_ranked"] == 0
    assert all(math.isnan(m[key]) for key in ("hit@1", "mrr@10", "ndcg@10", "mrr", "ndcg", "mean_rank", "median_rank", "auc"))
    m = rank_metrics([0, 1], [10, 1], [4, 0], ks=(1,))                 # one seen target, one single-candidate row
    assert m["n"] == 2 and m["n_ranked"] == 1 and m["hit@1"] == 0.5 and m["mean_rank"] == 1.0 and math.isnan(m["auc"])
    with pytest.raises(ValueError):
        rank_metrics([1, 2], [10], [0, 1])


def test_popularity_ranks_agree_with_popularity_recommend():
    from dae_rnn_news_recommendation_amd.helpers import popularity_ranks, popularity_recommend
    hist = [[0, 0, 1], [0, 2, 2], [3], []]                               # clicks: article 0: 3, 2: 2, 1: 1, 3: 1, 4: 0
    tgt = np.array([4, 1, 3, -1])                                        # orders: [2, 3, 4], [1, 3, 4], [0, 2, 1, 4] (3 is seen)
    rank, ncand = popularity_ranks(hist, 5, tgt)
    assert rank.tolist() == [3, 1, 0, 0] and ncand.tolist() == [3, 3, 5, 5]
    rng = np.random.default_rng(1)
    hist = [rng.integers(0, 40, rng.integers(0, 12)) for _ in range(60)]
    tgt = rng.integers(-1, 40, 60)
    rank, ncand = popularity_ranks(hist, 40, tgt)
    lists = popularity_recommend(hist, 40, 40)
    for u in range(60):
        pos = np.nonzero(lists[u] == tgt[u])[0] if tgt[u] >= 0 else []
        assert rank[u] == (pos[0] + 1 if len(pos) else 0), u
        seen_t = tgt[u] >= 0 and tgt[u] in hist[u]
        assert ncand[u] == (lists[u] >= 0).sum() + int(seen_t), u
