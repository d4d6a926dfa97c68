"""The co-visitation model without a GPU: the NumPy reference (tests/covisit_reference.py) against a brute-force dense count matrix,
dae_covisit_record_bound, the argument errors of the two entry points (reported before any HIP call), the host code of
helpers.covisit, and the claim the feature rests on -- the model beats the popularity baseline on the project's synthetic logs."""
import ctypes

import numpy as np
import pytest

from covisit_reference import covisit_recommend_reference, covisit_records, covisit_reference
from dae_rnn_news_recommendation_amd import _lib, helpers
from dae_rnn_news_recommendation_amd.helpers.covisit import fill_popular_tails
from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions

F32 = np.float32


def _random_log(rng, users, Na, max_len):
    return _csr([rng.integers(0, Na, rng.integers(0, max_len + 1)) for _ in range(users)])


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if indptr[-1] else np.zeros(0, dtype=np.int64)
    return indptr, items


def _dense_counts(indptr, items, Na, window, both):
    C = np.zeros((Na, Na), dtype=np.int64)
    for u in range(indptr.size - 1):
        h = items[indptr[u]:indptr[u + 1]]
        for p in range(h.size):
            for q in range(p + 1, h.size):
                if q - p <= window and h[p] != h[q]:
                    C[h[p], h[q]] += 1
                    if both:
                        C[h[q], h[p]] += 1
    return C


@pytest.mark.parametrize("window", [1, 2, 5, 100])
@pytest.mark.parametrize("both", [0, 1])
@pytest.mark.parametrize("cosine", [0, 1])
def test_reference_against_dense_counts(window, both, cosine):
    rng = np.random.default_rng(7 + window)
    Na, K = 40, 6
    indptr, items = _random_log(rng, 60, Na, 12)
    ref = covisit_reference(indptr, items, Na, window, both, cosine, K)
    C = _dense_counts(indptr, items, Na, window, both)
    clicks = np.bincount(items, minlength=Na)
    assert np.array_equal(ref["clicks"], clicks) and np.array_equal(ref["degree"], (C > 0).sum(axis=1))
    assert ref["n_records"] == C.sum() and ref["n_pairs"] == (C > 0).sum()
    if cosine:
        with np.errstate(divide="ignore", invalid="ignore"):
            S = C.astype(F32) / np.sqrt(np.outer(clicks, clicks).astype(F32))
    else:
        S = C.astype(F32)
    for a in range(Na):
        b = np.flatnonzero(C[a] > 0)
        order = b[np.lexsort((b, -S[a, b].astype(np.float64)))][:K]
        n = order.size
        assert np.array_equal(ref["nbr"][a, :n], order) and (ref["nbr"][a, n:] == -1).all()
        assert np.array_equal(ref["sim"][a, :n].view(np.uint32), S[a, order].view(np.uint32)) and (ref["sim"][a, n:] == 0).all()
        assert np.array_equal(ref["cnt"][a, :n], C[a, order]) and (ref["cnt"][a, n:] == 0).all()
    if both:
        assert np.array_equal(C, C.T)


def test_record_bound():
    lib = _lib.load()
    bound = lambda ptr, w, both: int(lib.dae_covisit_record_bound(ptr.ctypes.data_as(ctypes.c_void_p), ptr.size - 1, w, both))  # noqa: E731
    rng = np.random.default_rng(11)
    indptr, items = _random_log(rng, 80, 30, 15)
    for w in (1, 3, 14, 15, 1000):
        for both in (0, 1):
            n = covisit_records(indptr, items, w, both).shape[0]
            assert bound(indptr, w, both) >= n
            want = sum(min(w, L - 1 - p) for L in np.diff(indptr) for p in range(L)) * (2 if both else 1)
            assert bound(indptr, w, both) == want
    # no adjacent equal items within the window: the bound is the record count
    rows = [rng.permutation(30)[:rng.integers(0, 16)] for _ in range(50)]
    ptr, it = _csr(rows)
    for w in (1, 4, 1000):
        for both in (0, 1):
            assert bound(ptr, w, both) == covisit_records(ptr, it, w, both).shape[0]
    assert bound(np.zeros(1, dtype=np.int64), 3, 1) == 0                 # no user
    assert bound(ptr, 0, 1) == 0                                         # no window
    assert bound(_csr([[], [5], [5, 5, 5]])[0], 2, 0) == 3               # the bound counts the equal pairs too
    assert int(lib.dae_covisit_record_bound(None, 3, 2, 1)) == 0


def _neighbors_args(**over):
    """Arguments of dae_covisit_neighbors that pass every check but the one a test breaks; no pointer is ever followed."""
    ptr = np.array([0, 3], dtype=np.int64)
    fake = ctypes.c_void_p(256)
    a = dict(indptr=fake, items=fake, indptr_host=ptr.ctypes.data_as(ctypes.c_void_p), M=1, nnz=3, Na=10, window=2, both=1, normalize=1,
             K=4, nbr=fake, sim=fake, cnt=fake, ld=4, degree=fake, clicks=fake, totals=fake, ws=ctypes.c_void_p(512), ws_bytes=0,
             stream=None)
    a.update(over)
    return list(a.values()), ptr


@pytest.mark.parametrize("over, text", [
    (dict(K=0), "K (0) must be in 1..128"), (dict(K=129, ld=200), "K (129) must be in 1..128"),
    (dict(window=0), "window (0) must be at least 1"), (dict(Na=0), "Na (0) must be at least 1"),
    (dict(ld=3), "ld (3) must be >= K (4)"), (dict(nbr=None), "an output is NULL"), (dict(totals=None), "an output is NULL"),
    (dict(both=2), "both (2)"), (dict(normalize=5), "normalize (5)"), (dict(indptr_host=None), "indptr_host is NULL"),
    (dict(items=None), "indptr / items is NULL"), (dict(nnz=4), "must start at 0 and end at nnz"),
    (dict(ws=ctypes.c_void_p(513), ws_bytes=1 << 20), "256-byte aligned"), (dict(ws=None, ws_bytes=1 << 20), "256-byte aligned"),
    (dict(ws_bytes=256), "workspace too small"), (dict(M=-1), "must not be negative"),
])
def test_neighbors_argument_errors_without_a_gpu(over, text):
    lib = _lib.load()
    args, _keep = _neighbors_args(**over)
    assert lib.dae_covisit_neighbors(*args) == 1
    msg = lib.dae_last_error().decode()
    assert msg.startswith("covisit_neighbors: ") and text in msg, msg


def test_workspace_size_argument_errors():
    lib = _lib.load()
    assert lib.dae_covisit_neighbors_workspace(0, 10, 4) == 0            # nothing to sort
    for bound, Na, K in ((100, 0, 4), (100, 10, 0), (100, 10, 129), (1 << 31, 10, 4)):
        assert lib.dae_covisit_neighbors_workspace(bound, Na, K) == 0


@pytest.mark.parametrize("over, text", [
    (dict(K=0), "K (0) must be in 1..128"), (dict(K=129, ld=129), "K (129)"), (dict(Na=0), "Na (0)"), (dict(ld=3), "ld (3) must be >= K (4)"),
    (dict(last=0), "last (0) must be in 1..32"), (dict(last=33), "last (33) must be in 1..32"), (dict(k=0), "k (0) must be in 1..128"),
    (dict(k=129, ldo=129), "k (129) must be in 1..128"), (dict(ldo=4), "ldo (4) must be >= k (5)"), (dict(nbr=None), "the table is NULL"),
    (dict(win_lo=ctypes.c_void_p(256)), "win_lo and win_hi go together"), (dict(M=-1), "M (-1)"), (dict(age_weight=None), "is NULL"),
    (dict(seen_indptr=None), "is NULL"),
])
def test_recommend_argument_errors_without_a_gpu(over, text):
    lib = _lib.load()
    fake = ctypes.c_void_p(256)
    a = dict(nbr=fake, sim=fake, ld=4, Na=10, K=4, indptr=fake, items=fake, M=2, seen_indptr=fake, seen_items=fake, win_lo=None, win_hi=None,
             age_weight=fake, last=3, k=5, idx=fake, score=fake, ldo=5, stream=None)
    a.update(over)
    assert lib.dae_covisit_recommend(*a.values()) == 1
    msg = lib.dae_last_error().decode()
    assert msg.startswith("covisit_recommend: ") and text in msg, msg


def test_list_overlap():
    a = np.array([[1, 2, 3, -1], [4, 5, -1, -1], [-1, -1, -1, -1], [7, 8, 9, 10]])
    b = np.array([[3, 1, 9], [6, 7, 8], [1, 2, 3], [10, 9, -1]])
    per, mean = helpers.list_overlap(a, b)
    assert np.allclose(per[[0, 1, 3]], [2 / 3, 0.0, 0.5]) and np.isnan(per[2])
    assert mean == pytest.approx((2 / 3 + 0.0 + 0.5) / 3)
    per, mean = helpers.list_overlap(np.full((2, 3), -1), np.zeros((2, 1), dtype=np.int64))
    assert np.isnan(per).all() and np.isnan(mean)
    assert helpers.list_overlap(a, a)[1] == 1.0
    with pytest.raises(ValueError):
        helpers.list_overlap(a, b[:3])
    big = np.arange(5000 * 3).reshape(5000, 3)                           # more than one row block
    assert helpers.list_overlap(big, big[:, ::-1])[1] == 1.0


def test_fill_popular_tails():
    clicks = np.array([5, 9, 9, 1, 0, 7])                                # by popularity: 1, 2, 5, 0, 3, 4
    idx = np.array([[3, -1, -1], [1, 2, 5], [-1, -1, -1], [-1, -1, -1], [4, -1, -1]])
    seen = (np.array([0, 1, 1, 3, 9, 9]), np.array([1, 1, 2, 0, 1, 2, 3, 4, 5]))
    out = fill_popular_tails(idx, clicks, seen)
    assert np.array_equal(out, [[3, 2, 5], [1, 2, 5], [5, 0, 3], [-1, -1, -1], [4, 1, 2]])
    assert np.array_equal(idx[0], [3, -1, -1])                           # the input is not touched
    out = fill_popular_tails(idx, clicks, seen, window=(np.array([0, 0, 3, 0, 2]), np.array([3, 6, 6, 6, 2])))
    assert np.array_equal(out, [[3, 2, 0], [1, 2, 5], [5, 3, 4], [-1, -1, -1], [4, -1, -1]])


def _index(Na=6, K=3):
    nbr = np.full((Na, K), -1, dtype=np.int64)
    return helpers.CovisitIndex(nbr, np.zeros((Na, K), dtype=F32), np.zeros((Na, K), dtype=np.int32), np.zeros(Na, dtype=np.int32),
                                np.zeros(Na, dtype=np.int32), 0, 0, 3, "both", "cosine", K)


@pytest.mark.parametrize("kw, text", [
    (dict(k=0), "k must be in 1..128"), (dict(k=129), "k must be in 1..128"), (dict(last=0), "last must be in 1..32"),
    (dict(last=33), "last must be in 1..32"), (dict(position_decay=float("nan")), "position_decay"),
    (dict(histories=[[0, 6]]), "history items must be in 0..5"), (dict(histories=[[0.5]]), "integer"),
    (dict(seen=[[1], [2]]), "exclude has 2 rows for 1 queries"), (dict(window=([0], [7])), "window hi"),
    (dict(window=([3], [2])), "window lo must not exceed hi"),
])
def test_recommend_host_checks(kw, text):
    kw = dict(kw)
    hist = kw.pop("histories", [[0, 1]])
    with pytest.raises(ValueError, match=text):
        _index().recommend(hist, **kw)


def test_build_host_checks_and_index_round_trip(tmp_path):
    for kw in (dict(window=0), dict(direction="backward"), dict(normalize="l2"), dict(n_neighbors=0), dict(n_neighbors=129)):
        with pytest.raises(ValueError):
            helpers.covisit_neighbors([[0, 1]], 4, **kw)
    with pytest.raises(ValueError):
        helpers.covisit_neighbors([[0, 4]], 4)
    with pytest.raises(ValueError):
        helpers.covisit_neighbors([[0, 1]], 0)
    with pytest.raises(ValueError):
        helpers.CovisitIndex(np.zeros((3, 2), dtype=np.int64), np.zeros((3, 3), dtype=F32), None, None, None, 0, 0, 3, "both", "cosine", 2)
    ix = _index()
    ix.neighbors[2, :2] = [4, 1]
    ix.save(str(tmp_path / "ix.npz"))
    back = helpers.CovisitIndex.load(str(tmp_path / "ix.npz"))
    assert np.array_equal(back.neighbors, ix.neighbors) and back.sims.dtype == F32 and back.neighbors.dtype == np.int64
    assert (back.window, back.direction, back.normalize, back.n_neighbors, back.n_articles) == (3, "both", "cosine", 3, 6)
    n, s, c = back.similar([2, 0], 2)
    assert np.array_equal(n, [[4, 1], [-1, -1]]) and s.shape == c.shape == (2, 2)
    with pytest.raises(ValueError):
        back.similar([6])
    with pytest.raises(ValueError):
        back.similar([0], 4)


def test_recommend_reference_on_a_hand_made_table():
    """Two sources, one shared candidate: the order of the additions, the seen list, the window and the tie-break."""
    nbr = np.array([[1, 2, -1], [0, 2, 3], [0, 1, -1], [1, -1, -1]], dtype=np.int32)
    sim = np.array([[0.5, 0.25, 0], [0.5, 0.75, 0.125], [0.25, 0.75, 0], [0.125, 0, 0]], dtype=F32)
    w = np.array([1.0, 0.5], dtype=F32)
    ptr, it = _csr([[3, 0, 1], [], [2]])
    idx, sc = covisit_recommend_reference(nbr, sim, ptr, it, ptr, it, w, 2, 3)
    # user 0: sources 0 (age 1) and 1 (age 0): 1 <- .25 (seen), 2 <- .125 + .75, 0 <- .5 (seen), 3 <- .125 (seen)
    assert idx.tolist() == [[2, -1, -1], [-1, -1, -1], [1, 0, -1]]
    assert sc[0, 0] == F32(0.875) and np.isneginf(sc[0, 1:]).all() and sc[2].tolist()[:2] == [0.75, 0.25] and np.isneginf(sc[1]).all()
    idx, sc = covisit_recommend_reference(nbr, sim, ptr, it, *_csr([[], [], []]), w, 2, 3)
    assert idx[0].tolist() == [2, 0, 1] and sc[0].tolist() == [0.875, 0.5, 0.25]
    idx, _ = covisit_recommend_reference(nbr, sim, ptr, it, *_csr([[], [], []]), w, 2, 3, window=([1, 0, 0], [4, 4, 0]))
    assert idx.tolist() == [[2, 1, 3], [-1, -1, -1], [-1, -1, -1]]


def test_reference_beats_popularity_on_the_seeded_log():
    """The claim the feature rests on: on synthetic_sessions(3000, labels, mean_len=8, seed=1), the last click held out, window 3,
    both directions, cosine, 50 neighbours, last 10 clicks, decay 0.8, the co-visitation lists hit at least twice as often as the
    most-clicked-unseen baseline (measured: 0.0324 against 0.0057)."""
    labels = np.random.default_rng(0).integers(0, 20, 2000)
    indptr, items = synthetic_sessions(3000, labels, mean_len=8, seed=1)
    lens = np.diff(indptr)
    targets = np.where(lens >= 2, items[np.maximum(indptr[1:] - 1, 0)], -1).astype(np.int64)
    keep = np.ones(items.size, dtype=bool)
    keep[indptr[1:][lens >= 2] - 1] = False
    h_ptr = np.zeros(lens.size + 1, dtype=np.int64)
    h_ptr[1:] = np.cumsum(lens - (lens >= 2))
    hist = (h_ptr, items[keep])
    ref = covisit_reference(*hist, 2000, 3, 1, 1, 50)
    age_weight = (np.float64(0.8) ** np.arange(10)).astype(F32)
    xp, xi = helpers.normalize_exclusions(hist, lens.size, 2000)
    idx, _ = covisit_recommend_reference(ref["nbr"], ref["sim"], *hist, xp, xi, age_weight, 10, 10)
    mine = helpers.next_click_metrics(idx, targets)
    base = helpers.next_click_metrics(helpers.popularity_recommend(hist, 2000, 10), targets)
    print("hit@10: co-visitation %.4f, popularity %.4f" % (mine["hit"], base["hit"]))
    assert base["hit"] > 0 and mine["hit"] >= 2 * base["hit"]
