"""dae_word_profiles / dae_word_topk / dae_word_rank and helpers.words on the GPU against tests/words_reference.py: indices equal,
scores bit-equal.  The score kernel stages the articles' rows through LDS in passes of 32 entries per article (WORD_PASS in
csrc/dae_words.hip): the long row of the V = 2100 cases has 1100 entries, 35 passes, and every case has rows of other lengths
beside it, so a tile's passes end at different entries for different lanes."""
import ctypes
import functools
import glob
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from dae_rnn_news_recommendation_amd import _lib as L
from dae_rnn_news_recommendation_amd import helpers
from words_reference import profiles_reference, ranks_reference, scores_reference, topk_reference

pytestmark = pytest.mark.gpu
F32 = np.float32
WORD_PASS = 32                                                           # the staging pass the long row is meant to exceed
LONG_ROW = 1100


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a) if a.size else np.zeros(1, dtype=a.dtype)).cuda()


@functools.lru_cache(maxsize=None)
def case(M, Na, V, kind="binary", seed=0):
    """Articles, histories, weights and the reference scores of one shape.  Row 0 is empty (Na > 1), row 2 is the long row
    (V >= 2 * LONG_ROW - 100); user 0 has no history (M > 1), user 1 clicks one article three times."""
    rng = np.random.default_rng(1000 * M + 10 * Na + V + seed)
    per = max(1, min(V, 12))
    rows = []
    for a in range(Na):
        n = int(rng.integers(1, per + 1))
        if a == 0 and Na > 1:
            n = 0
        if a == 2 and V >= 2 * LONG_ROW - 100:
            n = LONG_ROW
        rows.append(np.sort(rng.choice(V, size=min(n, V), replace=False)))
    indptr = np.zeros(Na + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, dtype=np.int32)
    data = np.ones(indices.size, dtype=F32)
    tw = None
    if kind != "binary":
        data = rng.uniform(0.05, 1.0, indices.size).astype(F32)          # tf-idf-like values
        if kind == "negative":
            data[::3] *= F32(-1)
        df = np.bincount(indices, minlength=V)
        tw = (np.log((1.0 + Na) / (1.0 + df)) + 1.0).astype(F32)
        if kind == "negative":
            tw[1::2] *= F32(-1)
    A = sp.csr_matrix((data, indices, indptr), shape=(Na, V))
    hist = [rng.integers(0, Na, rng.integers(1, 7)) for _ in range(M)]
    if M > 1:
        hist[0] = np.zeros(0, dtype=np.int64)
        hist[1] = np.full(3, Na // 2, dtype=np.int64)
    if M > 2 and Na > 2:
        hist[2] = np.array([2, Na - 1], dtype=np.int64)                  # a reader of the long row
    h_ptr = np.zeros(M + 1, dtype=np.int64)
    h_ptr[1:] = np.cumsum([h.size for h in hist])
    h_items = np.concatenate(hist).astype(np.int64)
    P = profiles_reference(h_ptr, h_items, A, V)
    R = scores_reference(P, A, tw)
    return dict(A=A, hist=(h_ptr, h_items), tw=tw, P=P, R=R, M=M, Na=Na, V=V, kind=kind)


def articles_of(c):
    """What the helper is given: for the binary kind a device CSR dict without values, else the scipy matrix."""
    if c["kind"] != "binary":
        return c["A"]
    A = c["A"]
    return dict(indptr=_up(A.indptr.astype(np.int64)), indices=_up(A.indices.astype(np.int32)), values=None, n_rows=A.shape[0], nnz=int(A.nnz),
                n_cols=A.shape[1])


def check_lists(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == F32
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(_bits(got[1]), _bits(want[1]))


SHAPES = ([(M, 129, 33) for M in (1, 64, 65, 127, 128, 129, 300)] + [(129, Na, 1000) for Na in (1, 127, 128, 700)]
          + [(65, 129, V) for V in (1, 1000, 2100)] + [(300, 700, 2100)])


@pytest.mark.parametrize("kind", ["binary", "tfidf"])
@pytest.mark.parametrize("M,Na,V", SHAPES)
def test_recommend_equals_the_reference(M, Na, V, kind):
    c = case(M, Na, V, kind)
    art = articles_of(c)
    for k in (1, 10, 128):                                               # 128 > Na at Na in (1, 127): short rows end in -1 / -inf
        check_lists(helpers.word_recommend(c["hist"], art, k, term_weights=c["tw"]), topk_reference(c["R"], k))
    if M > 1:                                                            # the user without a history: all scores +0, the lowest indices
        idx, score = helpers.word_recommend(c["hist"], art, 10, term_weights=c["tw"])
        n = min(10, Na)
        assert idx[0, :n].tolist() == list(range(n)) and (_bits(score[0, :n]) == 0).all()


def test_negative_weights():
    c = case(129, 129, 1000, "negative")
    assert (c["R"] < 0).any() and (c["R"] > 0).any()
    for k in (1, 10, 128):
        check_lists(helpers.word_recommend(c["hist"], c["A"], k, term_weights=c["tw"]), topk_reference(c["R"], k))


@pytest.mark.parametrize("max_events", [None, 1, 3])
@pytest.mark.parametrize("M,Na,V", [(129, 129, 33), (300, 700, 2100)])
def test_profiles_and_max_events(M, Na, V, max_events):
    c = case(M, Na, V, "tfidf")
    P = profiles_reference(*c["hist"], c["A"], V, max_events)
    prof = helpers.word_profiles(c["hist"], c["A"], max_events=max_events)
    assert prof.n_users == M and prof.n_words == V and tuple(prof.bitmaps.shape) == ((M + 127) // 128, V, 4)
    assert np.array_equal(prof.to_scipy().toarray(), P)
    assert prof.sizes.dtype == np.int32 and np.array_equal(prof.sizes, P.sum(axis=1))
    want = topk_reference(scores_reference(P, c["A"], c["tw"]), 10)
    check_lists(helpers.word_recommend(prof, c["A"], 10, term_weights=c["tw"]), want)
    check_lists(helpers.word_recommend(c["hist"], c["A"], 10, term_weights=c["tw"], max_events=max_events), want)


def raw_profiles(h_ptr, h_items, ip, ix, Na, V, M, max_events=0):
    import torch
    lib = L.load()
    nbytes = int(lib.dae_word_profiles_bytes(M, V))
    assert nbytes == (M + 127) // 128 * V * 16
    bitmaps = torch.full((nbytes // 4 + 8,), -1, dtype=torch.int32, device="cuda")
    sizes = torch.full((M + 3,), -7, dtype=torch.int32, device="cuda")
    d = [_up(h_ptr.astype(np.int64)), _up(h_items.astype(np.int32)), _up(ip.astype(np.int64)), _up(ix.astype(np.int32))]
    L.call("dae_word_profiles", L.ptr(d[0]), L.ptr(d[1]), int(h_items.size), M, max_events, L.ptr(d[2]), L.ptr(d[3]), int(ix.size), Na, V,
           L.ptr(bitmaps), nbytes, L.ptr(sizes), L.current_stream())
    torch.cuda.synchronize()
    assert (bitmaps[nbytes // 4:] == -1).all() and (sizes[M:] == -7).all()          # nothing behind the ends is written
    return bitmaps[:nbytes // 4].view(-1, V, 4), sizes[:M]


def test_raw_profiles_drop_what_is_out_of_range():
    c = case(129, 129, 33, "binary")
    A, (h_ptr, h_items) = c["A"], c["hist"]
    items = h_items.copy()
    items[::5] = 129 + np.arange(items[::5].size)                        # items >= Na
    items[1::7] = -3
    cols = A.indices.astype(np.int64).copy()
    cols[::4] = 33 + (np.arange(cols[::4].size) % 5)                     # columns >= V
    cols[2::9] = -1
    bitmaps, sizes = raw_profiles(h_ptr, items, A.indptr, cols, 129, 33, 129)
    P = profiles_reference(h_ptr, items, (A.indptr, cols, None), 33)
    got = helpers.WordProfiles(bitmaps, 129, 33, sizes.cpu().numpy())
    assert np.array_equal(got.to_scipy().toarray(), P) and np.array_equal(got.sizes, P.sum(axis=1))


def raw_articles(c, cols=None, values=True):
    """The articles of a case on the device as the entry points take them: ``(indptr, indices, weights, nnz)``, the weights from
    dae_word_entry_weights.  ``cols``: other column indices for the same rows (e.g. some out of range)."""
    import torch
    A, V = c["A"], c["V"]
    ip, ix = _up(A.indptr.astype(np.int64)), _up((A.indices if cols is None else cols).astype(np.int32))
    w = torch.full((max(A.nnz, 1) + 2,), -7.0, dtype=torch.float32, device="cuda")
    tw = None if c["tw"] is None else _up(c["tw"])
    vals = _up(A.data.astype(F32)) if values and c["kind"] != "binary" else None
    assert int(L.load().dae_word_entry_weights_bytes(int(A.nnz))) >= 4 * A.nnz
    L.call("dae_word_entry_weights", L.ptr(ix), L.ptr(vals), int(A.nnz), V, L.ptr(tw), L.ptr(w), L.current_stream())
    torch.cuda.synchronize()
    assert (w[A.nnz:] == -7).all()
    return ip, ix, w, int(A.nnz)


def _raw_workspace(nbytes):
    import torch
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    return ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256), ws


def raw_topk(c, bitmaps, k, xp=None, xi=None, lo=None, hi=None, extra=0, cols=None):
    """dae_word_topk through the C ABI, into buffers wider than k pre-filled with -7."""
    import torch
    M, Na, V = c["M"], c["Na"], c["V"]
    ip, ix, w, nnz = raw_articles(c, cols)
    idx = torch.full((M, k + 3), -7, dtype=torch.int32, device="cuda")
    score = torch.full((M, k + 3), -7.0, dtype=torch.float32, device="cuda")
    ws_bytes = int(L.load().dae_word_topk_workspace(M, Na, k)) + extra
    ws_p, ws = _raw_workspace(ws_bytes)
    d = [None if x is None else _up(x) for x in (xp, xi, lo, hi)]
    L.call("dae_word_topk", L.ptr(bitmaps), M, V, L.ptr(ip), L.ptr(ix), L.ptr(w), nnz, Na, k, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]),
           L.ptr(d[3]), L.ptr(idx), L.ptr(score), idx.stride(0), ws_p, ws_bytes, L.current_stream())
    torch.cuda.synchronize()
    assert (idx[:, k:] == -7).all() and (score[:, k:] == -7).all()
    return idx[:, :k].long().cpu().numpy(), score[:, :k].contiguous().cpu().numpy()


def raw_rank(c, bitmaps, targets, xp=None, xi=None, lo=None, hi=None, extra=0, cols=None):
    """dae_word_rank through the C ABI, into buffers longer than M pre-filled with -7: ``(rank int64, target_score float32)``."""
    import torch
    M, Na, V = c["M"], c["Na"], c["V"]
    ip, ix, w, nnz = raw_articles(c, cols)
    rank = torch.full((M + 3,), -7, dtype=torch.int32, device="cuda")
    ts = torch.full((M + 3,), -7.0, dtype=torch.float32, device="cuda")
    ws_bytes = int(L.load().dae_word_rank_workspace(M)) + extra
    ws_p, ws = _raw_workspace(ws_bytes)
    d = [None if x is None else _up(x) for x in (xp, xi, lo, hi)]
    t_d = _up(np.asarray(targets).astype(np.int32))
    L.call("dae_word_rank", L.ptr(bitmaps), M, V, L.ptr(ip), L.ptr(ix), L.ptr(w), nnz, Na, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]),
           L.ptr(t_d), L.ptr(rank), L.ptr(ts), ws_p, ws_bytes, L.current_stream())
    torch.cuda.synchronize()
    assert (rank[M:] == -7).all() and (ts[M:] == -7).all()
    return rank[:M].long().cpu().numpy(), ts[:M].cpu().numpy()


def test_raw_topk_and_extra_workspace():
    c = case(300, 700, 2100, "tfidf")
    prof = helpers.word_profiles(c["hist"], c["A"])
    want = topk_reference(c["R"], 10)
    a = raw_topk(c, prof.bitmaps, 10)
    b = raw_topk(c, prof.bitmaps, 10, extra=1 << 20)
    check_lists(a, want)
    check_lists(b, want)


def _raw_filters(c, seed):
    M, Na = c["M"], c["Na"]
    rng = np.random.default_rng(seed)
    seen = [rng.integers(0, Na, rng.integers(0, 40)) for _ in range(M)]
    lo = rng.integers(0, Na, M).astype(np.int32)
    hi = np.minimum(lo + rng.integers(0, 400, M), Na).astype(np.int32)
    targets = rng.integers(-1, Na, M)
    xp, xi = helpers.normalize_exclusions(seen, M, Na)
    return seen, (lo, hi), targets, xp, xi


def test_raw_rank_and_extra_workspace():
    c = case(300, 700, 2100, "tfidf")
    prof = helpers.word_profiles(c["hist"], c["A"])
    seen, win, targets, xp, xi = _raw_filters(c, 11)
    for sn, w, lists, wins in ((None, None, (None, None), (None, None)), (seen, None, (xp, xi), (None, None)),
                               (None, win, (None, None), win), (seen, win, (xp, xi), win)):
        want = ranks_reference(c["R"], targets, sn, w)
        for extra in (0, 1 << 20):
            rank, ts = raw_rank(c, prof.bitmaps, targets, *lists, *wins, extra=extra)
            assert np.array_equal(rank, want[0]) and np.array_equal(_bits(ts), _bits(want[1]))


def test_raw_columns_out_of_range_are_dropped_by_every_kernel():
    """Columns outside [0, V): +0 from dae_word_entry_weights, passed over by the sweep's staging (top-k and rank), by the
    target's score and by the rank's fix-up -- the scores are those of the entries that are left."""
    c = case(129, 700, 1000, "tfidf")
    A, (h_ptr, h_items), M, Na, V = c["A"], c["hist"], c["M"], c["Na"], c["V"]
    cols = A.indices.astype(np.int64).copy()
    cols[::4] = V + (np.arange(cols[::4].size) % 7)
    cols[2::9] = -1 - (np.arange(cols[2::9].size) % 3)
    bitmaps, _ = raw_profiles(h_ptr, h_items, A.indptr, cols, Na, V, M)
    bad = (A.indptr, cols, A.data)
    R = scores_reference(profiles_reference(h_ptr, h_items, bad, V), bad, c["tw"])
    assert not np.array_equal(R, c["R"])
    seen, win, targets, xp, xi = _raw_filters(c, 12)
    check_lists(raw_topk(c, bitmaps, 10, cols=cols), topk_reference(R, 10))
    check_lists(raw_topk(c, bitmaps, 128, xp, xi, *win, cols=cols), topk_reference(R, 128, seen, win))
    for sn, lists, w, wins in ((None, (None, None), None, (None, None)), (seen, (xp, xi), win, win)):
        want = ranks_reference(R, targets, sn, w)
        rank, ts = raw_rank(c, bitmaps, targets, *lists, *wins, cols=cols)
        assert np.array_equal(rank, want[0]) and np.array_equal(_bits(ts), _bits(want[1]))


def filters_of(c):
    """seen lists and windows of the 129 x 700 case: user 3 sees its whole unfiltered top-10, user 4 everything, user 5 nothing;
    windows: empty (user 6), inside one tile (7), straddling the edge of tiles 0 and 1 (8), the whole corpus (9), random else."""
    M, Na = c["M"], c["Na"]
    rng = np.random.default_rng(5)
    top = topk_reference(c["R"], 10)[0]
    seen = [rng.integers(0, Na, rng.integers(0, 30)) for _ in range(M)]
    seen[3] = top[3][top[3] >= 0]
    seen[4] = np.arange(Na)
    seen[5] = np.zeros(0, dtype=np.int64)
    lo = rng.integers(0, Na, M)
    hi = np.minimum(lo + rng.integers(0, 300, M), Na)
    lo[6], hi[6] = 50, 50
    lo[7], hi[7] = 130, 200
    lo[8], hi[8] = 120, 135
    lo[9], hi[9] = 0, Na
    return seen, (lo, hi)


@pytest.mark.parametrize("kind", ["binary", "tfidf"])
def test_seen_lists_and_windows(kind):
    c = case(129, 700, 1000, kind)
    art = articles_of(c)
    seen, win = filters_of(c)
    for sn, w in ((seen, None), (None, win), (seen, win)):
        for k in (10, 128):
            got = helpers.word_recommend(c["hist"], art, k, seen=sn, term_weights=c["tw"], window=w)
            check_lists(got, topk_reference(c["R"], k, sn, w))
    idx, score = helpers.word_recommend(c["hist"], art, 10, seen=seen, term_weights=c["tw"])
    assert not np.isin(idx[3], seen[3]).any() and (idx[3] >= 0).all()    # excluded articles take none of the k slots
    assert (idx[4] == -1).all() and np.isneginf(score[4]).all()
    idx, score = helpers.word_recommend(c["hist"], art, 10, term_weights=c["tw"], window=win)
    assert (idx[6] == -1).all() and ((idx[7] >= 130) & (idx[7] < 200)).all() and ((idx[8] >= 120) & (idx[8] < 135)).all()


def test_integer_case_equals_most_similar():
    """Both routes are exact on co-occurrence counts, so this ties the kernel to the existing order without the new reference."""
    c = case(129, 700, 1000, "binary")
    seen, _ = filters_of(c)
    prof = helpers.word_profiles(c["hist"], articles_of(c))
    binary = sp.csr_matrix((np.ones(c["A"].nnz, dtype=F32), c["A"].indices, c["A"].indptr), shape=c["A"].shape)
    for sn in (None, seen):
        got = helpers.word_recommend(prof, articles_of(c), 10, seen=sn)
        want = helpers.most_similar(prof.to_scipy().astype(F32), 10, norm="", metric="linear kernel", candidates=binary, exclude=sn)
        check_lists(got, want)


@pytest.mark.parametrize("kind", ["binary", "tfidf"])
def test_ranks(kind):
    c = case(129, 700, 1000, kind)
    art = articles_of(c)
    M, Na, R = c["M"], c["Na"], c["R"]
    seen, win = filters_of(c)
    rng = np.random.default_rng(8)
    targets = rng.integers(0, Na, M)
    targets[0] = -1                                                      # no target
    targets[3] = seen[3][0]                                              # a target in the user's seen list: ranked all the same
    targets[7] = 150
    seen[7] = np.array([10, 150, 160, 650])                              # seen items inside and outside the window of user 7
    for sn, w in ((None, None), (seen, None), (None, win), (seen, win)):
        rank, ts, n_cand = helpers.word_ranks(c["hist"], art, targets, seen=sn, term_weights=c["tw"], window=w)
        want_rank, want_ts = ranks_reference(R, targets, sn, w)
        assert rank.dtype == np.int64 and n_cand.dtype == np.int64 and ts.dtype == F32
        assert np.array_equal(rank, want_rank) and np.array_equal(_bits(ts), _bits(want_ts))
        assert rank[0] == 0 and np.isneginf(ts[0]) and (rank[1:] >= 1).all()
        idx, score = helpers.word_recommend(c["hist"], art, 128, seen=sn, term_weights=c["tw"], window=w)
        for u in range(M):
            at = np.flatnonzero(idx[u] == targets[u]) if targets[u] >= 0 else np.zeros(0, dtype=np.int64)
            if at.size:                                                  # in the list: at position rank - 1 with that score, bit for bit
                assert rank[u] == at[0] + 1 and _bits(score[u, at[0]:at[0] + 1])[0] == _bits(ts[u:u + 1])[0]
            elif targets[u] >= 0 and (sn is None or targets[u] not in sn[u]) and (w is None or w[0][u] <= targets[u] < w[1][u]):
                assert rank[u] > 128
        m = helpers.rank_metrics(rank, n_cand, targets)
        assert m["n"] == M - 1 and (n_cand >= 0).all()
    assert helpers.word_ranks(c["hist"], art, targets, seen=seen, term_weights=c["tw"])[0][3] >= 1


def test_stability():
    c = case(300, 700, 2100, "tfidf")
    seen = [np.random.default_rng(u).integers(0, 700, 5) for u in range(300)]
    kw = dict(seen=seen, term_weights=c["tw"])
    first = helpers.word_recommend(c["hist"], c["A"], 10, **kw)
    check_lists(helpers.word_recommend(c["hist"], c["A"], 10, **kw), first)                            # run to run
    check_lists(helpers.word_recommend(c["hist"], c["A"], 10, batch_users=128, **kw), first)           # three batches against one
    targets = np.random.default_rng(3).integers(-1, 700, 300)
    r_first = helpers.word_ranks(c["hist"], c["A"], targets, **kw)
    r_batch = helpers.word_ranks(c["hist"], c["A"], targets, batch_users=128, **kw)
    assert np.array_equal(r_first[0], r_batch[0]) and np.array_equal(_bits(r_first[1]), _bits(r_batch[1]))
    perm = np.random.default_rng(4).permutation(300)                                                   # the users in another order
    hist_p = helpers.permute_histories(*c["hist"], perm)
    got = helpers.word_recommend(hist_p, c["A"], 10, seen=[seen[u] for u in perm], term_weights=c["tw"])
    check_lists(got, (first[0][perm], first[1][perm]))
    r_perm = helpers.word_ranks(hist_p, c["A"], targets[perm], seen=[seen[u] for u in perm], term_weights=c["tw"])
    assert np.array_equal(r_perm[0], r_first[0][perm]) and np.array_equal(_bits(r_perm[1]), _bits(r_first[1][perm]))


def test_idf_weights_and_tensors():
    import torch
    c = case(129, 129, 33, "tfidf")
    df = np.bincount(c["A"].indices, minlength=33)
    want = (np.log((1.0 + 129) / (1.0 + df)) + 1.0).astype(F32)
    assert np.array_equal(_bits(helpers.idf_weights(c["A"])), _bits(want))
    idx, score = helpers.word_recommend(c["hist"], c["A"], 5, term_weights=c["tw"], return_tensor=True)
    assert isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int64 and score.dtype == torch.float32
    check_lists((idx.cpu().numpy(), score.cpu().numpy()), topk_reference(c["R"], 5))


def test_cli_words(tmp_path, monkeypatch, capsys):
    """--words with --rank_metrics and --max_age at the smallest shape the CLI tests use: the two files with their keys, and the
    printed hit@5 equal to next_click_metrics on the saved lists."""
    import main_autoencoder as cli
    monkeypatch.chdir(tmp_path)
    cli.main(["--model_name", "words", "--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4", "--sessions",
              "synthetic", "--recommend", "5", "--words", "--rank_metrics", "--max_age", "48", "--similarity", "False"])
    out = capsys.readouterr().out
    lists = glob.glob(str(tmp_path / "**" / "article_encoded_recommend5_window_words.npz"), recursive=True)
    ranks = glob.glob(str(tmp_path / "**" / "article_encoded_ranks_window_words.npz"), recursive=True)
    assert len(lists) == 1 and len(ranks) == 1
    r, q = np.load(lists[0]), np.load(ranks[0])
    assert set(r.files) == {"indices", "scores", "targets", "hist_indptr", "hist_items", "profile_sizes"}
    assert set(q.files) == {"rank", "score", "n_candidates", "targets"}
    assert r["indices"].shape == r["scores"].shape == (200, 5) and r["indices"].dtype == np.int64 and q["rank"].shape == (200,)
    m = helpers.next_click_metrics(r["indices"], r["targets"])
    line = re.search(r"hit@5 word-based model +([0-9.]+)  MRR ([0-9.]+)  nDCG ([0-9.]+)", out)
    assert line and line.group(1) == "%.4f" % m["hit"] and line.group(2) == "%.4f" % m["mrr"]
    assert re.search(r"ranks word-based model +AUC [0-9.]+", out)
    hit = q["rank"][(q["targets"] >= 0)]
    assert abs(float(((hit > 0) & (hit <= 5)).mean()) - m["hit"]) < 1e-12    # the full ranks agree with the lists
