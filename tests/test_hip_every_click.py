"""The shared stamped exclusion lists on the GPU (dae_topk_similarity_seq, dae_rank_similarity_seq; helpers.most_similar /
target_ranks(exclude_shared=...)) and the every-click protocol on top of them.  The yardstick of every kernel case is the existing
_win / _ex path given, per row, the materialised list {item : stamp <= limit} -- compared bit for bit, no tolerance anywhere -- and,
on integer-valued data whose products are exact in fp32, a float64 NumPy brute force with the (score desc, index asc) order."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [0, 1, 2, 5, 40, 33, 17, 29, 38, 3, 36, 40]      # 244 event rows: two query tiles, the second partial; user 8 holds rows 127..164
NC, H = 300, 24                                          # three corpus tiles, the last partial; H padded to 128
PLANTED = [0, 127, 128, 255, 256, 299]                   # list items on the tile edges
I32MAX = np.iinfo(np.int32).max


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _materialise(lp, li, ls, row_list, row_limit):
    """Per query row the list the stamped form means: {item : stamp <= limit} of the row's list, nothing for a row without one."""
    out = []
    for u, lim in zip(row_list.tolist(), row_limit.tolist()):
        if 0 <= u < lp.size - 1:
            a, b = lp[u], lp[u + 1]
            out.append(li[a:b][ls[a:b] <= lim].astype(np.int64))
        else:
            out.append(np.zeros(0, dtype=np.int64))
    return out


def _windows(rng, n, tgt):
    lo = rng.integers(0, NC, n)
    near = (rng.random(n) < 0.7) & (tgt >= 0)                                       # most targets inside their window
    lo[near] = np.maximum(tgt[near] - rng.integers(0, 100, n)[near], 0)
    hi = np.minimum(lo + np.where(near, 100, 0) + rng.integers(0, 150, n), NC)
    lo[:6], hi[:6] = [0, 128, 299, 120, 0, 250], [300, 256, 300, 130, 0, 300]      # everything, one tile, one column, an edge, empty
    return lo, hi


@pytest.fixture(scope="module")
def base():
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(11)
    hist = []
    for n in LENS:
        pool = np.union1d(rng.choice(NC, 30, replace=False), PLANTED)
        h = rng.choice(pool, n)                                                    # a small pool: repeated clicks
        if n >= 17:
            h[rng.choice(n, len(PLANTED), replace=False)] = PLANTED                # every planted column is clicked, some twice
        hist.append(h.astype(np.int64))
    nnz = sum(LENS)
    assert nnz == 244 and sum(LENS[:8]) < 128 < sum(LENS[:9])
    assert sum(len(h) - len(set(h.tolist())) for h in hist) > 40                   # stamp = FIRST occurrence matters
    lp, li, ls = helpers.click_prefix_lists(hist)
    rows = helpers.every_click_rows(hist)
    # the event rows, some of them without a list or with a limit below every stamp
    rl, rm = rows["row_list"].copy(), rows["row_limit"].copy()
    rl[rng.choice(nnz, 12, replace=False)] = -1
    rl[rng.choice(nnz, 6, replace=False)] = len(LENS) + 5
    rm[rng.choice(nnz, 12, replace=False)] = -1
    tgt = rows["targets"].copy()
    # 300 generic rows for the case where the corpus is in_df itself (exclude_self): any row may read any list
    rl300 = rng.integers(0, len(LENS), NC).astype(np.int32)
    rl300[rng.random(NC) < 0.1] = -1
    rm300 = rng.integers(-1, 41, NC).astype(np.int32)
    tgt300 = rng.integers(-1, NC, NC)
    for i in range(0, NC, 5):                                                      # targets from the row's own list, and the row itself
        u = rl300[i]
        if u >= 0 and lp[u + 1] > lp[u]:
            tgt300[i] = li[rng.integers(lp[u], lp[u + 1])]
    tgt300[40:46] = np.arange(40, 46)
    tgt300[50:56] = -1
    for i, c in enumerate(PLANTED):                                                # a row that is itself a listed column
        rl300[c], rm300[c] = 4 + i % 2, 40
    return dict(hist=hist, lists=(lp, li, ls), rl=rl, rm=rm, tgt=tgt, win=_windows(rng, nnz, tgt), rl300=rl300, rm300=rm300,
                tgt300=tgt300, win300=_windows(rng, NC, tgt300), rows=rows)


def _with_vectors(base, kind):
    rng = np.random.default_rng(12)
    if kind == "ints":                                                             # massive ties: the index order decides
        E = rng.integers(-2, 3, (40, H)).astype(np.float32)[rng.integers(0, 40, NC)]
        S = rng.integers(-2, 3, (sum(LENS), H)).astype(np.float32)
    else:
        E = rng.standard_normal((NC, H)).astype(np.float32)
        S = rng.standard_normal((sum(LENS), H)).astype(np.float32)
    return dict(base, E=E, S=S)


@pytest.fixture(scope="module", params=["ints", "real"])
def data(request, base):
    return _with_vectors(base, request.param)


def _cases(d):
    """The four combinations: (queries against the corpus | the corpus against itself, exclude_self) x (no windows | windows)."""
    lp, li, ls = d["lists"]
    for self_corpus in (False, True):
        Q, rl, rm, tgt, win = ((d["E"], d["rl300"], d["rm300"], d["tgt300"], d["win300"]) if self_corpus
                               else (d["S"], d["rl"], d["rm"], d["tgt"], d["win"]))
        for w in (None, win):
            yield dict(Q=Q, kw=dict(metric="linear kernel", candidates=None if self_corpus else d["E"], window=w), tgt=tgt, win=w,
                       shared=((lp, li), ls, rl, rm), lists=_materialise(lp, li, ls, rl, rm), self_corpus=self_corpus)


@pytest.mark.parametrize("k", [1, 10, 128])
def test_topk_equals_the_windowed_kernel_given_the_materialised_lists(data, k):
    from dae_rnn_news_recommendation_amd import helpers
    changed = 0
    for c in _cases(data):
        got = helpers.most_similar(c["Q"], k=k, exclude_shared=c["shared"], **c["kw"])
        want = helpers.most_similar(c["Q"], k=k, exclude=c["lists"], **c["kw"])
        assert np.array_equal(got[0], want[0]) and np.array_equal(_u32(got[1]), _u32(want[1])), (c["self_corpus"], c["win"] is None)
        plain = helpers.most_similar(c["Q"], k=k, **c["kw"])
        changed += int((plain[0] != got[0]).any(axis=1).sum())
    assert changed >= 20                                                           # the lists did remove candidates


def test_rank_equals_the_windowed_kernel_given_the_materialised_lists(data):
    from dae_rnn_news_recommendation_amd import helpers
    changed = 0
    for c in _cases(data):
        got = helpers.target_ranks(c["Q"], c["tgt"], exclude_shared=c["shared"], **c["kw"])
        want = helpers.target_ranks(c["Q"], c["tgt"], exclude=c["lists"], **c["kw"])
        assert np.array_equal(got[0], want[0]) and np.array_equal(_u32(got[1]), _u32(want[1])) and np.array_equal(got[2], want[2]), \
            (c["self_corpus"], c["win"] is None)
        plain = helpers.target_ranks(c["Q"], c["tgt"], **c["kw"])
        changed += int((plain[0] != got[0]).sum())
        assert (got[0] > 0).sum() >= 60
    assert changed >= 40


def _truth(c):
    """float64 scores with -inf wherever row i may not return column j, and the plain scores."""
    Q = c["Q"].astype(np.float64)
    C = Q if c["kw"]["candidates"] is None else c["kw"]["candidates"].astype(np.float64)
    S = Q @ C.T
    R = S.copy()
    if c["win"] is not None:
        cols = np.arange(S.shape[1])[None, :]
        R[(cols < c["win"][0][:, None]) | (cols >= c["win"][1][:, None])] = -np.inf
    for i, x in enumerate(c["lists"]):
        R[i, x] = -np.inf
    if c["self_corpus"]:
        np.fill_diagonal(R, -np.inf)
    return S, R


def test_exact_truth_on_integer_valued_data(base):
    """Every product is exactly representable: indices, scores and ranks equal the float64 brute force with the order (score
    descending, index ascending), bit for bit."""
    from dae_rnn_news_recommendation_amd import helpers
    data = _with_vectors(base, "ints")
    for c in _cases(data):
        S, R = _truth(c)
        for k in (10, 128):
            idx, sc = helpers.most_similar(c["Q"], k=k, exclude_shared=c["shared"], **c["kw"])
            want = np.argsort(-R, axis=1, kind="stable")[:, :k]
            ws = np.take_along_axis(R, want, 1)
            assert np.array_equal(idx, np.where(np.isneginf(ws), -1, want)) and np.array_equal(sc, ws.astype(np.float32))
        rank, score, _ = helpers.target_ranks(c["Q"], c["tgt"], exclude_shared=c["shared"], **c["kw"])
        n_ranked = n_barred = 0
        for i, t in enumerate(c["tgt"].tolist()):
            if t < 0:
                assert rank[i] == 0 and np.isneginf(score[i])
                continue
            assert score[i] == S[i, t]
            if np.isneginf(R[i, t]):                                               # seen by then, outside the window, or the row itself
                assert rank[i] == 0
                n_barred += 1
                continue
            row = R[i]
            assert rank[i] == 1 + int(((row > S[i, t]) | ((row == S[i, t]) & (np.arange(row.size) < t))).sum()), i
            n_ranked += 1
        assert n_ranked >= 60 and n_barred >= 5


@pytest.fixture(scope="module")
def six_forms():
    """One small problem for all six (EXCL, WIN, SEQ) forms of both kernels: 130 query rows (two query tiles, the second with 2
    rows), 300 candidates (three corpus tiles, the last partial), 24 features, integers in [-3, 3] -- every fp32 product sum is
    exact, so the float64 brute force is the truth bit for bit.  17 shared stamped lists of 0..40 items; per row the list it reads
    (-1 and 17: none) and a limit, and the same content as per-row lists of 0..40 items."""
    rng = np.random.default_rng(21)
    Nq, Nc, D, n_lists = 130, 300, 24, 17
    Q = rng.integers(-3, 4, (Nq, D)).astype(np.float32)
    E = rng.integers(-3, 4, (Nc, D)).astype(np.float32)
    sizes = rng.integers(0, 41, n_lists)
    sizes[:3] = [0, 40, 1]
    items = [np.sort(rng.choice(Nc, n, replace=False)) for n in sizes]
    items[1][[0, -1]] = [0, 299]                                                    # the corpus' first and last column are listed
    stamps = [rng.permutation(n) for n in sizes]
    rl = rng.integers(0, n_lists, Nq)
    rl[[3, 64, 129]], rl[[5, 128]] = -1, n_lists                                   # no list, on either side of [0, n_lists)
    rm = rng.integers(-1, 41, Nq)
    rl[[0, 127]], rm[[0, 127]] = 1, 40                                             # the whole 40-item list, in both query tiles
    rl[7] = 0                                                                      # an empty list
    lists = _materialise(np.concatenate([[0], np.cumsum(sizes)]), np.concatenate(items), np.concatenate(stamps), rl, rm)
    assert {0, 40} <= {len(x) for x in lists} and max(len(x) for x in lists) == 40
    tgt = rng.integers(0, Nc, Nq)
    tgt[::9] = -1
    for i in range(1, Nq, 6):                                                      # targets from the row's own list
        if len(lists[i]):
            tgt[i] = lists[i][rng.integers(len(lists[i]))]
    lo = rng.integers(0, Nc, Nq)
    hi = np.minimum(lo + rng.integers(1, 200, Nq), Nc)
    near = (rng.random(Nq) < 0.7) & (tgt >= 0)                                      # most targets inside their window
    lo[near] = np.maximum(tgt[near] - rng.integers(0, 100, Nq)[near], 0)
    hi[near] = np.minimum(tgt[near] + 1 + rng.integers(0, 100, Nq)[near], Nc)
    lo[:5], hi[:5] = [0, 50, 0, 140, 260], [300, 50, 120, 290, 300]                # all, empty, misses tiles 1-2, ends inside the last tile, inside it
    lo[128:], hi[128:] = [0, 256], [128, 300]                                      # exactly the first tile, and only the last
    S = Q.astype(np.float64) @ E.astype(np.float64).T
    cols = np.arange(Nc)[None, :]
    listed, outside = np.zeros((Nq, Nc), dtype=bool), (cols < lo[:, None]) | (cols >= hi[:, None])
    for i, x in enumerate(lists):
        listed[i, x] = True
    return dict(Q=Q, E=E, S=S, tgt=tgt, lists=lists, shared=((items, stamps, rl, rm)), win=(lo, hi), listed=listed, outside=outside)


def _six_forms(d):
    """(name, arguments of most_similar / target_ranks, the columns a row may not return) per form; the two SEQ forms last."""
    for win in (False, True):
        w, out = (d["win"], d["outside"]) if win else (None, np.zeros_like(d["outside"]))
        yield f"<false, {win}>", dict(window=w), out
        yield f"<true, {win}>", dict(window=w, exclude=d["lists"]), out | d["listed"]
        yield f"<true, {win}, true>", dict(window=w, exclude_shared=d["shared"]), out | d["listed"]


@pytest.mark.parametrize("k", [1, 128])
def test_six_forms_topk_equals_the_brute_force(six_forms, k):
    from dae_rnn_news_recommendation_amd import helpers
    d, per_row = six_forms, None
    for name, kw, barred in _six_forms(d):
        R = np.where(barred, -np.inf, d["S"])
        want = np.argsort(-R, axis=1, kind="stable")[:, :k]                         # score descending, ties by index ascending
        ws = np.take_along_axis(R, want, 1)
        idx, sc = helpers.most_similar(d["Q"], k=k, metric="linear kernel", norm="", candidates=d["E"], **kw)
        assert np.array_equal(idx, np.where(np.isneginf(ws), -1, want)), name
        assert np.array_equal(_u32(sc), _u32(ws.astype(np.float32))), name
        if "exclude" in kw:
            per_row = (idx, sc)
        elif "exclude_shared" in kw:                                                # the per-row and the shared form of one filter
            assert np.array_equal(idx, per_row[0]) and np.array_equal(_u32(sc), _u32(per_row[1])), name


def test_six_forms_rank_equals_the_brute_force(six_forms):
    from dae_rnn_news_recommendation_amd import helpers
    d, per_row = six_forms, None
    tgt, S = d["tgt"], d["S"]
    has = tgt >= 0
    st = S[np.arange(tgt.size), np.maximum(tgt, 0)]
    ahead = (S > st[:, None]) | ((S == st[:, None]) & (np.arange(S.shape[1])[None, :] < tgt[:, None]))
    for name, kw, barred in _six_forms(d):
        ok = has & ~barred[np.arange(tgt.size), np.maximum(tgt, 0)]                 # the target itself may be returned
        want = np.where(ok, 1 + (ahead & ~barred).sum(axis=1), 0)
        rank, score, _ = helpers.target_ranks(d["Q"], tgt, metric="linear kernel", norm="", candidates=d["E"], **kw)
        assert np.array_equal(rank, want), name
        assert np.array_equal(_u32(score), _u32(np.where(has, st, -np.inf).astype(np.float32))), name
        assert ok.sum() >= 40 and (not barred.any() or (has & ~ok).sum() >= 5), name          # ranked targets, and barred ones
        if "exclude" in kw:
            per_row = (rank, score)
        elif "exclude_shared" in kw:
            assert np.array_equal(rank, per_row[0]) and np.array_equal(_u32(score), _u32(per_row[1])), name


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(fn, Q, E, k, lists, win, tgt=None):
    """One call of dae_{topk,rank}_similarity_{seq,win} through ctypes on device copies.  ``lists``: the five device arrays of the
    stamped form and n_lists, or None for five NULL pointers (seq) / no per-row lists (win)."""
    from dae_rnn_news_recommendation_amd import _lib as L
    lib = L.load()
    Nq, D = Q.shape
    Nc = E.shape[0]
    lo, hi = (None, None) if win is None else win
    n_lists = 0 if lists is None else lists[5]
    lp = [None] * 5 if lists is None else [L.ptr(x) for x in lists[:5]]
    head = [L.ptr(Q), Q.stride(0), Nq, L.ptr(E), E.stride(0), Nc, D, 0, 1]
    mid = lp[:3] + [n_lists] + lp[3:] if fn == "seq" else [None, None]
    if tgt is None:
        idx = torch.empty((Nq, k), dtype=torch.int32, device="cuda")
        sc = torch.empty((Nq, k), dtype=torch.float32, device="cuda")
        nbytes = int(getattr(lib, f"dae_topk_similarity_{fn}_workspace")(Nq, Nc, D, k))
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
        wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
        L.call(f"dae_topk_similarity_{fn}", *head, k, 0, *mid, L.ptr(lo), L.ptr(hi), L.ptr(idx), L.ptr(sc), k, wp, nbytes, L.current_stream())
    else:
        idx = torch.empty(Nq, dtype=torch.int32, device="cuda")
        sc = torch.empty(Nq, dtype=torch.float32, device="cuda")
        nbytes = int(getattr(lib, f"dae_rank_similarity_{fn}_workspace")(Nq, Nc, D))
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
        wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
        L.call(f"dae_rank_similarity_{fn}", *head, 0, *mid, L.ptr(lo), L.ptr(hi), L.ptr(tgt), L.ptr(idx), L.ptr(sc), wp, nbytes,
               L.current_stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), _u32(sc.cpu().numpy())


def test_degenerate_forms(data):
    from dae_rnn_news_recommendation_amd import helpers
    lp, li, ls = data["lists"]
    S, E, tgt, win, rl, rm = (data[n] for n in ("S", "E", "tgt", "win", "rl", "rm"))
    n = S.shape[0]
    Sd, Ed = _dev(S), _dev(E)
    td = _dev(np.where(tgt >= 0, tgt, -1).astype(np.int32))
    wd = (_dev(win[0].astype(np.int32)), _dev(win[1].astype(np.int32)))
    none = (_dev(lp), _dev(li), _dev(ls), _dev(np.full(n, -1, np.int32)), _dev(rm), len(LENS))
    below = (_dev(lp), _dev(li), _dev(ls), _dev(rl), _dev(np.full(n, -1, np.int32)), len(LENS))
    for w in (None, wd):
        for k, t in ((10, None), (128, None), (0, td)):
            want = _raw("win", Sd, Ed, k, None, w, t)
            for name, lists in (("all list pointers NULL", None), ("every row_list -1", none), ("every row_limit -1", below)):
                got = _raw("seq", Sd, Ed, k, lists, w, t)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, k, w is None)
    # row_limit = INT32_MAX: every row is barred from its user's whole list, which is the _ex call given that list per row
    users = data["rows"]["row_list"]
    full = [li[lp[u]:lp[u + 1]] for u in users]
    shared = ((lp, li), ls, users, np.full(n, I32MAX))
    for w in (None, win):
        a = helpers.most_similar(S, k=10, metric="linear kernel", candidates=E, exclude_shared=shared, window=w)
        b = helpers.most_similar(S, k=10, metric="linear kernel", candidates=E, exclude=full, window=w)
        assert np.array_equal(a[0], b[0]) and np.array_equal(_u32(a[1]), _u32(b[1]))
        a = helpers.target_ranks(S, tgt, metric="linear kernel", candidates=E, exclude_shared=shared, window=w)
        b = helpers.target_ranks(S, tgt, metric="linear kernel", candidates=E, exclude=full, window=w)
        assert all(np.array_equal(_u32(x) if x.dtype == np.float32 else x, _u32(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


def test_determinism_row_order_and_chunking(data):
    from dae_rnn_news_recommendation_amd import helpers
    lp, li, ls = data["lists"]
    S, E, tgt, win, rl, rm, hist = (data[n] for n in ("S", "E", "tgt", "win", "rl", "rm", "hist"))
    kw = dict(metric="linear kernel", candidates=E)
    perm = np.random.default_rng(13).permutation(S.shape[0])
    for w in (None, win):
        a = helpers.most_similar(S, k=10, exclude_shared=((lp, li), ls, rl, rm), window=w, **kw)
        b = helpers.most_similar(S, k=10, exclude_shared=((lp, li), ls, rl, rm), window=w, **kw)
        c = helpers.most_similar(S[perm], k=10, exclude_shared=((lp, li), ls, rl[perm], rm[perm]),
                                 window=None if w is None else (w[0][perm], w[1][perm]), **kw)
        for x in (b, (np.empty_like(c[0]), np.empty_like(c[1]))):
            if x is not b:
                x[0][perm], x[1][perm] = c[0], c[1]                                # put the shuffled rows back
            assert np.array_equal(a[0], x[0]) and np.array_equal(_u32(a[1]), _u32(x[1]))
        a = helpers.target_ranks(S, tgt, exclude_shared=((lp, li), ls, rl, rm), window=w, **kw)
        b = helpers.target_ranks(S, tgt, exclude_shared=((lp, li), ls, rl, rm), window=w, **kw)
        c = helpers.target_ranks(S[perm], tgt[perm], exclude_shared=((lp, li), ls, rl[perm], rm[perm]),
                                 window=None if w is None else (w[0][perm], w[1][perm]), **kw)
        back = tuple(np.empty_like(x) for x in c)
        for x, y in zip(back, c):
            x[perm] = y
        for x in (b, back):
            assert np.array_equal(a[0], x[0]) and np.array_equal(_u32(a[1]), _u32(x[1])) and np.array_equal(a[2], x[2])
        # the every-click sweeps in chunks of 100 rows against one chunk
        one = helpers.recommend_every_click(S, E, hist, k=10, window=w)
        many = helpers.recommend_every_click(torch.from_numpy(S).cuda(), E, hist, k=10, window=w, batch_rows=100)
        assert np.array_equal(one[0], many[0]) and np.array_equal(_u32(one[1]), _u32(many[1])) and np.array_equal(one[2], many[2])
        one = helpers.recommend_ranks_every_click(S, E, hist, window=w)
        many = helpers.recommend_ranks_every_click(S, E, hist, window=w, batch_rows=100)
        assert np.array_equal(one[0], many[0]) and np.array_equal(_u32(one[1]), _u32(many[1])) and np.array_equal(one[2], many[2])
        assert np.array_equal(one[3], data["rows"]["targets"]) and (one[0] > 0).sum() >= 60


def _gru_model(rng, h):
    from dae_rnn_news_recommendation_amd.helpers import GRUUserModel
    return GRUUserModel(*(rng.uniform(-0.3, 0.3, s).astype(np.float32) for s in ((3 * h, h), (3 * h, h), (3 * h,), (3 * h,))))


@pytest.mark.parametrize("model", ["decay", "gru"])
def test_the_second_to_last_row_is_the_last_click_protocol(base, model):
    """For every user with at least two events, the every-click row of the second-to-last event -- the state that predicts the last
    click -- equals the existing last-click protocol bit for bit: recommend / recommend_ranks on the states of the history without
    its last click, with seen = that history.  dae_user_states and dae_gru_user_states promise the state equality this rests on."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(14)
    E = rng.standard_normal((NC, H)).astype(np.float32)
    hist, win = base["hist"], base["win"]
    cut = [h[:-1] for h in hist]
    users = np.array([u for u, h in enumerate(hist) if len(h) >= 2])
    rows = np.cumsum(LENS)[users] - 2
    last = np.array([hist[u][-1] for u in users])
    if model == "decay":
        every = helpers.user_states(hist, E, 0.8, all_states=True, return_tensor=True)
        final = helpers.user_states(cut, E, 0.8, return_tensor=True)
    else:
        gru = _gru_model(rng, H)
        every = helpers.gru_user_states(hist, E, gru, all_states=True, return_tensor=True)
        final = helpers.gru_user_states(cut, E, gru, return_tensor=True)
    assert np.array_equal(_u32(every[torch.from_numpy(rows).cuda()].cpu().numpy()), _u32(final[torch.from_numpy(users).cuda()].cpu().numpy()))
    for w in (None, win):
        wu = None if w is None else (np.zeros(len(hist), dtype=np.int64), np.zeros(len(hist), dtype=np.int64))
        if w is not None:
            wu[0][users], wu[1][users] = w[0][rows], w[1][rows]
        idx, sc, tg = helpers.recommend_every_click(every, E, hist, k=10, window=w)
        idx0, sc0 = helpers.recommend(final, E, k=10, seen=cut, window=wu)
        assert np.array_equal(tg[rows], last)
        assert np.array_equal(idx[rows], idx0[users]) and np.array_equal(_u32(sc[rows]), _u32(sc0[users]))
        rank, rsc, nc, _ = helpers.recommend_ranks_every_click(every, E, hist, window=w)
        t0 = np.full(len(hist), -1)
        t0[users] = last
        rank0, rsc0, nc0 = helpers.recommend_ranks(final, E, t0, seen=cut, window=wu)
        assert np.array_equal(rank[rows], rank0[users]) and np.array_equal(_u32(rsc[rows]), _u32(rsc0[users]))
        assert np.array_equal(nc[rows], nc0[users])
        if w is None:
            assert (rank[rows] > 0).sum() >= 2 and (rank[rows] == 0).sum() >= 1       # ranked ones, and re-clicks of a seen article


def test_evaluate_every_click_batches_users_without_changing_a_bit(base):
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(15)
    E = rng.standard_normal((NC, H)).astype(np.float32)
    hist, win = base["hist"], base["win"]
    t = np.concatenate([np.sort(rng.random(len(h)) * 50) for h in hist])
    fitted = helpers.UserModel(rng.uniform(0.5, 1.5, H), 0.7, 2.0, np.zeros(0))
    for model, kw in ((0.8, dict()), (0.8, dict(timestamps=t, time_unit=3.0, window=win)), (fitted, dict(timestamps=t)),
                      (_gru_model(rng, H), dict(window=win))):
        whole = helpers.evaluate_every_click(hist, E, model, ks=(1, 10), **kw)
        parts = helpers.evaluate_every_click(hist, E, model, ks=(1, 10), batch_users=5, **kw)
        for name in ("rank", "n_candidates", "targets", "positions"):
            assert np.array_equal(whole[name], parts[name]), name
        assert np.array_equal(_u32(whole["score"]), _u32(parts["score"]))
        assert whole["metrics"] == helpers.rank_metrics(whole["rank"], whole["n_candidates"], whole["targets"], ks=(1, 10))
        assert whole["metrics"]["n"] == sum(n - 1 for n in LENS if n) and np.array_equal(whole["positions"], base["rows"]["positions"])
    # the fitted model's alpha and time unit are applied the way UserModel.states applies them
    S = helpers.user_states(hist, E, fitted.beta, timestamps=t, time_unit=fitted.time_unit, all_states=True, return_tensor=True)
    S = S * torch.from_numpy(fitted.alpha.astype(np.float32)).cuda()
    rank, score, _, _ = helpers.recommend_ranks_every_click(S, E, hist)
    got = helpers.evaluate_every_click(hist, E, fitted, timestamps=t)
    assert np.array_equal(got["rank"], rank) and np.array_equal(_u32(got["score"]), _u32(score))


def test_fit_gru_user_model_validation():
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(16)
    h, na = 8, 50
    E = rng.standard_normal((na, h)).astype(np.float32)
    hist = [rng.integers(0, na, rng.integers(2, 13)) for _ in range(40)]
    val = [rng.integers(0, na, rng.integers(2, 13)) for _ in range(12)]
    kw = dict(epochs=3, batch_users=16, seed=5, lr=0.05)
    plain = helpers.fit_gru_user_model(hist, E, **kw)
    seen = helpers.fit_gru_user_model(hist, E, validation=val, **kw)
    assert plain.validation is None and len(seen.validation) == 3 and [m["epoch"] for m in seen.validation] == [1, 2, 3]
    for name in helpers.GRUUserModel.NAMES:                                        # the validation pass touched nothing
        assert np.array_equal(_u32(getattr(plain, name)), _u32(getattr(seen, name))), name
    assert np.array_equal(plain.history, seen.history)
    want = helpers.evaluate_every_click(val, E, seen)["metrics"]
    assert {k: v for k, v in seen.validation[-1].items() if k != "epoch"} == want and want["n"] == sum(len(v) - 1 for v in val)
    best = helpers.fit_gru_user_model(hist, E, validation=val, keep_best=True, **kw)
    mrr = [m["mrr"] for m in best.validation]
    assert mrr == [m["mrr"] for m in seen.validation]
    fresh = helpers.fit_gru_user_model(hist, E, **dict(kw, epochs=int(np.argmax(mrr)) + 1))
    for name in helpers.GRUUserModel.NAMES:
        assert np.array_equal(_u32(getattr(best, name)), _u32(getattr(fresh, name))), name
    second = helpers.fit_gru_user_model(hist, E, validation=val, validation_every=2, **kw)
    assert [m["epoch"] for m in second.validation] == [2] and second.validation[0]["mrr"] == mrr[1]


LINE = (r"every click %s\s+AUC ([0-9.]+|nan)\s+MRR ([0-9.]+)\s+mean rank ([0-9.]+)\s+median rank ([0-9.]+)\s+hit@1 ([0-9.]+)\s+"
        r"hit@10 ([0-9.]+)\s+hit@100 ([0-9.]+)")


def _check_line(out, name, arrays):
    from dae_rnn_news_recommendation_amd import helpers
    m = helpers.rank_metrics(arrays["rank"], arrays["n_candidates"], arrays["targets"], ks=(1, 10, 100))
    line = re.search(LINE % name, out)
    assert [line.group(i) for i in range(1, 8)] == ["%.4f" % m["auc"], "%.4f" % m["mrr"], "%.1f" % m["mean_rank"], "%.1f" % m["median_rank"],
                                                     "%.4f" % m["hit@1"], "%.4f" % m["hit@10"], "%.4f" % m["hit@100"]]
    return m


def test_cli_every_click(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    common = ["--model_name", "ec", "--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4",
              "--sessions", "synthetic", "--recommend", "5", "--rank_metrics", "--similarity", "False"]
    outs, dirs = [], []
    for i, extra in enumerate(([], ["--every_click"])):
        os.makedirs(tmp_path / str(i))
        monkeypatch.chdir(tmp_path / str(i))
        dirs.append(os.path.abspath(cli.main(common + extra).data_dir) + os.sep)
        outs.append(capsys.readouterr().out)
    # the last-click evaluation is what it was: the same files with the same contents, the same lines
    for name in ("article_encoded_recommend5.npz", "article_encoded_ranks.npz"):
        a, b = np.load(dirs[0] + name), np.load(dirs[1] + name)
        assert a.files == b.files and all(np.array_equal(a[f], b[f]) for f in a.files), name
    assert not os.path.exists(dirs[0] + "article_encoded_every_click.npz")
    keep = lambda out: [ln for ln in out.splitlines() if ln.startswith(("  ", "calculate")) and "every click" not in ln
                        and "every_click" not in ln and not ln.startswith(("  seen ", "  MRR by clicks seen"))]
    assert keep(outs[0]) == keep(outs[1]) and "calculate every click" not in outs[0]
    out = outs[1]
    ec = np.load(dirs[1] + "article_encoded_every_click.npz")
    assert sorted(ec.files) == ["n_candidates", "positions", "rank", "score", "targets"]
    users = 200
    clicks = ec["rank"].shape[0]
    m = _check_line(out, "decayed user state", ec)
    assert m["n"] == clicks - users and ("%d users, %d clicks, %d with a next click" % (users, clicks, m["n"])) in out
    assert re.search(LINE % "most clicked unseen", out) and "MRR by clicks seen" in out
    table = re.findall(r"^  seen (\S+)\s+n\s+(\d+)\s+([0-9.]+|nan)\s+([0-9.]+|nan)$", out, flags=re.M)
    by = helpers.rank_metrics_by_position(ec["rank"], ec["n_candidates"], ec["targets"], ec["positions"])
    assert [r[0] for r in table] == ["1", "2", "3-4", "5-9", "10-19", "20-49", "50+"]
    assert [int(r[1]) for r in table] == [b["n"] for b in by] and sum(int(r[1]) for r in table) == m["n"]
    assert [r[2] for r in table] == ["%.4f" % b["mrr"] for b in by]
    # --max_age, the GRU model fitted with held-out users
    os.makedirs(tmp_path / "w")
    monkeypatch.chdir(tmp_path / "w")
    d = cli.main(common[:-3] + ["--similarity", "False", "--max_age", "48", "--every_click", "--user_model", "gru", "--fit_gru",
                                "--gru_epochs", "2", "--gru_validation", "0.25"]).data_dir
    d = os.path.abspath(d) + os.sep
    out = capsys.readouterr().out
    assert len(re.findall(r"fit epoch \d: validation MRR [0-9.]+  hit@10 [0-9.]+  \(\d+ clicks of \d+ held-out users\)", out)) == 2
    for tag, name in (("", "decayed user state"), ("_gru", "gru user state")):
        ec = np.load(d + "article_encoded_every_click%s_window.npz" % tag)
        _check_line(out, name, ec)
        assert ec["rank"].shape == (clicks,) and (ec["n_candidates"] <= 400).all()
    assert not os.path.exists(d + "article_encoded_every_click.npz") and os.path.exists(d + "article_encoded_recommend5_window.npz")
