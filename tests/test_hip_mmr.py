"""GPU checks of the list diversification (dae_mmr_lists; helpers.diversify_lists, recommend_diverse, the CLI's --rec_mmr) against
tests/mmr_reference.py.

The bit contract leaves nothing out: on the library's OWN fp32 scores (pairwise_similarity) with float32 relevance and lambda, every
output of every row equals the reference bit for bit.  Against the oracle's float64 scores a selection can differ only where two
criteria lie close: a score carries the project's tolerance tol = 1e-5 x max |S| (test_hip_topk.py, test_hip_dedup.py), the
criterion lam * rel - (1 - lam) * m therefore (1 - lam) * tol plus three fp32 roundings of values of magnitude <= 1 (<= 2e-7), and a
gap between two criteria twice that: band = 2 (1 - lam) tol + 2e-6.  Rows with a gap inside the band (or a score within tol of a
finite threshold) are left out, and it is asserted on the oracle alone that they are at most 5 % of the rows.

Left-out rows as test_against_float64 prints them (of 256; plain / cap 2 / threshold), for lambda = 0, 0.3, 0.7, 1:
  ("", cosine, 48) and ("l2", linear kernel, 48):  1 2 1 / 2 2 2 / 1 1 1 / 2 0 2        ("", cosine, 200):  4 3 7 / 6 6 8 / 2 2 1 / 1 1 1
On every other row the kernel agreed with the float64 rule; the reference reorders all 256 rows for lambda < 1."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle as O
from dedup_reference import dedup_reference
from mmr_reference import mmr_reference, near_tie_rows_mmr
from test_hip_dedup import _abi as _abi_dedup
from test_hip_dedup import _cluster_lists, sessions_case  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NORM = {"": 0, "l1": 1, "l2": 2, "max": 3}
_METRIC = {"cosine": 0, "linear kernel": 1}
INF = float("inf")
_NAMES = ("out_idx", "out_pos", "out_val", "out_near", "counts")


def _abi(E, lists, rel, k, lam, norm="", metric="cosine", labels=None, cap=0, threshold=INF, ws_lists=None):
    """dae_mmr_lists through ctypes; ws_lists: the workspace holds the image and that many lists (None: the recommended size).
    Returns (out_idx, out_pos int64, out_val, out_near float32, counts int64); the output buffers are pre-filled with -7 and wider
    than k, the input tables wider than L."""
    from dae_rnn_news_recommendation_amd import _lib as L
    lib = L.load()
    Ed = torch.from_numpy(np.ascontiguousarray(E, dtype=np.float32)).cuda()
    Nr, Ll = np.shape(lists)
    ld = torch.full((Nr, Ll + 2), 3, dtype=torch.int32, device="cuda")
    ld[:, :Ll] = torch.from_numpy(np.ascontiguousarray(lists, dtype=np.int32)).cuda()
    rd = torch.full((Nr, Ll + 5), 9.0, dtype=torch.float32, device="cuda")
    rd[:, :Ll] = torch.from_numpy(np.ascontiguousarray(rel, dtype=np.float32)).cuda()
    lab = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    Na, D = Ed.shape
    ldo = k + 3
    oi = torch.full((Nr, ldo), -7, dtype=torch.int32, device="cuda")
    op = torch.full((Nr, ldo), -7, dtype=torch.int32, device="cuda")
    ov = torch.full((Nr, ldo), -7.0, dtype=torch.float32, device="cuda")
    on = torch.full((Nr, ldo), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((Nr, 2), -7, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.dae_mmr_lists_workspace(Nr if ws_lists is None else ws_lists, Na, D, Ll))
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    off = (-ws.data_ptr()) % 256
    rc = lib.dae_mmr_lists(L.ptr(Ed), Ed.stride(0), Na, D, _NORM[norm], _METRIC[metric], L.ptr(ld), ld.stride(0), L.ptr(rd), rd.stride(0),
                           L.ptr(lab), cap, Nr, Ll, k, float(lam), float(threshold), L.ptr(oi), L.ptr(op), L.ptr(ov), L.ptr(on), ldo,
                           L.ptr(cnt), ctypes.c_void_p(ws.data_ptr() + off), ws_bytes, L.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.dae_last_error()
    oi, op = oi.cpu().numpy().astype(np.int64), op.cpu().numpy().astype(np.int64)
    ov, on = ov.cpu().numpy(), on.cpu().numpy()
    for a in (oi, op, ov, on):
        assert (a[:, k:] == -7).all()                                          # nothing past k is written
    return oi[:, :k], op[:, :k], ov[:, :k], on[:, :k], cnt.cpu().numpy().astype(np.int64)


def _same(got, want, rows=None, what=""):
    """Every output equal, bit for bit (float32 compared as its bits)."""
    for g, w, name in zip(got, want, _NAMES):
        g, w = (g, w) if rows is None else (g[rows], w[rows])
        if g.dtype == np.float32:
            assert w.dtype == np.float32
            g, w = g.view(np.int32), w.view(np.int32)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (what, name, bad[:5], g[bad[:2]], w[bad[:2]])


def _s32(E, norm, metric):
    from dae_rnn_news_recommendation_amd import helpers
    S = helpers.pairwise_similarity(E, norm=norm, metric=metric, set_diagonal_zero=False, return_tensor=True).cpu().numpy()
    assert S.dtype == np.float32
    return S


def _spoil(rel, rng):
    """About 1 % each of NaN, +inf and -inf."""
    u = rng.random(rel.shape)
    rel = rel.copy()
    rel[u < 0.01] = np.nan
    rel[(u >= 0.01) & (u < 0.02)] = np.inf
    rel[(u >= 0.02) & (u < 0.03)] = -np.inf
    return rel


_RANDOM_CASES = [("", "cosine", 48), ("l2", "linear kernel", 48), ("", "cosine", 200)]
_LAMS = [0.0, 0.3, 0.7, 1.0]


@pytest.fixture(scope="module")
def random_cases():
    """Per case: 600 x D standard-normal rows (seed 0), 256 lists of 32 distinct articles (as test_hip_dedup.py draws them); the
    oracle's float64 scores and the library's own fp32 scores; per list the cosine of its articles to a random unit query as the
    relevance (float32, |rel| <= 1), the list sorted best first; labels 0..7 with some -1."""
    out = {}
    for norm, metric, D in _RANDOM_CASES:
        rng = np.random.default_rng(0)
        E = rng.standard_normal((600, D)).astype(np.float32)
        lists = np.stack([rng.permutation(600)[:32] for _ in range(256)])
        q = rng.standard_normal((256, D))
        En = E.astype(np.float64) / np.linalg.norm(E.astype(np.float64), axis=1, keepdims=True)
        rel = np.einsum("rld,rd->rl", En[lists], q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        order = np.argsort(-rel, axis=1, kind="stable")
        lists, rel = np.take_along_axis(lists, order, 1), np.take_along_axis(rel, order, 1)
        labels = rng.integers(-1, 8, 600)
        out[norm, metric, D] = dict(E=E, lists=lists, rel=rel, labels=labels, S32=_s32(E, norm, metric),
                                    S=O.pairwise_similarity(E, norm=norm, metric=metric, set_diagonal_zero=False))
    return out


@pytest.fixture(scope="module")
def clustered():
    """The clustered corpus of test_hip_dedup.py (600 x 48: 40 centres + 0.05 x noise) with its cluster numbers, about 5 % of them
    set to -1, as labels; the oracle's cosine matrix and the library's own."""
    rng = np.random.default_rng(11)
    cluster = rng.integers(0, 40, 600)
    E = (rng.standard_normal((40, 48))[cluster] + 0.05 * rng.standard_normal((600, 48))).astype(np.float32)
    S = O.pairwise_similarity(E, norm="", metric="cosine", set_diagonal_zero=False)
    same = cluster[:, None] == cluster[None, :]
    labels = np.where(np.random.default_rng(12).random(600) < 0.05, -1, cluster)
    return dict(E=E, S=S, S32=_s32(E, "", "cosine"), labels=labels, within=float(S[same].min()), across=float(S[~same].max()))


def _ragged_lists(L, seed, Nr=40):
    """_cluster_lists (repeats, about 3 % -1 and 3 % Na, an all-invalid row, a one-valid row, a short row) with a relevance per
    entry, about 3 % of them NaN / +inf / -inf."""
    lists = _cluster_lists(L, seed=seed, Nr=Nr)
    rng = np.random.default_rng(1000 + seed)
    return lists, _spoil(rng.standard_normal(lists.shape).astype(np.float32), rng)


# ---- 1. the bit contract: nothing left out ----

@pytest.mark.parametrize("lam", _LAMS)
@pytest.mark.parametrize("norm, metric, D", _RANDOM_CASES)
def test_bit_contract(random_cases, norm, metric, D, lam):
    c = random_cases[norm, metric, D]
    E, S32, lam32 = c["E"], c["S32"], np.float32(lam)
    if lam == 0.0:
        print("score tile bit-symmetric:", bool(np.array_equal(S32, S32.T)))
    rel = _spoil(np.random.default_rng(5).standard_normal(c["lists"].shape).astype(np.float32), np.random.default_rng(6))
    for k in (1, 10, 32):
        _same(_abi(E, c["lists"], rel, k, lam32, norm, metric), mmr_reference(c["lists"], rel, S32, k, lam32), what=("distinct", k))
    for L in (128, 100, 32, 7, 1):
        lists, rel = _ragged_lists(L, seed=L)
        for k in sorted({1, min(10, L), L}):
            got = _abi(E, lists, rel, k, lam32, norm, metric)
            _same(got, mmr_reference(lists, rel, S32, k, lam32), what=(L, k))
            assert got[4][-1].tolist() == [0, 0] and (got[0][-1] == -1).all() and np.isneginf(got[2][-1]).all()      # no valid entry


@pytest.mark.parametrize("lam", [0.3, 0.7, 1.0])
@pytest.mark.parametrize("cap, threshold", [(1, INF), (2, INF), (0, 0.8), (2, 0.8)])
def test_bit_contract_with_cap_and_threshold(clustered, random_cases, cap, threshold, lam):
    E, S32, labels, lam32 = clustered["E"], clustered["S32"], clustered["labels"], np.float32(lam)
    assert (labels == -1).sum() > 10
    for L, k in ((128, 10), (128, 128), (100, 10), (32, 32), (7, 7)):
        lists, rel = _ragged_lists(L, seed=L + 1)
        want = mmr_reference(lists, rel, S32, k, lam32, labels, cap, threshold)
        _same(_abi(E, lists, rel, k, lam32, labels=labels, cap=cap, threshold=threshold), want, what=(L, k))
    # random scores: a threshold that IS one of the library's scores (>= against >), and the labels of the random corpus
    c = random_cases["", "cosine", 48]
    T = np.float32(c["S32"][c["lists"][0, 0], c["lists"][0, 1]])
    for t in (T, np.nextafter(T, np.float32(np.inf)), np.float32(0.3)):
        _same(_abi(c["E"], c["lists"], c["rel"], 10, lam32, labels=c["labels"], cap=cap, threshold=float(t)),
              mmr_reference(c["lists"], c["rel"], c["S32"], 10, lam32, c["labels"], cap, t), what=("random", float(t)))


# ---- 2. against float64 ----

@pytest.mark.parametrize("lam", _LAMS)
@pytest.mark.parametrize("norm, metric, D", _RANDOM_CASES)
def test_against_float64(random_cases, norm, metric, D, lam):
    c = random_cases[norm, metric, D]
    E, S, lists, rel, labels = c["E"], c["S"], c["lists"], c["rel"], c["labels"]
    assert np.abs(rel).max() <= 1.0
    k, lam32 = 10, np.float32(lam)
    tol = 1e-5 * np.abs(S).max()
    band = 2 * (1 - lam) * tol + 2e-6
    moved_any = False
    for cap, threshold in ((0, INF), (2, INF), (0, 0.3 if D == 48 else 0.15)):
        kw = dict(labels=labels, max_per_label=cap, threshold=threshold)
        out = near_tie_rows_mmr(lists, rel, S, k, float(lam32), band, tol=tol, **kw)
        want = mmr_reference(lists, rel, S, k, float(lam32), **kw)
        moved = (want[1] != np.arange(k)).any(axis=1)
        print(f"cap {cap} threshold {threshold}: {int(out.sum())} of 256 rows left out (tol {tol:.3g}, band {band:.3g}); the reference "
              f"moves an entry in {int(moved.sum())} rows, {int((want[4][:, 0] < k).sum())} rows end short of {k}")
        assert out.sum() <= 0.05 * 256                                         # on the oracle alone
        if lam < 1 and cap == 0 and threshold == INF:
            assert moved.mean() > 0.5                                          # the rule bites
            moved_any = True
        got = _abi(E, lists, rel, k, lam32, norm, metric, labels=labels, cap=cap, threshold=threshold)
        keep = ~out
        assert np.array_equal(got[0][keep], want[0][keep]) and np.array_equal(got[1][keep], want[1][keep])
        assert np.array_equal(got[4][keep], want[4][keep])
        sel = want[1][keep] >= 0
        for g, w in ((got[2], want[2]), (got[3], want[3])):
            assert np.array_equal(np.isneginf(g[keep]), ~sel)
            assert np.abs(g[keep][sel] - w[keep][sel]).max() <= band
    assert moved_any or lam == 1


# ---- 3. properties ----

def test_lambda_one_is_the_first_k_valid_entries(clustered):
    E = clustered["E"]
    for L in (128, 100, 7):
        lists = _cluster_lists(L, seed=L + 2, Nr=40)
        rel = np.tile(-np.arange(L, dtype=np.float32), (40, 1))                # best first
        for k in sorted({1, min(10, L), L}):
            oi, op, ov, on, cnt = _abi(E, lists, rel, k, 1.0)
            for i in range(40):
                v = np.flatnonzero((lists[i] >= 0) & (lists[i] < 600))[:k]
                assert op[i, :v.size].tolist() == v.tolist() and (op[i, v.size:] == -1).all()
                assert oi[i, :v.size].tolist() == lists[i, v].tolist() and cnt[i].tolist() == [v.size, 0]
                assert np.array_equal(ov[i, :v.size], rel[i, v])


@pytest.mark.parametrize("L", [128, 32])
def test_lambda_one_with_a_threshold_is_dedup_lists(clustered, L):
    E = clustered["E"]
    print(f"min within-cluster cosine {clustered['within']:.4f}, max across-cluster cosine {clustered['across']:.4f}")
    assert clustered["within"] > 0.99 and clustered["across"] < 0.6            # on the oracle alone: no decision near 0.8
    lists = _cluster_lists(L, seed=L)
    rel = np.tile(-np.arange(L, dtype=np.float32), (lists.shape[0], 1))
    for k in (10, L):
        d_idx, d_pos, d_cnt = _abi_dedup(E, lists, k, 0.8)
        oi, op, _, _, cnt = _abi(E, lists, rel, k, 1.0, threshold=0.8)
        assert np.array_equal(oi, d_idx) and np.array_equal(op, d_pos) and np.array_equal(cnt[:, 0], d_cnt[:, 0])
        assert np.array_equal(oi, dedup_reference(lists, clustered["S"], k, 0.8)[0])
        assert (cnt[:, 0] < k).any()


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_cap_holds_and_rows_end_short_where_the_reference_says(clustered, cap):
    E, S32, labels = clustered["E"], clustered["S32"], clustered["labels"]
    lists, rel = _ragged_lists(32, seed=77, Nr=120)
    k, lam32 = 32, np.float32(0.7)
    oi, op, _, _, cnt = _abi(E, lists, rel, k, lam32, labels=labels, cap=cap)
    want = mmr_reference(lists, rel, S32, k, lam32, labels, cap)
    for i in range(lists.shape[0]):
        lab = labels[oi[i][oi[i] >= 0]]
        lab = lab[lab >= 0]
        assert lab.size == 0 or np.bincount(lab).max() <= cap
    assert np.array_equal(cnt[:, 0] < k, want[4][:, 0] < k) and np.array_equal(cnt, want[4])
    valid = ((lists >= 0) & (lists < 600) & np.isfinite(rel)).sum(axis=1)
    assert (cnt[:, 0] < np.minimum(valid, k)).any()                            # the cap itself ended rows, not the pool


# ---- 4. chunking ----

def test_chunking_does_not_change_the_result(random_cases, clustered):
    c = random_cases["", "cosine", 200]
    lists, rel = c["lists"][:10].copy(), c["rel"][:10].copy()
    lists[3, 5] = -1
    lists[7, 20:] = -1
    rel[2, 4] = np.nan
    kw = dict(labels=c["labels"], cap=3, threshold=0.2)
    whole = _abi(c["E"], lists, rel, 10, np.float32(0.7), **kw)
    _same(_abi(c["E"], lists, rel, 10, np.float32(0.7), **kw), whole)           # run to run
    for n in (3, 1):                                                           # chunks of 3 + 3 + 3 + 1 lists; of one list
        _same(_abi(c["E"], lists, rel, 10, np.float32(0.7), ws_lists=n, **kw), whole)
    big, big_rel = np.tile(lists, (30, 1)), np.tile(rel, (30, 1))              # 300 lists at 7 per chunk
    _same(_abi(c["E"], big, big_rel, 10, np.float32(0.7), ws_lists=7, **kw), tuple(np.tile(a, (30, 1)) for a in whole))
    _same(whole, mmr_reference(lists, rel, c["S32"], 10, np.float32(0.7), c["labels"], 3, np.float32(0.2)))


# ---- 5. the helpers ----

def test_helper_matches_the_abi(clustered):
    from dae_rnn_news_recommendation_amd import helpers
    E, labels = clustered["E"], clustered["labels"]
    lists, rel = _ragged_lists(32, seed=1, Nr=60)
    oi, op, ov, on, cnt = _abi(E, lists, rel, 10, 0.7, labels=labels, cap=2, threshold=0.8)
    idx, sc, d = helpers.diversify_lists(lists, rel, E, 10, 0.7, labels=labels, max_per_label=2, dedup_threshold=0.8, return_details=True)
    assert idx.dtype == np.int64 and sc.dtype == np.float32 and idx.shape == sc.shape == (60, 10)
    assert np.array_equal(idx, oi) and np.array_equal(d["positions"], op) and np.array_equal(d["n_selected"], cnt[:, 0])
    assert np.array_equal(d["n_beyond_topk"], cnt[:, 1]) and d["n_selected"].dtype == np.int64
    assert np.array_equal(d["value"].view(np.int32), ov.view(np.int32)) and np.array_equal(d["nearest"].view(np.int32), on.view(np.int32))
    assert np.array_equal(d["relevance_used"].view(np.int32), rel.view(np.int32))
    want_sc = np.where(op >= 0, np.take_along_axis(rel, np.maximum(op, 0), axis=1), -np.inf).astype(np.float32)
    assert np.array_equal(sc, want_sc)
    assert len(helpers.diversify_lists(lists, rel, E, 10, 0.7)) == 2
    t = helpers.diversify_lists(torch.from_numpy(lists).cuda(), torch.from_numpy(rel).cuda(), torch.from_numpy(E).cuda(), 10, 0.7,
                                labels=torch.from_numpy(labels).cuda(), max_per_label=2, dedup_threshold=0.8, return_details=True,
                                return_tensor=True)
    assert t[0].is_cuda and t[0].dtype == torch.int64 and t[1].is_cuda and t[2]["nearest"].is_cuda
    assert np.array_equal(t[0].cpu().numpy(), oi) and np.array_equal(t[1].cpu().numpy(), want_sc)
    assert np.array_equal(t[2]["n_beyond_topk"].cpu().numpy(), cnt[:, 1])


def test_helper_minmax_scaling(clustered):
    from dae_rnn_news_recommendation_amd import helpers
    E, S32 = clustered["E"], clustered["S32"]
    lists, rel = _ragged_lists(32, seed=3, Nr=60)
    rel = (rel * np.float32(37.5) + np.float32(11)).astype(np.float32)          # unbounded, as an inner product is
    rel[5] = np.where(np.isfinite(rel[5]), np.float32(2.5), rel[5])            # a row with max == min
    idx, sc, d = helpers.diversify_lists(lists, rel, E, 10, 0.7, scale_relevance="minmax", return_details=True)
    used = d["relevance_used"]
    ok = (lists >= 0) & (lists < 600) & np.isfinite(rel)
    lo = np.where(ok, rel, np.inf).min(axis=1, keepdims=True).astype(np.float32)
    hi = np.where(ok, rel, -np.inf).max(axis=1, keepdims=True).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(hi == lo, np.float32(1), (rel - lo) / (hi - lo)).astype(np.float32)
    assert used.dtype == np.float32 and used.shape == rel.shape
    assert (np.abs(used[ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32).astype(np.int64)) <= 1).all()      # 1 ulp
    assert used[ok].min() >= 0 and used[ok].max() <= 1 and (used[5][ok[5]] == 1).all()
    assert np.array_equal(used[~ok].view(np.int32), rel[~ok].view(np.int32))   # invalid entries as they came
    ref = mmr_reference(lists, used, S32, 10, np.float32(0.7))
    assert np.array_equal(idx, ref[0]) and np.array_equal(d["positions"], ref[1])
    assert np.array_equal(d["value"].view(np.int32), ref[2].view(np.int32))
    want_sc = np.where(ref[1] >= 0, np.take_along_axis(rel, np.maximum(ref[1], 0), axis=1), -np.inf).astype(np.float32)
    assert np.array_equal(sc, want_sc)                                         # the caller's own relevance comes back


def test_recommend_diverse_and_the_old_calls_unchanged(sessions_case):
    from dae_rnn_news_recommendation_amd import helpers
    E, hist, states, S = sessions_case
    k, pool = 10, 40
    rng = np.random.default_rng(5)
    lo = rng.integers(0, 400, 300)
    hi = lo + rng.integers(0, 200, 300)
    hi[0] = lo[0]                                                              # an empty window
    before = (helpers.recommend(states, E, k=pool, seen=hist), helpers.recommend(states, E, k=k, seen=hist, window=(lo, hi)),
              helpers.most_similar(E, 5), helpers.recommend(states, E, k=k, seen=hist, dedup_threshold=0.9))
    labels = np.concatenate([np.repeat(np.arange(30), 15), np.full(150, -1)])
    S32 = _s32(E, "", "cosine")
    idx40, sc40 = before[0]
    idx, sc, d = helpers.recommend_diverse(states, E, k=k, seen=hist, lam=0.6, pool=pool, labels=labels, max_per_label=2,
                                           return_details=True)
    assert idx.shape == sc.shape == (300, k) and idx.dtype == np.int64 and sc.dtype == np.float32
    want = mmr_reference(idx40, d["relevance_used"], S32, k, np.float32(0.6), labels, 2)
    assert np.array_equal(idx, want[0]) and np.array_equal(d["positions"], want[1]) and np.array_equal(d["n_beyond_topk"], want[4][:, 1])
    assert np.array_equal(sc, np.where(want[1] >= 0, np.take_along_axis(sc40, np.maximum(want[1], 0), axis=1), -np.inf).astype(np.float32))
    assert d["relevance_used"].min() >= 0 and d["relevance_used"].max() <= 1 and d["n_beyond_topk"].sum() > 0
    for u in range(300):
        v = idx[u][idx[u] >= 0]
        assert not np.isin(v, hist[u]).any()                                   # no seen article
        lab = labels[v][labels[v] >= 0]
        assert lab.size == 0 or np.bincount(lab).max() <= 2
    # the default pool is min(128, 4 k); without details two items
    again = helpers.recommend_diverse(states, E, k=k, seen=hist, lam=0.6, labels=labels, max_per_label=2)
    assert len(again) == 2 and np.array_equal(again[0], idx)
    div = helpers.list_diversity(idx, d["nearest"], labels)
    plain = helpers.diversify_lists(idx40, sc40, E, k, 1.0, return_details=True)
    assert div["mean_nearest"] < helpers.list_diversity(plain[0], plain[2]["nearest"])["mean_nearest"]
    # inside windows: an empty window gives -1 / -inf
    w_idx, w_sc = helpers.recommend_diverse(states, E, k=k, seen=hist, window=(lo, hi), pool=pool)
    inside = (w_idx >= lo[:, None]) & (w_idx < hi[:, None])
    assert (inside | (w_idx == -1)).all() and inside.any() and (w_idx[0] == -1).all() and np.isneginf(w_sc[0]).all()
    assert np.array_equal(w_sc == -np.inf, w_idx == -1)
    # recommend and most_similar return what they did before any new call
    after = (helpers.recommend(states, E, k=pool, seen=hist), helpers.recommend(states, E, k=k, seen=hist, window=(lo, hi)),
             helpers.most_similar(E, 5), helpers.recommend(states, E, k=k, seen=hist, dedup_threshold=0.9))
    for x, y in zip(before, after):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.int32), y[1].view(np.int32))


# ---- 6. the CLI ----

def test_cli_rec_mmr(tmp_path, monkeypatch, capsys):
    """--rec_mmr 0.7 --rec_max_per_label 3 in a fresh child process: the _mmr.npz with its six arrays, no list over the cap, the
    "after" nearest similarity at or below "before".  The run without the flags (in this process, same arguments): the same files
    but that one, and the same printed lines but the MMR block."""
    import main_autoencoder as cli
    args = ["--model_name", "rec", "--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4",
            "--sessions", "synthetic", "--recommend", "10", "--similarity", "False"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    child = tmp_path / "with"
    child.mkdir()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "main_autoencoder.py")] + args + ["--rec_mmr", "0.7", "--rec_max_per_label", "3"],
                         cwd=str(child), env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    found = glob.glob(str(child / "**" / "article_encoded_recommend10_mmr.npz"), recursive=True)
    assert len(found) == 1
    d = os.path.dirname(found[0])
    r = np.load(found[0])
    assert set(r.files) == {"indices", "scores", "targets", "n_selected", "n_beyond_topk", "nearest"}
    assert r["indices"].shape == r["scores"].shape == r["nearest"].shape == (200, 10)
    assert r["n_selected"].shape == r["n_beyond_topk"].shape == r["targets"].shape == (200,)
    assert r["indices"].dtype == np.int64 and r["scores"].dtype == r["nearest"].dtype == np.float32
    assert r["n_selected"].dtype == r["n_beyond_topk"].dtype == np.int64
    assert np.array_equal(r["n_selected"], (r["indices"] >= 0).sum(axis=1)) and (r["n_selected"] >= 1).all()
    plain = np.load(os.path.join(d, "article_encoded_recommend10.npz"))
    assert np.array_equal(plain["targets"], r["targets"]) and np.array_equal(plain["indices"][:, 0], r["indices"][:, 0])
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_labels
    labels = np.unique(synthetic_labels(400, kind="category", seed=4), return_inverse=True)[1]
    for row in r["indices"]:
        assert np.bincount(labels[row[row >= 0]]).max() <= 3                   # no list exceeds the cap
    m = re.search(r"nearest similarity in a list: before ([0-9.-]+)  after ([0-9.-]+)", run.stdout)
    assert m and float(m.group(2)) <= float(m.group(1))
    assert run.stdout.count("hit@10") == 4 and "mmr user state" in run.stdout
    # without the flags
    other = tmp_path / "without"
    other.mkdir()
    monkeypatch.chdir(other)
    model = cli.main(args)
    out = capsys.readouterr().out
    assert "mmr" not in out and out.count("hit@10") == 2
    names = lambda top: sorted(os.path.relpath(os.path.join(b, f), top) for b, _, fs in os.walk(top) for f in fs)
    with_flag, without = names(str(child)), names(str(other))
    assert [n for n in with_flag if not n.endswith("_mmr.npz")] == without and len(with_flag) == len(without) + 1
    shape = lambda text: [re.sub(r"\d[\d.eE+-]*", "#", l) for l in text.splitlines()]      # a line with its numbers blanked
    lines, block, keep = shape(run.stdout), False, []
    for l in lines:                                                            # cut the MMR block out of the child's output
        block = block or l.startswith("calculate recommend # mmr #")
        if not block:
            keep.append(l)
        block = block and not l.startswith("calculate recommend # mmr done")
    assert keep == shape(out) and len(lines) == len(keep) + 7
    assert np.array_equal(np.load(model.data_dir + "article_encoded_recommend10.npz")["targets"], plain["targets"])
