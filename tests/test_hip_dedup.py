"""GPU checks of the list de-duplication (dae_dedup_lists; helpers.dedup_lists, recommend(dedup_threshold=), the CLI's
--rec_dedup) against the float64 greedy of tests/dedup_reference.py on the oracle's scores.

A decision of the kernel is an fp32 compare s(p, q) >= T, so it can differ from float64 only where a score lies within the
project's tolerance tol = 1e-5 x max |S| (test_hip_topk.py, test_hip_near_dup.py) of T.  The clustered case has no such pair
(asserted on the oracle alone) and is compared exactly, every row; the random cases leave out the rows with a pair in the band
and assert, on the oracle alone, that those are at most 2 % of the rows.  The bit contract (the decisions are those of the
library's OWN fp32 scores, dae_pairwise_similarity) leaves nothing out."""
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
from dedup_reference import dedup_reference, near_tie_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NORM = {"": 0, "l1": 1, "l2": 2, "max": 3}
_METRIC = {"cosine": 0, "linear kernel": 1}


def _abi(E, lists, k, threshold, norm="", metric="cosine", ws_lists=None):
    """dae_dedup_lists through ctypes; ws_lists: the workspace holds the image and that many lists (None: the recommended size).
    Returns (out_idx, out_pos, counts) as int64 ndarrays; the output buffers are pre-filled with -7 and wider than k."""
    from dae_rnn_news_recommendation_amd import _lib as L
    lib = L.load()
    Ed = torch.from_numpy(np.ascontiguousarray(E, dtype=np.float32)).cuda()
    ld = torch.from_numpy(np.ascontiguousarray(lists, dtype=np.int32)).cuda()
    Nr, Ll = ld.shape
    Na, D = Ed.shape
    ldo = k + 3
    oi = torch.full((Nr, ldo), -7, dtype=torch.int32, device="cuda")
    op = torch.full((Nr, ldo), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((Nr, 2), -7, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.dae_dedup_lists_workspace(Nr if ws_lists is None else ws_lists, Na, D, Ll))
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    off = (-ws.data_ptr()) % 256
    rc = lib.dae_dedup_lists(L.ptr(Ed), Ed.stride(0), Na, D, _NORM[norm], _METRIC[metric], L.ptr(ld), ld.stride(0), Nr, Ll, k, threshold,
                             L.ptr(oi), L.ptr(op), ldo, L.ptr(cnt), ctypes.c_void_p(ws.data_ptr() + off), ws_bytes, L.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.dae_last_error()
    oi, op = oi.cpu().numpy().astype(np.int64), op.cpu().numpy().astype(np.int64)
    assert (oi[:, k:] == -7).all() and (op[:, k:] == -7).all()                 # nothing past k is written
    return oi[:, :k], op[:, :k], cnt.cpu().numpy().astype(np.int64)


def _same(got, want, rows=None):
    for g, w, what in zip(got, want, ("out_idx", "out_pos", "counts")):
        g, w = (g, w) if rows is None else (g[rows], w[rows])
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (what, bad[:5], g[bad[:2]], w[bad[:2]])


# ---- 1. clear margins: exact equality, every row ----

@pytest.fixture(scope="module")
def clustered():
    """600 x 48: 40 cluster centres ~ N(0, I), rows = centre + 0.05 x noise; the oracle's cosine matrix (float64)."""
    rng = np.random.default_rng(11)
    cluster = rng.integers(0, 40, 600)
    E = (rng.standard_normal((40, 48))[cluster] + 0.05 * rng.standard_normal((600, 48))).astype(np.float32)
    S = O.pairwise_similarity(E, norm="", metric="cosine", set_diagonal_zero=False)
    same = cluster[:, None] == cluster[None, :]
    return E, S, float(S[same].min()), float(S[~same].max())


def _cluster_lists(L, seed, Na=600, Nr=300):
    """Nr lists of L entries drawn with repeats (so with many same-cluster pairs), about 3 % set to -1 and 3 % to Na; the last
    rows hold no valid entry, one valid entry, and a short list with a -1 tail."""
    rng = np.random.default_rng(seed)
    lists = rng.integers(0, Na, (Nr, L))
    u = rng.random((Nr, L))
    lists[u < 0.03] = -1
    lists[u > 0.97] = Na
    lists[-1] = -1
    lists[-2] = -1
    lists[-2, L // 2] = 5
    lists[-3, max(L // 3, 1):] = -1
    return lists


@pytest.mark.parametrize("L", [128, 100, 32, 7])
def test_clear_margins_exact(clustered, L):
    E, S, min_within, max_across = clustered
    T = 0.8
    tol = 1e-5 * np.abs(S).max()
    print(f"min within-cluster cosine {min_within:.4f}, max across-cluster cosine {max_across:.4f}")
    assert min_within > 0.99 and max_across < 0.6                              # the gap, on the oracle alone: no decision near T
    assert min_within > T + 100 * tol and max_across < T - 100 * tol
    lists = _cluster_lists(L, seed=L)
    for k in sorted({1, min(10, L), L}):
        want = dedup_reference(lists, S, k, T)
        assert (want[2][:-3, 0] >= 1).all()
        if k > 1:
            assert want[2][:, 1].max() > 0
            assert (want[0][:, -1] == -1).any() and (k == L or (want[0][:, -1] >= 0).any())     # short rows, and (k < L) full ones
        _same(_abi(E, lists, k, T), want)
    assert _abi(E, lists, L, T)[2][-1].tolist() == [0, 0]                      # the row without a valid entry


def test_helper_matches_the_abi_and_gathers_scores(clustered):
    from dae_rnn_news_recommendation_amd import helpers
    E, S, _, _ = clustered
    lists = _cluster_lists(32, seed=1)
    rel = np.random.default_rng(2).standard_normal(lists.shape).astype(np.float32)
    oi, op, cnt = _abi(E, lists, 10, 0.8)
    idx, sc, (n_kept, n_dup) = helpers.dedup_lists(lists, E, 10, 0.8, scores=rel, return_counts=True)
    assert idx.dtype == np.int64 and sc.dtype == np.float32 and n_kept.dtype == np.int64 and idx.shape == sc.shape == (300, 10)
    assert np.array_equal(idx, oi) and np.array_equal(n_kept, cnt[:, 0]) and np.array_equal(n_dup, cnt[:, 1])
    want_sc = np.where(op >= 0, np.take_along_axis(rel, np.maximum(op, 0), axis=1), -np.inf).astype(np.float32)
    assert np.array_equal(sc, want_sc)
    t = helpers.dedup_lists(torch.from_numpy(lists).cuda(), torch.from_numpy(E).cuda(), 10, 0.8, return_tensor=True)
    assert t[0].is_cuda and t[0].dtype == torch.int64 and t[1] is None and np.array_equal(t[0].cpu().numpy(), oi)
    again = helpers.dedup_lists(idx, E, 10, 0.8, return_counts=True)          # a de-duplicated list holds no duplicate pair
    assert np.array_equal(again[0], idx) and again[2][1].sum() == 0


# ---- 2. random scores: the near-tie rule; 3. the bit contract ----

_RANDOM_CASES = [("", "cosine", 48), ("l2", "linear kernel", 48), ("", "cosine", 200)]


@pytest.fixture(scope="module")
def random_cases():
    """Per case: 600 x D standard-normal rows (seed 0), the oracle's float64 scores, 256 lists of 32 distinct articles."""
    out = {}
    for norm, metric, D in _RANDOM_CASES:
        rng = np.random.default_rng(0)
        E = rng.standard_normal((600, D)).astype(np.float32)
        lists = np.stack([rng.permutation(600)[:32] for _ in range(256)])
        out[norm, metric, D] = E, O.pairwise_similarity(E, norm=norm, metric=metric, set_diagonal_zero=False), lists
    return out


# (The cosine of two random rows spreads about 1 / sqrt(D): 0.3 is 2.1 standard deviations at D = 48 and drops an entry per row,
#  but 4.2 at D = 200, where it drops nothing; so that case also runs at 0.15, the same 2.1 standard deviations.)
@pytest.mark.parametrize("norm, metric, D, T", [c + (0.3,) for c in _RANDOM_CASES] + [("", "cosine", 200, 0.15)])
def test_random_scores_near_tie_rule(random_cases, norm, metric, D, T):
    E, S, lists = random_cases[norm, metric, D]
    k = 10
    tol = 1e-5 * np.abs(S).max()
    out = near_tie_rows(lists, S, T, tol)
    want = dedup_reference(lists, S, k, T)
    dropped = float(np.mean(want[1].max(axis=1) + 1 - want[2][:, 0]))            # entries skipped before the walk ended
    print(f"{int(out.sum())} of 256 rows left out (tol {tol:.3g}); the reference drops {dropped:.2f} entries per row, "
          f"{int((want[2][:, 0] < k).sum())} rows end short of {k}")
    assert out.sum() <= 0.02 * 256                                             # on the oracle alone
    assert (D == 200 and T == 0.3) or dropped > 0.5                            # the threshold bites
    _same(_abi(E, lists, k, T, norm, metric), want, rows=~out)


@pytest.mark.parametrize("norm, metric, D", _RANDOM_CASES)
def test_bit_contract_with_pairwise_similarity(random_cases, norm, metric, D):
    """Nothing left out: the decisions are those of the library's own fp32 scores, pairwise_similarity[list[p], list[q]] >= T in
    fp32 -- for a T that IS one of those scores, at positions (1, 0) of a row, where >= against > decides whether position 1 stays
    (position 0 is always kept)."""
    from dae_rnn_news_recommendation_amd import helpers
    E, _, lists = random_cases[norm, metric, D]
    k = 10
    S32 = helpers.pairwise_similarity(E, norm=norm, metric=metric, set_diagonal_zero=False, return_tensor=True).cpu().numpy()
    assert S32.dtype == np.float32
    first = S32[lists[:, 1], lists[:, 0]]
    r = int(np.argmin(np.abs(first - 0.3)))
    T = np.float32(first[r])
    got = _abi(E, lists, k, float(T), norm, metric)
    _same(got, dedup_reference(lists, S32, k, T))
    assert got[1][r, 0] == 0 and got[1][r, 1] != 1                             # a pair AT the threshold is a duplicate
    above = np.nextafter(T, np.float32(np.inf))
    got = _abi(E, lists, k, float(above), norm, metric)
    _same(got, dedup_reference(lists, S32, k, above))
    assert got[1][r, 1] == 1
    _same(_abi(E, lists, k, 0.3, norm, metric), dedup_reference(lists, S32, k, np.float32(0.3)))


# ---- 4. chunking ----

def test_chunking_does_not_change_the_result(random_cases):
    E, _, lists = random_cases["", "cosine", 200]
    lists = lists[:10].copy()
    lists[3, 5] = -1
    lists[7, 20:] = -1
    whole = _abi(E, lists, 10, 0.3)
    _same(_abi(E, lists, 10, 0.3), whole)                                      # run to run
    for n in (3, 1):                                                           # chunks of 3 + 3 + 3 + 1 lists; of one list
        _same(_abi(E, lists, 10, 0.3, ws_lists=n), whole)
    big = np.tile(lists, (30, 1))                                              # more lists than workgroup slots per chunk of 7
    _same(_abi(E, big, 10, 0.3, ws_lists=7), tuple(np.tile(a, (30, 1)) for a in whole))


# ---- 5. through recommend ----

@pytest.fixture(scope="module")
def sessions_case():
    """600 articles in D = 32: 450 in 30 classes (class centre + noise), then 150 noisy copies of earlier ones (cosine ~ 0.999);
    300 users with synthetic sessions, the last click held out; the decayed user states."""
    from dae_rnn_news_recommendation_amd import helpers
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
    rng = np.random.default_rng(3)
    labels = np.repeat(np.arange(30), 15)
    E = (rng.standard_normal((30, 32))[labels] + rng.standard_normal((450, 32))).astype(np.float32)
    src = rng.integers(0, 450, 150)
    E = np.vstack([E, E[src] + 0.02 * rng.standard_normal((150, 32)).astype(np.float32)])
    labels = np.concatenate([labels, labels[src]])
    indptr, items = synthetic_sessions(300, labels, mean_len=12, seed=2)
    hist = [items[indptr[u]:max(indptr[u + 1] - 1, indptr[u])] for u in range(300)]
    states = helpers.user_states(hist, E, 0.9, return_tensor=True)
    S = O.pairwise_similarity(E, norm="", metric="cosine", set_diagonal_zero=False)
    return E, hist, states, S


def test_recommend_with_dedup(sessions_case):
    from dae_rnn_news_recommendation_amd import helpers
    E, hist, states, S = sessions_case
    T, k, pool = 0.9, 10, 40
    tol = 1e-5 * np.abs(S).max()
    idx40, sc40 = helpers.recommend(states, E, k=pool, seen=hist)
    idx, sc = helpers.recommend(states, E, k=k, seen=hist, dedup_threshold=T, dedup_pool=pool)
    assert idx.shape == sc.shape == (300, k) and idx.dtype == np.int64 and sc.dtype == np.float32
    out = near_tie_rows(idx40, S, T, tol)
    assert out.sum() <= 0.02 * 300
    want_idx, want_pos, want_cnt = dedup_reference(idx40, S, k, T)
    print(f"{int(out.sum())} rows left out; duplicate pairs in the plain top-{k}: {want_cnt[:, 1].mean():.2f} per list")
    assert want_cnt[:, 1].mean() > 0.5                                         # the plain lists do show copies
    assert np.array_equal(idx[~out], want_idx[~out])
    want_sc = np.where(want_pos >= 0, np.take_along_axis(sc40, np.maximum(want_pos, 0), axis=1), -np.inf).astype(np.float32)
    assert np.array_equal(sc[~out], want_sc[~out])
    for u in range(300):
        v = idx[u][idx[u] >= 0]
        assert np.tril(S[np.ix_(v, v)] >= T + tol, -1).sum() == 0              # no kept pair is a duplicate
        assert not np.isin(v, hist[u]).any()                                   # no seen article
    # the default pool is min(128, 4 k)
    d_idx, _ = helpers.recommend(states, E, k=k, seen=hist, dedup_threshold=T)
    assert np.array_equal(d_idx, idx)
    # most_similar takes the same keywords, in self mode too
    m_idx, m_sc = helpers.most_similar(states, k, metric="linear kernel", candidates=E, exclude=hist, dedup_threshold=T, dedup_pool=pool)
    assert np.array_equal(m_idx, idx) and np.array_equal(m_sc, sc)
    s_idx, _ = helpers.most_similar(E, 5, dedup_threshold=T, dedup_pool=20)
    want = dedup_reference(helpers.most_similar(E, 20)[0], S, 5, T)[0]
    near = near_tie_rows(helpers.most_similar(E, 20)[0], S, T, tol)
    assert near.sum() <= 0.02 * 600 and np.array_equal(s_idx[~near], want[~near])


def test_recommend_with_dedup_inside_windows_and_default_unchanged(sessions_case):
    from dae_rnn_news_recommendation_amd import helpers
    E, hist, states, S = sessions_case
    rng = np.random.default_rng(5)
    lo = rng.integers(0, 400, 300)
    hi = lo + rng.integers(0, 200, 300)                                        # some windows are shorter than the pool,
    hi[0] = lo[0]                                                              # one is empty
    idx, sc = helpers.recommend(states, E, k=10, seen=hist, window=(lo, hi), dedup_threshold=0.9, dedup_pool=40)
    inside = (idx >= lo[:, None]) & (idx < hi[:, None])
    assert (inside | (idx == -1)).all() and inside.any() and (idx == -1).any()
    assert np.array_equal(sc == -np.inf, idx == -1)
    for u in range(300):
        assert not np.isin(idx[u][idx[u] >= 0], hist[u]).any()
    # dedup_threshold=None: the arrays of the call as it was
    a = helpers.recommend(states, E, k=10, seen=hist, window=(lo, hi))
    b = helpers.recommend(states, E, k=10, seen=hist, window=(lo, hi), dedup_threshold=None, dedup_pool=40)
    c = helpers.most_similar(states, 10, metric="linear kernel", candidates=E, exclude=hist, window=(lo, hi))
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)


# ---- 6. the CLI ----

def test_cli_rec_dedup(tmp_path, monkeypatch, capsys):
    """--rec_dedup in a fresh child process: the _dedup.npz with its five arrays, an "after" count of 0.  The run without the flag
    (in this process, same arguments): the same files but that one, and the same printed lines but the de-dup block."""
    import main_autoencoder as cli
    args = ["--model_name", "rec", "--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4",
            "--sessions", "synthetic", "--recommend", "10", "--similarity", "False"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    child = tmp_path / "with"
    child.mkdir()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "main_autoencoder.py")] + args + ["--rec_dedup", "0.9"], cwd=str(child), env=env,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    found = glob.glob(str(child / "**" / "article_encoded_recommend10_dedup.npz"), recursive=True)
    assert len(found) == 1
    d = os.path.dirname(found[0])
    r = np.load(found[0])
    assert set(r.files) == {"indices", "scores", "targets", "n_kept", "dup_pairs_before"}
    assert r["indices"].shape == r["scores"].shape == (200, 10) and r["n_kept"].shape == r["dup_pairs_before"].shape == (200,)
    assert r["indices"].dtype == np.int64 and r["scores"].dtype == np.float32
    assert np.array_equal(r["n_kept"], (r["indices"] >= 0).sum(axis=1)) and (r["n_kept"] >= 1).all()
    plain = np.load(os.path.join(d, "article_encoded_recommend10.npz"))
    assert np.array_equal(plain["targets"], r["targets"]) and np.array_equal(plain["indices"][:, 0], r["indices"][:, 0])
    m = re.search(r"duplicate pairs per list: before ([0-9.]+)  after ([0-9.]+)", run.stdout)
    assert m and float(m.group(2)) == 0.0 and abs(float(m.group(1)) - r["dup_pairs_before"].mean()) < 1e-4
    assert run.stdout.count("hit@10") == 3 and "dedup user state" in run.stdout
    # without the flag
    other = tmp_path / "without"
    other.mkdir()
    monkeypatch.chdir(other)
    model = cli.main(args)
    out = capsys.readouterr().out
    assert "dedup" not in out and out.count("hit@10") == 2
    names = lambda top: sorted(os.path.relpath(os.path.join(b, f), top) for b, _, fs in os.walk(top) for f in fs)
    with_flag, without = names(str(child)), names(str(other))
    assert [n for n in with_flag if not n.endswith("_dedup.npz")] == without and len(with_flag) == len(without) + 1
    shape = lambda text: [re.sub(r"\d[\d.eE+-]*", "#", l) for l in text.splitlines()]      # a line with its numbers blanked
    lines, block, keep = shape(run.stdout), False, []
    for l in lines:                                                            # cut the de-dup block out of the child's output
        block = block or l.startswith("calculate recommend # dedup #")
        if not block:
            keep.append(l)
        block = block and not l.startswith("calculate recommend # dedup done")
    assert keep == shape(out) and len(lines) == len(keep) + 5
    assert np.array_equal(np.load(model.data_dir + "article_encoded_recommend10.npz")["targets"], plain["targets"])
