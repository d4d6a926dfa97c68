"""dae_covisit_neighbors / dae_covisit_recommend and helpers.covisit on the GPU against tests/covisit_reference.py: integers equal,
floats bit-equal.  The raw calls write into buffers pre-filled with -7 that are wider than K / k; the extra columns must stay."""
import ctypes
import functools
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from covisit_reference import covisit_recommend_reference, covisit_reference
from dae_rnn_news_recommendation_amd import _lib as L
from dae_rnn_news_recommendation_amd import helpers
from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PAD = 3                                                                  # extra columns of every output buffer


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if indptr[-1] else np.zeros(0, dtype=np.int64)
    return indptr, items


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a) if a.size else np.zeros(1, dtype=a.dtype)).cuda()


def build(indptr, items, Na, window, both, cosine, K, extra_ws=0):
    """The raw call: a dict like covisit_reference's, plus ``raw`` (the whole buffers as bytes)."""
    import torch
    lib = L.load()
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    M, nnz, ld = indptr.size - 1, int(items.size), K + PAD
    i32 = dict(dtype=torch.int32, device="cuda")
    nbr, cnt = torch.full((Na, ld), -7, **i32), torch.full((Na, ld), -7, **i32)
    sim = torch.full((Na, ld), -7.0, dtype=torch.float32, device="cuda")
    degree, clicks = torch.full((Na,), -7, **i32), torch.full((Na,), -7, **i32)
    totals = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    host = indptr.ctypes.data_as(ctypes.c_void_p)
    bound = int(lib.dae_covisit_record_bound(host, M, window, both))
    ws_bytes = int(lib.dae_covisit_neighbors_workspace(bound, Na, K))
    assert (ws_bytes > 0) == (bound > 0)
    ws_bytes += extra_ws if bound > 0 else 0
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    ws_p = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256) if bound > 0 else None
    d_ptr, d_items = _up(indptr), _up(items.astype(np.int32))
    L.call("dae_covisit_neighbors", L.ptr(d_ptr), L.ptr(d_items), host, M, nnz, Na, window, both, cosine, K, L.ptr(nbr), L.ptr(sim),
           L.ptr(cnt), ld, L.ptr(degree), L.ptr(clicks), L.ptr(totals), ws_p, ws_bytes if bound > 0 else 0, L.current_stream())
    torch.cuda.synchronize()
    out = {"nbr": nbr.cpu().numpy(), "sim": sim.cpu().numpy(), "cnt": cnt.cpu().numpy(), "degree": degree.cpu().numpy(),
           "clicks": clicks.cpu().numpy(), "totals": totals.cpu().numpy(), "bound": bound}
    out["raw"] = b"".join(out[n].tobytes() for n in ("nbr", "sim", "cnt", "degree", "clicks", "totals"))
    return out


def check_table(got, ref, K):
    """``got`` (wide buffers) against a reference built with at least K columns."""
    assert np.array_equal(got["nbr"][:, :K], ref["nbr"][:, :K])
    assert np.array_equal(_bits(got["sim"][:, :K]), _bits(ref["sim"][:, :K]))
    assert np.array_equal(got["cnt"][:, :K], ref["cnt"][:, :K])
    assert (got["nbr"][:, K:] == -7).all() and (got["sim"][:, K:] == -7).all() and (got["cnt"][:, K:] == -7).all()
    assert np.array_equal(got["degree"], ref["degree"]) and np.array_equal(got["clicks"], ref["clicks"])
    assert got["totals"].tolist() == [ref["n_records"], ref["n_pairs"]] and ref["n_records"] <= got["bound"]


# ---- build: the small random log ----
@functools.lru_cache(maxsize=None)
def random_log():
    labels = np.random.default_rng(3).integers(0, 6, 300)
    return synthetic_sessions(400, labels, mean_len=10, seed=5)


@functools.lru_cache(maxsize=None)
def random_ref(window, both, cosine):
    """The reference at K = 128; the first K columns are the table at a smaller K (the order is total)."""
    return covisit_reference(*random_log(), 300, window, both, cosine, 128)


def _cut(ref, K):
    """The reference at K < 128: the first K columns."""
    return dict(ref, nbr=ref["nbr"][:, :K], sim=ref["sim"][:, :K], cnt=ref["cnt"][:, :K])


@pytest.mark.parametrize("K", [1, 10, 128])
@pytest.mark.parametrize("cosine", [0, 1])
@pytest.mark.parametrize("both", [0, 1])
@pytest.mark.parametrize("window", [1, 3, 1000])
def test_build_random_log(window, both, cosine, K):
    indptr, items = random_log()
    assert np.diff(indptr).max() < 1000
    ref = random_ref(window, both, cosine)
    check_table(build(indptr, items, 300, window, both, cosine, K), _cut(ref, K), K)
    if window == 3 and both == 1:
        assert ref["degree"].min() > 10 and ref["degree"].max() < 128      # K = 10 cuts every row, K = 128 none
        tied = (_bits(ref["sim"][:, 9]) == _bits(ref["sim"][:, 10])).sum()      # a tie exactly at the cut of K = 10
        assert tied > 100


# ---- build: the hub log ----
@functools.lru_cache(maxsize=None)
def hub_log():
    return _csr([[0, j] for j in range(1, 5001)] + [[7, 9, 7, 9, 11]] * 3 + [[], [5], [5, 5, 5]])


@pytest.mark.parametrize("both", [0, 1])
@pytest.mark.parametrize("cosine", [0, 1])
def test_build_hub_log(both, cosine):
    indptr, items = hub_log()
    ref = covisit_reference(indptr, items, 6000, 2, both, cosine, 128)
    got = build(indptr, items, 6000, 2, both, cosine, 128)
    check_table(got, ref, 128)
    assert got["degree"][0] == 5000 and got["clicks"][5] == 5
    assert got["degree"][5] == (1 if both else 0)                        # [0, 5] alone reaches article 5: (5, 0) exists only mirrored
    if not cosine:
        assert got["nbr"][0, :128].tolist() == list(range(1, 129)) and (got["cnt"][0, :128] == 1).all()
    if both:
        assert got["nbr"][7, :4].tolist() == [9, 11, 0, -1] and got["cnt"][7, :4].tolist() == [9, 3, 1, 0]
    else:
        assert got["nbr"][7, :3].tolist() == [9, 11, -1] and got["cnt"][7, :3].tolist() == [6, 3, 0]
    # the histories [], [5] and [5, 5, 5] emit nothing: 5000 pairs [0, j] and three times [7, 9, 7, 9, 11] at window 2
    # [7, 9, 7, 9, 11]: seven pairs, (7, 7) and (9, 9) among them, so five records
    assert got["totals"][0] == (5000 + 3 * 5) * (2 if both else 1) and got["bound"] == (5000 + 3 * 7 + 3) * (2 if both else 1)


# ---- build: further cases ----
@pytest.mark.parametrize("window", [1, 700])
@pytest.mark.parametrize("cosine", [0, 1])
def test_build_one_long_history(window, cosine):
    items = np.random.default_rng(9).integers(0, 1000, 700)
    indptr = np.array([0, 700], dtype=np.int64)
    ref = covisit_reference(indptr, items, 1000, window, 1, cosine, 128)
    if window == 700:
        assert ref["degree"].max() > 256                                 # rows of the workgroup-per-row kernel, with real scores
    check_table(build(indptr, items, 1000, window, 1, cosine, 128), ref, 128)


@pytest.mark.parametrize("name", ["Na1", "Na37", "M0", "norecord", "nnz0"])
def test_build_edges(name):
    rng = np.random.default_rng(21)
    Na, K = {"Na1": (1, 4), "Na37": (37, 40)}.get(name, (9, 5))
    rows = {"Na1": [[0, 0, 0], [0]], "Na37": [rng.integers(0, 37, rng.integers(0, 30)) for _ in range(90)], "M0": [],
            "norecord": [[3], [], [4, 4, 4], [8]], "nnz0": [[], [], []]}[name]
    indptr, items = _csr(rows)
    ref = covisit_reference(indptr, items, Na, 4, 1, 1, K)
    got = build(indptr, items, Na, 4, 1, 1, K)
    check_table(got, ref, K)
    if name != "Na37":
        assert (got["nbr"][:, :K] == -1).all() and (got["sim"][:, :K] == 0).all() and got["totals"].tolist() == [0, 0]
    else:
        assert ref["degree"].max() > 30 and ref["degree"].min() < K


def test_build_invariants():
    indptr, items = random_log()
    one = build(indptr, items, 300, 3, 1, 1, 10)
    assert build(indptr, items, 300, 3, 1, 1, 10)["raw"] == one["raw"]                       # run to run
    assert build(indptr, items, 300, 3, 1, 1, 10, extra_ws=1 << 20)["raw"] == one["raw"]     # a larger workspace
    perm = np.random.default_rng(1).permutation(indptr.size - 1)
    assert build(*helpers.permute_histories(indptr, items, perm), 300, 3, 1, 1, 10)["raw"] == one["raw"]      # the order of the users


# ---- recommend ----
@functools.lru_cache(maxsize=None)
def table():
    ref = random_ref(3, 1, 1)
    return ref["nbr"], ref["sim"]


def rec(indptr, items, seen, age_weight, last, k, window=None, K=128):
    import torch
    nbr, sim = table()
    nbr, sim = nbr[:, :K], sim[:, :K]
    M, ldo, ld = indptr.size - 1, k + PAD, K + 2
    d_nbr, d_sim = torch.full((300, ld), -1, dtype=torch.int32, device="cuda"), torch.zeros((300, ld), dtype=torch.float32, device="cuda")
    d_nbr[:, :K], d_sim[:, :K] = torch.from_numpy(np.ascontiguousarray(nbr)).cuda(), torch.from_numpy(np.ascontiguousarray(sim)).cuda()
    idx = torch.full((M, ldo), -7, dtype=torch.int32, device="cuda")
    score = torch.full((M, ldo), -7.0, dtype=torch.float32, device="cuda")
    xp, xi = helpers.normalize_exclusions(seen, M, 300)
    d = [_up(a) for a in (indptr.astype(np.int64), items.astype(np.int32), xp, xi, np.asarray(age_weight, dtype=F32))]
    w = (None, None) if window is None else tuple(_up(np.asarray(a, dtype=np.int32)) for a in window)
    L.call("dae_covisit_recommend", L.ptr(d_nbr), L.ptr(d_sim), ld, 300, K, L.ptr(d[0]), L.ptr(d[1]), M, L.ptr(d[2]), L.ptr(d[3]),
           L.ptr(w[0]), L.ptr(w[1]), L.ptr(d[4]), last, k, L.ptr(idx), L.ptr(score), ldo, L.current_stream())
    torch.cuda.synchronize()
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    assert (idx[:, k:] == -7).all() and (score[:, k:] == -7).all()
    want = covisit_recommend_reference(nbr, sim, indptr, items, xp, xi, age_weight, last, k, window)
    assert np.array_equal(idx[:, :k], want[0]) and np.array_equal(_bits(score[:, :k]), _bits(want[1]))
    return idx[:, :k], score[:, :k]


@functools.lru_cache(maxsize=None)
def query_log():
    """100 users of the random log, and the special ones: no history, one click, the last clicks one article, a long history."""
    indptr, items = random_log()
    rows = [items[indptr[u]:indptr[u + 1]] for u in range(100)]
    rows += [[], [17], [5, 5, 5, 5], [3, 8, 8, 8, 2, 8], np.random.default_rng(2).integers(0, 300, 60)]
    return _csr(rows)


def _weights(decay, last):
    return (np.float64(decay) ** np.arange(last)).astype(F32)


@pytest.mark.parametrize("last", [1, 10, 32])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_recommend_last_and_k(last, k):
    indptr, items = query_log()
    lens = np.diff(indptr)
    assert lens.min() == 0 and (lens == 1).any() and ((lens > 1) & (lens < 10)).any() and lens.max() > 32
    idx, score = rec(indptr, items, (indptr, items), _weights(0.8, last), last, k)
    assert (idx[100] == -1).all() and np.isneginf(score[100]).all()      # the user without a history
    if k == 128 and last == 32:
        assert (idx[104] >= 0).sum() > 100                               # 32 sources x up to 91 neighbours: a full-size sort


@pytest.mark.parametrize("decay", [0.0, 0.8, 1.0])
def test_recommend_position_decay(decay):
    indptr, items = query_log()
    idx, score = rec(indptr, items, (indptr, items), _weights(decay, 10), 10, 128)
    if decay == 0.0:
        assert ((score == 0) & (idx >= 0)).any()                         # reached by older clicks alone: score 0, still listed


@pytest.mark.parametrize("K", [1, 50])
def test_recommend_narrow_tables(K):
    indptr, items = query_log()
    rec(indptr, items, (indptr, items), _weights(0.8, 10), 10, 10, K=K)


def test_recommend_seen_lists_and_windows():
    indptr, items = query_log()
    M = indptr.size - 1
    everything = [np.arange(300)] * M                                    # every candidate seen: a list of 300 > 256 items
    idx, _ = rec(indptr, items, everything, _weights(0.8, 10), 10, 10)
    assert (idx == -1).all()
    nothing = [[]] * M
    free, _ = rec(indptr, items, nothing, _weights(0.8, 10), 10, 10)
    own, _ = rec(indptr, items, (indptr, items), _weights(0.8, 10), 10, 10)
    assert not np.array_equal(free, own)
    rng = np.random.default_rng(4)
    lo = rng.integers(0, 300, M)
    hi = np.minimum(lo + rng.integers(0, 200, M), 300)
    hi[:5] = lo[:5]                                                      # empty windows
    idx, _ = rec(indptr, items, (indptr, items), _weights(0.8, 10), 10, 10, window=(lo, hi))
    assert (idx[:5] == -1).all() and (((idx >= lo[:, None]) & (idx < hi[:, None])) | (idx < 0)).all()
    again, _ = rec(indptr, items, (indptr, items), _weights(0.8, 10), 10, 10, window=(lo, hi))
    assert np.array_equal(idx, again)                                    # run to run


# ---- helpers and the CLI ----
def test_helpers_against_the_reference(tmp_path):
    indptr, items = random_log()
    ref = random_ref(3, 1, 1)
    index = helpers.covisit_neighbors((indptr, items), 300, n_neighbors=20)
    assert index.neighbors.dtype == np.int64 and index.sims.dtype == F32 and index.counts.dtype == np.int32
    assert np.array_equal(index.neighbors, ref["nbr"][:, :20]) and np.array_equal(_bits(index.sims), _bits(ref["sim"][:, :20]))
    assert np.array_equal(index.counts, ref["cnt"][:, :20]) and np.array_equal(index.degree, ref["degree"])
    assert np.array_equal(index.clicks, ref["clicks"]) and (index.n_records, index.n_pairs) == (ref["n_records"], ref["n_pairs"])
    fwd = helpers.covisit_neighbors((indptr, items), 300, window=1, direction="forward", normalize="none", n_neighbors=128, max_events=4)
    want = covisit_reference(*helpers.trim_histories((indptr, items), 4), 300, 1, 0, 0, 128)
    assert np.array_equal(fwd.neighbors, want["nbr"]) and np.array_equal(fwd.counts, want["cnt"])
    q_ptr, q_items = query_log()
    xp, xi = helpers.normalize_exclusions((q_ptr, q_items), q_ptr.size - 1, 300)
    want = covisit_recommend_reference(ref["nbr"][:, :20], ref["sim"][:, :20], q_ptr, q_items, xp, xi, (np.float64(0.8) ** np.arange(10)).astype(F32),
                                       10, 10)
    idx, score = index.recommend((q_ptr, q_items), 10)                    # seen=None: the own histories
    assert idx.dtype == np.int64 and np.array_equal(idx, want[0]) and np.array_equal(_bits(score), _bits(want[1]))
    idx2, score2 = index.recommend((q_ptr, q_items), 10, seen=(q_ptr, q_items), return_tensor=True)
    assert idx2.is_cuda and np.array_equal(idx2.cpu().numpy(), idx) and np.array_equal(_bits(score2.cpu().numpy()), _bits(score))
    index.save(str(tmp_path / "ix.npz"))
    back = helpers.CovisitIndex.load(str(tmp_path / "ix.npz"))
    idx3, score3 = back.recommend((q_ptr, q_items), 10)
    assert np.array_equal(idx3, idx) and np.array_equal(_bits(score3), _bits(score))
    # fill_popular: the short lists grow by the most clicked unseen articles, the scores stay
    filled, score4 = index.recommend((q_ptr, q_items), 10, fill_popular=True)
    short = (idx < 0).any(axis=1)
    assert short.any() and (filled >= 0).all() and np.array_equal(filled[idx >= 0], idx[idx >= 0]) and np.array_equal(_bits(score4), _bits(score))
    order = np.argsort(-index.clicks.astype(np.int64), kind="stable")
    u = 100                                                              # no history: the list is the popularity list
    assert np.array_equal(filled[u], order[:10])
    for u in np.flatnonzero(short):
        row = filled[u]
        assert np.unique(row).size == 10 and not np.isin(row, xi[xp[u]:xp[u + 1]]).any()
    one, _ = helpers.covisit_recommend((q_ptr, q_items), 300, 10, n_neighbors=20)
    own = helpers.covisit_neighbors((q_ptr, q_items), 300, n_neighbors=20).recommend((q_ptr, q_items), 10)[0]
    assert np.array_equal(one, own)
    n, s, c = index.similar([4, 0], 5)
    assert np.array_equal(n, ref["nbr"][[4, 0], :5]) and np.array_equal(c, ref["cnt"][[4, 0], :5])


def test_cli_covisit(tmp_path, monkeypatch, capsys):
    """--covisit in a fresh child process: the _covisit.npz with its arrays, the lists equal to the reference on the saved
    histories, the third metrics line.  The run without the flag (in this process, same arguments): the same files but that one,
    and the same printed lines but the co-visitation block."""
    import main_autoencoder as cli
    args = ["--model_name", "rec", "--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4",
            "--sessions", "synthetic", "--recommend", "10", "--similarity", "False"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    child = tmp_path / "with"
    child.mkdir()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "main_autoencoder.py")] + args + ["--covisit"], cwd=str(child), env=env,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    found = glob.glob(str(child / "**" / "article_encoded_recommend10_covisit.npz"), recursive=True)
    assert len(found) == 1
    r = np.load(found[0])
    assert set(r.files) == {"indices", "scores", "targets", "hist_indptr", "hist_items", "neighbors", "sims", "counts"}
    assert r["indices"].shape == r["scores"].shape == (200, 10) and r["neighbors"].shape == r["sims"].shape == r["counts"].shape == (400, 50)
    assert r["indices"].dtype == r["neighbors"].dtype == np.int64 and r["scores"].dtype == r["sims"].dtype == F32
    ref = covisit_reference(r["hist_indptr"], r["hist_items"], 400, 3, 1, 1, 50)
    assert np.array_equal(r["neighbors"], ref["nbr"]) and np.array_equal(_bits(r["sims"]), _bits(ref["sim"]))
    assert np.array_equal(r["counts"], ref["cnt"])
    xp, xi = helpers.normalize_exclusions((r["hist_indptr"], r["hist_items"]), 200, 400)
    want = covisit_recommend_reference(ref["nbr"], ref["sim"], r["hist_indptr"], r["hist_items"], xp, xi,
                                       (np.float64(0.8) ** np.arange(10)).astype(F32), 10, 10)
    assert np.array_equal(r["indices"], want[0]) and np.array_equal(_bits(r["scores"]), _bits(want[1]))
    plain = np.load(os.path.join(os.path.dirname(found[0]), "article_encoded_recommend10.npz"))
    assert np.array_equal(plain["targets"], r["targets"])
    assert run.stdout.count("hit@10") == 3 and re.search(r"hit@10 co-visited articles +[0-9.]+  MRR [0-9.]+  nDCG [0-9.]+", run.stdout)
    assert re.search(r"co-click neighbours among the 50 nearest embedding neighbours: [0-9.]+", run.stdout)
    # without the flag
    other = tmp_path / "without"
    other.mkdir()
    monkeypatch.chdir(other)
    cli.main(args)
    out = capsys.readouterr().out
    assert "covisit" not in out and "co-visited" not in out and out.count("hit@10") == 2
    names = lambda top: sorted(os.path.relpath(os.path.join(b, f), top) for b, _, fs in os.walk(top) for f in fs)      # noqa: E731
    with_flag, without = names(str(child)), names(str(other))
    assert [n for n in with_flag if not n.endswith("_covisit.npz")] == without and len(with_flag) == len(without) + 1
    shape = lambda text: [re.sub(r"\d[\d.eE+-]*", "#", l) for l in text.splitlines()]      # noqa: E731  a line with its numbers blanked
    lines, block, keep = shape(run.stdout), False, []
    for l in lines:                                                      # cut the block out of the child's output
        block = block or l.startswith("calculate recommend # covisit")
        if not block:
            keep.append(l)
        block = block and not l.startswith("calculate recommend # covisit done")
    assert keep == shape(out) and len(lines) == len(keep) + 5
