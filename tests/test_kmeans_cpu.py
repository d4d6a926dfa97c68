"""CPU checks of the clustering (dae_kmeans_assign / dae_kmeans_update; helpers.kmeans, kmeans_assign, cluster_label_scores,
ClusterIndex): both builds export the four symbols with the header's arity, every argument error of the two entries is reported
before any HIP call, cluster_label_scores against sklearn and a hand count, the float64 reference of tests/kmeans_reference.py on
planted blobs, the relocation rule, the merge rule of ClusterIndex.search on CPU tensors, and the ValueErrors of the helpers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kmeans_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first
NEW = {"dae_kmeans_assign_workspace": 2, "dae_kmeans_assign": 12, "dae_kmeans_update_workspace": 3, "dae_kmeans_update": 14}


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


# ---- the C entries ----

@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_builds_export_the_symbols(fmt):
    lib = _lib(fmt)
    for name in NEW:
        assert hasattr(lib, name), name


def test_arity_matches_the_header_and_the_abi_version_stays():
    from dae_rnn_news_recommendation_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dae_hip.h")).read(), flags=re.S)
    for name, want in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == want == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is (ctypes.c_uint64 if name.endswith("workspace") else ctypes.c_int32)
    assert _lib.ABI_VERSION == 9 and _lib.load().dae_abi_version() == 9


def test_workspace_sizes():
    lib = _lib()
    assert lib.dae_kmeans_assign_workspace(0, 5) == 0 and lib.dae_kmeans_assign_workspace(5, 0) == 0
    assert lib.dae_kmeans_update_workspace(0, 5, 3) == 0 and lib.dae_kmeans_update_workspace(5, 0, 3) == 0 == lib.dae_kmeans_update_workspace(5, 5, 0)
    one = lib.dae_kmeans_assign_workspace(200000, 1024)               # 1563 row tiles fill the device: one centroid slice
    assert 0 < one < 1 << 22 and one % 256 == 0
    assert lib.dae_kmeans_assign_workspace(100, 1000) > 8 * 128 * 8                                   # several slices of keys
    # the update holds (N / 256 + K) segment partials of pad(D) doubles, three N-long arrays and the sort's scratch
    assert lib.dae_kmeans_update_workspace(1000, 10, 70) > (4 + 10) * 128 * 8 + 3 * 1000 * 4


def _assign(lib, Xi=P, N=300, Ci=P, K=130, D=70, prev=None, labels=P, scores=P, out=None, ws=P, ws_bytes=None):
    out = (ctypes.c_double * 4)() if out is None else out
    if ws_bytes is None:
        ws_bytes = lib.dae_kmeans_assign_workspace(N, K)
    return lib.dae_kmeans_assign(Xi, N, Ci, K, D, prev, labels, scores, out, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(K=0, ws_bytes=1 << 20), b"must be positive"),
    (dict(N=0, ws_bytes=1 << 20), b"must be positive"),
    (dict(D=0), b"must be positive"),
    (dict(Xi=None), b"NULL"),
    (dict(Ci=None), b"NULL"),
    (dict(labels=None), b"NULL"),
    (dict(scores=None), b"NULL"),
    (dict(ws=None), b"NULL"),
    (dict(ws_bytes=255), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
    (dict(Xi=ctypes.c_void_p((1 << 20) + 4)), b"256-byte aligned"),
    (dict(N=2 ** 21, D=512, ws_bytes=1 << 40), b"exceeds 4 GiB"),
])
def test_assign_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _assign(lib, **kw) != 0
    assert msg in lib.dae_last_error() and b"kmeans_assign" in lib.dae_last_error(), lib.dae_last_error()


def _update(lib, Xi=P, N=300, D=70, labels=P, K=130, cent=P, ldc=None, counts=P, order=P, offsets=P, ws=P, ws_bytes=None):
    out = (ctypes.c_double * 4)()
    if ws_bytes is None:
        ws_bytes = lib.dae_kmeans_update_workspace(N, K, D)
    return lib.dae_kmeans_update(Xi, N, D, labels, K, cent, D if ldc is None else ldc, counts, order, offsets, out, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(K=0, ws_bytes=1 << 20), b"must be positive"),
    (dict(N=0, ws_bytes=1 << 20), b"must be positive"),
    (dict(D=0, ws_bytes=1 << 20), b"must be positive"),
    (dict(Xi=None), b"NULL"),
    (dict(labels=None), b"NULL"),
    (dict(counts=None), b"NULL"),
    (dict(order=None), b"NULL"),
    (dict(offsets=None), b"NULL"),
    (dict(ws=None), b"NULL"),
    (dict(ldc=69), b"ldc"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
    (dict(N=2 ** 21, D=512, ws_bytes=1 << 40), b"exceeds 4 GiB"),
])
def test_update_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _update(lib, **kw) != 0
    assert msg in lib.dae_last_error() and b"kmeans_update" in lib.dae_last_error(), lib.dae_last_error()


# ---- cluster_label_scores ----

def test_cluster_label_scores_equal_sklearn_and_a_hand_count():
    metrics = pytest.importorskip("sklearn.metrics")
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.RandomState(0)
    for n, kp, kt in ((200, 5, 4), (57, 9, 3), (300, 2, 11), (40, 1, 5), (40, 6, 1)):
        pred = rng.randint(0, kp, n)
        true = rng.randint(0, kt, n).astype(np.float64)
        true = np.where(rng.rand(n) < 0.5, true, pred % kt)            # correlated with the clustering
        true[::7] = -1
        true[3::11] = np.nan
        ok = np.isfinite(true) & (true >= 0)
        got = helpers.cluster_label_scores(pred, true)
        assert got["n"] == int(ok.sum()) and got["n_clusters"] == np.unique(pred[ok]).size and got["n_labels"] == np.unique(true[ok]).size
        assert got["nmi"] == pytest.approx(metrics.normalized_mutual_info_score(true[ok], pred[ok]), abs=1e-12)
        assert got["ari"] == pytest.approx(metrics.adjusted_rand_score(true[ok], pred[ok]), abs=1e-12)
        by_hand = sum(max(int(((pred == c) & (true == t) & ok).sum()) for t in np.unique(true[ok])) for c in np.unique(pred[ok]))
        assert got["purity"] == by_hand / ok.sum()
    same = helpers.cluster_label_scores([3, 3, 1, 1, 2], [0, 0, 5, 5, 9])
    assert same["purity"] == 1.0 and same["nmi"] == pytest.approx(1.0) and same["ari"] == 1.0
    one = helpers.cluster_label_scores([0, 0, 0], [4, 4, 4])
    assert one["nmi"] == 1.0 and one["ari"] == 1.0 and one["purity"] == 1.0
    none = helpers.cluster_label_scores([0, 1], [-1, np.nan])
    assert none["n"] == 0 and np.isnan(none["purity"]) and np.isnan(none["nmi"]) and np.isnan(none["ari"])
    with pytest.raises(ValueError, match="cluster ids"):
        helpers.cluster_label_scores([0, 1, 2], [0, 1])


def test_cluster_label_scores_need_no_sklearn():
    src = open(os.path.join(ROOT, "dae_rnn_news_recommendation_amd", "helpers", "clustering.py")).read()
    assert not re.search(r"^\s*(from|import)\s+sklearn", src, flags=re.M)


# ---- the reference ----

def test_reference_recovers_planted_blobs():
    X, y, centres = R.blobs(400, 7, 30, 0.05, 3)
    first = np.array([np.flatnonzero(y == c)[0] for c in range(7)])
    r = R.lloyd(X, X[first], max_iter=20, tol=0)
    assert (r["labels"] == y).all() and r["relocated"] == 0
    assert r["history"][-1][1] == 0 and len(r["history"]) == r["n_iter"] + 1 <= 4
    assert np.abs(r["centroids"] - centres).max() < 0.05
    assert np.allclose((r["centroids"] ** 2).sum(axis=1), 1.0, atol=1e-12)
    means = [h[0] for h in r["history"]]
    assert all(b >= a - 1e-15 for a, b in zip(means, means[1:]))      # Lloyd never lowers the mean score


def test_reference_ties_and_zero_rows_go_to_the_lower_id():
    C = R.normalize(np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, 0]]))
    X = np.array([[2.0, 0, 0], [0, 0, 0], [0, 3.0, 0], [1.0, 1.0, 0]])
    labels, scores, gap, gaps = R.assign(R.normalize(X), C)
    assert labels.tolist() == [0, 0, 1, 0] and scores[1] == 0 and gap == 0


def test_reference_relocation_rule_and_the_helper_agree():
    from dae_rnn_news_recommendation_amd import helpers
    scores = np.array([0.9, 0.1, 0.1, 0.5, 0.05, 0.3], dtype=np.float32)
    labels = np.array([0, 0, 0, 2, 3, 2])
    counts = np.array([3, 0, 2, 1, 0])                                # clusters 1 and 4 are empty; row 4 is alone in cluster 3
    rows, gap = R.relocation(scores, labels, counts)
    assert rows.tolist() == [1, 2] and gap == 0.0                     # the tie of rows 1 and 2 is a decision of gap 0
    assert helpers.relocation_rows(scores, labels, counts).tolist() == [1, 2]
    rng = np.random.RandomState(5)
    for _ in range(20):
        K = 12
        labels = rng.randint(0, K, 60)
        labels[labels % 3 == 0] = 1
        counts = np.bincount(labels, minlength=K)
        scores = rng.randint(0, 8, 60).astype(np.float32) / 8          # many ties
        assert helpers.relocation_rows(scores, labels, counts).tolist() == R.relocation(scores, labels, counts)[0].tolist()
    r = R.lloyd(*_relocating_case(), max_iter=12, tol=0)
    assert r["relocated"] >= 1 and (r["counts"] > 0).all()


def _relocating_case():
    X, _, _ = R.blobs(300, 130, 70, 0.05, 4)
    return X, X[np.random.RandomState(104).choice(300, 130, replace=False)]


# ---- the merge rule of ClusterIndex.search ----

def test_merge_probe_lists_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    from dae_rnn_news_recommendation_amd import helpers
    order = torch.tensor([40, 10, 30, 20, 50, 60, 0])                 # position in the cluster-ordered corpus -> the caller's id
    inf = float("inf")
    idx = [torch.tensor([[0, 1, -1], [2, -1, -1]]), torch.tensor([[3, 4, 5], [-1, -1, -1]]), torch.tensor([[6, -1, -1], [1, 0, -1]])]
    sc = [torch.tensor([[0.75, 0.5, -inf], [0.25, -inf, -inf]]), torch.tensor([[0.75, 0.5, 0.125], [-inf, -inf, -inf]]),
          torch.tensor([[-0.5, -inf, -inf], [0.25, 0.25, -inf]])]
    i, s = helpers.merge_probe_lists(idx, sc, order, 4)
    assert i.dtype == torch.int64 and s.dtype == torch.float32
    assert i.tolist() == [[20, 40, 10, 50], [10, 30, 40, -1]]         # equal scores: the lower id of the CALLER first
    assert s.tolist() == [[0.75, 0.75, 0.5, 0.5], [0.25, 0.25, 0.25, -inf]]
    i, s = helpers.merge_probe_lists(idx[:1], sc[:1], order, 5)       # fewer candidates than k: a -1 / -inf tail
    assert i.tolist() == [[40, 10, -1, -1, -1], [30, -1, -1, -1, -1]] and s[0].tolist() == [0.75, 0.5, -inf, -inf, -inf]
    i, s = helpers.merge_probe_lists([t[:, :0] for t in idx], [t[:, :0] for t in sc], order, 2)
    assert i.tolist() == [[-1, -1], [-1, -1]]
    z = helpers.merge_probe_lists([torch.tensor([[0, 1]])], [torch.tensor([[0.0, -0.0]])], torch.tensor([9, 3]), 2)
    assert z[0].tolist() == [[3, 9]]                                 # -0 and +0 are one score


def test_cluster_index_checks_and_npz_round_trip(tmp_path):
    from dae_rnn_news_recommendation_amd import helpers
    corpus = np.arange(12, dtype=np.float32).reshape(4, 3)
    order, offsets, cent = [2, 0, 3, 1], [0, 2, 2, 4], np.eye(3, dtype=np.float32)
    ix = helpers.ClusterIndex(corpus[order], order, offsets, cent, "l2", "linear kernel")
    assert ix.inverse.tolist() == [1, 3, 0, 2] and ix.n_clusters == 3
    ix.save(str(tmp_path / "ix.npz"))
    back = helpers.ClusterIndex.load(str(tmp_path / "ix.npz"))
    assert (back.corpus == ix.corpus).all() and (back.order == ix.order).all() and (back.offsets == ix.offsets).all()
    assert (back.centroids == cent).all() and back.norm == "l2" and back.metric == "linear kernel"
    for kw in (dict(window=([0], [1])), dict(exclude_shared=((), (), (), ()))):
        with pytest.raises(ValueError, match="window= or exclude_shared="):
            ix.search(corpus, **kw)
    with pytest.raises(ValueError, match="n_probe"):
        ix.search(corpus, n_probe=0)
    with pytest.raises(ValueError, match="k must be in 1..128"):
        ix.search(corpus, k=129)
    with pytest.raises(ValueError, match="order must hold"):
        helpers.ClusterIndex(corpus, [0, 1, 2], offsets, cent)
    with pytest.raises(ValueError, match="metric"):
        helpers.ClusterIndex(corpus, order, offsets, cent, "", "euclid")
    res = helpers.KMeansResult(order=np.array(order), offsets=np.array(offsets), centroids=cent)
    built = helpers.ClusterIndex.from_kmeans(corpus, res)
    assert (built.corpus == corpus[order]).all() and built.metric == "cosine"
    with pytest.raises(ValueError, match="have no cluster"):          # a row labelled -1 lies behind offsets[K]
        helpers.ClusterIndex.from_kmeans(corpus, helpers.KMeansResult(order=np.array(order), offsets=np.array([0, 2, 2, 3]), centroids=cent))


def test_helper_argument_errors_before_the_device():
    from dae_rnn_news_recommendation_amd import helpers
    X = np.ones((5, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="empty must be"):
        helpers.kmeans(X, 2, empty="drop")
    with pytest.raises(ValueError, match="max_iter"):
        helpers.kmeans(X, 2, max_iter=-1)
    with pytest.raises(ValueError, match="metric must be"):
        helpers.kmeans_assign(X, X[:2], "euclid")


# ---- the package ----

def test_helpers_import_needs_numpy_alone_and_exports_the_new_names():
    code = ("import sys; from dae_rnn_news_recommendation_amd import helpers as h; "
            "assert all(hasattr(h, n) for n in ('kmeans', 'kmeans_assign', 'KMeansResult', 'cluster_label_scores', 'ClusterIndex', "
            "'merge_probe_lists', 'relocation_rows')); "
            "print(sorted(m for m in ('torch', 'scipy', 'pandas', 'sklearn') if m in sys.modules))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "[]", out.stdout


def test_the_new_source_is_built_and_launches_through_the_timed_launcher():
    csrc = os.path.join(ROOT, "dae_rnn_news_recommendation_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bdae_kmeans\.hip\b", mk, flags=re.M)
    text = open(os.path.join(csrc, "dae_kmeans.hip")).read()
    assert '#include "dae_score_sweep.h"' in text and text.count("DAE_LAUNCH(") >= 8 and "atomicAdd" not in text
    assert not re.search(r"\bhipLaunchKernelGGL\(|<<<", text)
