"""GPU checks of the clustering (dae_kmeans_assign, dae_kmeans_update; helpers.kmeans, kmeans_assign, ClusterIndex) against
most_similar, NumPy and the float64 reference of tests/kmeans_reference.py.

The assignment is compared with most_similar(k = 1) bit for bit: the same images, the same products, the same total order.  Against
float64 a label may differ only where two scores lie closer than tau = 2 D 2^-24, a conservative bound on the fp32 error of a dot
product of two unit vectors of length D; every input below is chosen so that the REFERENCE alone shows no such row (asserted first),
and then the labels of every iteration must equal the reference's exactly.  The update's integer outputs equal NumPy's; its
centroids lie within 2^-21 of float64 (about three fp32 roundings of the row normalisation per entry <= 1, an fp64 accumulation,
one final rounding: <= 4 * 2^-24, with a 2x margin)."""
import ctypes

import numpy as np
import pytest
import torch

import kmeans_reference as R

pytestmark = pytest.mark.gpu

CENTROID_TOL = 2.0 ** -21


def tau(D):
    return 2 * D * 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _image(lib, L, A, metric):
    A = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).cuda()
    n, D = A.shape
    nb = int(lib.dae_sweep_image_bytes(n, D))
    t = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(t.data_ptr() + (-t.data_ptr()) % 256)
    L.call("dae_sweep_image_dense", L.ptr(A), A.stride(0), n, D, 0, metric, p, nb, L.current_stream())
    return p, t


def _ws(nbytes, fill):
    t = torch.full((nbytes + 256,), fill, dtype=torch.uint8, device="cuda")
    return ctypes.c_void_p(t.data_ptr() + (-t.data_ptr()) % 256), t


def _abi_assign(X, C, metric=1, prev=None, ws_scale=1, fill=0):
    """dae_kmeans_assign through ctypes: (labels int64, scores float32, record)."""
    from dae_rnn_news_recommendation_amd import _lib as L
    lib = L.load()
    (N, D), K = X.shape, C.shape[0]
    xp, xt = _image(lib, L, X, metric)
    cp, ct = _image(lib, L, C, metric)
    labels = torch.full((N + 3,), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((N + 3,), -7.0, dtype=torch.float32, device="cuda")
    pv = None if prev is None else torch.from_numpy(np.ascontiguousarray(prev, dtype=np.int32)).cuda()
    nb = int(lib.dae_kmeans_assign_workspace(N, K)) * ws_scale
    wp, wt = _ws(nb, fill)
    rec = (ctypes.c_double * 4)()
    L.call("dae_kmeans_assign", xp, N, cp, K, D, L.ptr(pv), L.ptr(labels), L.ptr(scores), rec, wp, nb, L.current_stream())
    labels, scores = labels.cpu().numpy(), scores.cpu().numpy()
    assert (labels[N:] == -7).all() and (scores[N:] == -7).all()       # nothing past N is written
    return labels[:N].astype(np.int64), scores[:N], list(rec)


def _check_assign_equals_topk(X, C):
    from dae_rnn_news_recommendation_amd import helpers
    want_i, want_s = helpers.most_similar(X, 1, metric="linear kernel", candidates=C)
    got_i, got_s = helpers.kmeans_assign(X, C, "linear kernel")
    assert got_i.dtype == np.int64 and got_s.dtype == np.float32
    assert (got_i == want_i[:, 0]).all() and (_bits(got_s) == _bits(want_s[:, 0])).all()
    a = _abi_assign(X, C)
    assert (a[0] == got_i).all() and (_bits(a[1]) == _bits(got_s)).all()
    b = _abi_assign(X, C, ws_scale=2, fill=0xFF)                       # a larger workspace full of other bytes, and a second run
    assert (b[0] == got_i).all() and (_bits(b[1]) == _bits(got_s)).all() and b[2] == a[2]
    assert a[2][0] == pytest.approx(float(got_s.astype(np.float64).sum()), rel=1e-12, abs=1e-12) and a[2][1] == X.shape[0]
    return got_i, got_s, a[2]


@pytest.mark.parametrize("N, K, D", [(300, 130, 70), (1, 1, 3), (129, 5, 200), (100, 1000, 40), (700, 257, 129)])
def test_assign_equals_most_similar_bit_for_bit(N, K, D):
    X, y, centres = R.blobs(N, K, D, 0.05, 0)
    labels, _, rec = _check_assign_equals_topk(X, centres.astype(np.float32))
    assert (labels == y).all()                                         # well-separated blobs against their own centres
    qt, ct = (N + 127) // 128, (K + 127) // 128                       # (700, 257, 129) and (100, 1000, 40) take the split path
    assert rec[3] == max(1, min(512 // qt, ct, 32)) == {(100, 1000): 8, (700, 257): 3, (300, 130): 2}.get((N, K), 1) and rec[2] == rec[3] * qt


def test_assign_when_every_score_is_negative():
    """Rows with positive entries against C = -|blob centres|: every real score is negative, so the zero scores of the padded
    centroid rows K .. 255 would win every row if they competed.  (-centres alone does not do it: random directions in 70
    dimensions have dot products of either sign.)"""
    X, y, centres = R.blobs(300, 130, 70, 0.05, 1)
    X, C = np.abs(X), (-np.abs(centres)).astype(np.float32)
    labels, scores, _ = _check_assign_equals_topk(X, C)
    S = X.astype(np.float64) @ C.astype(np.float64).T
    assert (S.max(axis=1) < 0).all() and (scores < 0).all() and 0 <= labels.min() and labels.max() < 130
    assert (S[np.arange(300), labels] >= S.max(axis=1) - tau(70)).all()
    assert len(np.unique(labels)) > 1


def test_assign_carries_the_best_across_the_tiles_of_a_slice():
    """More centroid tiles than slices, so a workgroup walks several tiles with its running best in registers.
    (100, 4300, 40): 34 tiles over 32 slices, slices 15 and 31 walk two tiles each.  Rows with positive entries; every centroid is
    -|noise| (a negative score) but three copies of |centre[y]|: at columns 1930 + y and 2060 + y (tiles 15 and 16, both of slice 15)
    and at 4200 + y (tile 32, slice 31).  The copy in the FIRST tile of slice 15 must win: carried over the second tile under a
    strict >, and preferred to slice 31's equal score by the finish pass."""
    X, y, centres = R.blobs(100, 40, 40, 0.05, 3)
    X, good = np.abs(X), np.abs(centres).astype(np.float32)
    C = -np.abs(np.random.RandomState(9).randn(4300, 40)).astype(np.float32)
    for first in (1930, 2060, 4200):
        C[first:first + 40] = good
    labels, scores, rec = _check_assign_equals_topk(X, C)
    assert rec[3] == 32 < (4300 + 127) // 128 and rec[2] == 32
    assert (labels == 1930 + y).all() and (scores > 0).all()
    C[1930:1970] = C[0]                                                # without the first copy the second tile of slice 15 wins
    labels, _, _ = _check_assign_equals_topk(X, C)
    assert (labels == 2060 + y).all()


def test_assign_one_slice_of_several_tiles():
    """257 row tiles leave one slice (512 // 257), which then walks all three centroid tiles and finishes inside the sweep kernel --
    the path of every large N.  The second half of the centroids repeats the first 150 rows, so every row's best score occurs twice,
    150 columns apart: in tiles 0 and 1 or in tiles 1 and 2.  The lower column must win."""
    N, K, D = 257 * 128 - 31, 300, 8
    X, _, centres = R.blobs(N, 150, D, 0.3, 4)
    C = np.concatenate([centres, centres]).astype(np.float32)
    labels, _, rec = _check_assign_equals_topk(X, C)
    assert rec[3] == 1 < (K + 127) // 128 and rec[2] == 257
    assert labels.max() < 150 and (np.bincount(labels, minlength=150) > 0).all()
    assert ((labels >= 128) & (labels < 150)).any() and (labels < 106).any()     # ties inside tile 1 + tile 2, and tile 0 + tile 1


def test_assign_duplicated_centroids_go_to_the_lower_id():
    X, y, centres = R.blobs(300, 40, 70, 0.05, 2)
    C = np.concatenate([centres, centres[::-1], centres[5:9]]).astype(np.float32)      # row j, row 79 - j and four more copies
    labels, _, _ = _check_assign_equals_topk(X, C)
    assert (labels == np.minimum(y, 79 - y)).all() and labels.max() < 40
    Z = np.zeros((5, 70), dtype=np.float32)                            # all-zero rows: score 0 everywhere, cluster 0
    zl, zs, _ = _check_assign_equals_topk(Z, C)
    assert (zl == 0).all() and (_bits(zs) == 0).all()


def test_assign_counts_changed_labels():
    X, y, centres = R.blobs(300, 130, 70, 0.05, 0)
    prev = y.copy()
    prev[[0, 7, 128, 299]] = [129, -1, 5, 0]
    want = int((prev != y).sum())
    assert _abi_assign(X, centres.astype(np.float32), prev=prev)[2][1] == want
    Xs, ys, cs = R.blobs(100, 1000, 40, 0.05, 0)                       # the split path
    prev = ys.copy()
    prev[::9] = 1000
    assert _abi_assign(Xs, cs.astype(np.float32), prev=prev)[2][1] == int((prev != ys).sum())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_assign_against_float64(seed):
    from dae_rnn_news_recommendation_amd import helpers
    N, K, D = 300, 130, 70
    X, _, _ = R.blobs(N, K, D, 0.05, seed)
    C = X[np.random.RandomState(100 + seed).choice(N, K, replace=False)]       # rows as centroids: far harder than the centres
    want, _, gap, gaps = R.assign(R.normalize(X), R.normalize(C))
    print(f"seed {seed}: smallest top-2 gap {gap:.3g}, tau {tau(D):.3g}, rows below tau {(gaps < tau(D)).sum()}")
    assert (gaps < tau(D)).mean() < 0.01                               # the condition, from the reference alone
    labels, scores = helpers.kmeans_assign(X, C, "cosine")
    S = R.normalize(X) @ R.normalize(C).T
    chosen = S[np.arange(N), labels]
    print(f"  largest shortfall {float((S.max(axis=1) - chosen).max()):.3g}, labels differing {(labels != want).sum()}")
    assert (chosen >= S.max(axis=1) - tau(D)).all()
    assert (labels != want).mean() <= 0.01
    assert np.abs(scores - chosen).max() <= tau(D)


# ---- the update ----

def _abi_update(X, labels, K, ws_scale=1, fill=0, centroids=True):
    from dae_rnn_news_recommendation_amd import _lib as L
    lib = L.load()
    N, D = X.shape
    xp, xt = _image(lib, L, X, 0)
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    ldc = D + 3
    cent = torch.full((K, ldc), 7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((K + 2,), -7, dtype=torch.int32, device="cuda")
    order = torch.full((N + 2,), -7, dtype=torch.int32, device="cuda")
    offsets = torch.full((K + 3,), -7, dtype=torch.int64, device="cuda")
    nb = int(lib.dae_kmeans_update_workspace(N, K, D)) * ws_scale
    wp, wt = _ws(nb, fill)
    rec = (ctypes.c_double * 4)()
    L.call("dae_kmeans_update", xp, N, D, L.ptr(lab), K, L.ptr(cent) if centroids else None, ldc, L.ptr(counts), L.ptr(order), L.ptr(offsets), rec,
           wp, nb, L.current_stream())
    cent, counts, order, offsets = cent.cpu().numpy(), counts.cpu().numpy(), order.cpu().numpy(), offsets.cpu().numpy()
    assert (cent[:, D:] == 7).all() and (counts[K:] == -7).all() and (order[N:] == -7).all() and (offsets[K + 1:] == -7).all()
    return cent[:, :D], counts[:K], order[:N], offsets[:K + 1], list(rec)


@pytest.mark.parametrize("D", [70, 300])
def test_update_equals_numpy_and_float64(D):
    rng = np.random.RandomState(7)
    N, K = 1500, 9
    labels = rng.randint(4, K, N)
    labels[:600] = 0                                                   # three segments
    labels[600:900] = 1                                                # two
    labels[900:1156] = 3                                               # exactly one full segment; cluster 2 stays empty
    rng.shuffle(labels)
    labels[np.flatnonzero(labels >= 4)[:40]] = np.r_[np.full(25, -1), np.full(15, K + 5)]       # rows that take no part
    X = rng.randn(N, D).astype(np.float32) + 0.5
    cent, counts, order, offsets, rec = _abi_update(X, labels, K)
    inside = (labels >= 0) & (labels < K)
    key = np.where(inside, labels, K)
    assert (counts == np.bincount(labels[inside], minlength=K)).all() and counts[:4].tolist() == [600, 300, 0, 256]
    assert (offsets == np.r_[0, np.cumsum(counts)]).all()
    assert (order == np.argsort(key, kind="stable")).all()
    assert rec[0] == 40 and rec[1] == 1 and rec[2] == 0 and rec[3] == sum((int(c) + 255) // 256 for c in counts)
    want, _ = R.update(R.normalize(X), np.where(inside, labels, -1), K, np.full((K, D), 7.0))
    err = np.abs(cent.astype(np.float64) - want).max()
    print(f"D {D}: largest centroid error {err:.3g} (bound {CENTROID_TOL:.3g})")
    assert (cent[2] == 7).all()                                        # the empty cluster's row is untouched
    assert err <= CENTROID_TOL
    again = _abi_update(X, labels, K)
    wide = _abi_update(X, labels, K, ws_scale=2, fill=0xFF)
    for other in (again, wide):
        assert (_bits(other[0]) == _bits(cent)).all() and (other[1] == counts).all() and (other[2] == order).all() and other[4] == rec
    sort_only = _abi_update(X, labels, K, centroids=False)
    assert (sort_only[0] == 7).all() and (sort_only[2] == order).all() and (sort_only[3] == offsets).all()


def test_update_of_zero_rows_keeps_the_centroid():
    X = np.zeros((10, 5), dtype=np.float32)
    X[5:] = np.eye(5, dtype=np.float32)
    cent, counts, _, _, rec = _abi_update(X, np.r_[np.zeros(5, int), np.ones(5, int)], 2)
    assert (cent[0] == 7).all() and counts.tolist() == [5, 5] and rec[1] == 0 and rec[2] == 1      # n2 == 0 counts as empty
    assert np.abs(cent[1] - 1 / np.sqrt(5)).max() <= CENTROID_TOL


# ---- the iterations ----

TRAJECTORIES = [  # (N, K, D, noise, blob seed, init seed, relocations of the reference run)
    (700, 6, 70, 0.05, 2, 102, 0),                                     # the largest cluster (338) crosses a segment
    (300, 130, 70, 0.05, 0, 100, 0),
    (300, 130, 70, 0.05, 1, 101, 0),
    (300, 130, 70, 0.05, 2, 102, 0),
    (300, 130, 70, 0.05, 4, 104, 2),                                   # two clusters run empty and are relocated
    (700, 12, 70, 0.05, 5, 105, 1),
]


@pytest.mark.parametrize("N, K, D, noise, seed, init_seed, relocations", TRAJECTORIES)
def test_kmeans_follows_the_reference(N, K, D, noise, seed, init_seed, relocations):
    from dae_rnn_news_recommendation_amd import helpers
    X, _, _ = R.blobs(N, K, D, noise, seed)
    init = X[np.random.RandomState(init_seed).choice(N, K, replace=False)]
    ref = R.lloyd(X, init, max_iter=12, tol=0)
    print(f"reference: {ref['n_iter']} updates, smallest gap {min(ref['gaps']):.3g} (tau {tau(D):.3g}), relocation gap "
          f"{min(ref['relocation_gaps']):.3g}, relocated {ref['relocated']}, largest cluster {ref['counts'].max()}")
    assert min(ref["gaps"]) >= tau(D) and min(ref["relocation_gaps"]) >= tau(D)      # the conditions, from the reference alone
    assert ref["relocated"] == relocations and ref["history"][-1][1] == 0
    got = helpers.kmeans(X, K, init=init, max_iter=12, tol=0)
    assert len(got.history) == len(ref["history"]) and got.n_iter == ref["n_iter"] and got.relocated == ref["relocated"]
    assert [h[1] for h in got.history] == [h[1] for h in ref["history"]]
    assert np.allclose([h[0] for h in got.history], [h[0] for h in ref["history"]], rtol=0, atol=tau(D))
    assert (got.labels == ref["labels"]).all() and got.labels.dtype == np.int64
    for t in range(ref["n_iter"]):                                     # the labels of every iteration, not only the last
        step = helpers.kmeans(X, K, init=init, max_iter=t, tol=0)
        assert step.n_iter == t and len(step.history) == t + 1 and (step.labels == ref["all_labels"][t]).all(), t
    err = np.abs(got.centroids.astype(np.float64) - ref["centroids"]).max()
    print(f"largest centroid error {err:.3g} (bound {CENTROID_TOL:.3g})")
    assert err <= CENTROID_TOL
    # the rest of the result describes the final labels
    assert (got.counts == ref["counts"]).all() and (got.offsets == np.r_[0, np.cumsum(ref["counts"])]).all()
    assert (got.order == np.argsort(got.labels, kind="stable")).all()
    assert got.mean_score == got.history[-1][0] == pytest.approx(float(got.scores.astype(np.float64).sum()) / N, rel=1e-12)
    assert got.centroids.dtype == np.float32 and np.abs((got.centroids.astype(np.float64) ** 2).sum(axis=1) - 1).max() < 1e-6


def test_predict_equals_labels_and_sparse_equals_dense():
    sp = pytest.importorskip("scipy.sparse")
    from dae_rnn_news_recommendation_amd import helpers
    X, _, _ = R.blobs(700, 6, 70, 0.05, 2)
    X[np.abs(X) < 0.08] = 0                                            # a sparse matrix worth the name
    X[17] = 0                                                          # and an all-zero row
    dense = helpers.kmeans(X, 6, seed=3, max_iter=3, tol=0)            # stopped by max_iter: the final assignment is a pass of its own
    assert (dense.predict(X) == dense.labels).all()
    li, ls = helpers.kmeans_assign(X, dense.centroids, "cosine")
    assert (li == dense.labels).all() and (_bits(ls) == _bits(dense.scores)).all()
    assert dense.scores[17] == 0 and dense.labels[17] == 0
    sparse = helpers.kmeans(sp.csr_matrix(X), 6, seed=3, max_iter=3, tol=0)
    assert (sparse.labels == dense.labels).all() and (_bits(sparse.centroids) == _bits(dense.centroids)).all()
    assert sparse.history == dense.history and (sparse.predict(sp.csr_matrix(X)) == dense.labels).all()
    t = helpers.kmeans(torch.from_numpy(X).cuda(), 6, seed=3, max_iter=3, tol=0, return_tensor=True)
    assert t.labels.is_cuda and (t.labels.cpu().numpy() == dense.labels).all() and (_bits(t.centroids.cpu().numpy()) == _bits(dense.centroids)).all()
    best = helpers.kmeans(X, 6, seed=3, n_init=3, max_iter=3, tol=0)
    runs = [helpers.kmeans(X, 6, seed=s, max_iter=3, tol=0).mean_score for s in (3, 4, 5)]
    assert best.mean_score == max(runs) and best.seed == 3 + int(np.argmax(runs))
    kept = helpers.kmeans(X, 6, init=np.r_[X[:5], -X[:1]], max_iter=2, tol=0, empty="keep")
    assert kept.relocated == 0


# ---- ClusterIndex ----

@pytest.mark.parametrize("norm, metric", [("", "cosine"), ("l2", "linear kernel"), ("", "linear kernel")])
def test_cluster_index_search(norm, metric):
    from dae_rnn_news_recommendation_amd import helpers
    X, _, _ = R.blobs(300, 12, 70, 0.3, 6)
    X = (X * np.random.RandomState(1).uniform(0.5, 2.0, (300, 1))).astype(np.float32)
    X[40] = X[7]                                                       # equal scores: the caller's lower id first
    X[41] = X[7]
    k = 10
    ix = helpers.ClusterIndex.build(X, 12, norm, metric, seed=1, max_iter=5)
    assert ix.n_clusters == 12 and sorted(ix.order.tolist()) == list(range(300))
    exclude = [[i, (i * 7) % 300, 299 - i] for i in range(300)]
    for kw in (dict(), dict(exclude=exclude)):
        want_i, want_s = helpers.most_similar(X, k, norm, metric, candidates=X, **kw)
        got_i, got_s = ix.search(X, k, n_probe=12, **kw)
        assert got_i.dtype == np.int64 and (got_i == want_i).all() and (_bits(got_s) == _bits(want_s)).all()
    more_i, _ = ix.search(X, k, n_probe=500)                           # more probes than clusters: every cluster
    assert (more_i == helpers.most_similar(X, k, norm, metric, candidates=X)[0]).all()
    # any n_probe: the exact top-k of the members of the probed clusters -- most_similar with every other row excluded
    labels = np.empty(300, dtype=np.int64)
    for c in range(12):
        labels[ix.order[ix.offsets[c]:ix.offsets[c + 1]]] = c
    for n_probe in (1, 3):
        probes, _ = helpers.most_similar(X, n_probe, "", metric, candidates=ix.centroids)
        others = [np.flatnonzero(~np.isin(labels, probes[i])) for i in range(300)]
        want_i, want_s = helpers.most_similar(X, k, norm, metric, candidates=X, exclude=others)
        got_i, got_s = ix.search(X, k, n_probe=n_probe)
        assert (got_i == want_i).all() and (_bits(got_s) == _bits(want_s)).all(), n_probe
        assert 0 < ix.probed_fraction(X, n_probe) <= 1
    t_i, t_s = ix.search(torch.from_numpy(X).cuda(), k, n_probe=3, return_tensor=True)
    assert t_i.is_cuda and (t_i.cpu().numpy() == got_i).all()


# ---- the command line ----

def test_cli_cluster_and_ann_flags(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    monkeypatch.chdir(tmp_path)
    model = cli.main(["--model_name", "topics", "--num_epochs", "1", "--train_row", "300", "--validate_row", "100", "--validation",
                      "--max_features", "600", "--seed", "3", "--similarity", "false", "--cluster", "8", "--cluster_iters", "6",
                      "--cluster_seed", "2", "--sessions", "synthetic", "--recommend", "5", "--ann_clusters", "6", "--ann_probe", "6"])
    out = capsys.readouterr().out
    with np.load(model.data_dir + "article_encoded_clusters.npz") as z:
        labels, centroids, counts, history = z["labels"], z["centroids"], z["counts"], z["history"]
    emb = np.load(model.data_dir + "article_encoded_train.npy")
    emb_v = np.load(model.data_dir + "article_encoded_validate.npy")
    want = helpers.kmeans(emb, 8, max_iter=6, seed=2)
    assert (labels == want.labels).all() and (_bits(centroids) == _bits(want.centroids)).all() and (counts == want.counts).all()
    assert history.shape == (len(want.history), 2) and counts.sum() == 300
    with np.load(model.data_dir + "article_encoded_validate_clusters.npz") as z:
        assert (z["labels"] == helpers.kmeans_assign(emb_v, centroids)[0]).all() and z["labels"].shape == (100,)
    assert "calculate clusters 8" in out and "purity" in out and "NMI" in out and "ARI" in out and "validate  mean score" in out
    # every cluster probed: the index returns the exact lists
    with np.load(model.data_dir + "article_encoded_recommend5.npz") as z, np.load(model.data_dir + "article_encoded_recommend5_ann.npz") as y:
        assert (z["indices"] == y["indices"]).all() and (_bits(z["scores"]) == _bits(y["scores"])).all() and int(y["n_probe"]) == 6
        assert y["offsets"].shape == (7,) and sorted(y["order"].tolist()) == list(range(300))
    assert "recall@5 against the exact lists 1.0000, 1.0000 of the corpus scored per user" in out and "cluster index" in out
