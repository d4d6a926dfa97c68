"""GPU checks of the label statistics without the N x N matrix (dae_pair_hist through helpers.label_similarity_stats) against
NumPy (exact arithmetic), the fp64 oracle, and the matrix route on the device; and of the CLI's --label_stats.

Against the fp64 oracle a device score is trusted to delta = 1e-5 x the largest |score| among the counted pairs (the relative
tolerance test_hip_near_dup.py / test_hip_topk.py use).  Every cumulative count of a histogram is bracketed two-sidedly by the
oracle's counts below (edge - delta) and (edge + delta); the oracle's exact AUROC must lie in the reported bracket widened by
eta = the share of (related, unrelated) pairs whose oracle scores differ by at most 2 delta, and the bracket must be no wider
than the tie mass of the oracle's own binned scores + 2 eta.  So that eta cannot hide a failure, each case first asserts on the
oracle alone that eta <= 0.1 x that tie mass."""
import json

import numpy as np
import pytest
import torch
from scipy import sparse

import oracle as O

pytestmark = pytest.mark.gpu

Q3 = (("q1", 25), ("median", 50), ("q3", 75))


# ---- restatements on the host ---------------------------------------------------------------------------------------------------
def populations(S, labels, labels_c=None):
    """Sorted related / unrelated scores of the score matrix S: the strict lower triangle (labels_c None) or the whole rectangle."""
    S = np.asarray(S)
    lq = np.asarray(labels)
    lc = lq if labels_c is None else np.asarray(labels_c)
    ok = (lq[:, None] >= 0) & (lc[None, :] >= 0)
    if labels_c is None:
        ok &= np.tril(np.ones(S.shape, bool), -1)
    same = lq[:, None] == lc[None, :]
    return np.sort(S[ok & same]), np.sort(S[ok & ~same])


def exact_auroc(rel, un):
    """Tie-aware AUROC of two sorted populations (what oracle.pair_stats computes by ranks)."""
    twice = np.searchsorted(un, rel, "left").astype(np.float64).sum() + np.searchsorted(un, rel, "right").astype(np.float64).sum()
    return twice / (2.0 * len(rel) * len(un))


def near_share(rel, un, delta):
    """eta: the share of (related, unrelated) pairs whose scores differ by at most 2 delta."""
    n = np.searchsorted(un, rel + 2 * delta, "right") - np.searchsorted(un, rel - 2 * delta, "left")
    return float(n.astype(np.float64).sum()) / (len(rel) * len(un))


def bin_index(s, lo, hi, bins):
    """The library's bin of a score, in fp32 exactly as the header writes it."""
    s, lo, hi = np.asarray(s, np.float32), np.float32(lo), np.float32(hi)
    x = np.floor((s - lo) * np.float32(bins) / (hi - lo))
    return np.clip(x, 0, bins - 1).astype(np.int64)


def binned_tie_mass(rel, un, lo, hi, bins):
    hr = np.bincount(bin_index(rel, lo, hi, bins), minlength=bins).astype(np.float64)
    hu = np.bincount(bin_index(un, lo, hi, bins), minlength=bins).astype(np.float64)
    return float((hr * hu).sum()) / (len(rel) * len(un))


def check_against_oracle(res, rel, un, label=""):
    """Rule of the module docstring; res from label_similarity_stats(..., return_histograms=True).  Returns (auroc, eta, tie)."""
    delta = 1e-5 * max(np.abs(rel).max(), np.abs(un).max())
    lo, hi = res["score_range"]
    bins = res["bins"]
    tie = binned_tie_mass(rel, un, lo, hi, bins)
    eta = near_share(rel, un, delta)
    auroc = exact_auroc(rel, un)
    width = res["auroc_high"] - res["auroc_low"]
    print(f"{label}: oracle AUROC {auroc:.6f}, device [{res['auroc_low']:.6f}, {res['auroc_high']:.6f}] width {width:.3e}, "
          f"oracle tie mass {tie:.3e}, eta {eta:.3e} (eta / tie {eta / tie:.4f}), delta {delta:.3e}, range [{lo:.6g}, {hi:.6g}]")
    assert eta <= 0.1 * tie, (eta, tie)                                 # on the oracle alone
    assert res["n_related"] == len(rel) and res["n_unrelated"] == len(un) and res["n_nan"] == 0
    edges = res["bin_edges"]
    for name, v, h in (("related", rel, res["hist_related"]), ("unrelated", un, res["hist_unrelated"])):
        assert int(h.sum()) == len(v)
        five = res[name]
        print(f"   {name}: min err {abs(five['min'] - v[0]):.2e}, max err {abs(five['max'] - v[-1]):.2e}, "
              f"mean err {abs(res['mean_' + name] - v.mean()):.2e}")
        assert abs(five["min"] - v[0]) <= delta and abs(five["max"] - v[-1]) <= delta
        assert abs(res["mean_" + name] - v.mean()) <= delta
        below = np.concatenate([[0], np.cumsum(h.astype(np.int64))])[1:bins]          # device count below edges[1 .. bins - 1]
        least = np.searchsorted(v, edges[1:bins] - delta, "left")
        most = np.searchsorted(v, edges[1:bins] + delta, "left")
        assert (least <= below).all() and (below <= most).all(), name
        for k, q in Q3:
            want = np.percentile(v, q)
            b = res[name + "_bounds"][k]
            assert b[0] - delta <= want <= b[1] + delta, (name, k, b, want)
            assert b[0] <= five[k] <= b[1]
    assert res["auroc_low"] - eta <= auroc <= res["auroc_high"] + eta
    assert res["auroc_low"] <= res["auroc"] <= res["auroc_high"]
    assert width <= tie + 2 * eta
    return auroc, eta, tie


def clustered(seed=11, N=1500, D=64, classes=12, centre=0.35):
    """Rows = centre x class centre + standard-normal noise; 5 % of the labels missing (-1)."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes, N)
    X = (centre * rng.standard_normal((classes, D))[labels] + rng.standard_normal((N, D))).astype(np.float32)
    labels[rng.random(N) < 0.05] = -1
    return X, labels


@pytest.fixture(scope="module")
def data1500():
    return clustered()


# ---- 5. exact arithmetic --------------------------------------------------------------------------------------------------------
def _integer_rows():
    rng = np.random.default_rng(5)
    base = rng.integers(-2, 3, (40, 24)).astype(np.float32)
    X = base[rng.integers(0, 40, 700)]                                            # ~17 copies of every row
    labels = rng.integers(0, 6, 700)
    labels[rng.random(700) < 0.1] = -1
    return X, labels


def _check_exact(res, rel, un, R):
    """Every bin of (-R - 0.5, R + 0.5) with 2R + 1 bins holds one integer score: the histograms are NumPy's, the rest is exact."""
    hr = np.bincount((rel + R).astype(np.int64), minlength=2 * R + 1)
    hu = np.bincount((un + R).astype(np.int64), minlength=2 * R + 1)
    assert res["hist_related"].dtype == np.uint64 and res["hist_unrelated"].dtype == np.uint64
    assert np.array_equal(res["hist_related"], hr.astype(np.uint64)) and np.array_equal(res["hist_unrelated"], hu.astype(np.uint64))
    assert res["n_related"] == len(rel) and res["n_unrelated"] == len(un) and res["n_nan"] == 0
    assert abs(res["auroc"] - exact_auroc(rel, un)) <= 1e-12
    tie = float((hr.astype(np.float64) * hu).sum()) / (len(rel) * len(un))
    assert tie > 0.01 and abs((res["auroc_high"] - res["auroc_low"]) - tie) <= 1e-12
    for name, v in (("related", rel), ("unrelated", un)):
        assert res[name]["min"] == v[0] and res[name]["max"] == v[-1]
        assert abs(res["mean_" + name] - v.mean()) <= 1e-12
        for k, q in Q3:
            want = np.percentile(v, q)
            assert abs(res[name][k] - want) <= 1e-12, (name, k)
            b = res[name + "_bounds"][k]
            assert b[0] <= want <= b[1] and b[0] <= np.floor(want) and np.ceil(want) <= b[1]


def test_exact_arithmetic_matches_numpy_bit_for_bit():
    from dae_rnn_news_recommendation_amd import helpers
    X, labels = _integer_rows()
    S = X.astype(np.float64) @ X.T.astype(np.float64)
    R = int(np.abs(S).max())
    assert 2 * R + 1 <= 2048
    assert (labels < 0).sum() > 20
    res = helpers.label_similarity_stats(X, labels, metric="linear kernel", bins=2 * R + 1, score_range=(-R - 0.5, R + 0.5),
                                         return_histograms=True)
    rel, un = populations(S, labels)
    _check_exact(res, rel, un, R)
    want = O.pair_stats(labels, S)                                                 # and the oracle's own restatement
    assert res["n_related"] == want["n_related"] and res["n_unrelated"] == want["n_unrelated"]
    assert abs(res["auroc"] - want["auroc"]) <= 1e-12
    for name in ("related", "unrelated"):
        assert abs(res["mean_" + name] - want["mean_" + name]) <= 1e-12
        for k in ("min", "q1", "median", "q3", "max"):
            assert abs(res[name][k] - want[name][k]) <= 1e-12
    # float labels with NaN / inf / negative values are the same missing labels
    lf = labels.astype(np.float64)
    lf[labels < 0] = np.array([np.nan, np.inf, -3.0])[np.arange((labels < 0).sum()) % 3]
    again = helpers.label_similarity_stats(X, lf, metric="linear kernel", bins=2 * R + 1, score_range=(-R - 0.5, R + 0.5),
                                           return_histograms=True)
    assert np.array_equal(again["hist_related"], res["hist_related"]) and again["auroc"] == res["auroc"]


def test_exact_arithmetic_with_candidates():
    from dae_rnn_news_recommendation_amd import helpers
    X, labels = _integer_rows()
    Q, C, lq, lc = X[:300], X[300:], labels[:300], labels[300:]
    S = Q.astype(np.float64) @ C.T.astype(np.float64)
    R = int(np.abs(X.astype(np.float64) @ X.T.astype(np.float64)).max())
    res = helpers.label_similarity_stats(Q, lq, metric="linear kernel", candidates=C, candidate_labels=lc, bins=2 * R + 1,
                                         score_range=(-R - 0.5, R + 0.5), return_histograms=True)
    rel, un = populations(S, lq, lc)                                               # every (query, candidate) pair, the diagonal too
    assert len(rel) + len(un) == int((lq >= 0).sum()) * int((lc >= 0).sum())
    _check_exact(res, rel, un, R)
    with pytest.raises(ValueError, match="go together"):
        helpers.label_similarity_stats(Q, lq, candidates=C)
    with pytest.raises(ValueError, match="columns"):
        helpers.label_similarity_stats(Q, lq, candidates=C[:, :20], candidate_labels=lc)
    with pytest.raises(ValueError, match="labels for"):
        helpers.label_similarity_stats(Q, lq[:-1])
    with pytest.raises(ValueError, match="bins"):
        helpers.label_similarity_stats(Q, lq, bins=4096)


# ---- 6. real values against the fp64 oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm, metric", [("", "cosine"), ("l2", "linear kernel"), ("", "linear kernel"), ("l1", "linear kernel"),
                                          ("max", "linear kernel"), ("l1", "cosine"), ("max", "cosine")])
def test_dense_random_all_norms(data1500, norm, metric):
    from dae_rnn_news_recommendation_amd import helpers
    X, labels = data1500
    S = O.pairwise_similarity(X, norm=norm, metric=metric, set_diagonal_zero=False)
    rel, un = populations(S, labels)
    res = helpers.label_similarity_stats(X, labels, norm=norm, metric=metric, return_histograms=True)
    assert res["bins"] == 2048
    auroc, _, _ = check_against_oracle(res, rel, un, f"norm={norm!r} metric={metric!r}")
    assert 0.6 < auroc < 0.9                                                       # well away from 0.5 and 1
    if metric == "cosine":
        assert res["score_range"] == (-1.0, 1.0)
    else:                                                                          # Cauchy-Schwarz: no score leaves the range
        assert res["score_range"][0] == -res["score_range"][1] and res["score_range"][1] >= max(np.abs(rel).max(), np.abs(un).max())
        assert res["score_range"][1] <= 1.001 * np.sqrt((_normed(X, norm) ** 2).sum(axis=1)).max() ** 2


def _normed(X, norm):
    X = X.astype(np.float64)
    if norm == "":
        return X
    n = {"l1": np.abs(X).sum(axis=1), "l2": np.sqrt((X * X).sum(axis=1)), "max": np.abs(X).max(axis=1)}[norm]
    return X / np.where(n == 0, 1.0, n)[:, None]


def test_queries_against_a_corpus(data1500):
    from dae_rnn_news_recommendation_amd import helpers
    X, labels = data1500
    Q, C, lq, lc = X[:333], X[333:], labels[:333], labels[333:]
    S = O.pairwise_similarity(X, metric="cosine", set_diagonal_zero=False)[:333, 333:]
    rel, un = populations(S, lq, lc)
    res = helpers.label_similarity_stats(Q, lq, candidates=C, candidate_labels=lc, return_histograms=True)
    check_against_oracle(res, rel, un, "candidates")
    coarse = helpers.label_similarity_stats(Q, lq, candidates=C, candidate_labels=lc, bins=64, return_histograms=True)
    check_against_oracle(coarse, rel, un, "candidates, 64 bins")
    assert coarse["auroc_high"] - coarse["auroc_low"] > 10 * (res["auroc_high"] - res["auroc_low"])     # a coarse grid shows as a wide bracket


# ---- 7. refine ------------------------------------------------------------------------------------------------------------------
def test_refine_narrows_the_bracket_of_raw_linear_scores(data1500):
    from dae_rnn_news_recommendation_amd import helpers
    X, labels = data1500
    X = X.copy()
    X[700] *= 10.0
    assert labels[700] >= 0
    S = O.pairwise_similarity(X, metric="linear kernel", set_diagonal_zero=False)
    rel, un = populations(S, labels)
    first = helpers.label_similarity_stats(X, labels, metric="linear kernel", return_histograms=True)
    second = helpers.label_similarity_stats(X, labels, metric="linear kernel", refine=True, return_histograms=True)
    check_against_oracle(first, rel, un, "automatic range")
    check_against_oracle(second, rel, un, "refined")
    delta = 1e-5 * max(np.abs(rel).max(), np.abs(un).max())
    assert abs(second["score_range"][0] - min(rel[0], un[0])) <= delta and abs(second["score_range"][1] - max(rel[-1], un[-1])) <= delta
    assert second["first_pass"]["auroc_low"] == first["auroc_low"] and second["first_pass"]["score_range"] == first["score_range"]
    w1, w2 = first["auroc_high"] - first["auroc_low"], second["auroc_high"] - second["auroc_low"]
    print(f"bracket width {w1:.3e} -> {w2:.3e} ({w1 / w2:.1f} x)")
    assert w2 * 5 <= w1


# ---- 8. against the matrix route on the device ----------------------------------------------------------------------------------
def _device_clustered(N, D, classes, centre, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lab = torch.randint(0, classes, (N,), device="cuda", generator=g)
    X = centre * torch.randn((classes, D), device="cuda", generator=g)[lab] + torch.randn((N, D), device="cuda", generator=g)
    lab[torch.rand((N,), device="cuda", generator=g) < 0.05] = -1
    return X, lab.cpu().numpy()


def matrix_route_in_bracket(res, labels, S, label=""):
    """Rule 8: the exact AUROC of the device matrix S lies in the bracket widened by eta computed from that matrix."""
    from dae_rnn_news_recommendation_amd import helpers
    vis = helpers.visualize_pairwise_similarity(labels, S)
    Sh = S.cpu().numpy() if isinstance(S, torch.Tensor) else np.asarray(S)
    rel, un = populations(Sh.astype(np.float64), labels)
    delta = 1e-5 * max(np.abs(rel).max(), np.abs(un).max())
    eta = near_share(rel, un, delta)
    tie = binned_tie_mass(rel, un, *res["score_range"], res["bins"])
    print(f"{label}: matrix route AUROC {vis['auroc']:.6f}, bracket [{res['auroc_low']:.6f}, {res['auroc_high']:.6f}], eta {eta:.3e}, "
          f"tie mass {tie:.3e}")
    assert eta <= 0.1 * tie
    assert res["n_related"] == vis["n_related"] and res["n_unrelated"] == vis["n_unrelated"]
    assert res["auroc_low"] - eta <= vis["auroc"] <= res["auroc_high"] + eta
    return vis


def test_against_the_matrix_route_at_8000_x_500():
    from dae_rnn_news_recommendation_amd import helpers
    X, labels = _device_clustered(8000, 500, 20, 0.15, 3)
    res = helpers.label_similarity_stats(X, labels)
    S = helpers.pairwise_similarity(X, return_tensor=True)
    vis = matrix_route_in_bracket(res, labels, S, "8000 x 500")
    assert 0.55 < vis["auroc"] < 0.95
    assert set(vis) <= set(res)                                                    # a caller can switch routes
    for name in ("related", "unrelated"):
        assert abs(res["mean_" + name] - vis["mean_" + name]) <= 1e-5
        for k in ("min", "max"):
            assert abs(res[name][k] - vis[name][k]) <= 1e-5
        for k, _ in Q3:
            b = res[name + "_bounds"][k]
            assert b[0] - 1e-5 <= vis[name][k] <= b[1] + 1e-5
    del S


# ---- 9. determinism, independence of the grid -----------------------------------------------------------------------------------
def test_deterministic_and_independent_of_the_grid():
    from dae_rnn_news_recommendation_amd import helpers
    X, labels = clustered(seed=2, N=5200, D=64, classes=15)                         # 41 x 42 / 2 = 861 tiles: strips hold several tiles
    for metric in ("cosine", "linear kernel"):
        a = helpers.label_similarity_stats(X, labels, metric=metric, return_histograms=True)
        b = helpers.label_similarity_stats(X, labels, metric=metric, return_histograms=True)
        assert a["n_related"] > 0 and a["n_unrelated"] > 0
        for k in ("hist_related", "hist_unrelated", "bin_edges"):
            assert np.array_equal(a[k], b[k])
        assert {k: v for k, v in a.items() if not isinstance(v, np.ndarray)} == {k: v for k, v in b.items() if not isinstance(v, np.ndarray)}
        perm = np.random.default_rng(8).permutation(len(X))                        # every pair moves to another tile, strip and operand side
        c = helpers.label_similarity_stats(X[perm], labels[perm], metric=metric, return_histograms=True)
        assert np.array_equal(a["hist_related"], c["hist_related"]) and np.array_equal(a["hist_unrelated"], c["hist_unrelated"])
        for k in ("n_related", "n_unrelated", "n_nan", "auroc", "auroc_low", "auroc_high", "score_range", "related_bounds"):
            assert a[k] == c[k], k
        for name in ("related", "unrelated"):
            assert a[name] == c[name]
            assert abs(a["mean_" + name] - c["mean_" + name]) <= 1e-12 * abs(a["mean_" + name])
        # self mode = the lower triangle; the rectangle of X against itself counts every ordered pair and the diagonal
        full = helpers.label_similarity_stats(X, labels, metric=metric, candidates=X, candidate_labels=labels, return_histograms=True)
        n_lab = int((labels >= 0).sum())
        assert full["n_related"] == 2 * a["n_related"] + n_lab and full["n_unrelated"] == 2 * a["n_unrelated"]
        assert np.array_equal(full["hist_unrelated"], 2 * a["hist_unrelated"])


def test_nan_scores_are_counted_apart():
    from dae_rnn_news_recommendation_amd import helpers
    X, labels = clustered(seed=4, N=400, D=32, classes=5)
    labels[7] = 1
    base = helpers.label_similarity_stats(np.delete(X, 7, axis=0), np.delete(labels, 7), return_histograms=True)
    X[7, 3] = np.nan                                                               # every score of row 7 is NaN
    res = helpers.label_similarity_stats(X, labels, return_histograms=True)
    assert res["n_nan"] == int((labels >= 0).sum()) - 1
    assert np.array_equal(res["hist_related"], base["hist_related"]) and np.array_equal(res["hist_unrelated"], base["hist_unrelated"])
    assert res["auroc"] == base["auroc"] and res["related"]["max"] == base["related"]["max"]


# ---- 10. no N x N buffer --------------------------------------------------------------------------------------------------------
def test_no_n_by_n_buffer():
    from dae_rnn_news_recommendation_amd import helpers
    N, D = 60000, 128
    X, labels = _device_clustered(N, D, 20, 0.3, 1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    res = helpers.label_similarity_stats(X, labels)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    print(f"peak growth {grow} bytes; AUROC [{res['auroc_low']:.5f}, {res['auroc_high']:.5f}]")
    assert grow < N * N * 4 // 8, grow
    n_lab = int((labels >= 0).sum())
    assert res["n_related"] + res["n_unrelated"] == n_lab * (n_lab - 1) // 2
    counts = np.bincount(labels[labels >= 0])
    assert res["n_related"] == int((counts * (counts - 1) // 2).sum())
    assert 0.6 < res["auroc_low"] <= res["auroc"] <= res["auroc_high"] < 1.0 and res["auroc_high"] - res["auroc_low"] < 0.01


# ---- 11. containers -------------------------------------------------------------------------------------------------------------
def test_sparse_bow_and_tensor_inputs():
    from dae_rnn_news_recommendation_amd import helpers
    bow = sparse.random(500, 3000, density=0.02, random_state=np.random.RandomState(3), format="csr", dtype=np.float32)
    bow.data[:] = 1.0
    dense = bow.toarray()
    labels = np.random.default_rng(3).integers(0, 7, 500)
    a = helpers.label_similarity_stats(bow, labels, return_histograms=True)
    b = helpers.label_similarity_stats(dense, labels, return_histograms=True)
    t = helpers.label_similarity_stats(torch.from_numpy(dense).cuda(), labels, return_histograms=True)
    l = helpers.label_similarity_stats(dense.tolist(), labels.tolist(), return_histograms=True)
    assert a["n_related"] > 0 and a["hist_related"].sum() == a["n_related"]
    for other in (b, t, l):
        for k, v in a.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, other[k]), k
            else:
                assert v == other[k] or (v != v and other[k] != other[k]), k
    rel, un = populations(O.pairwise_similarity(bow, set_diagonal_zero=False), labels)
    assert a["n_related"] == len(rel) and a["n_unrelated"] == len(un)
    assert abs(a["mean_related"] - rel.mean()) <= 1e-5 and abs(a["mean_unrelated"] - un.mean()) <= 1e-5


# ---- 12. CLI --------------------------------------------------------------------------------------------------------------------
CLI = ["--model_name", "ls", "--num_epochs", "1", "--train_row", "400", "--validate_row", "150", "--validation", "--max_features", "800",
       "--seed", "4"]
STEMS = ("binary_count", "encoded", "binary_count_validate", "encoded_validate")


def _job_inputs(model, helpers):
    """(matrix, label ids) of the four jobs, from the artefacts the run saved."""
    d = model.data_dir
    y = {v: helpers.read_file(d + "article_label_category_publish_name" + v + ".pkl", data_type="pandas_series").to_numpy()
         for v in ("", "_validate")}
    ids = {v: np.unique(y[v], return_inverse=True)[1] for v in y}
    return {"binary_count": (helpers.read_file(d + "article_binary_count_vectorized.npz"), ids[""]),
            "encoded": (np.load(d + "article_encoded_train.npy"), ids[""]),
            "binary_count_validate": (helpers.read_file(d + "article_binary_count_vectorized_validate.npz"), ids["_validate"]),
            "encoded_validate": (np.load(d + "article_encoded_validate.npy"), ids["_validate"])}


def test_cli_label_stats_without_the_matrix(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    monkeypatch.chdir(tmp_path)
    model = cli.main(CLI + ["--similarity", "false", "--label_stats"])
    out = capsys.readouterr().out
    assert "calculate similarity" not in out and "calculate label statistics" in out
    lines = [ln for ln in out.splitlines() if "AUROC" in ln]
    assert len(lines) == 4 and all("[" in ln and "]" in ln for ln in lines)
    got = {}
    for stem in STEMS:
        with open(model.plot_dir + "similarity_stats_" + stem + ".json") as fh:
            got[stem] = json.load(fh)
        assert got[stem]["auroc_low"] <= got[stem]["auroc"] <= got[stem]["auroc_high"]
    emb, ids = _job_inputs(model, helpers)["encoded"]
    want = helpers.label_similarity_stats(emb, ids, title="embedding (train)")
    assert json.loads(json.dumps(want)) == got["encoded"]
    assert got["encoded"]["n_related"] + got["encoded"]["n_unrelated"] == 400 * 399 // 2


def test_cli_label_stats_beside_the_matrix_route(tmp_path, monkeypatch, capsys):
    """Rule 8 per job (on the oracle the binary bag-of-words jobs have eta / tie = 0.03: their cosines k / sqrt(n_i n_j)
    tie exactly across the classes now and then, far less often than they share a bin)."""
    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    monkeypatch.chdir(tmp_path)
    model = cli.main(CLI + ["--similarity", "true", "--label_stats"])
    out = capsys.readouterr().out
    assert "calculate similarity" in out and "calculate label statistics" in out
    assert len([ln for ln in out.splitlines() if "AUROC" in ln]) == 8
    for stem, (M, ids) in _job_inputs(model, helpers).items():
        with open(model.plot_dir + "similarity_boxplot_" + stem + ".json") as fh:
            vis = json.load(fh)
        with open(model.plot_dir + "similarity_stats_" + stem + ".json") as fh:
            res = json.load(fh)
        S = helpers.pairwise_similarity(M, return_tensor=True)
        again = matrix_route_in_bracket(res, ids, S, stem)
        assert again["auroc"] == vis["auroc"] and again["related"] == vis["related"]          # the existing files are unchanged
