"""GPU checks of the sparse / chunked operands of top-k and label statistics: the operand image built from CSR rows
(csr_row_normalize_kernel) equals the one built from the densified rows, and helpers.most_similar / label_similarity_stats with
chunk_rows= equal the one-shot route -- indices, scores, histograms, counts, min, max and the score range exactly, the means to
1e-12 relative (their fp64 sums are folded in another order)."""
import ctypes
import json

import numpy as np
import pytest
import torch
from scipy import sparse

from test_hip_topk import _check, _ref_scores

pytestmark = pytest.mark.gpu

NORMS = {"": 0, "l1": 1, "l2": 2, "max": 3}
CHUNKS = (128, 256, 1024)


# ---- the image ---------------------------------------------------------------------------------------------------------------------
def _csr(rows, D, rng):
    """A CSR matrix from a list of (columns, values) rows, stored exactly as given (explicit zeros stay stored)."""
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(c) for c, _ in rows])
    indices = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows]) if indptr[-1] else np.zeros(0, np.int32)
    data = np.concatenate([np.asarray(v, dtype=np.float32) for _, v in rows]) if indptr[-1] else np.zeros(0, np.float32)
    m = sparse.csr_matrix((data, indices, indptr), shape=(len(rows), D))
    assert m.has_sorted_indices and m.nnz == indptr[-1]
    return m


def _special_matrix(N, D, density, seed, extra=()):
    """N x D: row 0 empty, row 1 fully dense, row 2 the columns j, j + 256, j + 512 (one thread of the fold; as many as fit),
    row 3 with a stored explicit zero, row 4 with the last column set, then the rows `extra`, the rest at `density`."""
    rng = np.random.default_rng(seed)
    val = lambda n: (rng.standard_normal(n) * rng.choice([0.01, 1.0, 30.0], n)).astype(np.float32)      # noqa: E731
    rows = [([], []), (np.arange(D), val(D))]
    same = [j for j in (7, 7 + 256, 7 + 512) if j < D]
    rows.append((same, val(len(same))))
    c3 = np.sort(rng.choice(D, 5, replace=False))
    v3 = val(5); v3[2] = 0.0
    rows.append((c3, v3))
    c4 = np.sort(np.concatenate([rng.choice(D - 1, 3, replace=False), [D - 1]]))
    rows.append((c4, val(4)))
    rows += list(extra)
    while len(rows) < N:
        n = max(1, rng.binomial(D, density))
        rows.append((np.sort(rng.choice(D, n, replace=False)), val(n)))
    return _csr(rows, D, rng)


def _images(m, binary, row0=0):
    """For every norm x metric: (image from CSR rows [row0, N), image from the densified rows), as float32 [Np x Dp] arrays."""
    from dae_rnn_news_recommendation_amd import _lib as L
    lib = L.load()
    N, D = m.shape
    rows = N - row0
    ip = torch.from_numpy(m.indptr.astype(np.int64)).cuda()
    ix = torch.from_numpy(m.indices.astype(np.int32)).cuda()
    vl = None if binary else torch.from_numpy(m.data.astype(np.float32)).cuda()
    dense = m.toarray()
    if binary:                                                                     # values == NULL: every stored entry is 1
        dense = sparse.csr_matrix((np.ones(m.nnz, np.float32), m.indices, m.indptr), shape=m.shape).toarray()
    X = torch.from_numpy(np.ascontiguousarray(dense[row0:])).cuda()
    nb = int(lib.dae_sweep_image_bytes(rows, D))
    Np, Dp = L.pad(rows), L.pad(D)
    assert nb == Np * Dp * 4
    out = []
    for norm in NORMS.values():
        for metric in (0, 1):
            a = torch.full((Np, Dp), float("nan"), dtype=torch.float32, device="cuda")     # garbage: every word must be written
            b = torch.full((Np, Dp), float("nan"), dtype=torch.float32, device="cuda")
            L.call("dae_sweep_image_csr", ctypes.c_void_p(ip.data_ptr() + 8 * row0), L.ptr(ix), L.ptr(vl), rows, D, norm, metric, L.ptr(a),
                   nb, L.current_stream())
            L.call("dae_sweep_image_dense", L.ptr(X), X.stride(0), rows, D, norm, metric, L.ptr(b), nb, L.current_stream())
            out.append((norm, metric, a.cpu().numpy(), b.cpu().numpy()))
    return out


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("N,D,density", [(200, 1000, 0.02), (200, 70, 0.02), (40, 20000, 0.02)])
def test_csr_image_equals_the_dense_image(N, D, density, binary):
    """200 x 1000, D = 70 (below 256 and no multiple of 128) and D = 20 000 (three LDS windows of the CSR kernel, the last one
    ragged), with values and with values == NULL, every norm x metric."""
    extra = ()
    if D == 20000:                                                                 # rows whose stored entries skip whole windows
        extra = (([16390, 19999], [2.5, -1.5]),                                    # only the last window
                 ([3, 8191, 16384], [1.0, 2.0, 3.0]),                              # the middle window empty; both edges of the first
                 ([8192], [4.0]))                                                  # first word of the second window
    m = _special_matrix(N, D, density, seed=D, extra=extra)
    for norm, metric, a, b in _images(m, binary):
        assert np.isfinite(b).all()
        assert np.array_equal(a, b), (norm, metric, np.argwhere(a != b)[:5])
        assert not a[N:].any() and not a[:, D:].any()                              # the padding is zero
    if D == 1000 and not binary:                                                   # a chunk: indptr points at its first row, offsets stay absolute
        full = {(n, t): b for n, t, _, b in _images(m, False)}
        for norm, metric, a, b in _images(m, False, row0=64):
            assert np.array_equal(a, b) and np.array_equal(a[:N - 64], full[(norm, metric)][64:N])
    if D == 1000 and binary:
        got = {(n, t): a for n, t, a, _ in _images(m, True)}
        assert (got[(0, 1)][3] != 0).sum() == 5                                    # the stored zero counts as 1 without values


# ---- top-k -------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype


@pytest.fixture(scope="module")
def bow():
    m = sparse.random(500, 3000, density=0.02, random_state=np.random.RandomState(3), format="csr", dtype=np.float32)
    m.data[:] = 1.0
    return m


@pytest.fixture(scope="module")
def ties():
    rng = np.random.default_rng(5)
    base = rng.integers(-2, 3, (40, 24)).astype(np.float32)
    return base[rng.integers(0, 40, 700)]                                          # ~17 copies of every row: ties cross chunks


def test_topk_bow_chunked_equals_one_shot(bow):
    from dae_rnn_news_recommendation_amd import helpers
    S = _ref_scores(bow, "", "cosine")
    for k, excl in ((1, True), (37, True), (128, True), (37, False)):
        ref = helpers.most_similar(bow, k=k, exclude_self=excl)
        for c in CHUNKS:
            got = helpers.most_similar(bow, k=k, exclude_self=excl, chunk_rows=c)
            assert _same(got, ref), (k, excl, c)
        if k == 37:
            _check(got[0], got[1], S, k, exclude_self=excl)                        # and against fp64
    ref = helpers.most_similar(bow, k=10, norm="l1", metric="linear kernel")       # tf-idf's route: a norm, the linear kernel
    assert _same(helpers.most_similar(bow, k=10, norm="l1", metric="linear kernel", chunk_rows=128), ref)
    assert _same(helpers.most_similar(bow, k=10, norm="l1", metric="linear kernel", chunk_rows="auto"), ref)
    assert _same(helpers.most_similar(bow.toarray(), k=10, norm="l1", metric="linear kernel", chunk_rows=256), ref)   # dense row slices


def test_topk_exact_ties_across_chunks(ties):
    from dae_rnn_news_recommendation_amd import helpers
    S = ties.astype(np.float64) @ ties.T.astype(np.float64)
    for k, excl in ((1, True), (37, True), (128, True), (37, False), (128, False)):
        ref = helpers.most_similar(ties, k=k, metric="linear kernel", exclude_self=excl)
        R = S.copy()
        if excl:
            np.fill_diagonal(R, -np.inf)
        want = np.argsort(-R, axis=1, kind="stable")[:, :k]
        assert np.array_equal(ref[0], want)
        for c in CHUNKS:
            got = helpers.most_similar(ties, k=k, metric="linear kernel", exclude_self=excl, chunk_rows=c)
            assert _same(got, ref), (k, excl, c)
        t = torch.from_numpy(ties).cuda()                                          # a device tensor, returned as tensors
        gi, gs = helpers.most_similar(t, k=k, metric="linear kernel", exclude_self=excl, chunk_rows=256, return_tensor=True)
        assert gi.is_cuda and gi.dtype == torch.int64 and _same((gi.cpu().numpy(), gs.cpu().numpy()), ref)


def test_topk_queries_against_candidates():
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((129, 90)).astype(np.float32)
    C = rng.standard_normal((1000, 90)).astype(np.float32)
    C[300:420] = C[:120]                                                           # duplicates in other chunks
    Cs = sparse.random(1000, 90, density=0.1, random_state=np.random.RandomState(2), format="csr", dtype=np.float32)
    for metric in ("cosine", "linear kernel"):
        for k in (1, 37, 128):
            ref = helpers.most_similar(Q, k=k, metric=metric, candidates=C)
            for c in CHUNKS:
                assert _same(helpers.most_similar(Q, k=k, metric=metric, candidates=C, chunk_rows=c), ref), (metric, k, c)
        ref = helpers.most_similar(Q, k=16, metric=metric, candidates=Cs)          # dense queries against a CSR corpus
        assert _same(helpers.most_similar(Q, k=16, metric=metric, candidates=Cs, chunk_rows=128), ref)
    with pytest.raises(ValueError, match="exclude_self"):
        helpers.most_similar(Q, k=5, candidates=C, exclude_self=True, chunk_rows=128)
    with pytest.raises(RuntimeError, match="k must be in 1..128"):
        helpers.most_similar(Q, k=129, candidates=C, chunk_rows=128)
    with pytest.raises(ValueError, match="columns"):
        helpers.most_similar(Q, k=5, candidates=C[:, :80], chunk_rows=128)


def test_topk_ragged_last_chunk_with_more_corpus_slices():
    """9504 rows in chunks of 5248 (41 tiles: 12 corpus slices per query tile) and 4256 (34 tiles: 15 slices): the ragged block's
    partial lists are the larger ones, which its workspace must hold."""
    from dae_rnn_news_recommendation_amd import _lib as L, helpers
    lib = L.load()
    assert lib.dae_topk_images_workspace(4256, 5248, 10) > lib.dae_topk_images_workspace(5248, 5248, 10)
    g = torch.Generator(device="cuda").manual_seed(3)
    X = torch.randn((9504, 32), device="cuda", generator=g)
    ref = helpers.most_similar(X, k=10, return_tensor=True)
    got = helpers.most_similar(X, k=10, chunk_rows=5248, return_tensor=True)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_topk_exclusion_lists_across_chunks(ties):
    """exclude= lists whose items lie in several corpus chunks, with and without exclude_self; and rows left with fewer than k
    admissible candidates, which lie in different chunks."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(17)
    X = rng.standard_normal((600, 40)).astype(np.float32)
    first = helpers.most_similar(X, k=20)[0]
    lists = [np.concatenate([first[i, ::2], rng.choice(600, 25, replace=False)]) for i in range(600)]     # half of the winners, and more
    for k, excl in ((1, True), (37, True), (128, False)):
        ref = helpers.most_similar(X, k=k, exclude_self=excl, exclude=lists)
        assert not any(np.isin(ref[0][i], lists[i]).any() for i in range(0, 600, 37))
        for c in CHUNKS:
            assert _same(helpers.most_similar(X, k=k, exclude_self=excl, exclude=lists, chunk_rows=c), ref), (k, excl, c)
    C = rng.standard_normal((700, 40)).astype(np.float32)
    cl = [rng.choice(700, 60, replace=False) for _ in range(600)]
    ref = helpers.most_similar(X, k=37, candidates=C, exclude=cl)
    assert _same(helpers.most_similar(X, k=37, candidates=C, exclude=cl, chunk_rows=256), ref)
    # fewer than k admissible: row i may only return 9 candidates spread over the operand (itself among them, taken by exclude_self)
    allow = [np.unique(np.concatenate([[i], (i + np.arange(1, 9) * 83) % 700])) for i in range(700)]
    bar = [np.setdiff1d(np.arange(700), a) for a in allow]
    for k in (37, 128):
        ref = helpers.most_similar(ties, k=k, metric="linear kernel", exclude=bar)
        assert (ref[0][:, 8:] == -1).all() and np.isneginf(ref[1][:, 8:]).all() and (ref[0][:, :8] >= 0).all()
        for c in CHUNKS:
            assert _same(helpers.most_similar(ties, k=k, metric="linear kernel", exclude=bar, chunk_rows=c), ref), (k, c)


# ---- label statistics ----------------------------------------------------------------------------------------------------------------
EXACT = ("n_related", "n_unrelated", "n_nan", "score_range", "bins", "related", "unrelated", "auroc", "auroc_low", "auroc_high",
         "related_bounds", "unrelated_bounds")


def _stats_equal(got, ref):
    for key in ("hist_related", "hist_unrelated", "bin_edges"):
        assert np.array_equal(got[key], ref[key]), key
    for key in EXACT:                                                              # counts, n_nan, min / max / quartiles, range: all from integers
        assert got[key] == ref[key], (key, got[key], ref[key])
    for key in ("mean_related", "mean_unrelated"):
        assert abs(got[key] - ref[key]) <= 1e-12 * abs(ref[key]), (key, got[key], ref[key])


def test_label_stats_chunked_equals_one_shot(bow):
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(23)
    lab = rng.integers(0, 6, 500).astype(np.float64)
    lab[rng.choice(500, 40, replace=False)] = -1                                   # missing labels ...
    lab[rng.choice(500, 10, replace=False)] = np.nan                               # ... of both kinds
    tfidf = bow.copy().astype(np.float32)
    tfidf.data = (rng.random(tfidf.nnz) * 5 + 0.1).astype(np.float32)
    cand = sparse.random(300, 3000, density=0.02, random_state=np.random.RandomState(8), format="csr", dtype=np.float32)
    clab = rng.integers(-1, 6, 300)
    emb = rng.standard_normal((500, 50)).astype(np.float32)
    cases = [("bow cosine", bow, "", "cosine"), ("tfidf linear, automatic range", tfidf, "", "linear kernel"),
             ("tfidf l2 linear", tfidf, "l2", "linear kernel"), ("dense cosine", emb, "", "cosine")]
    for name, X, norm, metric in cases:
        ref = helpers.label_similarity_stats(X, lab, norm=norm, metric=metric, return_histograms=True)
        assert ref["n_related"] > 0 and ref["n_unrelated"] > 0
        for c in CHUNKS:
            _stats_equal(helpers.label_similarity_stats(X, lab, norm=norm, metric=metric, return_histograms=True, chunk_rows=c), ref)
        if metric == "linear kernel":
            refc = helpers.label_similarity_stats(X, lab, norm=norm, metric=metric, candidates=cand, candidate_labels=clab,
                                                  return_histograms=True)
            for c in (128, 256):
                _stats_equal(helpers.label_similarity_stats(X, lab, norm=norm, metric=metric, candidates=cand, candidate_labels=clab,
                                                            return_histograms=True, chunk_rows=c), refc)
    refc = helpers.label_similarity_stats(bow, lab, candidates=cand, candidate_labels=clab, return_histograms=True, bins=100)
    _stats_equal(helpers.label_similarity_stats(bow, lab, candidates=cand, candidate_labels=clab, return_histograms=True, bins=100,
                                                chunk_rows=128), refc)
    ref = helpers.label_similarity_stats(tfidf, lab, metric="linear kernel", refine=True, return_histograms=True)
    got = helpers.label_similarity_stats(tfidf, lab, metric="linear kernel", refine=True, return_histograms=True, chunk_rows=256)
    _stats_equal(got, ref)
    assert got["first_pass"] == ref["first_pass"]
    ref = helpers.label_similarity_stats(emb, lab, score_range=(-0.5, 0.75), return_histograms=True)
    _stats_equal(helpers.label_similarity_stats(emb, lab, score_range=(-0.5, 0.75), return_histograms=True, chunk_rows=128), ref)


# ---- memory ------------------------------------------------------------------------------------------------------------------------
def test_chunked_topk_never_holds_a_dense_operand():
    """4096 x 20 000 at 1 %, k = 10, chunk_rows = 256: the peak over the call stays below half of ONE full operand image
    (4096 x 20 096 x 4 bytes = 329 MB; the one-shot route holds two of them).  The parts, derived: two chunk images of
    256 x 20 096 x 4 = 20.6 MB each, the CSR (4096 x 200 entries x 8 bytes + indptr = 6.6 MB), carry and split lists (< 1 MB),
    the results (4096 x 10 x (4 + 4 + 8) bytes)."""
    from dae_rnn_news_recommendation_amd import helpers
    m = sparse.random(4096, 20000, density=0.01, random_state=np.random.RandomState(4), format="csr", dtype=np.float32)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx, sc = helpers.most_similar(m, k=10, chunk_rows=256, return_tensor=True)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    print(f"peak growth {grow / 1e6:.1f} MB, one operand image {4096 * 20096 * 4 / 1e6:.1f} MB")
    assert grow < 4096 * 20096 * 4 // 2, grow
    assert idx.shape == (4096, 10) and (idx >= 0).all() and (idx != torch.arange(4096, device="cuda")[:, None]).all()
    assert torch.isfinite(sc).all() and (sc[:, :-1] >= sc[:, 1:]).all()
    rows = np.array([0, 255, 256, 2000, 4095])                                     # a few rows against fp64 cosines from the CSR itself
    m64 = m.astype(np.float64)
    nrm = np.sqrt(np.asarray(m64.multiply(m64).sum(axis=1)).ravel())
    S = (m64[rows] @ m64.T).toarray() / (nrm[rows][:, None] * nrm[None, :])
    S[np.arange(rows.size), rows] = -np.inf
    gi, gs = idx[rows].cpu().numpy(), sc[rows].cpu().numpy()
    tol = 1e-5 * np.abs(S[np.isfinite(S)]).max()
    for r in range(rows.size):
        assert np.abs(S[r][gi[r]] - gs[r]).max() <= tol
        kth = np.sort(S[r])[-10]
        assert (S[r][gi[r]] >= kth - tol).all() and np.isin(np.nonzero(S[r] > kth + tol)[0], gi[r]).all()


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_sweep_chunk_rows(tmp_path, monkeypatch, capsys):
    """--top_k 5 --label_stats with --sweep_chunk_rows 256 saves the arrays and prints the numbers of the run without the flag."""
    import main_autoencoder as cli
    monkeypatch.chdir(tmp_path)
    common = ["--num_epochs", "1", "--train_row", "400", "--validate_row", "150", "--validation", "--max_features", "800",
              "--seed", "4", "--similarity", "false", "--top_k", "5", "--label_stats"]
    runs = []
    for name, extra in (("plain", []), ("chunked", ["--sweep_chunk_rows", "256"])):
        model = cli.main(["--model_name", name] + common + extra)
        out = capsys.readouterr().out
        lines = [l for l in out.splitlines() if "precision@5" in l or "AUROC" in l or "queries ->" in l]
        d = model.data_dir
        arrays = {f: np.load(d + f) for f in ("article_encoded_top5.npz", "article_encoded_validate_top5.npz")}
        emb = np.load(d + "article_encoded_train.npy")
        stats = {s: json.load(open(model.plot_dir + "similarity_stats_" + s + ".json"))
                 for s in ("binary_count", "encoded", "binary_count_validate", "encoded_validate")}
        runs.append((lines, arrays, emb, stats))
    (l0, a0, e0, s0), (l1, a1, e1, s1) = runs
    assert np.array_equal(e0, e1)                                                  # the two runs trained the same model
    assert len(l0) == 2 + 2 + 4 and l0 == l1, (l0, l1)
    for f in a0:
        assert np.array_equal(a0[f]["indices"], a1[f]["indices"]) and np.array_equal(a0[f]["scores"], a1[f]["scores"]), f
    for s in s0:
        for key in ("n_related", "n_unrelated", "n_nan", "score_range", "related", "unrelated", "auroc", "auroc_low", "auroc_high"):
            assert s0[s][key] == s1[s][key], (s, key)
        assert abs(s0[s]["mean_related"] - s1[s]["mean_related"]) <= 1e-12 * abs(s0[s]["mean_related"])
