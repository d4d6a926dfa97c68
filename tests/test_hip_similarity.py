"""GPU parity of the evaluation step after the path: dae_pairwise_similarity through the mirror of
helpers.pairwise_similarity vs the oracle (which test_oracle.py pins against scikit-learn), and dae_pair_stats through
helpers.visualize_pairwise_similarity vs oracle.pair_stats.  The later sweeps (pair-hist, top-k, rank) are checked against this
matrix route, so it is held to float64 here: element by element for the product (exact integers at the tile edges, an entrywise
fp32 dot-product bound elsewhere), and to the derived bounds of ``_check_stats`` for the pair statistics.

Out of scope: rows whose squared norm overflows or underflows fp32 (scikit-learn in fp32 behaves the same way), and NaN scores
in dae_pair_stats (the reference's roc_curve raises on them)."""
import ctypes
import math

import numpy as np
import pytest
import torch
from scipy import sparse

import oracle as O

pytestmark = pytest.mark.gpu

NORMS = ["", "l1", "l2", "max"]
METRICS = ["cosine", "linear kernel"]


def _close(got, want, tol=1e-5):
    """fp32 product vs the fp64 oracle: error relative to the largest entry (entries near zero are sums that cancel)."""
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want))) <= tol * float(np.max(np.abs(want)) + 1e-30)


@pytest.mark.parametrize("norm", ["", "l1", "l2", "max"])
@pytest.mark.parametrize("metric", ["cosine", "linear kernel"])
def test_pairwise_similarity_dense(norm, metric):
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(2)
    X = rng.standard_normal((300, 70)).astype(np.float32)            # ragged against every tile size
    X[11] = 0.0
    got = helpers.pairwise_similarity(X, norm=norm, metric=metric)
    want = O.pairwise_similarity(X, norm=norm, metric=metric)
    assert got.shape == (300, 300) and got.dtype == np.float32
    assert _close(got, want)
    assert (np.diag(got) == 0).all()
    keep = helpers.pairwise_similarity(X, norm=norm, metric=metric, set_diagonal_zero=False)
    assert _close(keep, O.pairwise_similarity(X, norm=norm, metric=metric, set_diagonal_zero=False))
    assert _close(got, got.T, 1e-6)                                   # symmetric, as X X^T must be


def test_pairwise_similarity_sparse_bow_and_embeddings():
    """The two shapes main_autoencoder.py:307-317 feeds: a sparse binary BoW matrix and a dense embedding matrix."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(3)
    bow = sparse.random(500, 3000, density=0.02, format="csr", dtype=np.float32, random_state=np.random.RandomState(1))
    bow.data[:] = 1.0
    got = helpers.pairwise_similarity(bow, metric="cosine")
    assert _close(got, O.pairwise_similarity(bow, metric="cosine"))
    emb = rng.random((500, 500)).astype(np.float32)
    t = helpers.pairwise_similarity(torch.from_numpy(emb).cuda(), metric="cosine", return_tensor=True)
    assert t.is_cuda and t.shape == (500, 500)
    assert _close(t.cpu().numpy(), O.pairwise_similarity(emb, metric="cosine"))


def test_pairwise_similarity_rejects_other_metrics():
    from dae_rnn_news_recommendation_amd import helpers
    with pytest.raises(AssertionError):
        helpers.pairwise_similarity(np.eye(4, dtype=np.float32), metric="euclidean")
    with pytest.raises(ValueError):
        helpers.pairwise_similarity(np.eye(4, dtype=np.float32), norm="l3")


# ---------------------------------------------------------------------------------------------------------------------
# dae_pairwise_similarity: every element, at the tile edges and through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _small_integers(n, d, seed):
    """[n x d] fp32 integers in [-3, 3], about a third of them zero, one all-zero row: every product and every partial sum of
    X X^T is an integer of magnitude <= 9 d < 2^24, i.e. exact in fp32 in any summation order."""
    assert 9 * d < 2 ** 24
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, (n, d)) * (rng.random((n, d)) < 0.75)
    if n > 2:
        X[n // 2] = 0
    return X.astype(np.float32)


def _pad(n):
    from dae_rnn_news_recommendation_amd import _lib as L
    return L.pad(n)


def _exact_product(X):
    Xi = X.astype(np.int64)
    assert (Xi == X).all()
    return Xi @ Xi.T


@pytest.mark.parametrize("d", [1, 127, 129, 300])
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 257])
def test_pairwise_similarity_exact_integers(n, d):
    """B1: integer rows, linear kernel, no norm: the fp32 result IS the int64 product, element by element -- below one tile, at
    128 +/- 1, over two tiles, with K below / over one 128-column panel and ragged -- and the cleared diagonal is exactly 0."""
    from dae_rnn_news_recommendation_amd import helpers
    X = _small_integers(n, d, 1000 * n + d)
    want = _exact_product(X)
    keep = helpers.pairwise_similarity(X, metric="linear kernel", set_diagonal_zero=False)
    assert keep.shape == (n, n) and keep.dtype == np.float32
    assert np.array_equal(keep.astype(np.int64), want) and np.array_equal(keep, want.astype(np.float32))
    got = helpers.pairwise_similarity(X, metric="linear kernel")
    np.fill_diagonal(want, 0)
    assert np.array_equal(got, want.astype(np.float32))
    assert (np.diag(got) == 0).all()


def _rows64(X, norm, metric):
    """The float64-normalised rows Y whose product Y Y^T the oracle returns (oracle.pairwise_similarity's own steps)."""
    Y = np.asarray(X, np.float64)
    for kind in ([norm] if norm else []) + (["l2"] if metric == "cosine" else []):
        n = {"l1": np.abs(Y).sum(axis=1), "l2": np.sqrt((Y * Y).sum(axis=1)), "max": np.abs(Y).max(axis=1)}[kind]
        Y = Y / np.where(n == 0, 1.0, n)[:, None]
    return Y


def _assert_entrywise(got, X, norm, metric, set_diagonal_zero=True):
    """|got - want|_ij <= (3 D + 32) 2^-24 (|Y| |Y|^T)_ij, Y the float64-normalised rows, want the float64 oracle.

    Derivation (u = 2^-24, first order).  The kernel computes y = (x * s1) * s2 in fp32 and then an fp32 dot product of two such
    rows whose products are exact (fp32 MFMA, see the header of dae_similarity.hip).
    * The dot product of D terms, in ANY summation order: at most (D - 1) u sum_k |y_ik y_jk|.
    * A norm reduction of D non-negative terms, in any order: relative error at most (D - 1) u, plus u for each rounded term
      (two for a square of a rounded value), plus u each for the square root (which first halves what came before) and the
      reciprocal.  So s1 (l1: (D + 1) u; l2: (D / 2 + 3) u; max: u) and, for cosine, s2 ((D / 2 + 4) u; an error of s1 is a
      common factor of the row that s2, computed from the scaled row, cancels again).  With the one or two roundings of the
      multiplications, each y_ik carries at most (D + 3) u relative error, both operands together (2 D + 6) u.
    Sum: (3 D + 5) u sum_k |y_ik y_jk|; the bound leaves 27 u for the second-order terms and for the float64 reference."""
    D = X.shape[1]
    want = O.pairwise_similarity(X, norm=norm, metric=metric, set_diagonal_zero=set_diagonal_zero)
    Y = _rows64(X, norm, metric)
    full = Y @ Y.T
    if set_diagonal_zero:
        np.fill_diagonal(full, 0)
    assert np.allclose(full, want, rtol=1e-13, atol=0)                # Y is what the oracle multiplied
    bound = (3 * D + 32) * 2.0 ** -24 * (np.abs(Y) @ np.abs(Y).T)
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    excess = np.abs(got - want) - bound
    i, j = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess[i, j] <= 0, (norm, metric, int(i), int(j), got[i, j], want[i, j], bound[i, j])


def _similarity_abi(Xv, n, d, norm, metric, zero_diagonal, ldo):
    """dae_pairwise_similarity the way helpers/sweeps.py calls it, on the view Xv (any row stride) into a NaN-filled
    [dae_pad(n) x ldo] image."""
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd.helpers._device import norm_metric
    lib = L.load()
    npad = int(lib.dae_pad(n))
    assert npad == L.pad(n) and Xv.is_cuda and Xv.dtype == torch.float32 and Xv.stride(1) == 1
    out = torch.full((npad, ldo), float("nan"), dtype=torch.float32, device=Xv.device)
    ws_bytes = int(lib.dae_pairwise_similarity_workspace(n, d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=Xv.device)
    with torch.cuda.device(Xv.device):
        L.call("dae_pairwise_similarity", L.ptr(Xv), Xv.stride(0), n, d, *norm_metric(norm, metric), 1 if zero_diagonal else 0, L.ptr(out),
               ldo, L.ptr(ws), ws_bytes, L.current_stream())
        torch.cuda.synchronize()
    return out.cpu().numpy(), npad


def _poisoned_view(X, left=3):
    """X as a column view of a wider CUDA tensor: ``left`` NaN columns before it (an unaligned base), and NaN behind it to
    beyond the next multiple of 128, so a read of the columns D .. dae_pad(D) stays inside the tensor and meets NaN."""
    from dae_rnn_news_recommendation_amd import _lib as L
    n, d = X.shape
    wide = torch.full((n, left + L.pad(d) + 5), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, left:left + d] = torch.from_numpy(X).cuda()
    view = wide[:, left:left + d]
    assert view.stride(0) > d and view.stride(1) == 1
    return view


@pytest.mark.parametrize("extra", [8, 3])                             # ldo % 4 == 0: the epilogue's 16-byte stores; else dword stores
@pytest.mark.parametrize("n,d", [(1, 1), (129, 127), (257, 300)])
def test_pairwise_similarity_abi_strides_and_bounds(n, d, extra):
    """B2: ldx > D (X a view between NaN columns) and ldo > dae_pad(N) (out prefilled with NaN).  out[:N, :N] is the exact integer
    product of B1, the columns >= dae_pad(N) keep their NaN, and nothing of X beyond its D columns is read.

    What the padding inside dae_pad(N) holds: zeros.  The code guarantees it: row_normalize_kernel writes the padding rows
    N .. dae_pad(N) of the operand image as zeros, the GEMM covers all dae_pad(N) x dae_pad(N) outputs, so a padding entry is a sum
    of products with a zero factor -- asserted below (for finite X; 0 * inf would be NaN)."""
    X = _small_integers(n, d, 77 * n + d)
    want = _exact_product(X)
    Xv = _poisoned_view(X)
    for zero_diagonal in (False, True):
        out, npad = _similarity_abi(Xv, n, d, "", "linear kernel", zero_diagonal, _pad(n) + extra)
        if zero_diagonal:
            np.fill_diagonal(want, 0)
        assert np.array_equal(out[:n, :n], want.astype(np.float32))
        assert out.shape == (npad, npad + extra) and np.isnan(out[:, npad:]).all()
        pad_area = np.ones((npad, npad), bool)
        pad_area[:n, :n] = False
        assert (out[:, :npad][pad_area] == 0).all()


@pytest.mark.parametrize("norm,metric", [("l1", "cosine"), ("l2", "linear kernel"), ("max", "cosine")])
def test_pairwise_similarity_abi_norms_read_d_columns_only(norm, metric):
    """B2 for the norm reductions: the same poisoned view, D = 300 (a ragged second trip of the row loop), every result finite and
    within the entrywise bound -- a reduction that ran to dae_pad(D) or along ldx would meet NaN."""
    n, d = 129, 300
    X = _small_integers(n, d, 5)
    out, npad = _similarity_abi(_poisoned_view(X), n, d, norm, metric, True, _pad(n) + 8)
    _assert_entrywise(out[:n, :n], X, norm, metric)
    assert np.isnan(out[:, npad:]).all()


@pytest.mark.parametrize("norm,metric", [(nm, "linear kernel") for nm in NORMS] + [("", "cosine")])
def test_pairwise_similarity_rows_of_different_scale(norm, metric):
    """B3: rows scaled by 2^e, e over [-10, 10]: the entries of one matrix differ by up to 2^40, so an error is measured against
    its own entry's |y_i| . |y_j|, not against the largest entry of the matrix (``_assert_entrywise`` has the derivation)."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(21)
    n, d = 200, 70
    e = rng.permutation(np.round(np.linspace(-10, 10, n))).astype(np.int64)
    X = (rng.standard_normal((n, d)) * 2.0 ** e[:, None]).astype(np.float32)
    assert e.min() == -10 and e.max() == 10
    _assert_entrywise(helpers.pairwise_similarity(X, norm=norm, metric=metric), X, norm, metric)
    _assert_entrywise(helpers.pairwise_similarity(X, norm=norm, metric=metric, set_diagonal_zero=False), X, norm, metric, False)


@pytest.mark.parametrize("norm", ["l1", "max"])
@pytest.mark.parametrize("d", [257, 600])
def test_pairwise_similarity_ragged_row_loop(d, norm):
    """B4: D > 256 and D % 256 != 0: the 256-thread row loops of row_normalize_kernel take a ragged second (third) trip, with a
    norm whose reduction needs fabsf (half the entries are negative) followed by the cosine reduction."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(d)
    X = rng.standard_normal((131, d)).astype(np.float32)
    X[:, 256:] *= 4.0                                                 # the second trip carries most of every norm
    assert (X < 0).mean() > 0.4
    _assert_entrywise(helpers.pairwise_similarity(X, norm=norm, metric="cosine"), X, norm, "cosine")


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("metric", METRICS)
def test_pairwise_similarity_zero_input_and_one_row(norm, metric):
    """B5: all-zero input (every norm is 0 -> 1, never a division by zero) and N = 1: all zeros, no NaN."""
    from dae_rnn_news_recommendation_amd import helpers
    for shape in [(1, 1), (1, 300), (5, 70), (130, 257)]:
        for zero in (True, False):
            got = helpers.pairwise_similarity(np.zeros(shape, np.float32), norm=norm, metric=metric, set_diagonal_zero=zero)
            assert got.shape == (shape[0], shape[0]) and (got == 0).all()
    x = np.random.default_rng(4).standard_normal((1, 300)).astype(np.float32)
    got = helpers.pairwise_similarity(x, norm=norm, metric=metric)
    assert got.shape == (1, 1) and got[0, 0] == 0
    _assert_entrywise(helpers.pairwise_similarity(x, norm=norm, metric=metric, set_diagonal_zero=False), x, norm, metric, False)


# ---------------------------------------------------------------------------------------------------------------------
# dae_pair_stats
# ---------------------------------------------------------------------------------------------------------------------
FIVE = ("min", "q1", "median", "q3", "max")


def _symmetric(low):
    """The symmetric matrix whose strict lower triangle is that of ``low`` (copied, not added: -0.0 stays -0.0)."""
    S = np.array(low, dtype=np.float32)
    iu = np.triu_indices(S.shape[0], 1)
    S[iu] = S.T[iu]
    return S


def _populations(lab, S):
    """The related / unrelated scores (fp32 values as float64) by the rule of oracle.pair_stats: pairs j < i, labels >= 0."""
    lab = np.asarray(lab).reshape(len(lab), -1)[:, 0]
    S = np.asarray(S, np.float64)
    ok = (lab[None, :] >= 0) & (lab[:, None] >= 0)
    same = (lab[None, :] == lab[:, None]) & ok
    low = np.tril(np.ones(same.shape, bool), -1)
    return {"related": S[same & low], "unrelated": S[~same & ok & low]}


def _check_stats(got, lab, S):
    """``got`` (the dict of helpers.visualize_pairwise_similarity) against oracle.pair_stats on the same fp32 scores in float64.
    Bounds, all derived:
    * counts: equal.  AUROC: 1e-12 absolute -- integer counting on both sides, rank sums below 2^53, one division.
    * min, quartiles, max: 1e-13 max(|class min|, |class max|) -- a handful of fp64 roundings on the same two fp32 values
      (-0.0 == 0.0 counts as equal).
    * means: n 2^-53 mean|s| against math.fsum -- the worst case of any fp64 summation order ((n - 1) 2^-53 sum|s| / n) plus the
      rounding of the division.
    An empty class has NaN mean and five numbers, and the AUROC is NaN unless both classes have pairs."""
    lab = np.asarray(lab).reshape(len(lab), -1)[:, 0]
    want = O.pair_stats(lab, S)
    pops = _populations(lab, S)
    assert got["n_related"] == want["n_related"] == len(pops["related"])
    assert got["n_unrelated"] == want["n_unrelated"] == len(pops["unrelated"])
    if want["n_related"] and want["n_unrelated"]:
        assert abs(got["auroc"] - want["auroc"]) < 1e-12, (got["auroc"], want["auroc"])
    else:
        assert np.isnan(got["auroc"])
    for pop, v in pops.items():
        if len(v):
            scale = max(abs(v.min()), abs(v.max()))
            for k in FIVE:
                assert abs(got[pop][k] - want[pop][k]) <= 1e-13 * scale, (pop, k, got[pop][k], want[pop][k])
            mean = math.fsum(v) / len(v)
            assert abs(got["mean_" + pop] - mean) <= 2.0 ** -53 * math.fsum(np.abs(v)), (pop, got["mean_" + pop], mean)
        else:
            assert np.isnan(got["mean_" + pop]) and all(np.isnan(got[pop][k]) for k in FIVE)
    return want


def _numbers(res):
    """The 15 numbers of a visualize_pairwise_similarity result as float64 bit patterns (NaN-safe equality)."""
    v = [res["auroc"], res["n_related"], res["n_unrelated"], res["mean_related"], res["mean_unrelated"]]
    v += [res[pop][k] for pop in ("related", "unrelated") for k in FIVE]
    return np.array(v, np.float64).view(np.uint64)


@pytest.mark.parametrize("n,classes,missing", [(300, 5, True), (129, 2, False), (64, 64, False)])
def test_pair_stats_matches_oracle(n, classes, missing):
    """dae_pair_stats (AUROC + box-plot numbers of related vs unrelated pairs) vs the oracle that test_oracle.py pins against
    scikit-learn; tied scores (coarse embeddings) and missing labels included."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(n)
    lab = rng.integers(0, classes, n)
    if missing:
        lab[rng.choice(n, n // 10, replace=False)] = -1
    X = np.round(rng.standard_normal((n, 8)), 1).astype(np.float32)
    S = helpers.pairwise_similarity(X, metric="linear kernel", return_tensor=True)
    got = helpers.visualize_pairwise_similarity(lab, S)
    _check_stats(got, lab, S.cpu().numpy())


def test_pair_stats_signed_zeros_four_items():
    """A1: -0.0 and +0.0 are one score.  Labels [0, 0, 1, 1], the two related pairs at -0.0, the four unrelated ones at +0.0: every
    (related, unrelated) pair is a tie, AUROC 0.5 (oracle and scikit-learn, pinned in test_oracle.py); an order that puts -0.0
    below +0.0 gives 0.0."""
    from dae_rnn_news_recommendation_amd import helpers
    lab = np.array([0, 0, 1, 1])
    low = np.zeros((4, 4), np.float32)
    low[1, 0] = low[3, 2] = -0.0
    S = _symmetric(low)
    assert np.signbit(S[1, 0]) and np.signbit(S[3, 2]) and not np.signbit(S[2, 0])
    got = helpers.visualize_pairwise_similarity(lab, S)
    want = _check_stats(got, lab, S)
    assert want["auroc"] == 0.5 and got["auroc"] == 0.5


def test_pair_stats_signed_zeros():
    """A1: N = 130, 3 classes, 10 % missing labels, scores drawn from {-1, -0.0, +0.0, 0.5, 1}: both zeros in both classes."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(130)
    n = 130
    lab = rng.integers(0, 3, n)
    lab[rng.choice(n, n // 10, replace=False)] = -1
    S = _symmetric(rng.choice(np.array([-1.0, -0.0, 0.0, 0.5, 1.0], np.float32), (n, n)))
    for v in _populations(lab, S).values():
        zeros = v[v == 0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    _check_stats(helpers.visualize_pairwise_similarity(lab, S), lab, S)
    _check_stats(helpers.visualize_pairwise_similarity(lab, torch.from_numpy(S).cuda()), lab, S)


def test_pair_stats_beyond_one_grid_sweep():
    """A2: N = 1200, two balanced classes: about 3.6e5 pairs per class against the 1024 x 256 = 262 144 threads of auroc_count_kernel
    and key_sum_kernel, so their grid-stride loops take a ragged second trip; scores rounded to 0.1 (heavy ties)."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(1200)
    n = 1200
    lab = rng.permutation(np.arange(n) % 2)
    S = _symmetric(np.round(rng.standard_normal((n, n)), 1))
    got = helpers.visualize_pairwise_similarity(lab, S)
    assert 262144 < got["n_related"] < 2 * 262144 and 262144 < got["n_unrelated"] < 2 * 262144
    _check_stats(got, lab, S)


def test_pair_stats_reads_the_strict_lower_triangle_only():
    """A3: S a view big[:N, :N] of a 129 x 200 CUDA tensor (lds = 200) whose diagonal, strict upper triangle and columns >= N are
    NaN: every returned number equals that of the clean contiguous matrix, so only j < i is read, along lds."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(129)
    n = 129
    lab = rng.integers(0, 4, n)
    lab[rng.choice(n, 9, replace=False)] = -1
    S = _symmetric(np.round(rng.standard_normal((n, n)), 1))
    clean = helpers.visualize_pairwise_similarity(lab, S)
    _check_stats(clean, lab, S)
    big = torch.full((n, 200), float("nan"), dtype=torch.float32, device="cuda")
    view = big[:n, :n]
    view.copy_(torch.from_numpy(S).cuda())
    view[torch.triu(torch.ones(n, n, dtype=torch.bool, device="cuda"))] = float("nan")
    assert view.stride(0) == 200 and torch.isnan(big).sum().item() == n * 200 - n * (n - 1) // 2
    got = helpers.visualize_pairwise_similarity(lab, view)
    assert np.array_equal(_numbers(got), _numbers(clean))


_SMALL = [[0, 0], [0, 1], [0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 1],
          [0, 0, 0, 1, 1, 2, -1], [0, 0, 0, 0, 1, 1, 1],
          [0, 1, 2, 3, 4, 5, 6],                                      # all classes singletons: n_related = 0
          [2, 2, 2, 2, 2, 2],                                         # one class: n_unrelated = 0, AUROC NaN
          [-1, -1, -1, -1, -1],                                       # all labels missing
          [-1, -1, 3, -1, -1]]                                        # exactly one valid label: no pair


def test_pair_stats_small_cases_cover_every_quartile_fraction():
    """The cases of A4 as a whole: class sizes 1 to 6 occur, and the population sizes n make q (n - 1) hit every fraction of
    {0, 1/4, 1/2, 3/4} (n mod 4 = 1, 2, 3, 0) in both populations."""
    sizes, rel, un = set(), set(), set()
    for lab in _SMALL:
        valid = [x for x in lab if x >= 0]
        counts = [valid.count(c) for c in set(valid)]
        sizes.update(counts)
        r = sum(c * (c - 1) // 2 for c in counts)
        u = len(valid) * (len(valid) - 1) // 2 - r
        rel.update([r % 4] if r else [])
        un.update([u % 4] if u else [])
    assert sizes >= {1, 2, 3, 4, 5, 6} and rel == {0, 1, 2, 3} and un == {0, 1, 2, 3}


@pytest.mark.parametrize("case", range(len(_SMALL)))
def test_pair_stats_small_and_degenerate_classes(case):
    """A4: N = 2 .. 7; an empty class gives NaN means and five-number entries, and a NaN AUROC (all inside ``_check_stats``)."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(case)
    lab = rng.permutation(np.array(_SMALL[case]))
    n = len(lab)
    S = _symmetric(rng.standard_normal((n, n)))
    want = _check_stats(helpers.visualize_pairwise_similarity(lab, S), lab, S)
    valid = int((lab >= 0).sum())
    assert want["n_related"] + want["n_unrelated"] == valid * (valid - 1) // 2


def test_pair_stats_extreme_finite_values():
    """A5: denormals of both signs, both zeros, +/-3e38 and ordinary values in one matrix: the key order is that of the floats over
    the whole finite range, a denormal is not a zero, and the quartile interpolation does not overflow."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(64)
    n = 64
    lab = rng.integers(0, 3, n)
    pool = np.array([1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 0.0, -0.0, 3e38, -3e38, 1.0, -1.0, 0.25, -7.5, 1e-20,
                     123456.0], np.float32)
    assert (np.abs(pool[:6]) > 0).all() and (np.abs(pool[:6]) < np.finfo(np.float32).tiny).all()
    S = _symmetric(rng.choice(pool, (n, n)))
    for v in _populations(lab, S).values():
        assert set(np.unique(v)) == set(np.unique(pool.astype(np.float64)))
    _check_stats(helpers.visualize_pairwise_similarity(lab, S), lab, S)


def _pair_stats_abi(S, lab):
    """The 16 doubles of dae_pair_stats, as bit patterns."""
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd.helpers._device import workspace
    lib = L.load()
    n = int(S.shape[0])
    lab = np.ascontiguousarray(np.asarray(lab, np.int32))
    ws_bytes = int(lib.dae_pair_stats_workspace(n))
    ws_p, ws = workspace(S.device, ws_bytes)
    out = (ctypes.c_double * 16)()
    with torch.cuda.device(S.device):
        L.call("dae_pair_stats", L.ptr(S), S.stride(0), lab.ctypes.data_as(ctypes.c_void_p), n, ctypes.cast(out, ctypes.c_void_p), ws_p,
               ws_bytes, L.current_stream())
    return np.array(list(out), np.float64).view(np.uint64)


def test_pair_stats_deterministic_and_order_independent():
    """A6: the split pass appends through atomics, the sort makes the result independent of that order: the same input gives the
    same 16 doubles bit for bit, and a permutation of the items (S and labels together) leaves the counts and the AUROC exactly
    equal, the order statistics (the same multiset) too, and the means within their bound."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(6)
    n = 300
    lab = rng.integers(0, 4, n)
    lab[rng.choice(n, 30, replace=False)] = -1
    S = _symmetric(np.round(rng.standard_normal((n, n)), 1))
    Sd = torch.from_numpy(S).cuda()
    first = _pair_stats_abi(Sd, lab)
    assert np.array_equal(first, _pair_stats_abi(Sd, lab))
    got = helpers.visualize_pairwise_similarity(lab, Sd)
    assert np.array_equal(_numbers(got), first[:15])
    _check_stats(got, lab, S)
    p = rng.permutation(n)
    Sp, labp = np.ascontiguousarray(S[p][:, p]), lab[p]
    perm = helpers.visualize_pairwise_similarity(labp, Sp)
    _check_stats(perm, labp, Sp)
    assert perm["n_related"] == got["n_related"] and perm["n_unrelated"] == got["n_unrelated"] and perm["auroc"] == got["auroc"]
    for pop in ("related", "unrelated"):
        assert all(perm[pop][k] == got[pop][k] for k in FIVE)


def test_pair_stats_label_intake():
    """visualize_pairwise_similarity's labels: float labels that are NaN, +/-inf or negative (a fraction included) are missing, as
    the reference's ``labels >= 0`` filter has it (inf: this package's rule), and a 2-D [N, 1] array is its first column."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(9)
    n = 40
    S = _symmetric(np.round(rng.standard_normal((n, n)), 1))
    lab = rng.integers(0, 3, n).astype(np.float64)
    lab[[1, 7]] = np.nan
    lab[3], lab[12], lab[20], lab[21], lab[33] = np.inf, -np.inf, -1.0, -0.5, -3.0
    mapped = np.where(np.isfinite(lab) & (lab >= 0), lab, -1.0).astype(np.int64)
    assert (mapped < 0).sum() == 7
    got = helpers.visualize_pairwise_similarity(lab, S)
    _check_stats(got, mapped, S)
    assert np.array_equal(_numbers(helpers.visualize_pairwise_similarity(lab.astype(np.float32), S)), _numbers(got))
    assert np.array_equal(_numbers(helpers.visualize_pairwise_similarity(mapped.reshape(n, 1), S)), _numbers(got))
    assert np.array_equal(_numbers(helpers.visualize_pairwise_similarity(lab.reshape(n, 1), S)), _numbers(got))
