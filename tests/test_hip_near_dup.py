"""GPU checks of the near-duplicate search (dae_threshold_pairs through helpers.similar_pairs) against the fp64 oracle, and of
the CLI's --dup_threshold.

Membership uses the near-tie rule of test_hip_topk.py with its tolerance tol = 1e-5 x max |S|: every pair the oracle scores
above T + tol must be returned, every returned pair must score at least T - tol in the oracle, every returned score must be
within tol of the oracle's; pairs inside the band |S - T| <= tol may go either way.  The band must not hide a failure: every
case first asserts, on the oracle's matrix alone, that the band holds at most 0.1 % of the pairs at or above T."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import sparse

import oracle as O

pytestmark = pytest.mark.gpu


def _ref_scores(Q, norm, metric, C=None):
    """fp64 score matrix [Nq x Nc]: the oracle's pairwise similarity (no diagonal fill) of [Q; C], cut to its Q x C block."""
    if C is None:
        return O.pairwise_similarity(Q, norm=norm, metric=metric, set_diagonal_zero=False)
    Qd = Q.toarray() if sparse.issparse(Q) else np.asarray(Q)
    Cd = C.toarray() if sparse.issparse(C) else np.asarray(C)
    S = O.pairwise_similarity(np.vstack([Qd, Cd]), norm=norm, metric=metric, set_diagonal_zero=False)
    return S[:Qd.shape[0], Qd.shape[0]:]


def _check(res, S, T, triangle, tol_rel=1e-5):
    """The near-tie rule on the result ``res = (rows, cols, scores)`` against the fp64 scores S; ``triangle``: only j < i counts."""
    rows, cols, sc = res
    S = np.asarray(S)
    Nq, Nc = S.shape
    tol = tol_rel * np.abs(S).max()
    allowed = np.tril(np.ones((Nq, Nc), bool), -1) if triangle else np.ones((Nq, Nc), bool)
    n_at = int(((S >= T) & allowed).sum())
    n_band = int(((np.abs(S - T) <= tol) & allowed).sum())
    print(f"T={T}: {n_at} pairs >= T in the oracle, {n_band} in the band, tol={tol:.3g}, returned {rows.shape[0]}")
    assert n_at > 0 and n_band <= 1e-3 * n_at, (n_at, n_band)          # the band condition, on the oracle alone
    assert rows.dtype == np.int64 and cols.dtype == np.int64 and sc.dtype == np.float32
    assert rows.shape == cols.shape == sc.shape and rows.ndim == 1
    assert (rows >= 0).all() and (rows < Nq).all() and (cols >= 0).all() and (cols < Nc).all()
    assert allowed[rows, cols].all()
    key = rows * (1 << 32) + cols
    assert (np.diff(key) > 0).all()                                    # i ascending, then j ascending; no pair twice
    assert (S[rows, cols] >= T - tol).all()
    got = np.zeros((Nq, Nc), bool)
    got[rows, cols] = True
    assert not ((S > T + tol) & allowed & ~got).any()
    err = np.abs(sc.astype(np.float64) - S[rows, cols]).max() if rows.size else 0.0
    print(f"   max |score - oracle| = {err:.3g}")
    assert err <= tol


@pytest.fixture(scope="module")
def dups3000():
    """3000 x 64 standard-normal rows; the last 400 are earlier rows plus 0.05 x noise, rows 100..139 exact copies of rows
    0..39, row 17 all zero."""
    rng = np.random.default_rng(21)
    X = rng.standard_normal((3000, 64)).astype(np.float32)
    X[2600:] = X[rng.integers(0, 2600, 400)] + 0.05 * rng.standard_normal((400, 64)).astype(np.float32)
    X[100:140] = X[0:40]
    X[17] = 0.0
    return X


# thresholds per (norm, metric): picked on the oracle so that the band holds < 0.1 % of the pairs at or above T (asserted by _check)
@pytest.mark.parametrize("norm, metric, thresholds", [
    ("", "cosine", (0.9, 0.5, 0.2)),
    ("l2", "linear kernel", (0.9, 0.5, 0.2)),
    ("", "linear kernel", (20.0,)),
    ("l1", "linear kernel", (0.01, 0.005)),
    ("max", "linear kernel", (5.0, 3.0)),
    ("l1", "cosine", (0.9, 0.2)),
    ("max", "cosine", (0.9, 0.2)),
])
def test_dense_random_all_norms(dups3000, norm, metric, thresholds):
    from dae_rnn_news_recommendation_amd import helpers
    S = _ref_scores(dups3000, norm, metric)
    for T in thresholds:
        _check(helpers.similar_pairs(dups3000, T, norm=norm, metric=metric), S, T, triangle=True)


def test_exact_arithmetic_matches_numpy_bit_for_bit():
    """Integer rows with many duplicates, linear kernel: every score is exact in fp32, so rows, cols and scores must equal NumPy's
    np.nonzero(np.tril(S >= T, -1)) -- for a T that many pairs hit exactly (>= is inclusive) and for a T between two values."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(5)
    base = rng.integers(-2, 3, (40, 24)).astype(np.float32)
    X = base[rng.integers(0, 40, 700)]                                             # ~17 copies of every row
    S = X.astype(np.float64) @ X.T.astype(np.float64)
    low = S[np.tril_indices(700, -1)]
    vals, counts = np.unique(low, return_counts=True)
    T_hit = float(vals[vals > 0][np.argmax(counts[vals > 0])])                     # the most frequent positive score
    assert counts[vals == T_hit][0] > 1000
    for T in (T_hit, T_hit + 0.5, float(np.diag(S).min())):
        want_r, want_c = np.nonzero(np.tril(S >= T, -1))
        assert want_r.size > 0
        r, c, s = helpers.similar_pairs(X, T, metric="linear kernel")
        assert np.array_equal(r, want_r) and np.array_equal(c, want_c), T
        assert np.array_equal(s, S[want_r, want_c].astype(np.float32)), T


def test_queries_against_a_corpus():
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((129, 90)).astype(np.float32)
    C = rng.standard_normal((1000, 90)).astype(np.float32)
    C[rng.integers(0, 1000, 60)] = Q[rng.integers(0, 129, 60)] + 0.05 * rng.standard_normal((60, 90)).astype(np.float32)
    C[5] = Q[5]                                                                    # (5, 5) and pairs above the diagonal qualify here
    for metric, T in (("cosine", 0.9), ("cosine", 0.25), ("linear kernel", 30.0)):
        S = _ref_scores(Q, "", metric, C)
        res = helpers.similar_pairs(Q, T, metric=metric, candidates=C)
        _check(res, S, T, triangle=False)
        assert (res[1] >= res[0]).any()
    Cs = C[:50]                                                                    # less than one tile of candidates
    _check(helpers.similar_pairs(Q, 0.25, candidates=Cs), _ref_scores(Q, "", "cosine", Cs), 0.25, triangle=False)
    with pytest.raises(ValueError, match="columns"):
        helpers.similar_pairs(Q, 0.5, candidates=C[:, :80])


def test_sparse_bow_and_tensor_inputs():
    from dae_rnn_news_recommendation_amd import helpers
    bow = sparse.random(500, 3000, density=0.02, random_state=np.random.RandomState(3), format="csr", dtype=np.float32)
    bow.data[:] = 1.0
    dense = bow.toarray()
    for T in (0.05, 0.07):
        a = helpers.similar_pairs(bow, T)
        b = helpers.similar_pairs(dense, T)
        t = helpers.similar_pairs(torch.from_numpy(dense).cuda(), T, return_tensor=True)
        assert t[0].is_cuda and t[0].dtype == torch.int64 and t[1].dtype == torch.int64 and t[2].dtype == torch.float32
        assert a[0].size > 0
        for x, y, z in zip(a, b, t):
            assert np.array_equal(x, y) and np.array_equal(x, z.cpu().numpy())
        assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    # 0.07 lies between the attainable scores k / sqrt(n_i n_j) of these rows; 0.05 = 3 / 60 is one of them (81 pairs in the band)
    _check(helpers.similar_pairs(bow, 0.07), _ref_scores(bow, "", "cosine"), 0.07, triangle=True)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))


def test_deterministic_and_independent_of_the_grid(dups3000):
    from dae_rnn_news_recommendation_amd import helpers
    X = dups3000
    for T in (0.9, 0.2):
        a = helpers.similar_pairs(X, T)
        b = helpers.similar_pairs(X, T)
        assert a[0].size > 0 and _same(a, b)
        full = helpers.similar_pairs(X, T, candidates=X)                           # the rectangular grid, every tile
        again = helpers.similar_pairs(X, T, candidates=X)
        assert _same(full, again)
        m = full[1] < full[0]
        assert _same(a, tuple(v[m] for v in full))                                 # self mode = the rectangle's lower triangle
        first = helpers.similar_pairs(X[:100], T, candidates=X)                    # another grid
        m = full[0] < 100
        assert _same(first, tuple(v[m] for v in full))


def _abi_call(X, T, capacity):
    """dae_threshold_pairs in self mode, cosine, through ctypes; returns (rc, count, rows, cols, scores) with the arrays cut to capacity."""
    from dae_rnn_news_recommendation_amd import _lib as L
    lib = L.load()
    Xd = torch.from_numpy(X).cuda().contiguous()
    N, D = X.shape
    rows = torch.full((max(capacity, 1),), -7, dtype=torch.int32, device="cuda")
    cols = torch.full((max(capacity, 1),), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((max(capacity, 1),), -7.0, dtype=torch.float32, device="cuda")
    ws_bytes = int(lib.dae_threshold_pairs_workspace(N, N, D, capacity))
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    off = (-ws.data_ptr()) % 256
    count = ctypes.c_uint64(0)
    null = capacity == 0
    rc = lib.dae_threshold_pairs(L.ptr(Xd), Xd.stride(0), N, None, 0, N, D, 0, 0, T, None if null else L.ptr(rows),
                                 None if null else L.ptr(cols), None if null else L.ptr(sc), capacity, ctypes.byref(count),
                                 ctypes.c_void_p(ws.data_ptr() + off), ws_bytes, L.current_stream())
    torch.cuda.synchronize()
    return rc, int(count.value), rows.cpu().numpy()[:capacity], cols.cpu().numpy()[:capacity], sc.cpu().numpy()[:capacity]


def test_overflow_contract_through_the_c_abi(dups3000):
    from dae_rnn_news_recommendation_amd import helpers
    S = _ref_scores(dups3000, "", "cosine")
    want = int(np.tril(S >= 0.9, -1).sum())                                        # 474, and no pair of the oracle is in the band
    rc, n, r_big, c_big, s_big = _abi_call(dups3000, 0.9, 100000)
    assert rc == 0 and n == want
    assert (r_big[n:] == -7).all() and (c_big[n:] == -7).all() and (s_big[n:] == -7.0).all()      # nothing past the count is written
    for cap in (0, 1, 100, want - 1):                                              # too small: rc 0 and the exact count
        rc, m, _, _, _ = _abi_call(dups3000, 0.9, cap)
        assert rc == 0 and m == want, cap
    rc, m, r, c, s = _abi_call(dups3000, 0.9, want)                                # exactly enough: the same records
    assert rc == 0 and m == want
    assert np.array_equal(r, r_big[:n]) and np.array_equal(c, c_big[:n]) and np.array_equal(s.view(np.int32), s_big[:n].view(np.int32))
    hr, hc, hs = helpers.similar_pairs(dups3000, 0.9)
    assert np.array_equal(hr, r) and np.array_equal(hc, c) and np.array_equal(hs.view(np.int32), s.view(np.int32))
    with pytest.raises(ValueError, match=str(want)):
        helpers.similar_pairs(dups3000, 0.9, max_pairs=10)
    assert helpers.similar_pairs(dups3000, 0.9, max_pairs=want)[0].shape == (want,)
    # more pairs than the first call's capacity: the second call, with the exact count
    big = int(np.tril(S >= 0.2, -1).sum())
    assert big > 65536
    assert abs(helpers.similar_pairs(dups3000, 0.2)[0].shape[0] - big) <= 83       # the band of this case (see the first test)


def test_ends_of_the_range():
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(3)
    X = rng.standard_normal((300, 40)).astype(np.float32)
    r, c, s = helpers.similar_pairs(X, float("inf"))
    assert r.shape == c.shape == s.shape == (0,) and r.dtype == np.int64 and s.dtype == np.float32
    r, c, s = helpers.similar_pairs(X, -float("inf"))
    want_r, want_c = np.nonzero(np.tril(np.ones((300, 300), bool), -1))
    assert r.shape == (44850,) and np.array_equal(r, want_r) and np.array_equal(c, want_c)
    S = _ref_scores(X, "", "cosine")
    assert np.abs(s - S[want_r, want_c]).max() <= 1e-5
    with pytest.raises(ValueError, match="NaN"):
        helpers.similar_pairs(X, float("nan"))
    with pytest.raises(ValueError, match="not a supported norm"):
        helpers.similar_pairs(X, 0.5, norm="l3")


def _planted(N, D, n_dup, seed):
    """N x D standard-normal rows on the device; the last n_dup rows are earlier rows plus 0.05 x noise (cosine ~ 0.9988)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn((N, D), device="cuda", generator=g)
    src = torch.randint(0, N - n_dup, (n_dup,), device="cuda", generator=g)
    X[N - n_dup:] = X[src] + 0.05 * torch.randn((n_dup, D), device="cuda", generator=g)
    return X, src


def test_scale_against_the_materialised_path():
    """N = 20 000, D = 500 against pairwise_similarity on the device: lower triangle, near-tie rule, scores within 1e-6."""
    from dae_rnn_news_recommendation_amd import helpers
    N, D, T = 20000, 500, 0.9
    X, src = _planted(N, D, 1500, 0)
    rows, cols, sc = helpers.similar_pairs(X, T, return_tensor=True)
    assert rows.shape[0] >= 1500                                                   # every planted pair and a few siblings
    S = helpers.pairwise_similarity(X, set_diagonal_zero=False, return_tensor=True)
    at = S[rows, cols]
    assert (at - sc).abs().max().item() <= 1e-6                                    # the same fp32 products
    tol = 1e-5 * S.abs().max().item()
    assert (cols < rows).all() and (at >= T - tol).all()
    key = rows * N + cols
    assert (key[1:] > key[:-1]).all()
    must = torch.tril(S > T + tol, -1)
    assert int(must.sum().item()) >= 1500
    must[rows, cols] = False
    assert not must.any()
    tail = rows >= N - 1500                                                        # row N - 1500 + d pairs with its source src[d]
    d = rows[tail] - (N - 1500)
    found = torch.zeros((1500,), dtype=torch.bool, device="cuda")
    found[d[cols[tail] == src[d]]] = True
    assert found.all()
    del S, must


def test_no_n_by_n_buffer():
    from dae_rnn_news_recommendation_amd import helpers
    N, D = 60000, 128
    X, _ = _planted(N, D, 3000, 1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    rows, cols, sc = helpers.similar_pairs(X, 0.9, return_tensor=True)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    print(f"peak growth {grow} bytes, {rows.shape[0]} pairs")
    assert grow < N * N * 4 // 8, grow
    assert rows.shape[0] >= 3000 and (cols < rows).all() and (sc >= 0.9).all()
    assert torch.unique(rows[rows >= N - 3000]).shape[0] == 3000                   # every planted row found its source


def test_cli_dup_threshold(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    monkeypatch.chdir(tmp_path)
    T = 0.5
    model = cli.main(["--model_name", "dup", "--num_epochs", "1", "--train_row", "400", "--validate_row", "150", "--validation",
                      "--max_features", "800", "--seed", "4", "--similarity", "false", "--dup_threshold", str(T)])
    out = capsys.readouterr().out
    d = model.data_dir
    tr = np.load(d + "article_encoded_dups.npz")
    va = np.load(d + "article_encoded_validate_dups.npz")
    assert set(tr.files) == {"rows", "cols", "scores", "group", "keep", "threshold"}
    assert set(va.files) == {"rows", "cols", "scores", "threshold"}
    assert float(tr["threshold"]) == T and "calculate similarity" not in out
    assert out.count("pair precision") == 2 and "groups of more than one article" in out
    emb = np.load(d + "article_encoded_train.npy")
    emb_v = np.load(d + "article_encoded_validate.npy")
    r, c, s = helpers.similar_pairs(emb, T)
    assert r.size > 0                                                              # an almost untrained encoder: many pairs reach 0.5
    assert np.array_equal(tr["rows"], r) and np.array_equal(tr["cols"], c) and np.array_equal(tr["scores"], s)
    group, keep = helpers.duplicate_groups(r, c, 400)
    assert np.array_equal(tr["group"], group) and np.array_equal(tr["keep"], keep) and tr["keep"].dtype == bool
    rv, cv, _ = helpers.similar_pairs(emb_v, T, candidates=emb)
    assert np.array_equal(va["rows"], rv) and np.array_equal(va["cols"], cv)
