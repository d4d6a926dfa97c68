"""The implicit-feedback ALS model without a GPU: the NumPy reference (tests/als_reference.py) against an exact solve, the literal
objective and scipy.sparse; the fall of the objective at every half-sweep; the argument errors of helpers.als (raised before the
device is touched) and of the four entry points (reported before any HIP call)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from als_reference import (fit_reference, half_sweep_reference, interactions_reference, loss_literal, loss_reference)
from dae_rnn_news_recommendation_amd import _lib, helpers
from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if indptr[-1] else np.zeros(0, dtype=np.int64)
    return indptr, items


def _random_log(rng, users, Na, max_len):
    return _csr([rng.integers(0, Na, rng.integers(0, max_len + 1)) for _ in range(users)])


def test_reference_with_F_steps_is_the_exact_solve():
    """Conjugate gradient ends after F steps in exact arithmetic: in float64 it equals np.linalg.solve on the explicit A_u."""
    rng = np.random.default_rng(1)
    M, Na, F, lam, alpha = 30, 25, 6, 0.1, 40.0
    inter = interactions_reference(*_random_log(rng, M, Na, 9), Na)
    Y = rng.standard_normal((Na, F)) * 0.3
    X0 = rng.standard_normal((M, F)) * 0.1
    ptr, idx, cnt = inter["user_ptr"], inter["user_idx"], inter["user_cnt"]
    assert (np.diff(ptr) == 0).any() and cnt.max() > 1
    got = half_sweep_reference(ptr, idx, cnt, Y, X0, lam, alpha, F)
    for u in range(M):
        Yu, r = Y[idx[ptr[u]:ptr[u + 1]]], cnt[ptr[u]:ptr[u + 1]].astype(np.float64)
        if r.size == 0:
            assert (got[u] == 0).all()
            continue
        A = Y.T @ Y + lam * np.eye(F) + (Yu * (alpha * r)[:, None]).T @ Yu
        b = ((1 + alpha * r)[:, None] * Yu).sum(axis=0)
        assert np.abs(got[u] - np.linalg.solve(A, b)).max() <= 1e-8
    # fewer steps leave a residual, so the steps are what closes it
    assert np.abs(half_sweep_reference(ptr, idx, cnt, Y, X0, lam, alpha, 1) - got).max() > 1e-4


def test_loss_formula_equals_the_literal_double_sum():
    rng = np.random.default_rng(2)
    M, Na, F = 20, 15, 4
    inter = interactions_reference(*_random_log(rng, M, Na, 8), Na)
    X, Y = rng.standard_normal((M, F)) * 0.4, rng.standard_normal((Na, F)) * 0.4
    args = (inter["user_ptr"], inter["user_idx"], inter["user_cnt"], X, Y, 0.05, 7.0)
    assert loss_reference(*args) == pytest.approx(loss_literal(*args), rel=1e-12)
    # the article orientation is the same objective
    assert loss_reference(inter["item_ptr"], inter["item_idx"], inter["item_cnt"], Y, X, 0.05, 7.0) == pytest.approx(loss_literal(*args), rel=1e-12)


def test_interactions_reference_against_scipy():
    rng = np.random.default_rng(3)
    M, Na = 50, 90
    indptr, items = _random_log(rng, M, Na, 14)
    items[:40] = items[0]                                                # repeats, whatever the draw
    inter = interactions_reference(indptr, items, Na)
    m = sp.csr_matrix((np.ones(items.size, dtype=np.int64), items, indptr), shape=(M, Na))
    m.sum_duplicates()
    m.sort_indices()
    assert np.array_equal(inter["user_ptr"], m.indptr) and np.array_equal(inter["user_idx"], m.indices)
    assert np.array_equal(inter["user_cnt"], m.data) and inter["events"] == items.size and inter["pairs"] == m.nnz
    t = m.T.tocsr()
    t.sort_indices()
    assert np.array_equal(inter["item_ptr"], t.indptr) and np.array_equal(inter["item_idx"], t.indices)
    assert np.array_equal(inter["item_cnt"], t.data)
    assert m.data.max() > 1 and (np.diff(m.indptr) == 0).any() and (np.diff(t.indptr) == 0).any()


def test_objective_of_the_reference_falls_at_every_half_sweep():
    labels = np.random.default_rng(3).integers(0, 6, 300)
    indptr, items = synthetic_sessions(400, labels, mean_len=10, seed=5)
    inter = interactions_reference(indptr, items, 300)
    for dtype in (np.float64, np.float32):
        _, _, curve = fit_reference(inter, 400, 300, 16, 0.01, 40.0, 4, 3, dtype=dtype)
        assert len(curve) == 8 and all(b < a for a, b in zip(curve, curve[1:])), curve


@pytest.mark.parametrize("kw, text", [
    (dict(factors=0), "factors must be in 1..128"), (dict(factors=129), "factors must be in 1..128"),
    (dict(cg_steps=0), "cg_steps must be in 1..32"), (dict(cg_steps=33), "cg_steps must be in 1..32"),
    (dict(regularization=-1.0), "regularization"), (dict(regularization=float("nan")), "regularization"),
    (dict(alpha=float("inf")), "alpha"), (dict(alpha=-2), "alpha"), (dict(iterations=-1), "iterations"),
    (dict(n_articles=0), "n_articles must be at least 1"), (dict(histories=[[0, 4]]), "history items must be in 0..3"),
    (dict(histories=[[0.5]]), "integer"), (dict(init=np.zeros((4, 3))), "init must be"),
])
def test_fit_als_argument_errors(kw, text):
    kw = dict(kw)
    hist, Na = kw.pop("histories", [[0, 1]]), kw.pop("n_articles", 4)
    with pytest.raises(ValueError, match=text):
        helpers.fit_als(hist, Na, **dict(dict(factors=8), **kw))


def test_helper_argument_errors():
    ptr, idx, cnt = np.array([0, 2, 2]), np.array([0, 3]), np.array([1, 2])
    Y, X = np.zeros((4, 8), dtype=np.float32), np.zeros((2, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="n_articles"):
        helpers.als_interactions([[0]], 0)
    with pytest.raises(ValueError, match="history items"):
        helpers.als_interactions([[0, 9]], 4)
    with pytest.raises(ValueError, match="fixed must be"):
        helpers.als_solve_rows(ptr, idx, cnt, np.zeros((4, 129), dtype=np.float32))
    with pytest.raises(ValueError, match="fixed must be"):
        helpers.als_gram(np.zeros(5))
    with pytest.raises(ValueError, match="cg_steps"):
        helpers.als_solve_rows(ptr, idx, cnt, Y, X, cg_steps=0)
    with pytest.raises(ValueError, match="factors must be"):
        helpers.als_solve_rows(ptr, idx, cnt, Y, np.zeros((3, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="gram must be"):
        helpers.als_solve_rows(ptr, idx, cnt, Y, X, gram=np.zeros((4, 4)))
    with pytest.raises(ValueError, match="idx must be in 0..3"):
        helpers.als_solve_rows(ptr, np.array([0, 4]), cnt, Y, X)
    with pytest.raises(ValueError, match="ptr must start at 0"):
        helpers.als_solve_rows(np.array([0, 2, 3]), idx, cnt, Y, X)
    with pytest.raises(ValueError, match="same number of columns"):
        helpers.als_loss(ptr, idx, cnt, np.zeros((2, 4), dtype=np.float32), Y)
    with pytest.raises(ValueError, match="ptr must have 3 elements"):
        helpers.als_loss(np.array([0, 2]), idx, cnt, X, Y)
    with pytest.raises(ValueError, match="alpha"):
        helpers.als_loss(ptr, idx, cnt, X, Y, alpha=float("nan"))
    with pytest.raises(ValueError, match="factors"):
        helpers.ALSModel(X, Y, 4, 0.01, 40.0, 3, 1)


def test_model_round_trip_on_the_host(tmp_path):
    rng = np.random.default_rng(4)
    X, Y = rng.standard_normal((5, 3)).astype(np.float32), rng.standard_normal((7, 3)).astype(np.float32)
    m = helpers.ALSModel(X, Y, 3, 0.01, 40.0, 3, 2, [5.0, 4.0, 3.5, 3.25])
    m.save(str(tmp_path / "als.npz"))
    back = helpers.ALSModel.load(str(tmp_path / "als.npz"))
    assert np.array_equal(back.user_factors, X) and np.array_equal(back.item_factors, Y) and back.user_factors.dtype == np.float32
    assert (back.factors, back.cg_steps, back.iterations, back.n_articles) == (3, 3, 2, 7)
    assert back.regularization == m.regularization and back.alpha == 40.0 and back.loss_curve == [5.0, 4.0, 3.5, 3.25]
    with pytest.raises(ValueError, match="items must be in 0..6"):
        back.similar([7])


# ---- the entry points: argument errors without a GPU (no pointer is ever followed) ----
FAKE = ctypes.c_void_p(256)


def _message(lib, prefix, text):
    msg = lib.dae_last_error().decode()
    assert msg.startswith(prefix) and text in msg, msg


@pytest.mark.parametrize("over, text", [
    (dict(F=0), "F (0) must be in 1..128"), (dict(F=129, ldy=129, ldx=129), "F (129) must be in 1..128"),
    (dict(cg_steps=0), "cg_steps (0) must be in 1..32"), (dict(cg_steps=33), "cg_steps (33)"), (dict(ptr=None), "is NULL"),
    (dict(idx=None), "is NULL"), (dict(cnt=None), "is NULL"), (dict(Y=None), "is NULL"), (dict(G=None), "is NULL"), (dict(X=None), "is NULL"),
    (dict(ldy=7), "must be >= F (8)"), (dict(ldx=7), "must be >= F (8)"), (dict(R=-1), "R (-1)"), (dict(N=0), "N (0)"),
    (dict(X=FAKE, Y=FAKE), "must not be the fixed factors"), (dict(ws=None), "256-byte aligned"), (dict(ws=ctypes.c_void_p(513)), "256-byte aligned"),
    (dict(ws_bytes=16), "workspace too small"),
])
def test_solve_rows_argument_errors_without_a_gpu(over, text):
    lib = _lib.load()
    a = dict(ptr=FAKE, idx=FAKE, cnt=FAKE, R=5, Y=FAKE, ldy=8, N=10, F=8, G=FAKE, alpha=40.0, cg_steps=3, X=ctypes.c_void_p(1024), ldx=8,
             ws=ctypes.c_void_p(512), ws_bytes=1 << 20, stream=None)
    a.update(over)
    assert lib.dae_als_solve_rows(*a.values()) == 1
    _message(lib, "als_solve_rows: ", text)


@pytest.mark.parametrize("over, text", [
    (dict(F=0), "F (0) must be in 1..128"), (dict(F=129, ldy=200), "F (129)"), (dict(N=0), "N (0)"), (dict(Y=None), "is NULL"),
    (dict(G=None), "is NULL"), (dict(ldy=3), "ldy (3) must be >= F (8)"), (dict(ws=None), "256-byte aligned"),
    (dict(ws_bytes=8), "workspace too small"),
])
def test_gram_argument_errors_without_a_gpu(over, text):
    lib = _lib.load()
    a = dict(Y=FAKE, ldy=8, N=10, F=8, lam=0.01, G=FAKE, ws=ctypes.c_void_p(512), ws_bytes=1 << 20, stream=None)
    a.update(over)
    assert lib.dae_als_gram(*a.values()) == 1
    _message(lib, "als_gram: ", text)


@pytest.mark.parametrize("over, text", [
    (dict(F=0), "F (0) must be in 1..128"), (dict(F=129, ldx=129, ldy=129), "F (129)"), (dict(R=0), "R (0)"), (dict(N=0), "N (0)"),
    (dict(ptr=None), "is NULL"), (dict(X=None), "is NULL"), (dict(loss=None), "is NULL"), (dict(ldx=7), "must be >= F (8)"),
    (dict(ws=None), "256-byte aligned"), (dict(ws_bytes=8), "workspace too small"),
])
def test_loss_argument_errors_without_a_gpu(over, text):
    lib = _lib.load()
    a = dict(ptr=FAKE, idx=FAKE, cnt=FAKE, R=5, X=FAKE, ldx=8, Y=FAKE, ldy=8, N=10, F=8, alpha=40.0, lam=0.01, loss=FAKE,
             ws=ctypes.c_void_p(512), ws_bytes=1 << 20, stream=None)
    a.update(over)
    assert lib.dae_als_loss(*a.values()) == 1
    _message(lib, "als_loss: ", text)


@pytest.mark.parametrize("over, text", [
    (dict(user_ptr=None), "an output is NULL"), (dict(item_cnt=None), "an output is NULL"), (dict(totals=None), "an output is NULL"),
    (dict(M=-1), "must not be negative"), (dict(nnz=-1), "must not be negative"), (dict(Na=0), "Na (0) must be at least 1"),
    (dict(nnz=1 << 31, cap=1 << 32), "fewer than 2^31"), (dict(cap=2), "cap (2) must be >= nnz (3)"), (dict(M=0), "without a user"),
    (dict(indptr=None), "indptr / items is NULL"), (dict(items=None), "indptr / items is NULL"), (dict(ws=None), "256-byte aligned"),
    (dict(ws=ctypes.c_void_p(520)), "256-byte aligned"), (dict(ws_bytes=64), "workspace too small"),
])
def test_interactions_argument_errors_without_a_gpu(over, text):
    lib = _lib.load()
    a = dict(indptr=FAKE, items=FAKE, M=2, nnz=3, Na=10, user_ptr=FAKE, user_idx=FAKE, user_cnt=FAKE, item_ptr=FAKE, item_idx=FAKE,
             item_cnt=FAKE, cap=3, totals=FAKE, ws=ctypes.c_void_p(512), ws_bytes=1 << 20, stream=None)
    a.update(over)
    assert lib.dae_als_interactions(*a.values()) == 1
    _message(lib, "als_interactions: ", text)


def test_workspace_queries():
    lib = _lib.load()
    assert lib.dae_als_solve_rows_workspace(0) == 0 and lib.dae_als_solve_rows_workspace(1000) == 256 + 4096
    assert lib.dae_als_gram_workspace(10, 0) == 0 and lib.dae_als_gram_workspace(10, 129) == 0 and lib.dae_als_gram_workspace(0, 8) == 0
    assert lib.dae_als_gram_workspace(1, 8) == 512 and lib.dae_als_gram_workspace(10 ** 6, 128) == 256 * 128 * 128 * 8
    assert lib.dae_als_loss_workspace(5, 10, 0) == 0 and lib.dae_als_loss_workspace(0, 10, 8) == 0 and lib.dae_als_loss_workspace(5, 10, 8) > 0
    for nnz, M, Na in ((0, 5, 5), (1 << 31, 5, 5), (10, 0, 5), (10, 5, 0)):
        assert lib.dae_als_interactions_workspace(nnz, M, Na) == 0
