"""CPU checks of the trained decay user model (dae_user_pair_loss, helpers.fit_user_model and the host code around them): the
float64 restatement of the definition in include/dae_hip.h (``restate`` below, which tests/test_hip_user_fit.py holds the kernel
against) agrees with finite differences of its own loss; decay_factor_derivatives against a finite difference of decay_factors;
sample_negatives; and the argument checks of the entry point, which are reported before any HIP call."""
import ctypes

import numpy as np
import pytest

P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first


def restate(E, indptr, items, alpha, f, fp, negatives, dtype=np.float64):
    """The definition of dae_user_pair_loss, event by event.  ``f`` / ``fp``: the factor of every event and its derivative with
    respect to beta.  The chain and the dot products run in ``dtype``; every sum over pairs is float64.  Returns loss, dalpha,
    dbeta, n_pairs, margins [nnz x n_neg], the mask of the valid pairs, and the magnitude sums S_loss, S_alpha [H], S_beta that
    scale the gates of the GPU test; and for the exact cases ``num`` [nnz x n_neg], the numerator sum_h alpha_h s_h D_h of every
    margin, ``z`` [nnz], the denominator before every event, and ``exact_bound``: the largest sum_h |alpha_h s_h D_h| of a pair."""
    T = dtype
    E = np.asarray(E).astype(T)
    al = np.asarray(alpha).astype(T)
    f = np.asarray(f).astype(T)
    fp = np.asarray(fp).astype(T)
    neg = np.asarray(negatives)
    nnz, n_neg = neg.shape
    H = E.shape[1]
    out = dict(loss=0.0, dalpha=np.zeros(H), dbeta=0.0, n_pairs=0, margins=np.zeros((nnz, n_neg), T), valid=np.zeros((nnz, n_neg), bool),
               S_loss=0.0, S_alpha=np.zeros(H), S_beta=0.0, exact_bound=0.0, num=np.zeros((nnz, n_neg)), z=np.zeros(nnz))
    one = T(1)
    for u in range(len(indptr) - 1):
        s = g = np.zeros(H, T)
        z = zg = T(0)
        for e in range(int(indptr[u]), int(indptr[u + 1])):
            row = E[items[e]]
            if e == indptr[u]:
                s, z, g, zg = row.copy(), one, np.zeros(H, T), T(0)
                continue
            out["z"][e] = z
            for j in range(n_neg):
                n = int(neg[e, j])
                if n < 0 or n == items[e]:
                    continue
                D = row - E[n]
                x = T((al * s * D).sum(dtype=T) / z)
                xb = T((al * g * D).sum(dtype=T) / z - x * (zg / z))
                x64 = float(x)
                sp = max(-x64, 0.0) + np.log1p(np.exp(-abs(x64)))
                c = -np.exp(-np.logaddexp(0.0, x64))                        # -sigmoid(-x), no overflow
                uD = (s * D / z).astype(np.float64)
                out["loss"] += sp
                out["dalpha"] += c * uD
                out["dbeta"] += c * float(xb)
                out["n_pairs"] += 1
                out["margins"][e, j] = x
                out["valid"][e, j] = True
                out["num"][e, j] = (al * s * D).sum(dtype=T)
                al64, D64 = al.astype(np.float64), D.astype(np.float64)
                up = g.astype(np.float64) / float(z) - s.astype(np.float64) * float(zg) / float(z) ** 2      # d(s / z) / dbeta
                X = np.abs(al64 * uD).sum()
                XB = np.abs(al64 * up * D64).sum()
                out["S_loss"] += sp + X
                out["S_alpha"] += (abs(c) + X / 4) * np.abs(uD)
                out["S_beta"] += (abs(c) + X / 4) * XB
                out["exact_bound"] = max(out["exact_bound"], float(np.abs(al64 * s.astype(np.float64) * D64).sum()))
            g, zg, s, z = f[e] * g + fp[e] * s, f[e] * zg + fp[e] * z, f[e] * s + row, f[e] * z + one
    return out


def _case(seed=5, H=12, Na=40, lengths=(0, 1, 2, 9, 17, 5), n_neg=3):
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((Na, H))
    indptr = np.zeros(len(lengths) + 1, np.int64)
    indptr[1:] = np.cumsum(lengths)
    items = rng.integers(0, Na, int(indptr[-1]))
    neg = rng.integers(-1, Na, (items.size, n_neg))
    neg[3, 0] = items[3]                                                   # the click itself: no pair
    alpha = 1.0 + 0.3 * rng.standard_normal(H)
    return E, indptr, items, neg, alpha, rng


def test_restatement_agrees_with_finite_differences_scalar_beta():
    E, indptr, items, neg, alpha, _ = _case()
    nnz = items.size
    loss = lambda a, b: restate(E, indptr, items, a, np.full(nnz, b), np.ones(nnz), neg)["loss"]
    beta = 0.8
    r = restate(E, indptr, items, alpha, np.full(nnz, beta), np.ones(nnz), neg)
    assert r["n_pairs"] == int(r["valid"].sum()) > 50
    h = 1e-5
    fd = (loss(alpha, beta + h) - loss(alpha, beta - h)) / (2 * h)
    assert abs(fd - r["dbeta"]) <= 1e-7 * max(abs(r["dbeta"]), 1.0), (fd, r["dbeta"])
    for k in (0, 3, 11):
        d = np.zeros_like(alpha); d[k] = h
        fd = (loss(alpha + d, beta) - loss(alpha - d, beta)) / (2 * h)
        assert abs(fd - r["dalpha"][k]) <= 1e-7 * max(abs(r["dalpha"][k]), 1.0), (k, fd, r["dalpha"][k])


def test_restatement_agrees_with_finite_differences_timed_factors():
    """Per-event factors beta ** p with derivative p beta ** (p - 1), simultaneous events (p = 0) included."""
    E, indptr, items, neg, alpha, rng = _case(seed=6)
    p = rng.choice([0.0, 0.5, 1.0, 2.5], items.size)
    fac = lambda b: (np.power(b, p), np.where(p > 0, p * np.power(b, p - 1.0), 0.0))
    loss = lambda b: restate(E, indptr, items, alpha, *fac(b), neg)["loss"]
    beta, h = 0.7, 1e-5
    r = restate(E, indptr, items, alpha, *fac(beta), neg)
    fd = (loss(beta + h) - loss(beta - h)) / (2 * h)
    assert abs(fd - r["dbeta"]) <= 1e-7 * max(abs(r["dbeta"]), 1.0), (fd, r["dbeta"])
    # f' = 0 everywhere: dbeta is 0 and nothing else moves
    r0 = restate(E, indptr, items, alpha, fac(beta)[0], np.zeros(items.size), neg)
    assert r0["dbeta"] == 0.0 and r0["loss"] == r["loss"] and np.array_equal(r0["dalpha"], r["dalpha"])


def test_decay_factor_derivatives_against_a_finite_difference():
    """decay_factors is rounded to float32: a central difference with h = 1e-3 carries 2**-24 / (2 h) = 3e-5 of rounding and
    h**2 / 6 * |f'''| <= 1e-5 of truncation at these exponents (p <= 5, beta = 0.8); the bound is 1e-4."""
    from dae_rnn_news_recommendation_amd.helpers import decay_factor_derivatives, decay_factors
    indptr = np.array([0, 4, 4, 9])
    t = np.array([1.0, 3.0, 3.0, 8.0, 0.5, 1.5, 1.5, 4.0, 14.0])
    beta, unit, h = 0.8, 2.0, 1e-3
    d = decay_factor_derivatives(indptr, t, beta, unit)
    assert d.dtype == np.float32 and d.shape == (9,)
    fd = (decay_factors(indptr, t, beta + h, unit).astype(np.float64) - decay_factors(indptr, t, beta - h, unit)) / (2 * h)
    assert np.abs(fd - d).max() <= 1e-4, np.abs(fd - d).max()
    assert d[0] == 0 and d[4] == 0 and d[2] == 0 and d[6] == 0             # first events and simultaneous ones
    p = np.array([0, 1.0, 0, 2.5, 0, 0.5, 0, 1.25, 5.0])
    assert np.array_equal(d, np.where(p > 0, p * np.power(beta, p - 1.0), 0.0).astype(np.float32))      # float64, rounded once
    assert np.array_equal(decay_factor_derivatives(indptr, t, 1.0), np.where(p > 0, 2 * p, 0).astype(np.float32))
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="beta"):
            decay_factor_derivatives(indptr, t, bad)
    with pytest.raises(ValueError, match="decrease within a user"):
        decay_factor_derivatives(indptr, t[::-1].copy(), 0.5)


def test_sample_negatives():
    from dae_rnn_news_recommendation_amd.helpers import sample_negatives
    rng = np.random.default_rng(1)
    lengths = [0, 1, 5, 40, 1, 300]
    indptr = np.zeros(len(lengths) + 1, np.int64)
    indptr[1:] = np.cumsum(lengths)
    items = rng.integers(0, 50, int(indptr[-1])).astype(np.int32)
    a = sample_negatives(indptr, items, 50, 4, seed=7)
    assert a.dtype == np.int32 and a.shape == (items.size, 4) and a.flags.c_contiguous
    assert np.array_equal(a, sample_negatives(indptr, items, 50, 4, seed=7))
    assert not np.array_equal(a, sample_negatives(indptr, items, 50, 4, seed=8))
    first = np.zeros(items.size, bool)
    first[indptr[:-1][np.diff(indptr) > 0]] = True
    assert (a[first] == -1).all()
    rest = a[~first]
    assert rest.min() >= -1 and rest.max() < 50 and (rest != items[~first][:, None]).all()
    # -1 exactly where specified: the draw itself is uniform over the range, so with 50 articles about 1 in 50 hits the click
    share = (rest == -1).mean()
    assert 0.0 < share < 0.06, share
    assert len(np.unique(rest)) == 51                                     # every article and -1 occur among 1 368 draws
    # per-event windows: draws stay inside, an empty window gives -1, a window holding only the click gives -1
    lo = rng.integers(0, 40, items.size)
    hi = lo + rng.integers(0, 11, items.size)
    hi[5], lo[5] = lo[5], lo[5]
    lo[7], hi[7] = items[7], items[7] + 1
    w = sample_negatives(indptr, items, 50, 3, seed=2, window=(lo, hi))
    ok = w >= 0
    assert ((w >= lo[:, None]) & (w < hi[:, None]))[ok].all()
    assert (w[hi == lo] == -1).all() and (w[7] == -1).all() and (w[first] == -1).all()
    inside = ~first & (hi - lo >= 2)
    assert (w[inside] >= 0).mean() > 0.7
    assert np.array_equal(w, sample_negatives(indptr, items, 50, 3, seed=2, window=(lo, hi)))
    with pytest.raises(ValueError):
        sample_negatives(indptr, items, 50, 0, seed=1)
    with pytest.raises(ValueError):
        sample_negatives(indptr, items, 50, 2, seed=1, window=(lo[:-1], hi[:-1]))
    with pytest.raises(ValueError):
        sample_negatives(indptr, items[:-1], 50, 2, seed=1)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_new_symbols_are_exported_and_the_abi_version_stays(fmt):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load(fmt)
    for name in ("dae_user_pair_loss", "dae_user_pair_loss_workspace"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.dae_abi_version() == _lib.ABI_VERSION == 9


def _pl(lib, E=P, lde=64, Na=100, H=64, indptr=P, items=P, M=10, nnz=50, beta=0.9, decay=None, ddecay=None, alpha=P, neg=P, n_neg=4,
        loss=P, dalpha=P, dbeta=P, n_pairs=P, margin=None, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_user_pair_loss_workspace(M, H)
    return lib.dae_user_pair_loss(E, lde, Na, H, indptr, items, M, nnz, beta, decay, ddecay, alpha, neg, n_neg, loss, dalpha, dbeta,
                                  n_pairs, margin, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(E=None), b"E / indptr / alpha are NULL"),
    (dict(indptr=None), b"E / indptr / alpha are NULL"),
    (dict(alpha=None), b"E / indptr / alpha are NULL"),
    (dict(items=None), b"items / negatives are NULL"),
    (dict(neg=None), b"items / negatives are NULL"),
    (dict(loss=None), b"loss / dalpha / dbeta / n_pairs are NULL"),
    (dict(dalpha=None), b"loss / dalpha / dbeta / n_pairs are NULL"),
    (dict(dbeta=None), b"loss / dalpha / dbeta / n_pairs are NULL"),
    (dict(n_pairs=None), b"loss / dalpha / dbeta / n_pairs are NULL"),
    (dict(n_neg=0), b"n_neg must be in 1..16"),
    (dict(n_neg=17), b"n_neg must be in 1..16"),
    (dict(H=0, ws_bytes=1 << 20), b"H must be in 1..1024"),
    (dict(H=1025, lde=2048, ws_bytes=1 << 30), b"H must be in 1..1024"),
    (dict(lde=63), b"must be >= H"),
    (dict(Na=0), b"Na must be positive"),
    (dict(M=-1, ws_bytes=1 << 20), b"negative count"),
    (dict(nnz=-1), b"negative count"),
    (dict(beta=1.5), b"beta must be in [0, 1]"),
    (dict(beta=float("nan")), b"beta must be in [0, 1]"),
    (dict(ddecay=P), b"ddecay without decay"),
    (dict(ws=None), b"workspace too small"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
])
def test_pair_loss_argument_errors_without_a_gpu(kw, msg):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load()
    assert _pl(lib, **kw) != 0
    assert msg in lib.dae_last_error(), lib.dae_last_error()


def test_workspace_is_bounded_and_linear_in_h():
    from dae_rnn_news_recommendation_amd import _lib
    ws = _lib.load().dae_user_pair_loss_workspace
    assert 0 < ws(1, 1) <= 16 * 1024
    assert ws(10 ** 7, 500) == ws(10 ** 9, 500) < 64 << 20                 # one partial per wave, and the waves are capped: no term in M
    assert ws(10 ** 7, 1024) < 128 << 20
    assert ws(100, 70) < ws(100, 500) < ws(100, 1024)
    assert ws(5, 0) == 0 and ws(5, 1025) == 0 and ws(-1, 8) == 0


def test_host_errors_of_the_helpers_raise_before_any_device_work():
    from dae_rnn_news_recommendation_amd import helpers
    with pytest.raises(ValueError, match="beta0"):
        helpers.fit_user_model([[1, 2]], np.ones((4, 3), np.float32), beta0=1.5)
    with pytest.raises(ValueError, match="beta"):
        helpers.user_pair_loss([[1, 2]], np.ones((4, 3), np.float32), np.ones(3), -0.5, np.zeros((2, 1), np.int64))
