"""NumPy restatement of the implicit-feedback ALS model (include/dae_hip.h, "Implicit-feedback matrix factorisation"): the
interaction build with np.unique, one half-sweep of conjugate gradient per row with a ``dtype`` argument (float64: the reference;
float32: the yardstick of the device's rounding error), the loss in float64, and a whole fit."""
import numpy as np


def interactions_reference(indptr, items, Na):
    """Both orientations of the de-duplicated interaction matrix of a history CSR: a dict with ``user_ptr`` int64 [M + 1],
    ``user_idx`` / ``user_cnt`` int32, ``item_ptr`` int64 [Na + 1], ``item_idx`` / ``item_cnt`` int32, ``events``, ``pairs``.
    An item outside [0, Na) is no event."""
    indptr = np.asarray(indptr, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    M = indptr.size - 1
    user = np.repeat(np.arange(M, dtype=np.int64), np.diff(indptr))
    ok = (items >= 0) & (items < Na)
    user, item = user[ok], items[ok]
    key, cnt = np.unique(user * Na + item, return_counts=True)
    u, i = key // Na, key % Na
    out = {"events": int(ok.sum()), "pairs": int(key.size)}
    out["user_ptr"] = np.searchsorted(u, np.arange(M + 1)).astype(np.int64)
    out["user_idx"], out["user_cnt"] = i.astype(np.int32), cnt.astype(np.int32)
    order = np.lexsort((u, i))
    out["item_ptr"] = np.searchsorted(i[order], np.arange(Na + 1)).astype(np.int64)
    out["item_idx"], out["item_cnt"] = u[order].astype(np.int32), cnt[order].astype(np.int32)
    return out


def gram_reference(Y, lam):
    """Y^T Y + lambda I in float64."""
    Y = np.asarray(Y, dtype=np.float64)
    return Y.T @ Y + np.float64(lam) * np.eye(Y.shape[1])


def half_sweep_reference(ptr, idx, cnt, Y, X, lam, alpha, cg_steps, dtype=np.float64, G=None):
    """One half-sweep: the rows of ``X`` (a copy is returned) solved against the fixed ``Y`` by ``cg_steps`` steps of conjugate
    gradient from their current values, every operation in ``dtype``.  A row without entries gets 0; a row's iteration stops
    when rs <= 1e-20 or p . Ap <= 0; the entries are visited in stored order.  ``G``: Y^T Y + lambda I, when the caller has it
    (the float32 restatement takes the float64 Gram rounded once, as the device does)."""
    dt = np.dtype(dtype).type
    Y = np.asarray(Y).astype(dt)
    X = np.array(X, dtype=dt, copy=True)
    G = (gram_reference(Y, lam) if G is None else np.asarray(G)).astype(dt)
    alpha = dt(alpha)
    one = dt(1)
    for u in range(X.shape[0]):
        e0, e1 = int(ptr[u]), int(ptr[u + 1])
        if e1 == e0:
            X[u] = 0
            continue
        Yu = Y[idx[e0:e1]]
        a = alpha * cnt[e0:e1].astype(dt)

        def apply(v):
            return G @ v + (Yu * (a * (Yu @ v))[:, None]).sum(axis=0, dtype=dt)

        x = X[u].copy()
        b = (Yu * (one + a)[:, None]).sum(axis=0, dtype=dt)
        r = b - apply(x)
        p = r.copy()
        rs = r @ r
        for _ in range(cg_steps):
            if rs <= 1e-20:
                break
            Ap = apply(p)
            pAp = p @ Ap
            if not pAp > 0:
                break
            step = rs / pAp
            x = x + step * p
            r = r - step * Ap
            rsn = r @ r
            p = r + (rsn / rs) * p
            rs = rsn
        X[u] = x
    return X


def loss_reference(ptr, idx, cnt, X, Y, lam, alpha):
    """The objective in float64 without the M x Na matrix: sum_u x_u^T (Y^T Y) x_u + sum over the stored entries of
    [c (1 - s)^2 - s^2] + lambda (|X|^2 + |Y|^2)."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(ptr))
    s = np.einsum("ij,ij->i", X[rows], Y[idx])
    c = 1.0 + np.float64(alpha) * np.asarray(cnt, dtype=np.float64)
    quad = ((X @ (Y.T @ Y)) * X).sum()
    return float(quad + (c * (1.0 - s) ** 2 - s * s).sum() + np.float64(lam) * ((X * X).sum() + (Y * Y).sum()))


def loss_literal(ptr, idx, cnt, X, Y, lam, alpha):
    """The objective as it is written: the double sum over all rows x columns pairs.  For small cases only."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    R = np.zeros((X.shape[0], Y.shape[0]))
    for u in range(X.shape[0]):
        R[u, idx[ptr[u]:ptr[u + 1]]] = cnt[ptr[u]:ptr[u + 1]]
    total = 0.0
    for u in range(X.shape[0]):
        for i in range(Y.shape[0]):
            total += (1.0 + alpha * R[u, i]) * (float(R[u, i] > 0) - X[u] @ Y[i]) ** 2
    return total + lam * ((X * X).sum() + (Y * Y).sum())


def initial_item_factors(Na, F, seed):
    """The start of ``fit_als``: 0.01 * N(0, 1) from ``np.random.default_rng(seed)``, float32."""
    return (0.01 * np.random.default_rng(seed).standard_normal((Na, F))).astype(np.float32)


def fit_reference(inter, M, Na, F, lam, alpha, iterations, cg_steps, seed=0, dtype=np.float64, init=None):
    """``fit_als`` restated: per iteration a user half-sweep, then an article half-sweep, the loss after each.  ``lam`` and
    ``alpha`` are taken as the float32 numbers the device gets.  Returns ``(X, Y, loss_curve)``."""
    lam, alpha = float(np.float32(lam)), float(np.float32(alpha))
    Y = (initial_item_factors(Na, F, seed) if init is None else np.asarray(init)).astype(dtype)
    X = np.zeros((M, F), dtype=dtype)
    curve = []

    def gram(Z):
        G = gram_reference(Z, lam)
        return G.astype(np.float32) if np.dtype(dtype) == np.float32 else G

    for _ in range(iterations):
        X = half_sweep_reference(inter["user_ptr"], inter["user_idx"], inter["user_cnt"], Y, X, lam, alpha, cg_steps, dtype, gram(Y))
        curve.append(loss_reference(inter["user_ptr"], inter["user_idx"], inter["user_cnt"], X, Y, lam, alpha))
        Y = half_sweep_reference(inter["item_ptr"], inter["item_idx"], inter["item_cnt"], X, Y, lam, alpha, cg_steps, dtype, gram(X))
        curve.append(loss_reference(inter["user_ptr"], inter["user_idx"], inter["user_cnt"], X, Y, lam, alpha))
    return X, Y, curve
