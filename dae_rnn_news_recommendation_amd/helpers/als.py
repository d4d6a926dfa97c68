"""Implicit-feedback matrix factorisation by alternating least squares (Hu, Koren and Volinsky 2008): the ID-based collaborative
filter every recommender is compared against first.  ``als_interactions`` turns a click log into both orientations of the
de-duplicated interaction matrix on the device, ``als_gram`` / ``als_solve_rows`` / ``als_loss`` are the three device calls of a
half-sweep, ``fit_als`` alternates them and returns an ``ALSModel`` whose factors are ordinary ``[rows x F]`` float32 matrices:
``recommend``, ``recommend_ranks``, ``most_similar`` and the rest take them with ``metric='linear kernel'``.  The rules of the model
are stated in include/dae_hip.h."""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ._device import device_and_library, history_csr, result, upload, workspace
from .user_models import trim_histories

MAX_FACTORS = 128
MAX_CG_STEPS = 32


def _settings(factors, regularization, alpha, cg_steps):
    if not 1 <= int(factors) <= MAX_FACTORS:
        raise ValueError(f"factors must be in 1..{MAX_FACTORS} (got {factors})")
    if not 1 <= int(cg_steps) <= MAX_CG_STEPS:
        raise ValueError(f"cg_steps must be in 1..{MAX_CG_STEPS} (got {cg_steps})")
    if not (np.isfinite(float(regularization)) and float(regularization) >= 0):
        raise ValueError(f"regularization must be finite and not negative (got {regularization})")
    if not (np.isfinite(float(alpha)) and float(alpha) >= 0):
        raise ValueError(f"alpha must be finite and not negative (got {alpha})")
    return int(factors), float(np.float32(regularization)), float(np.float32(alpha)), int(cg_steps)


class ALSInteractions:
    """What ``als_interactions`` returns: ``user`` = ``(ptr int64 [users + 1], idx int32, cnt int32)`` -- per user the distinct
    articles ascending and how often each was clicked -- and ``item`` = the same per article over its users; ``n_users``,
    ``n_articles``, ``n_events`` and ``n_pairs``.  Arrays are ndarrays or CUDA tensors."""

    def __init__(self, user, item, n_users, n_articles, n_events, n_pairs):
        self.user, self.item = tuple(user), tuple(item)
        self.n_users, self.n_articles, self.n_events, self.n_pairs = int(n_users), int(n_articles), int(n_events), int(n_pairs)


def als_interactions(histories, n_articles, *, max_events=None, return_tensor=False, device=None):
    """Both orientations of the interaction matrix of a click log, built on the device (``dae_als_interactions``: 64-bit keys,
    radix sort, run-length encode; integers only).  ``histories``: a list of index sequences or an ``(indptr, items)`` tuple over
    ``n_articles`` articles; repeats in a history count.  ``max_events``: only every user's most recent events
    (``trim_histories``).  Returns an ``ALSInteractions``.  One call takes fewer than 2^31 events: a larger log raises
    ``ValueError`` with the figure -- build from fewer users."""
    Na = int(n_articles)
    if Na < 1:
        raise ValueError(f"n_articles must be at least 1 (got {n_articles})")
    indptr, items = history_csr(histories if max_events is None else trim_histories(histories, max_events), Na)
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    M, nnz = indptr.size - 1, int(items.size)
    if nnz >= 1 << 31:
        raise ValueError(f"the log has {nnz} events ({24 * nnz / 2 ** 30:.1f} GiB of build buffers); one call takes fewer than 2^31 -- "
                         "build from fewer users")
    torch, lib, dev = device_and_library(device)
    i32 = dict(dtype=torch.int32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    cap = max(nnz, 1)
    user = (torch.empty(M + 1, **i64), torch.empty(cap, **i32), torch.empty(cap, **i32))
    item = (torch.empty(Na + 1, **i64), torch.empty(cap, **i32), torch.empty(cap, **i32))
    totals = torch.empty(2, **i64)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.dae_als_interactions_workspace(nnz, M, Na)) if nnz > 0 else 0
        if nnz > 0 and ws_bytes == 0:
            raise RuntimeError("dae_als_interactions_workspace: the size query failed")
        ws_p, ws = workspace(dev, ws_bytes)
        d_ptr, d_items = upload(indptr, dev), upload(items.astype(np.int32), dev)
        L.call("dae_als_interactions", L.ptr(d_ptr), L.ptr(d_items), M, nnz, Na, L.ptr(user[0]), L.ptr(user[1]), L.ptr(user[2]),
               L.ptr(item[0]), L.ptr(item[1]), L.ptr(item[2]), cap, L.ptr(totals), ws_p if nnz > 0 else None, ws_bytes, L.current_stream())
        del ws
    n_events, n_pairs = (int(v) for v in totals.cpu().numpy())
    cut = lambda t: (t[0], t[1][:n_pairs], t[2][:n_pairs])      # noqa: E731
    return ALSInteractions(result(cut(user), return_tensor), result(cut(item), return_tensor), M, Na, n_events, n_pairs)


def _csr_on_device(torch, dev, ptr, idx, cnt):
    """``(ptr int64, idx int32, cnt int32)`` as contiguous device tensors."""
    out = []
    for a, dt in ((ptr, torch.int64), (idx, torch.int32), (cnt, torch.int32)):
        if isinstance(a, torch.Tensor):
            out.append(a.to(device=dev, dtype=dt).contiguous())
        else:
            out.append(upload(np.ascontiguousarray(a, dtype=np.int64 if dt == torch.int64 else np.int32), dev))
    return out


def _check_csr(ptr, idx, cnt, n_fixed):
    """The host-side check of a CSR that is still on the host (device tensors are bounds-checked by the kernels themselves)."""
    if hasattr(ptr, "is_cuda") or hasattr(idx, "is_cuda"):
        return
    ptr, idx, cnt = np.asarray(ptr), np.asarray(idx), np.asarray(cnt)
    if ptr.ndim != 1 or ptr.size < 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != idx.size or idx.size != cnt.size:
        raise ValueError("ptr must start at 0, be non-decreasing and end at len(idx) == len(cnt)")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n_fixed):
        raise ValueError(f"idx must be in 0..{n_fixed - 1} (got {int(idx.min())}..{int(idx.max())})")


def _factor_shape(a, what):
    shape = tuple(getattr(a, "shape", np.shape(a)))
    if len(shape) != 2 or shape[0] < 1 or not 1 <= shape[1] <= MAX_FACTORS:
        raise ValueError(f"{what} must be [rows x F] with 1 <= F <= {MAX_FACTORS} (got shape {shape})")
    return int(shape[0]), int(shape[1])


def _f32_on_device(torch, dev, a):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float32))
    t = t.to(device=dev, dtype=torch.float32)
    return t if t.stride(-1) == 1 and t.dim() == 2 else t.contiguous()


def als_gram(fixed, regularization=0.01, *, return_tensor=False, device=None):
    """``fixed^T fixed + regularization * I`` as float32 ``[F x F]``: fp64 sums in a fixed order, rounded once (``dae_als_gram``)."""
    N, F = _factor_shape(fixed, "fixed")
    _, lam, _, _ = _settings(F, regularization, 0.0, 1)
    torch, lib, dev = device_and_library(device)
    Y = _f32_on_device(torch, dev, fixed)
    G = torch.empty((F, F), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.dae_als_gram_workspace(N, F))
        ws_p, ws = workspace(dev, ws_bytes)
        L.call("dae_als_gram", L.ptr(Y), Y.stride(0), N, F, lam, L.ptr(G), ws_p, ws_bytes, L.current_stream())
        torch.cuda.current_stream().synchronize()
        del ws
    return result(G, return_tensor)


def als_solve_rows(ptr, idx, cnt, fixed, factors=None, *, regularization=0.01, alpha=40.0, cg_steps=3, gram=None, return_tensor=False,
                   device=None):
    """One half-sweep (``dae_als_solve_rows``): every row of ``factors`` (``[rows x F]``; None: zeros) moved ``cg_steps`` steps of
    conjugate gradient towards the minimiser of the implicit-feedback objective against the fixed factors ``fixed``
    ``[n x F]``, where row ``r`` has the entries ``idx[ptr[r]:ptr[r + 1]]`` (rows of ``fixed``) with the counts ``cnt``.  ``gram``:
    ``als_gram(fixed, regularization)`` when the caller has it.  A CUDA float32 tensor ``factors`` is updated in place and
    returned; anything else is copied.  A row without entries becomes 0.  Bit-identical from run to run, whatever the order of the
    rows."""
    N, F = _factor_shape(fixed, "fixed")
    _, lam, alpha, cg_steps = _settings(F, regularization, alpha, cg_steps)
    R = int(ptr.shape[0] if hasattr(ptr, "shape") else len(ptr)) - 1
    if R < 0:
        raise ValueError("ptr must have at least one element")
    if factors is not None and tuple(getattr(factors, "shape", np.shape(factors))) != (R, F):
        raise ValueError(f"factors must be [{R} x {F}] (got {tuple(getattr(factors, 'shape', np.shape(factors)))})")
    if gram is not None and tuple(gram.shape) != (F, F):
        raise ValueError(f"gram must be [{F} x {F}] (got {tuple(gram.shape)})")
    _check_csr(ptr, idx, cnt, N)
    torch, lib, dev = device_and_library(device)
    Y = _f32_on_device(torch, dev, fixed)
    if factors is None:
        X = torch.zeros((R, F), dtype=torch.float32, device=dev)
    else:
        X = _f32_on_device(torch, dev, factors)
        if X.data_ptr() == Y.data_ptr():
            raise ValueError("factors and fixed must be different matrices")
    if R == 0:
        return result(X, return_tensor)
    G = als_gram(Y, lam, return_tensor=True, device=dev) if gram is None else _f32_on_device(torch, dev, gram).contiguous()
    d_ptr, d_idx, d_cnt = _csr_on_device(torch, dev, ptr, idx, cnt)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.dae_als_solve_rows_workspace(R))
        ws_p, ws = workspace(dev, ws_bytes)
        L.call("dae_als_solve_rows", L.ptr(d_ptr), L.ptr(d_idx), L.ptr(d_cnt), R, L.ptr(Y), Y.stride(0), N, F, L.ptr(G), alpha, cg_steps,
               L.ptr(X), X.stride(0), ws_p, ws_bytes, L.current_stream())
        torch.cuda.current_stream().synchronize()
        del ws
    return result(X, return_tensor)


def als_loss(ptr, idx, cnt, factors, fixed, *, regularization=0.01, alpha=40.0, device=None):
    """The implicit-feedback objective over ALL rows x columns pairs, without that matrix (``dae_als_loss``, fp64 sums in a fixed
    order): ``factors`` ``[rows x F]`` are the rows of the CSR, ``fixed`` ``[n x F]`` what ``idx`` points into.  A float."""
    N, F = _factor_shape(fixed, "fixed")
    R, F2 = _factor_shape(factors, "factors")
    if F2 != F:
        raise ValueError(f"factors and fixed must have the same number of columns (got {F2} and {F})")
    _, lam, alpha, _ = _settings(F, regularization, alpha, 1)
    n_ptr = int(ptr.shape[0] if hasattr(ptr, "shape") else len(ptr))
    if n_ptr != R + 1:
        raise ValueError(f"ptr must have {R + 1} elements (got {n_ptr})")
    _check_csr(ptr, idx, cnt, N)
    torch, lib, dev = device_and_library(device)
    X, Y = _f32_on_device(torch, dev, factors), _f32_on_device(torch, dev, fixed)
    d_ptr, d_idx, d_cnt = _csr_on_device(torch, dev, ptr, idx, cnt)
    out = torch.empty(1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.dae_als_loss_workspace(R, N, F))
        ws_p, ws = workspace(dev, ws_bytes)
        L.call("dae_als_loss", L.ptr(d_ptr), L.ptr(d_idx), L.ptr(d_cnt), R, L.ptr(X), X.stride(0), L.ptr(Y), Y.stride(0), N, F, alpha, lam,
               L.ptr(out), ws_p, ws_bytes, L.current_stream())
        value = float(out.cpu().numpy()[0])
        del ws
    return value


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class ALSModel:
    """What ``fit_als`` returns: ``user_factors`` ``[users x F]`` and ``item_factors`` ``[articles x F]`` float32 (ndarrays or
    CUDA tensors), the settings ``factors``, ``regularization``, ``alpha``, ``cg_steps``, ``iterations``, and ``loss_curve`` -- the
    objective after every half-sweep when it was asked for, else empty."""

    _SCALARS = ("factors", "regularization", "alpha", "cg_steps", "iterations")

    def __init__(self, user_factors, item_factors, factors, regularization, alpha, cg_steps, iterations, loss_curve=()):
        self.user_factors, self.item_factors = user_factors, item_factors
        self.factors, self.cg_steps, self.iterations = int(factors), int(cg_steps), int(iterations)
        self.regularization, self.alpha = float(regularization), float(alpha)
        self.loss_curve = [float(v) for v in loss_curve]
        if len(item_factors.shape) != 2 or len(user_factors.shape) != 2 or item_factors.shape[1] != self.factors or \
                user_factors.shape[1] != self.factors:
            raise ValueError("user_factors and item_factors must be [rows x factors]")

    n_articles = property(lambda self: int(self.item_factors.shape[0]))

    def user_states(self, histories, *, return_tensor=False, device=None):
        """The factors of any users, new ones included, folded in from their ``histories``: one user half-sweep from zero
        against the stored article factors.  ``[users x F]`` float32."""
        inter = als_interactions(histories, self.n_articles, return_tensor=True, device=device)
        return als_solve_rows(*inter.user, self.item_factors, None, regularization=self.regularization, alpha=self.alpha,
                              cg_steps=self.cg_steps, return_tensor=return_tensor, device=device)

    def recommend(self, histories, k=10, *, window=None, return_tensor=False, device=None):
        """For every user of ``histories`` the ``k`` unseen articles with the largest inner product of ``user_states(histories)``
        and the article factors: ``helpers.recommend(user_states, item_factors, k, seen=histories)``.  ``window`` as there."""
        from .evaluation import recommend
        states = self.user_states(histories, return_tensor=True, device=device)
        return recommend(states, self.item_factors, k, seen=histories, window=window, return_tensor=return_tensor, device=device)

    def similar(self, items, k=10, *, return_tensor=False, device=None):
        """The ``k`` articles nearest to each of ``items`` by the cosine of the article factors (``most_similar``; the article
        itself is not returned): ``(indices, scores)``."""
        from .sweeps import most_similar
        rows = np.asarray(items, dtype=np.int64).ravel()
        if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= self.n_articles):
            raise ValueError(f"items must be in 0..{self.n_articles - 1}")
        Y = self.item_factors
        if hasattr(Y, "detach"):
            import torch
            Q = Y[torch.from_numpy(rows).to(Y.device)]
        else:
            Q = Y[rows]
        return most_similar(Q, k, "", "cosine", exclude_self=False, candidates=Y, exclude=[[int(r)] for r in rows],
                            return_tensor=return_tensor, device=device)

    def save(self, path):
        """The model as one ``.npz``."""
        np.savez(path, user_factors=_host(self.user_factors), item_factors=_host(self.item_factors),
                 loss_curve=np.asarray(self.loss_curve, dtype=np.float64),
                 **{n: np.float64(getattr(self, n)) for n in self._SCALARS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["user_factors"], z["item_factors"], int(z["factors"]), float(z["regularization"]), float(z["alpha"]),
                       int(z["cg_steps"]), int(z["iterations"]), z["loss_curve"].tolist())


def fit_als(histories, n_articles, *, factors=64, regularization=0.01, alpha=40.0, iterations=15, cg_steps=3, seed=0, init=None,
            compute_loss=False, return_tensor=False, device=None):
    """Implicit-feedback ALS of a click log on the device.  ``histories``: a list of index sequences or an ``(indptr, items)``
    tuple over ``n_articles`` articles; a user's clicks on one article add up to the count ``r``, the confidence is
    ``1 + alpha * r``.  The article factors start as ``0.01 * N(0, 1)`` from ``np.random.default_rng(seed)`` (or as ``init``
    ``[n_articles x factors]``), the user factors at 0; every iteration is Gram, user half-sweep, Gram, article half-sweep, each
    half-sweep ``cg_steps`` steps of conjugate gradient per row from the row's current factor.  ``compute_loss=True`` records the
    objective after every half-sweep in ``loss_curve``.  ``regularization`` and ``alpha`` are used as float32 numbers.  Returns an
    ``ALSModel``; the result is bit-identical from run to run, whatever the order of the users."""
    F, lam, alpha, cg_steps = _settings(factors, regularization, alpha, cg_steps)
    Na, iterations = int(n_articles), int(iterations)
    if iterations < 0:
        raise ValueError(f"iterations must not be negative (got {iterations})")
    if Na < 1:
        raise ValueError(f"n_articles must be at least 1 (got {n_articles})")
    if init is not None and tuple(getattr(init, "shape", np.shape(init))) != (Na, F):
        raise ValueError(f"init must be [{Na} x {F}] (got {tuple(getattr(init, 'shape', np.shape(init)))})")
    history_csr(histories, Na)                                          # the ValueErrors of the log, before the device
    inter = als_interactions(histories, Na, return_tensor=True, device=device)
    torch, lib, dev = device_and_library(device)
    M = inter.n_users
    if init is None:
        Y = torch.from_numpy((0.01 * np.random.default_rng(seed).standard_normal((Na, F))).astype(np.float32)).to(dev)
    else:
        Y = _f32_on_device(torch, dev, init).clone().contiguous()
    X = torch.zeros((max(M, 1), F), dtype=torch.float32, device=dev)[:M]
    kw = dict(regularization=lam, alpha=alpha, cg_steps=cg_steps, return_tensor=True, device=dev)
    curve = []
    for _ in range(iterations if M > 0 else 0):
        als_solve_rows(*inter.user, Y, X, **kw)
        if compute_loss:
            curve.append(als_loss(*inter.user, X, Y, regularization=lam, alpha=alpha, device=dev))
        als_solve_rows(*inter.item, X, Y, **kw)
        if compute_loss:
            curve.append(als_loss(*inter.user, X, Y, regularization=lam, alpha=alpha, device=dev))
    return ALSModel(result(X, return_tensor), result(Y, return_tensor), F, lam, alpha, cg_steps, iterations, curve)
