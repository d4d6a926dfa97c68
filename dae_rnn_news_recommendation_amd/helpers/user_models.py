"""The user models of "Embedding-based News Recommendation for Millions of Users" (KDD'17) on article embeddings.  The decaying
model: ``user_states`` (``decay_factors``), and its trained form ``fit_user_model`` -> ``UserModel`` on the loss and gradients of
``user_pair_loss`` (``sample_negatives``, ``decay_factor_derivatives``).  The recurrent model: ``GRUUserModel`` (weights in the
layout of ``torch.nn.GRU``), ``gru_user_states`` (``gru_schedule``, ``trim_histories``), and its training ``fit_gru_user_model`` on
``gru_pair_loss`` (back-propagation through time on the device).  The paper's other two recurrent cells, in the same
three parts: ``LSTMUserModel`` / ``lstm_user_states`` / ``fit_lstm_user_model`` on ``lstm_pair_loss`` and ``RNNUserModel`` /
``rnn_user_states`` / ``fit_rnn_user_model`` on ``rnn_pair_loss``."""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ._device import (check_item_kind, check_item_range, csr_lists, device_and_library, device_matrix, event_times, history_csr,
                      matrix_shape, result, upload, workspace)
from .sweeps import normalize_window


def decay_factors(indptr, timestamps, beta, time_unit=None):
    """Per-event decay factors of ``user_states`` from event times: ``beta ** ((t_e - t_{e-1}) / time_unit)`` for every event but a
    user's first (whose factor is ignored; 1 is written), computed in float64 and rounded once to float32.  ``timestamps`` has
    the layout of the items (one per event); within a user they must not decrease (``ValueError``).  ``time_unit`` defaults to
    1 and must be positive.  Host code."""
    indptr = np.asarray(indptr, dtype=np.int64)
    t = np.asarray(timestamps, dtype=np.float64).ravel()
    if t.size != int(indptr[-1]):
        raise ValueError(f"{t.size} timestamps for {int(indptr[-1])} events")
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta must be in [0, 1] (got {beta})")
    unit = 1.0 if time_unit is None else float(time_unit)
    if not (unit > 0.0 and np.isfinite(unit)):
        raise ValueError(f"time_unit must be positive and finite (got {time_unit})")
    if not np.isfinite(t).all():
        raise ValueError("timestamps must be finite")
    dt = np.zeros(t.size, dtype=np.float64)
    dt[1:] = t[1:] - t[:-1]
    first = indptr[:-1][np.diff(indptr) > 0]
    dt[first] = 0.0
    if (dt < 0).any():
        e = int(np.flatnonzero(dt < 0)[0])
        raise ValueError(f"timestamps decrease within a user (event {e}, user {int(np.searchsorted(indptr, e, side='right') - 1)})")
    with np.errstate(divide="ignore"):
        return np.power(beta, dt / unit).astype(np.float32)              # 0 ** 0 = 1: simultaneous events do not decay


def user_states(histories, embeddings, beta=0.9, *, timestamps=None, time_unit=None, all_states=False, return_tensor=False,
                device=None):
    """User states from browsing histories by the decaying model of "Embedding-based News Recommendation for Millions of Users"
    (KDD'17): per user, over the events oldest first, ``s = d * s + E[item]``, ``z = d * z + 1``, state = ``s / z`` -- a
    decay-weighted mean of the embeddings of the articles read, newest weighted most (``dae_user_states``, fp32, fixed order:
    bit-identical run to run and independent of the order of the users).

    ``histories``: a list of index sequences (one per user, oldest click first; an article may repeat) or an ``(indptr, items)``
    tuple.  ``embeddings`` [articles x H] takes the containers of ``most_similar``.  ``d`` is ``beta`` in [0, 1] for every event,
    or, with ``timestamps`` (same layout as the items), ``beta ** ((t_e - t_{e-1}) / time_unit)`` (``decay_factors``; a
    ``ValueError`` when a user's timestamps decrease).  An item outside ``[0, articles)`` raises ``ValueError``.

    Returns float32 ``[users x H]``: the state after each user's last event (zeros for an empty history); with
    ``all_states=True`` ``[events x H]``: row e is the state after event e, the one that predicts event e + 1 -- and the row of
    a user's last event equals that user's row of the default form bit for bit.  ndarray, or a CUDA tensor with
    ``return_tensor=True``."""
    indptr, items = history_csr(histories)
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta must be in [0, 1] (got {beta})")
    decay = None if timestamps is None else decay_factors(indptr, event_times(timestamps), beta, time_unit)
    torch, _, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev, in_place=True)          # a strided view is read in place
    Na, H = int(E.shape[0]), int(E.shape[1])
    check_item_range(items, Na)
    M, nnz = int(indptr.size - 1), int(items.size)
    rows = nnz if all_states else M
    U = torch.empty((rows, H), dtype=torch.float32, device=dev)
    if rows == 0 or H == 0:
        return result(U, return_tensor)
    ip_d, it_d, dc_d = torch.from_numpy(indptr).to(dev), upload(items.astype(np.int32), dev), upload(decay, dev)
    with torch.cuda.device(dev):
        L.call("dae_user_states", L.ptr(E), E.stride(0), Na, H, L.ptr(ip_d), L.ptr(it_d), M, nnz, beta, L.ptr(dc_d),
               1 if all_states else 0, L.ptr(U), U.stride(0), L.current_stream())
    return result(U, return_tensor)


class GRUUserModel:
    """The weights of the GRU user model, float32 in the layout of ``torch.nn.GRU`` (one layer, gate row blocks r, z, n):
    ``weight_ih`` [3H x D], ``weight_hh`` [3H x H], ``bias_ih`` and ``bias_hh`` [3H].  ``save`` / ``load`` keep them in an ``.npz``
    under those four names -- the hand-over format of any trainer (``fit_gru_user_model`` returns one, with the loss per pair of
    every epoch in ``.history``, which is not saved; ``tools/gru_fit_torch.py`` writes the file too).  Host code; the states come
    from ``gru_user_states`` (or ``.states``)."""
    NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")

    def __init__(self, weight_ih, weight_hh, bias_ih, bias_hh, history=None, validation=None):
        self.history = history                                              # a trainer's loss per pair of every epoch; not saved
        self.validation = validation                                        # and its validation metrics (fit_gru_user_model); not saved
        w = [np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in (weight_ih, weight_hh, bias_ih, bias_hh)]
        self.weight_ih, self.weight_hh, self.bias_ih, self.bias_hh = w
        if self.weight_hh.ndim != 2 or self.weight_hh.shape[0] != 3 * self.weight_hh.shape[1] or self.weight_hh.shape[1] < 1:
            raise ValueError(f"weight_hh must be [3H x H] (got {self.weight_hh.shape})")
        H = int(self.weight_hh.shape[1])
        if self.weight_ih.ndim != 2 or self.weight_ih.shape[0] != 3 * H or self.weight_ih.shape[1] < 1:
            raise ValueError(f"weight_ih must be [3H x D] with H = {H} (got {self.weight_ih.shape})")
        if self.bias_ih.shape != (3 * H,) or self.bias_hh.shape != (3 * H,):
            raise ValueError(f"bias_ih and bias_hh must be [3H] with H = {H} (got {self.bias_ih.shape}, {self.bias_hh.shape})")
        if not all(np.isfinite(a).all() for a in w):
            raise ValueError("GRU weights must be finite")

    @property
    def hidden_size(self):
        return int(self.weight_hh.shape[1])

    @property
    def input_size(self):
        return int(self.weight_ih.shape[1])

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, **{n: getattr(self, n) for n in self.NAMES})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            missing = [n for n in cls.NAMES if n not in z.files]
            if missing:
                raise ValueError(f"{path}: no array named {missing[0]} (a GRU weight file holds {', '.join(cls.NAMES)})")
            return cls(*(z[n] for n in cls.NAMES))

    @classmethod
    def from_torch(cls, x):
        """From a ``torch.nn.GRU`` (one layer, unidirectional, with bias) or its state dict."""
        if hasattr(x, "state_dict"):
            if getattr(x, "num_layers", 1) != 1 or getattr(x, "bidirectional", False) or not getattr(x, "bias", True):
                raise ValueError("from_torch takes a one-layer, unidirectional GRU with bias")
            if type(x).__name__ != "GRU":
                raise ValueError(f"from_torch takes a torch.nn.GRU (got {type(x).__name__})")
            x = x.state_dict()
        keys = [n + "_l0" for n in cls.NAMES]
        extra = [k for k in x if k not in keys]
        if extra or any(k not in x for k in keys):
            raise ValueError(f"a one-layer, unidirectional GRU with bias has the entries {keys} (got {sorted(x)})")
        return cls(*(x[k].detach().cpu().numpy() if hasattr(x[k], "detach") else x[k] for k in keys))

    def states(self, histories, embeddings, **kw):
        return gru_user_states(histories, embeddings, self, **kw)


def gru_schedule(indptr):
    """The time-major schedule ``dae_gru_user_states`` runs: ``(order int32 [users], active int64 [T])``.  ``order`` lists the
    users by history length, longest first -- a stable sort, so equal lengths keep the input order; ``active[t]`` is the number
    of users with more than t events (non-increasing; T = the longest history, 0 without events).  Host code."""
    indptr = np.asarray(indptr, dtype=np.int64).ravel()
    if indptr.size < 1 or (np.diff(indptr) < 0).any():
        raise ValueError("indptr must be non-decreasing and hold at least one entry")
    n = np.diff(indptr)
    order = np.argsort(-n, kind="stable").astype(np.int32)
    T = int(n.max()) if n.size else 0
    active = n.size - np.cumsum(np.bincount(n, minlength=T + 1))[:T]
    return order, np.ascontiguousarray(active.astype(np.int64))


def trim_histories(histories, max_events):
    """Every user's ``max_events`` most recent events as an ``(indptr, items)`` tuple (the order within a user is kept).  Host code."""
    indptr, items = csr_lists(histories)
    k = int(max_events)
    if k < 0:
        raise ValueError(f"max_events must not be negative (got {max_events})")
    n = np.minimum(np.diff(indptr), k)
    out = np.zeros(indptr.size, dtype=np.int64)
    out[1:] = np.cumsum(n)
    start = indptr[1:] - n                                              # first kept event of every user
    pos = np.repeat(start - out[:-1], n) + np.arange(int(out[-1]), dtype=np.int64)
    return out, items[pos]


def _recurrent_user_states(cell, cls, histories, embeddings, model, initial, max_events, all_states, batch_users, return_tensor, device,
                           return_cell=False):
    """The intake, chunk loop and schedule shared by ``gru_user_states``, ``lstm_user_states`` and ``rnn_user_states``:
    ``dae_{cell}_user_states`` on the weights of ``model`` (a ``cls``).  ``initial``: a tuple of start states, ``(h,)`` or, for the
    LSTM, ``(h, c)``, each ``[users x H]`` or None.  Returns ``(U, C)``; ``C`` (LSTM with ``return_cell``) is the cell state after
    every user's last event, else None."""
    import torch
    if not isinstance(model, cls):
        raise TypeError(f"model must be a {cls.__name__} ({cls.__name__}.load / from_torch)")
    if max_events is not None and all_states:
        raise ValueError("max_events and all_states do not go together: the rows of all_states are the caller's events")
    if int(batch_users) < 1:
        raise ValueError(f"batch_users must be positive (got {batch_users})")
    indptr, items = history_csr(histories)
    if max_events is not None:
        indptr, items = trim_histories((indptr, items), max_events)
    H, D = model.hidden_size, model.input_size
    M, nnz = int(indptr.size - 1), int(items.size)

    def check_embeddings(shape):
        if int(shape[1]) != D:
            raise ValueError(f"embeddings have {int(shape[1])} columns, the model's weight_ih has {D}")
        check_item_range(items, int(shape[0]))
    if not isinstance(embeddings, torch.Tensor):                        # a host container: refused before any device work
        check_embeddings(matrix_shape(embeddings))
    initial = list(initial)
    for k, name in enumerate(("initial", "initial c")[:len(initial)]):
        if initial[k] is not None and not isinstance(initial[k], torch.Tensor):
            initial[k] = np.asarray(initial[k], dtype=np.float32)
        if initial[k] is not None and tuple(initial[k].shape) != (M, H):
            raise ValueError(f"{name} must be [users x H] = [{M} x {H}] (got {tuple(initial[k].shape)})")
    _, lib, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev, in_place=True)
    Na = int(E.shape[0])
    check_embeddings(E.shape)
    rows = nnz if all_states else M
    U = torch.empty((rows, H), dtype=torch.float32, device=dev)

    def on_device(x):
        return (x.to(device=dev, dtype=torch.float32) if isinstance(x, torch.Tensor) else torch.as_tensor(x).to(dev)).contiguous()
    if rows == 0:                                                       # no row of U; C is the initial c, or zeros
        C = None
        if return_cell:
            C = on_device(initial[1]).clone() if initial[1] is not None else torch.zeros((M, H), dtype=torch.float32, device=dev)
        return result(U, return_tensor), (None if C is None else result(C, return_tensor))
    if Na == 0:
        raise ValueError("embeddings hold no articles")
    start = [None if x is None else on_device(x) for x in initial]
    C = torch.empty((M, H), dtype=torch.float32, device=dev) if return_cell else None     # every row is written: last step, or the init kernel
    w = [torch.from_numpy(getattr(model, n)).to(dev) for n in cls.NAMES]
    it_d = upload(items.astype(np.int32), dev)
    chunk = min(int(batch_users), M)
    ws_bytes = int(getattr(lib, f"dae_{cell}_user_states_workspace")(Na, D, H, chunk))
    ws_ptr, ws = workspace(dev, ws_bytes)
    import ctypes
    with torch.cuda.device(dev):
        for c0 in range(0, M, chunk):
            c1 = min(c0 + chunk, M)
            e0, e1 = int(indptr[c0]), int(indptr[c1])
            ip = np.ascontiguousarray(indptr[c0:c1 + 1] - e0)
            order, active = gru_schedule(ip)
            ip_d, or_d = torch.from_numpy(ip).to(dev), torch.from_numpy(order).to(dev)
            Uc = U[e0:e1] if all_states else U[c0:c1]
            first = []                                                  # (h0, ldh0) and, for the LSTM, (c0, ldc0)
            for x in start:
                first += [L.ptr(None if x is None else x[c0:c1]), H]
            out = [ctypes.c_void_p(Uc.data_ptr()), U.stride(0)]         # (U, ldu) and, for the LSTM, (C, ldc)
            if cell == "lstm":
                out += [None if C is None else ctypes.c_void_p(C[c0:c1].data_ptr()), H]
            L.call(f"dae_{cell}_user_states", L.ptr(E), E.stride(0), Na, D, H, L.ptr(w[0]), D, L.ptr(w[1]), H, L.ptr(w[2]), L.ptr(w[3]),
                   L.ptr(ip_d), ctypes.c_void_p(it_d.data_ptr() + 4 * e0), L.ptr(or_d), c1 - c0, e1 - e0, int(active.size),
                   active.ctypes.data_as(ctypes.c_void_p), *first, 1 if all_states else 0, *out, ws_ptr, ws_bytes, L.current_stream())
    del ws
    return result(U, return_tensor), (None if C is None else result(C, return_tensor))


def gru_user_states(histories, embeddings, model, *, initial=None, max_events=None, all_states=False, batch_users=262144,
                    return_tensor=False, device=None):
    """User states from browsing histories by the recurrent (GRU) user model of "Embedding-based News Recommendation for Millions
    of Users" (KDD'17): per user, over the events oldest first, with ``x = E[item]`` and the weights of ``model`` (a
    ``GRUUserModel``; gate order and "reset-after" form of ``torch.nn.GRU``)

        r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)   z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
        n = tanh(W_in x + b_in + r * (W_hn h + b_hn))   h' = (1 - z) * n + z * h

    (``dae_gru_user_states``: time-major, one exact-fp32 MFMA GEMM launch per step over the users still active; fixed order, no
    atomics: bit-identical run to run and independent of the other users of the call and of their order).

    ``histories`` and ``embeddings`` [articles x D] as for ``user_states``; ``model.input_size`` must be D.  The states have
    ``H = model.hidden_size`` columns (``recommend`` needs H = D).  ``h`` starts at zero, or at the rows of ``initial``
    [users x H]: the states of an earlier call, continued with the new clicks without replaying the history.  ``max_events``
    keeps every user's most recent events (trimmed on the host; with ``all_states`` a ``ValueError``: the rows would no longer
    be the caller's events).  The users are processed in chunks of at most ``batch_users``, which bounds the workspace; the
    chunking does not change a bit of the result.  An item outside ``[0, articles)`` raises ``ValueError``.

    Returns float32 ``[users x H]``: the state after each user's last event (zeros, or the ``initial`` row, for an empty
    history); with ``all_states=True`` ``[events x H]``: row e is the state after event e, the one that predicts event e + 1,
    and the row of a user's last event equals that user's row of the default form bit for bit."""
    return _recurrent_user_states("gru", GRUUserModel, histories, embeddings, model, (initial,), max_events, all_states, batch_users,
                                  return_tensor, device)[0]


class _TorchCellUserModel:
    """What ``LSTMUserModel`` and ``RNNUserModel`` share: float32 weights in the layout of the ``torch.nn`` module ``MODULE`` (one
    layer, unidirectional, with bias; ``GATES`` row blocks of H rows), ``save`` / ``load`` in an ``.npz`` under the four ``NAMES``,
    ``from_torch``.  Host code."""
    NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    GATES, MODULE = 0, ""

    def __init__(self, weight_ih, weight_hh, bias_ih, bias_hh, history=None, validation=None):
        self.history = history                                              # a trainer's loss per pair of every epoch; not saved
        self.validation = validation                                        # and its validation metrics; not saved
        G, rows = self.GATES, ("%dH" % self.GATES if self.GATES > 1 else "H")
        w = [np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in (weight_ih, weight_hh, bias_ih, bias_hh)]
        self.weight_ih, self.weight_hh, self.bias_ih, self.bias_hh = w
        if self.weight_hh.ndim != 2 or self.weight_hh.shape[0] != G * self.weight_hh.shape[1] or self.weight_hh.shape[1] < 1:
            raise ValueError(f"weight_hh of an {self.MODULE} must be [{rows} x H] (got {self.weight_hh.shape})")
        H = int(self.weight_hh.shape[1])
        if self.weight_ih.ndim != 2 or self.weight_ih.shape[0] != G * H or self.weight_ih.shape[1] < 1:
            raise ValueError(f"weight_ih must be [{rows} x D] with H = {H} (got {self.weight_ih.shape})")
        if self.bias_ih.shape != (G * H,) or self.bias_hh.shape != (G * H,):
            raise ValueError(f"bias_ih and bias_hh must be [{rows}] with H = {H} (got {self.bias_ih.shape}, {self.bias_hh.shape})")
        if not all(np.isfinite(a).all() for a in w):
            raise ValueError(f"{self.MODULE} weights must be finite")

    @property
    def hidden_size(self):
        return int(self.weight_hh.shape[1])

    @property
    def input_size(self):
        return int(self.weight_ih.shape[1])

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, **{n: getattr(self, n) for n in self.NAMES})

    @classmethod
    def load(cls, path):
        """From an ``.npz`` of the four arrays.  The row multiple of ``weight_hh`` tells the cells apart: a file of another cell
        (a GRU file handed to ``LSTMUserModel``, say) is a ``ValueError``."""
        with np.load(path) as z:
            missing = [n for n in cls.NAMES if n not in z.files]
            if missing:
                raise ValueError(f"{path}: no array named {missing[0]} (an {cls.MODULE} weight file holds {', '.join(cls.NAMES)})")
            return cls(*(z[n] for n in cls.NAMES))

    @classmethod
    def from_torch(cls, x):
        """From the ``torch.nn`` module of the cell (one layer, unidirectional, with bias, no projection, tanh) or its state dict."""
        if hasattr(x, "state_dict"):
            if type(x).__name__ != cls.MODULE:
                raise ValueError(f"from_torch takes a torch.nn.{cls.MODULE} (got {type(x).__name__})")
            if getattr(x, "num_layers", 1) != 1 or getattr(x, "bidirectional", False) or not getattr(x, "bias", True):
                raise ValueError(f"from_torch takes a one-layer, unidirectional {cls.MODULE} with bias")
            if getattr(x, "proj_size", 0) != 0:
                raise ValueError(f"from_torch takes an {cls.MODULE} without projection (proj_size = {x.proj_size})")
            if getattr(x, "nonlinearity", "tanh") != "tanh":
                raise ValueError(f"from_torch takes an {cls.MODULE} with nonlinearity='tanh' (got {x.nonlinearity!r})")
            x = x.state_dict()
        keys = [n + "_l0" for n in cls.NAMES]
        extra = [k for k in x if k not in keys]
        if extra or any(k not in x for k in keys):
            raise ValueError(f"a one-layer, unidirectional {cls.MODULE} with bias has the entries {keys} (got {sorted(x)})")
        return cls(*(x[k].detach().cpu().numpy() if hasattr(x[k], "detach") else x[k] for k in keys))


class LSTMUserModel(_TorchCellUserModel):
    """The weights of the LSTM user model, float32 in the layout of ``torch.nn.LSTM`` (one layer, gate row blocks i, f, g, o):
    ``weight_ih`` [4H x D], ``weight_hh`` [4H x H], ``bias_ih`` and ``bias_hh`` [4H].  ``save`` / ``load`` keep them in an ``.npz`` under
    those four names (``fit_lstm_user_model`` returns one, with ``.history`` and ``.validation``, which are not saved;
    ``tools/gru_fit_torch.py --cell lstm`` writes the file too).  Host code; the states come from ``lstm_user_states`` (or ``.states``)."""
    GATES, MODULE = 4, "LSTM"

    def states(self, histories, embeddings, **kw):
        return lstm_user_states(histories, embeddings, self, **kw)


class RNNUserModel(_TorchCellUserModel):
    """The weights of the plain-RNN user model, float32 in the layout of ``torch.nn.RNN(nonlinearity='tanh')`` (one layer):
    ``weight_ih`` [H x D], ``weight_hh`` [H x H], ``bias_ih`` and ``bias_hh`` [H].  ``save`` / ``load`` keep them in an ``.npz`` under
    those four names (``fit_rnn_user_model`` returns one, with ``.history`` and ``.validation``, which are not saved;
    ``tools/gru_fit_torch.py --cell rnn`` writes the file too).  Host code; the states come from ``rnn_user_states`` (or ``.states``)."""
    GATES, MODULE = 1, "RNN"

    def states(self, histories, embeddings, **kw):
        return rnn_user_states(histories, embeddings, self, **kw)


def rnn_user_states(histories, embeddings, model, *, initial=None, max_events=None, all_states=False, batch_users=262144,
                    return_tensor=False, device=None):
    """User states from browsing histories by the plain recurrent user model of "Embedding-based News Recommendation for Millions
    of Users" (KDD'17): per user, over the events oldest first, with ``x = E[item]`` and the weights of ``model`` (an
    ``RNNUserModel``; the form of ``torch.nn.RNN(nonlinearity='tanh')``)

        h' = tanh(W_ih x + b_ih + W_hh h + b_hh)

    (``dae_rnn_user_states``: time-major, one exact-fp32 MFMA GEMM launch per step over the users still active; fixed order, no
    atomics: bit-identical run to run and independent of the other users of the call and of their order).

    ``histories`` and ``embeddings`` [articles x D] as for ``user_states``; ``model.input_size`` must be D.  The states have
    ``H = model.hidden_size`` columns (``recommend`` needs H = D).  ``h`` starts at zero, or at the rows of ``initial``
    [users x H]: the states of an earlier call, continued with the new clicks without replaying the history.  ``max_events``
    keeps every user's most recent events (trimmed on the host; with ``all_states`` a ``ValueError``: the rows would no longer
    be the caller's events).  The users are processed in chunks of at most ``batch_users``, which bounds the workspace; the
    chunking does not change a bit of the result.  An item outside ``[0, articles)`` raises ``ValueError``.

    Returns float32 ``[users x H]``: the state after each user's last event (zeros, or the ``initial`` row, for an empty
    history); with ``all_states=True`` ``[events x H]``: row e is the state after event e, the one that predicts event e + 1,
    and the row of a user's last event equals that user's row of the default form bit for bit."""
    return _recurrent_user_states("rnn", RNNUserModel, histories, embeddings, model, (initial,), max_events, all_states, batch_users,
                                  return_tensor, device)[0]


def lstm_user_states(histories, embeddings, model, *, initial=None, max_events=None, all_states=False, batch_users=262144,
                     return_tensor=False, return_cell=False, device=None):
    """User states from browsing histories by the LSTM user model of "Embedding-based News Recommendation for Millions of Users"
    (KDD'17): per user, over the events oldest first, with ``x = E[item]`` and the weights of ``model`` (an ``LSTMUserModel``;
    gate order of ``torch.nn.LSTM``)

        i = sigmoid(W_ii x + b_ii + W_hi h + b_hi)   f = sigmoid(W_if x + b_if + W_hf h + b_hf)   o = sigmoid(W_io x + b_io + W_ho h + b_ho)
        g = tanh(W_ig x + b_ig + W_hg h + b_hg)   c' = f * c + i * g   h' = o * tanh(c')

    (``dae_lstm_user_states``: time-major, one launch per step over the users still active, the exact-fp32 MFMA K loop once per
    gate; fixed order, no atomics: bit-identical run to run and independent of the other users of the call and of their order).

    The contract of ``gru_user_states`` -- ``histories``, ``embeddings`` [articles x D], ``max_events``, ``all_states``,
    ``batch_users``, ``return_tensor``, the errors and the returned ``[users x H]`` / ``[events x H]`` states ``h`` -- with two
    additions.  ``initial`` is a pair ``(h, c)`` of ``[users x H]`` start states, either of which may be None (zeros).
    ``return_cell=True`` returns ``(U, C)``: ``C`` float32 ``[users x H]`` is every user's cell state after their last event (the
    ``c`` row of ``initial``, or zeros, for an empty history), whatever ``all_states``.  The last states and ``C`` of one call,
    handed to the next as ``initial=(U, C)``, continue the histories to the bits of the unsplit run."""
    if initial is None:
        initial = (None, None)
    if not isinstance(initial, (tuple, list)) or len(initial) != 2:
        raise ValueError("initial must be a pair (h, c); either may be None")
    U, C = _recurrent_user_states("lstm", LSTMUserModel, histories, embeddings, model, tuple(initial), max_events, all_states, batch_users,
                                  return_tensor, device, return_cell=bool(return_cell))
    return (U, C) if return_cell else U


def decay_factor_derivatives(indptr, timestamps, beta, time_unit=None):
    """The derivative of ``decay_factors`` with respect to ``beta``: ``(dt / time_unit) * beta ** (dt / time_unit - 1)`` per event,
    computed in float64 and rounded once to float32; 0 where ``dt = 0`` (simultaneous events do not decay, whatever beta) and at
    a user's first event (whose factor is ignored).  Same arguments and errors as ``decay_factors``, but ``0 < beta <= 1``.
    Host code."""
    beta = float(beta)
    if not 0.0 < beta <= 1.0:
        raise ValueError(f"beta must be in (0, 1] (got {beta})")
    decay_factors(indptr, timestamps, beta, time_unit)                     # the argument checks
    indptr = np.asarray(indptr, dtype=np.int64)
    t = np.asarray(timestamps, dtype=np.float64).ravel()
    unit = 1.0 if time_unit is None else float(time_unit)
    dt = np.zeros(t.size, dtype=np.float64)
    dt[1:] = t[1:] - t[:-1]
    dt[indptr[:-1][np.diff(indptr) > 0]] = 0.0
    p = dt / unit
    return np.where(p > 0.0, p * np.power(beta, p - 1.0), 0.0).astype(np.float32)


def sample_negatives(indptr, items, n_articles, n_neg, seed, *, window=None):
    """Sampled negatives for ``user_pair_loss``: ``int32 [events x n_neg]``, drawn uniformly over ``[0, n_articles)`` or, with
    ``window = (lo, hi)`` (one entry per EVENT), over the event's ``[lo, hi)``.  -1 ("no pair") is written where the draw equals
    the event's own article, where the window is empty, and at every user's first event, which has no state to predict from.
    Articles the user has read are NOT removed: a uniform negative is seen with small probability, and the standard form of
    this loss (BPR) samples that way.  Seeded (``numpy.random.default_rng(seed)``) and reproducible.  Host code."""
    indptr = np.asarray(indptr, dtype=np.int64)
    items = np.asarray(items).ravel()
    nnz, n_neg, Na = int(items.size), int(n_neg), int(n_articles)
    if indptr.size < 1 or int(indptr[-1]) != nnz:
        raise ValueError(f"indptr ends at {int(indptr[-1]) if indptr.size else None} for {nnz} events")
    if n_neg < 1:
        raise ValueError(f"n_neg must be positive (got {n_neg})")
    if Na < 1:
        raise ValueError(f"n_articles must be positive (got {Na})")
    if window is None:
        lo, hi = np.zeros(nnz, dtype=np.int64), np.full(nnz, Na, dtype=np.int64)
    else:
        lo, hi = (w.astype(np.int64) for w in normalize_window(window, nnz, Na))
    u = np.random.default_rng(seed).random((nnz, n_neg))
    width = (hi - lo)[:, None]
    neg = lo[:, None] + np.minimum((u * width).astype(np.int64), np.maximum(width - 1, 0))
    bad = (neg == items.astype(np.int64)[:, None]) | (width <= 0)
    bad[indptr[:-1][np.diff(indptr) > 0]] = True
    return np.ascontiguousarray(np.where(bad, -1, neg).astype(np.int32))


def _pair_loss_call(torch, E, ip_d, it_d, ng_d, M, nnz, n_neg, alpha, beta, dc_d=None, dd_d=None, margins=False):
    """One ``dae_user_pair_loss`` on device operands: ``ip_d`` int64 [M + 1] starting at 0, ``it_d`` int32 / ``ng_d`` int32
    [nnz x n_neg] / ``dc_d`` / ``dd_d`` float32 views of the batch's events.  Returns the result dict of ``user_pair_loss``."""
    dev = E.device
    Na, H = int(E.shape[0]), int(E.shape[1])
    lib = L.load()
    al_d = torch.from_numpy(np.ascontiguousarray(np.asarray(alpha, dtype=np.float32))).to(dev)
    out = torch.zeros(H + 3, dtype=torch.float64, device=dev)               # dalpha [H], loss, dbeta, n_pairs (int64 bits)
    mg = torch.empty((max(nnz, 1), n_neg), dtype=torch.float32, device=dev) if margins else None
    with torch.cuda.device(dev):
        ws_bytes = int(lib.dae_user_pair_loss_workspace(M, H))
        ws_ptr, ws = workspace(dev, ws_bytes)
        base = out.data_ptr()
        import ctypes
        L.call("dae_user_pair_loss", L.ptr(E), E.stride(0), Na, H, L.ptr(ip_d), L.ptr(it_d), M, nnz, float(beta), L.ptr(dc_d),
               L.ptr(dd_d), L.ptr(al_d), L.ptr(ng_d), n_neg, ctypes.c_void_p(base + 8 * H), ctypes.c_void_p(base),
               ctypes.c_void_p(base + 8 * (H + 1)), ctypes.c_void_p(base + 8 * (H + 2)), L.ptr(mg), ws_ptr, ws_bytes,
               L.current_stream())
        host = out.cpu().numpy()                                           # synchronises: the workspace may go after this
    res = {"loss": float(host[H]), "dalpha": host[:H].copy(), "dbeta": float(host[H + 1]), "n_pairs": int(host[H + 2:].view(np.int64)[0])}
    if margins:
        res["margins"] = mg[:nnz].cpu().numpy()
    return res


def _check_negatives(negatives, nnz, Na):
    neg = np.asarray(negatives)
    if neg.ndim != 2 or neg.shape[0] != nnz or not 1 <= neg.shape[1] <= 16:
        raise ValueError(f"negatives must be [{nnz} events x n_neg] with 1 <= n_neg <= 16 (got {tuple(neg.shape)})")
    check_item_kind(neg, "negatives")
    if neg.size and int(neg.max()) >= Na:
        raise ValueError(f"negatives must be below {Na}, or negative for no pair (got {int(neg.max())})")
    return np.ascontiguousarray(np.maximum(neg, -1).astype(np.int32))


def user_pair_loss(histories, embeddings, alpha, beta, negatives, *, timestamps=None, time_unit=None, return_margins=False,
                   device=None):
    """Pairwise ranking loss of the trained decay model of "Embedding-based News Recommendation for Millions of Users" (KDD'17) and
    its gradients, in one walk of every history (``dae_user_pair_loss``): with the state ``u = s / z`` of ``user_states`` BEFORE a
    click, relevance ``R(u, a) = (alpha * u) . a`` and margin ``x = R(u, clicked) - R(u, negative)``, the loss is the sum of
    ``softplus(-x)`` over all valid (click, negative) pairs.  Neither the [events x H] matrix of states nor its derivative is
    stored.

    ``histories``, ``embeddings``, ``beta``, ``timestamps``, ``time_unit``: as ``user_states`` (with timestamps the per-event factor
    is ``beta ** (dt / time_unit)`` and its derivative ``decay_factor_derivatives``; at ``beta = 0`` the factors are 0 or 1 -- session
    resets -- and ``dbeta`` comes out 0).  ``alpha``: one
    weight per embedding dimension.  ``negatives``: integer ``[events x n_neg]``, ``n_neg`` in 1..16, e.g. from ``sample_negatives``;
    a negative entry, the click itself and every entry of a user's first click are no pair.  An entry >= the number of articles
    raises ``ValueError``.

    Returns ``{'loss': float, 'dalpha': float64 [H], 'dbeta': float, 'n_pairs': int}`` -- sums over the valid pairs, NOT divided by
    ``n_pairs`` -- and with ``return_margins=True`` also ``'margins'``: float32 ``[events x n_neg]``, 0 where there is no pair.
    Bit-identical run to run; ``n_pairs`` and the margins do not depend on the order of the users."""
    indptr, items = history_csr(histories)
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta must be in [0, 1] (got {beta})")
    decay = ddecay = None
    if timestamps is not None:
        t = event_times(timestamps)
        decay = decay_factors(indptr, t, beta, time_unit)
        ddecay = decay_factor_derivatives(indptr, t, beta, time_unit) if beta > 0.0 else None      # beta = 0: factors in {0, 1}, dbeta = 0
    torch, _, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev, in_place=True)
    Na, H = int(E.shape[0]), int(E.shape[1])
    alpha = np.asarray(alpha, dtype=np.float64).ravel()
    if alpha.size != H:
        raise ValueError(f"alpha has {alpha.size} entries for {H} embedding dimensions")
    if not 1 <= H <= 1024:
        raise ValueError(f"the embedding dimension must be in 1..1024 (got {H})")
    check_item_range(items, Na)
    M, nnz = int(indptr.size - 1), int(items.size)
    neg = _check_negatives(negatives, nnz, Na)
    return _pair_loss_call(torch, E, torch.from_numpy(indptr).to(dev), upload(items.astype(np.int32), dev), upload(neg, dev), M, nnz,
                           int(neg.shape[1]), alpha, beta, upload(decay, dev), upload(ddecay, dev), margins=return_margins)


class UserModel:
    """A fitted decay user model (``fit_user_model``): ``alpha`` float64 [H], ``beta``, ``time_unit`` and ``history``, the loss per
    pair of every optimisation step."""

    def __init__(self, alpha, beta, time_unit, history):
        self.alpha, self.beta, self.time_unit, self.history = alpha, float(beta), time_unit, history

    def states(self, histories, embeddings, timestamps=None, return_tensor=False, device=None):
        """``alpha * user_states(histories, embeddings, beta, ...)``: with these vectors the plain inner product of ``recommend`` /
        ``recommend_ranks`` is the fitted relevance ``(alpha * u) . a``."""
        import torch
        U = user_states(histories, embeddings, self.beta, timestamps=timestamps, time_unit=self.time_unit, return_tensor=True,
                        device=device)
        U = U * torch.from_numpy(self.alpha.astype(np.float32)).to(U.device)
        return result(U, return_tensor)


def fit_user_model(histories, embeddings, *, beta0=0.9, fit_beta=True, n_neg=4, epochs=50, batch_users=None, lr=0.05, seed=0,
                   timestamps=None, time_unit=None, window=None, device=None):
    """Fits the decay user model of the KDD'17 paper to click histories: the scaling vector ``alpha`` (start: ones) and, with
    ``fit_beta``, the decay ``beta = sigmoid(theta)`` (start: ``beta0``), by Adam in float64 NumPy on the mean pairwise ranking
    loss of ``user_pair_loss``, whose sums ``dae_user_pair_loss`` delivers in one walk of the histories per step.  The article
    embeddings stay fixed.

    Every epoch draws ``n_neg`` negatives per click (``sample_negatives(..., seed + epoch, window=window)``; ``window``: per-EVENT
    candidate ranges) and takes one step per mini-batch of ``batch_users`` consecutive users (None: all users, one step per
    epoch).  The gradient is divided by the batch's number of pairs; ``d/dtheta = dbeta * beta * (1 - beta)``.  A batch without a
    valid pair takes no step and records NaN.  Deterministic per seed.

    Returns a ``UserModel``: ``alpha``, ``beta``, ``time_unit``, ``history`` (loss per pair of every step, before the step) and
    ``.states(histories, embeddings, timestamps=None)``, the vectors to hand to ``recommend`` / ``recommend_ranks``."""
    indptr, items = history_csr(histories)
    beta = float(beta0)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta0 must be in [0, 1] (got {beta0})")
    if int(epochs) < 0 or not float(lr) > 0.0:
        raise ValueError("epochs must not be negative and lr must be positive")
    t = None if timestamps is None else np.asarray(event_times(timestamps), dtype=np.float64).ravel()
    torch, _, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev, in_place=True)
    Na, H = int(E.shape[0]), int(E.shape[1])
    if not 1 <= H <= 1024:
        raise ValueError(f"the embedding dimension must be in 1..1024 (got {H})")
    check_item_range(items, Na)
    M, nnz = int(indptr.size - 1), int(items.size)
    step_users = M if batch_users is None else int(batch_users)
    if batch_users is not None and step_users < 1:
        raise ValueError(f"batch_users must be positive (got {batch_users})")
    if fit_beta:
        beta = min(max(beta, 1e-6), 1.0 - 1e-6)                             # theta is finite
    x = np.concatenate([np.ones(H), [np.log(beta / (1.0 - beta)) if fit_beta else 0.0]])      # (alpha, theta)
    m1, m2, step = np.zeros(H + 1), np.zeros(H + 1), 0
    history = []
    it_d = upload(items.astype(np.int32), dev)
    none = np.zeros(0, dtype=np.float32)                                   # the factors of a batch without events
    for epoch in range(int(epochs)):
        ng_d = upload(sample_negatives(indptr, items, Na, n_neg, int(seed) + epoch, window=window), dev)
        for u0 in range(0, M, max(step_users, 1)):
            u1 = min(u0 + step_users, M)
            a, b = int(indptr[u0]), int(indptr[u1])
            if fit_beta:
                beta = 1.0 / (1.0 + np.exp(-x[H]))
            beta32 = float(np.float32(beta))
            dc_d = dd_d = None
            if t is not None:
                ip = indptr[u0:u1 + 1] - a
                dc_d = upload(decay_factors(ip, t[a:b], beta32, time_unit) if b > a else none, dev)
                if fit_beta:
                    dd_d = upload(decay_factor_derivatives(ip, t[a:b], beta32, time_unit) if b > a else none, dev)
            r = _pair_loss_call(torch, E, torch.from_numpy(indptr[u0:u1 + 1] - a).to(dev), it_d[a:max(b, a + 1)],
                                ng_d[a:max(b, a + 1)], u1 - u0, b - a, int(n_neg), x[:H], beta32, dc_d, dd_d)
            if r["n_pairs"] == 0:
                history.append(float("nan"))
                continue
            history.append(r["loss"] / r["n_pairs"])
            grad = np.concatenate([r["dalpha"], [r["dbeta"] * beta * (1.0 - beta) if fit_beta else 0.0]]) / r["n_pairs"]
            step += 1
            m1 = 0.9 * m1 + 0.1 * grad
            m2 = 0.999 * m2 + 0.001 * grad * grad
            x = x - float(lr) * (m1 / (1.0 - 0.9 ** step)) / (np.sqrt(m2 / (1.0 - 0.999 ** step)) + 1e-8)
    if fit_beta:
        beta = 1.0 / (1.0 + np.exp(-x[H]))
    return UserModel(x[:H].copy(), float(np.float32(beta)), time_unit, np.asarray(history, dtype=np.float64))


def _gru_fit_checks(embeddings, H, D, items):
    """The host-side refusals of ``gru_pair_loss`` / ``fit_gru_user_model``, before any device work: ``(articles, H)``."""
    Na, De = matrix_shape(embeddings)
    check_item_kind(items)
    if De != D:
        raise ValueError(f"embeddings have {De} columns, the model's weight_ih has {D}")
    if D != H:
        raise ValueError(f"training scores the state against the embeddings: the hidden size ({H}) must equal the embedding size D = {D}")
    check_item_range(items, Na)
    if Na == 0:
        raise ValueError("embeddings hold no articles")
    return Na, H


def _gru_pair_loss_call(torch, E, w, indptr, it_d, ng_d, n_neg, grads, scal, margins=None, cell="gru"):
    """One ``dae_gru_pair_loss`` (``cell``: ``dae_lstm_pair_loss`` / ``dae_rnn_pair_loss``) on device operands, nothing read back.
    ``indptr``: host int64 [M + 1] starting at 0; ``it_d`` int32 [nnz], ``ng_d`` int32 [nnz x n_neg]; ``w`` / ``grads``: the four
    float32 weight tensors and their gradients (contiguous); ``scal``: float64 [2] that receives the loss and the bits of the int64
    pair count; ``margins``: float32 [nnz x n_neg] or None."""
    import ctypes
    dev = E.device
    lib = L.load()
    Na, H = int(E.shape[0]), int(E.shape[1])
    M, nnz = int(indptr.size - 1), int(indptr[-1])
    order, active = gru_schedule(indptr)
    T = int(active.size)
    ip_d = torch.from_numpy(np.array(indptr, dtype=np.int64)).to(dev)
    or_d = upload(order, dev)
    with torch.cuda.device(dev):
        ws_bytes = int(getattr(lib, f"dae_{cell}_pair_loss_workspace")(Na, H, M, nnz, T, n_neg))
        ws_ptr, ws = workspace(dev, ws_bytes)
        L.call(f"dae_{cell}_pair_loss", L.ptr(E), E.stride(0), Na, H, L.ptr(w[0]), H, L.ptr(w[1]), H, L.ptr(w[2]), L.ptr(w[3]), L.ptr(ip_d),
               L.ptr(it_d), L.ptr(or_d), M, nnz, T, active.ctypes.data_as(ctypes.c_void_p), L.ptr(ng_d), n_neg,
               ctypes.c_void_p(scal.data_ptr()), ctypes.c_void_p(scal.data_ptr() + 8), L.ptr(grads[0]), H, L.ptr(grads[1]), H,
               L.ptr(grads[2]), L.ptr(grads[3]), L.ptr(margins), ws_ptr, ws_bytes, L.current_stream())
    del ws


def gru_pair_loss(histories, embeddings, model, negatives, *, return_margins=False, device=None):
    """The training step of the GRU user model (``dae_gru_pair_loss``): the pairwise ranking loss of ``user_pair_loss`` on the states
    of ``gru_user_states`` -- with ``h`` the state BEFORE a click, margin ``x = h . (E[clicked] - E[negative])``, loss = the sum of
    ``softplus(-x)`` over the valid pairs -- and, by back-propagation through time on the device, its gradients with respect to the
    four weight arrays of ``model`` (a ``GRUUserModel`` whose hidden size equals the embedding size; ``h`` starts at zero).  The
    embeddings are fixed and get no gradient.

    ``histories``, ``embeddings``: as ``gru_user_states``; ``negatives``: as ``user_pair_loss`` (integer ``[events x n_neg]``, 1..16
    columns; a negative entry, the click itself and every entry of a user's first click are no pair).  The same ``ValueError``s:
    items outside the articles, negatives of the wrong shape or >= the number of articles, and ``D != H``.

    Returns ``{'loss': float, 'n_pairs': int, 'weight_ih', 'weight_hh', 'bias_ih', 'bias_hh': float32 gradients in the model's
    shapes}`` -- sums over the valid pairs, NOT divided by ``n_pairs`` -- and with ``return_margins=True`` also ``'margins'``:
    float32 ``[events x n_neg]``, 0 where there is no pair.  Bit-identical run to run; ``n_pairs`` and the margins do not depend
    on the order of the users, the gradients agree under a permutation of the users to rounding."""
    return _recurrent_pair_loss("gru", GRUUserModel, histories, embeddings, model, negatives, return_margins, device)


def _recurrent_pair_loss(cell, cls, histories, embeddings, model, negatives, return_margins, device):
    """The intake and read-back shared by ``gru_pair_loss``, ``lstm_pair_loss`` and ``rnn_pair_loss``: one ``dae_{cell}_pair_loss`` on
    the weights of ``model`` (a ``cls``)."""
    if not isinstance(model, cls):
        raise TypeError(f"model must be a {cls.__name__} ({cls.__name__}.load / from_torch)")
    indptr, items = csr_lists(histories)
    Na, H = _gru_fit_checks(embeddings, model.hidden_size, model.input_size, items)
    nnz = int(items.size)
    neg = _check_negatives(negatives, nnz, Na)
    n_neg = int(neg.shape[1])
    torch, _, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev, in_place=True)
    w = [torch.from_numpy(getattr(model, n)).to(dev) for n in cls.NAMES]
    grads = [torch.empty_like(a) for a in w]
    scal = torch.zeros(2, dtype=torch.float64, device=dev)
    mg = torch.empty((max(nnz, 1), n_neg), dtype=torch.float32, device=dev) if return_margins else None
    _gru_pair_loss_call(torch, E, w, indptr, upload(items.astype(np.int32), dev), upload(neg, dev), n_neg, grads, scal, mg, cell=cell)
    host = scal.cpu().numpy()
    res = {"loss": float(host[0]), "n_pairs": int(host[1:].view(np.int64)[0])}
    for name, g in zip(cls.NAMES, grads):
        res[name] = g.cpu().numpy()
    if return_margins:
        res["margins"] = mg[:nnz].cpu().numpy()
    return res


def lstm_pair_loss(histories, embeddings, model, negatives, *, return_margins=False, device=None):
    """The training step of the LSTM user model (``dae_lstm_pair_loss``): ``gru_pair_loss`` on the states of ``lstm_user_states`` --
    the same margins, loss, pairs and errors -- with the gradients of the four weight arrays of ``model`` (an ``LSTMUserModel``
    whose hidden size equals the embedding size; ``h`` and ``c`` start at zero) by back-propagation through time on the device.
    Returns the dict of ``gru_pair_loss`` with gradients in the model's shapes ([4H x H], [4H]; gate row blocks i, f, g, o)."""
    return _recurrent_pair_loss("lstm", LSTMUserModel, histories, embeddings, model, negatives, return_margins, device)


def rnn_pair_loss(histories, embeddings, model, negatives, *, return_margins=False, device=None):
    """The training step of the plain-RNN user model (``dae_rnn_pair_loss``): ``gru_pair_loss`` on the states of ``rnn_user_states``
    -- the same margins, loss, pairs and errors -- with the gradients of the four weight arrays of ``model`` (an ``RNNUserModel``
    whose hidden size equals the embedding size; ``h`` starts at zero) by back-propagation through time on the device.  Returns
    the dict of ``gru_pair_loss`` with gradients in the model's shapes ([H x H], [H])."""
    return _recurrent_pair_loss("rnn", RNNUserModel, histories, embeddings, model, negatives, return_margins, device)


def fit_gru_user_model(histories, embeddings, *, epochs=5, batch_users=256, n_neg=4, lr=1e-2, seed=0, max_events=50, init=None,
                       window=None, validation=None, validation_every=1, keep_best=False, device=None):
    """Trains the GRU user model of the KDD'17 paper on click histories, on the device: mini-batch Adam on the mean pairwise
    ranking loss of ``gru_pair_loss``, whose sums and gradients ``dae_gru_pair_loss`` delivers in one call per mini-batch.  The
    article embeddings [articles x H] stay fixed; the hidden size is H.

    Every user's ``max_events`` most recent events are kept (``trim_histories``).  Every epoch draws ``n_neg`` negatives per click
    (``sample_negatives(..., seed * 1000003 + epoch, window=window)``; ``window``: per-EVENT candidate ranges of the trimmed
    histories) and one permutation of the users with at least two events (``numpy.random.default_rng(seed)``), taken in
    mini-batches of ``batch_users``.  The gradient is divided by the batch's number of pairs; a batch without a pair takes no step.
    Adam (beta1 = 0.9, beta2 = 0.999, eps = 1e-8) runs on the device as tensor operations on the four float32 weight tensors: only
    the two scalars of a batch, its loss and its pair count, come back to the host.  The weights start from ``torch.nn.GRU``'s
    rule, uniform in +-1 / sqrt(H), drawn from the same generator before the permutations -- or from ``init``, a ``GRUUserModel``,
    to continue a fit.  Two fits with equal arguments return bit-equal weights.

    ``validation`` (histories of held-out users, default None): after every ``validation_every`` epochs the weights of that
    epoch are scored on them by ``evaluate_every_click`` -- every click ranked given the clicks before it -- and the metric dicts
    (``rank_metrics`` plus ``'epoch'``, counted from 1) are collected in ``.validation`` (not saved, like ``.history``).  The
    validation pass reads the weights and nothing else: it does not touch the generator or Adam's state, so without ``keep_best``
    the returned weights are bit-equal to those of a fit without ``validation``.  With ``keep_best`` the weights of the scored
    epoch with the highest validation ``mrr`` (the first of equals) are returned instead of the last epoch's.

    Returns a ``GRUUserModel`` whose ``.history`` is the loss per pair of every epoch (float64 [epochs])."""
    return _fit_recurrent_user_model("gru", GRUUserModel, 3, histories, embeddings, epochs, batch_users, n_neg, lr, seed, max_events, init,
                                     window, validation, validation_every, keep_best, device)


def _fit_recurrent_user_model(cell, cls, gates, histories, embeddings, epochs, batch_users, n_neg, lr, seed, max_events, init, window,
                              validation, validation_every, keep_best, device):
    """The loop of ``fit_gru_user_model``, ``fit_lstm_user_model`` and ``fit_rnn_user_model``: mini-batch Adam on
    ``dae_{cell}_pair_loss`` for a model class ``cls`` with ``gates`` row blocks of H rows."""
    from .evaluation import evaluate_every_click                      # (evaluation imports this module)
    if int(epochs) < 0 or not float(lr) > 0.0:
        raise ValueError("epochs must not be negative and lr must be positive")
    if int(validation_every) < 1:
        raise ValueError(f"validation_every must be positive (got {validation_every})")
    if keep_best and validation is None:
        raise ValueError("keep_best needs validation histories")
    if int(batch_users) < 1:
        raise ValueError(f"batch_users must be positive (got {batch_users})")
    if not 1 <= int(n_neg) <= 16:
        raise ValueError(f"n_neg must be in 1..16 (got {n_neg})")
    if init is not None and not isinstance(init, cls):
        raise TypeError(f"init must be a {cls.__name__}")
    indptr, items = csr_lists(histories)
    D = matrix_shape(embeddings)[1]
    H = D if init is None else init.hidden_size
    Na, H = _gru_fit_checks(embeddings, H, D if init is None else init.input_size, items)
    indptr, items = trim_histories((indptr, items), max_events)
    n_neg, batch_users = int(n_neg), int(batch_users)
    rng = np.random.default_rng(seed)
    if init is None:
        k = 1.0 / np.sqrt(H)
        start = [rng.uniform(-k, k, s).astype(np.float32) for s in ((gates * H, H), (gates * H, H), (gates * H,), (gates * H,))]
    else:
        start = [getattr(init, n) for n in cls.NAMES]
    torch, _, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev, in_place=True)
    w = [torch.from_numpy(np.array(a, dtype=np.float32)).to(dev) for a in start]
    grads = [torch.empty_like(a) for a in w]
    m1, m2 = [torch.zeros_like(a) for a in w], [torch.zeros_like(a) for a in w]
    scal = torch.zeros(2, dtype=torch.float64, device=dev)
    users = np.flatnonzero(np.diff(indptr) >= 2)
    history, step = [], 0
    scored, best, best_w = [], None, None
    for epoch in range(int(epochs)):
        neg = sample_negatives(indptr, items, Na, n_neg, int(seed) * 1000003 + epoch, window=window)
        perm = rng.permutation(users)
        total, pairs = 0.0, 0
        for b0 in range(0, perm.size, batch_users):
            ub = perm[b0:b0 + batch_users]
            n = np.diff(indptr)[ub]
            ip = np.zeros(ub.size + 1, dtype=np.int64)
            ip[1:] = np.cumsum(n)
            take = np.repeat(indptr[:-1][ub] - ip[:-1], n) + np.arange(int(ip[-1]), dtype=np.int64)
            it_d = torch.from_numpy(items[take].astype(np.int32)).to(dev)
            ng_d = torch.from_numpy(np.ascontiguousarray(neg[take])).to(dev)
            _gru_pair_loss_call(torch, E, w, ip, it_d, ng_d, n_neg, grads, scal, cell=cell)
            host = scal.cpu().numpy()                                  # two scalars; the gradients stay on the device
            n_pairs = int(host[1:].view(np.int64)[0])
            if n_pairs == 0:
                continue
            total += float(host[0])
            pairs += n_pairs
            step += 1
            c1, c2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
            for a, g, a1, a2 in zip(w, grads, m1, m2):
                g.div_(float(n_pairs))
                a1.mul_(0.9).add_(g, alpha=0.1)
                a2.mul_(0.999).addcmul_(g, g, value=0.001)
                a.sub_(float(lr) * (a1 / c1) / ((a2 / c2).sqrt_() + 1e-8))
        history.append(total / max(pairs, 1))
        if validation is not None and (epoch + 1) % int(validation_every) == 0:
            host = [a.cpu().numpy() for a in w]                       # a copy: the fit goes on with the device tensors
            m = evaluate_every_click(validation, E, cls(*host), device=device)["metrics"]
            m["epoch"] = epoch + 1
            scored.append(m)
            if keep_best and m["mrr"] == m["mrr"] and (best is None or m["mrr"] > best):      # NaN (no click to score): never the best
                best, best_w = m["mrr"], host
    final = best_w if keep_best and best_w is not None else [a.cpu().numpy() for a in w]
    return cls(*final, history=np.asarray(history, dtype=np.float64), validation=scored if validation is not None else None)


def fit_lstm_user_model(histories, embeddings, *, epochs=5, batch_users=256, n_neg=4, lr=1e-2, seed=0, max_events=50, init=None,
                        window=None, validation=None, validation_every=1, keep_best=False, device=None):
    """Trains the LSTM user model of the KDD'17 paper on click histories, on the device: ``fit_gru_user_model`` with the loss and
    gradients of ``lstm_pair_loss`` (``dae_lstm_pair_loss``) -- the same arguments, negatives, permutations, Adam, ``validation`` /
    ``keep_best`` and errors.  The weights start from ``torch.nn.LSTM``'s rule, uniform in +-1 / sqrt(H), drawn from
    ``numpy.random.default_rng(seed)`` in the order weight_ih, weight_hh, bias_ih, bias_hh before the permutations -- or from
    ``init``, an ``LSTMUserModel``.  Two fits with equal arguments return bit-equal weights.  Returns an ``LSTMUserModel`` with
    ``.history`` and ``.validation``."""
    return _fit_recurrent_user_model("lstm", LSTMUserModel, 4, histories, embeddings, epochs, batch_users, n_neg, lr, seed, max_events, init,
                                     window, validation, validation_every, keep_best, device)


def fit_rnn_user_model(histories, embeddings, *, epochs=5, batch_users=256, n_neg=4, lr=1e-2, seed=0, max_events=50, init=None,
                       window=None, validation=None, validation_every=1, keep_best=False, device=None):
    """Trains the plain-RNN user model of the KDD'17 paper on click histories, on the device: ``fit_gru_user_model`` with the loss
    and gradients of ``rnn_pair_loss`` (``dae_rnn_pair_loss``) -- the same arguments, negatives, permutations, Adam, ``validation`` /
    ``keep_best`` and errors.  The weights start from ``torch.nn.RNN``'s rule, uniform in +-1 / sqrt(H), drawn from
    ``numpy.random.default_rng(seed)`` in the order weight_ih, weight_hh, bias_ih, bias_hh before the permutations -- or from
    ``init``, an ``RNNUserModel``.  Two fits with equal arguments return bit-equal weights.  Returns an ``RNNUserModel`` with
    ``.history`` and ``.validation``."""
    return _fit_recurrent_user_model("rnn", RNNUserModel, 1, histories, embeddings, epochs, batch_users, n_neg, lr, seed, max_events, init,
                                     window, validation, validation_every, keep_best, device)
