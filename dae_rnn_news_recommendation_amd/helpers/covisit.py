"""The co-visitation baseline: "readers of this article also read ...", built from co-clicks alone -- no embeddings.
``covisit_neighbors`` builds the neighbour table of a click log on the device (``dae_covisit_neighbors``: emit, sort, run-length,
select -- never an articles x articles matrix) and returns a ``CovisitIndex``; ``CovisitIndex.recommend`` scores a user's unseen
articles from the neighbours of the last clicks (``dae_covisit_recommend``); ``covisit_recommend`` is both in one call.
``list_overlap`` (host code) compares two neighbour tables, e.g. the co-click neighbours with ``most_similar``'s embedding
neighbours.  The rules of the model are stated in include/dae_hip.h."""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ._device import csr_lists, device_and_library, history_csr, result, upload, workspace
from .sweeps import normalize_exclusions, normalize_window
from .user_models import trim_histories

DIRECTIONS = {"forward": 0, "both": 1}
NORMALIZE = {"none": 0, "cosine": 1}


def _settings(window, direction, normalize, n_neighbors):
    if direction not in DIRECTIONS:
        raise ValueError(f"direction must be 'both' or 'forward' (got {direction!r})")
    if normalize not in NORMALIZE:
        raise ValueError(f"normalize must be 'cosine' or 'none' (got {normalize!r})")
    if int(window) < 1:
        raise ValueError(f"window must be at least 1 (got {window})")
    if not 1 <= int(n_neighbors) <= 128:
        raise ValueError(f"n_neighbors must be in 1..128 (got {n_neighbors})")
    return min(int(window), 2 ** 31 - 1), int(n_neighbors)


def covisit_neighbors(histories, n_articles, *, window=3, direction="both", normalize="cosine", n_neighbors=50, max_events=None,
                      return_tensor=False, device=None):
    """The co-visitation neighbour table of a click log, built on the device.  ``histories``: a list of index sequences or an
    ``(indptr, items)`` tuple, oldest click first, over ``n_articles`` articles.  Two clicks of one user at most ``window``
    positions apart are a record ``(a, b)`` -- earlier, later -- and with ``direction='both'`` also ``(b, a)``; equal articles give
    none.  The similarity of ``a`` to ``b`` is the number of records ``c`` (``normalize='none'``) or
    ``c / sqrt(clicks[a] * clicks[b])`` (``'cosine'``), in float32.  ``max_events``: only every user's most recent events count
    (``trim_histories``).

    Returns a ``CovisitIndex``: ``neighbors`` int64 / ``sims`` float32 / ``counts`` int32 ``[n_articles x n_neighbors]`` -- per
    article the best neighbours by similarity descending, index ascending; tails -1 / 0 / 0 -- ``degree`` (distinct neighbours) and
    ``clicks`` int32 ``[n_articles]``, ``n_records`` and ``n_pairs``.  Arrays are ndarrays, or CUDA tensors with
    ``return_tensor=True``.  The result is exact and bit-identical from run to run, whatever the order of the users.

    The build holds 20 bytes per record of ``dae_covisit_record_bound`` on the device, and fewer than 2^31 records per call: a
    larger log raises ``ValueError`` with the figure -- build from fewer users."""
    import ctypes
    window, K = _settings(window, direction, normalize, n_neighbors)
    Na = int(n_articles)
    if Na < 1:
        raise ValueError(f"n_articles must be at least 1 (got {n_articles})")
    indptr, items = history_csr(histories if max_events is None else trim_histories(histories, max_events), Na)
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    M, nnz = indptr.size - 1, int(items.size)
    torch, lib, dev = device_and_library(device)
    both = DIRECTIONS[direction]
    bound = int(lib.dae_covisit_record_bound(indptr.ctypes.data_as(ctypes.c_void_p), M, window, both)) if M > 0 else 0
    if bound >= 1 << 31:
        raise ValueError(f"the log gives up to {bound} records ({20 * bound / 2 ** 30:.1f} GiB of build buffers); one call takes fewer "
                         "than 2^31 -- build from fewer users")
    i32 = dict(dtype=torch.int32, device=dev)
    nbr, cnt = torch.empty((Na, K), **i32), torch.empty((Na, K), **i32)
    sim = torch.empty((Na, K), dtype=torch.float32, device=dev)
    degree, clicks = torch.empty(Na, **i32), torch.empty(Na, **i32)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.dae_covisit_neighbors_workspace(bound, Na, K))
        if bound > 0 and ws_bytes == 0:
            raise RuntimeError("dae_covisit_neighbors_workspace: the size query failed")
        ws_p, ws = workspace(dev, ws_bytes)
        d_ptr, d_items = upload(indptr, dev), upload(items.astype(np.int32), dev)
        L.call("dae_covisit_neighbors", L.ptr(d_ptr), L.ptr(d_items), indptr.ctypes.data_as(ctypes.c_void_p), M, nnz, Na, window, both,
               NORMALIZE[normalize], K, L.ptr(nbr), L.ptr(sim), L.ptr(cnt), nbr.stride(0), L.ptr(degree), L.ptr(clicks), L.ptr(totals),
               ws_p if bound > 0 else None, ws_bytes, L.current_stream())
        del ws
    n_records, n_pairs = (int(v) for v in totals.cpu().numpy())
    fields = {name: result(t, return_tensor) for name, t in (("neighbors", nbr.long()), ("sims", sim), ("counts", cnt), ("degree", degree),
                                                              ("clicks", clicks))}
    return CovisitIndex(n_records=n_records, n_pairs=n_pairs, window=window, direction=direction, normalize=normalize, n_neighbors=K,
                        **fields)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class CovisitIndex:
    """What ``covisit_neighbors`` returns: the table ``neighbors`` int64 / ``sims`` float32 / ``counts`` int32
    ``[n_articles x n_neighbors]`` (tails -1 / 0 / 0), ``degree`` and ``clicks`` int32 ``[n_articles]``, ``n_records``, ``n_pairs``
    and the settings ``window``, ``direction``, ``normalize``, ``n_neighbors``."""

    _ARRAYS = ("neighbors", "sims", "counts", "degree", "clicks")
    _SCALARS = ("n_records", "n_pairs", "window", "n_neighbors")

    def __init__(self, neighbors, sims, counts, degree, clicks, n_records, n_pairs, window, direction, normalize, n_neighbors):
        self.neighbors, self.sims, self.counts, self.degree, self.clicks = neighbors, sims, counts, degree, clicks
        self.n_records, self.n_pairs, self.window, self.n_neighbors = int(n_records), int(n_pairs), int(window), int(n_neighbors)
        self.direction, self.normalize = str(direction), str(normalize)
        if tuple(neighbors.shape) != tuple(sims.shape) or len(neighbors.shape) != 2 or neighbors.shape[1] != self.n_neighbors:
            raise ValueError("neighbors and sims must both be [n_articles x n_neighbors]")

    n_articles = property(lambda self: int(self.neighbors.shape[0]))

    def similar(self, items, k=None):
        """The rows of the table for ``items``, cut to ``k`` columns (default: all): ``(neighbors, sims, counts)``."""
        k = self.n_neighbors if k is None else int(k)
        if not 1 <= k <= self.n_neighbors:
            raise ValueError(f"k must be in 1..{self.n_neighbors} (got {k})")
        rows = np.asarray(items, dtype=np.int64).ravel()
        if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= self.n_articles):
            raise ValueError(f"items must be in 0..{self.n_articles - 1}")
        if hasattr(self.neighbors, "detach"):
            import torch
            rows = torch.from_numpy(rows).to(self.neighbors.device)
        return self.neighbors[rows][:, :k], self.sims[rows][:, :k], self.counts[rows][:, :k]

    def save(self, path):
        """The index as one ``.npz``."""
        np.savez(path, **{n: _host(getattr(self, n)) for n in self._ARRAYS}, **{n: np.int64(getattr(self, n)) for n in self._SCALARS},
                 direction=np.array(self.direction), normalize=np.array(self.normalize))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(**{n: z[n] for n in cls._ARRAYS}, **{n: int(z[n]) for n in cls._SCALARS}, direction=str(z["direction"]),
                       normalize=str(z["normalize"]))

    def recommend(self, histories, k=10, seen=None, *, last=10, position_decay=0.8, window=None, fill_popular=False,
                  return_tensor=False, device=None):
        """For every user of ``histories`` (need not be the log the index was built from) the ``k`` unseen articles with the largest
        score: the neighbours of the user's ``last`` most recent clicks, each weighted by its similarity times
        ``position_decay ** age`` (age 0: the newest click), summed per article in float32, oldest click first.  ``seen``: per user
        the articles that must not be returned (as in ``recommend``; default: the own history).  ``window``: a pair ``(lo, hi)``
        per user, as in ``recommend``.  An article that is reached counts whatever its sum (``position_decay=0`` leaves scores of
        0).  1 <= k <= 128, 1 <= last <= 32.

        Returns ``(indices int64 [users x k], scores float32 [users x k])``, ordered by score descending, index ascending, with
        -1 / -inf where fewer than ``k`` candidates exist.  ``fill_popular=True`` fills those tails, on the host, with the most
        clicked articles (the index's ``clicks``, ties by index ascending) that are unseen, in the window and not yet listed; their
        score stays -inf."""
        k, last = int(k), int(last)
        if not 1 <= k <= 128:
            raise ValueError(f"k must be in 1..128 (got {k})")
        if not 1 <= last <= 32:
            raise ValueError(f"last must be in 1..32 (got {last})")
        if not np.isfinite(float(position_decay)):
            raise ValueError(f"position_decay must be finite (got {position_decay})")
        Na, K = self.n_articles, self.n_neighbors
        indptr, items = history_csr(histories, Na)
        M = indptr.size - 1
        xp, xi = normalize_exclusions((indptr, items) if seen is None else seen, M, Na)
        if window is not None:
            window = normalize_window(window, M, Na)
        age_weight = (np.float64(position_decay) ** np.arange(last)).astype(np.float32)
        torch, lib, dev = device_and_library(device)
        nbr = torch.as_tensor(self.neighbors).to(device=dev, dtype=torch.int32).contiguous()
        sim = torch.as_tensor(self.sims).to(device=dev, dtype=torch.float32).contiguous()
        idx = torch.empty((M, k), dtype=torch.int32, device=dev)
        score = torch.empty((M, k), dtype=torch.float32, device=dev)
        if M > 0:
            d = [upload(np.ascontiguousarray(a), dev) for a in (indptr.astype(np.int64), items.astype(np.int32), xp, xi, age_weight)]
            lo_d, hi_d = (None, None) if window is None else (upload(window[0], dev), upload(window[1], dev))
            with torch.cuda.device(dev):
                L.call("dae_covisit_recommend", L.ptr(nbr), L.ptr(sim), nbr.stride(0), Na, K, L.ptr(d[0]), L.ptr(d[1]), M, L.ptr(d[2]),
                       L.ptr(d[3]), L.ptr(lo_d), L.ptr(hi_d), L.ptr(d[4]), last, k, L.ptr(idx), L.ptr(score), idx.stride(0),
                       L.current_stream())
        idx = idx.long()
        if fill_popular:
            filled = fill_popular_tails(idx.cpu().numpy(), _host(self.clicks), (xp, xi), window)
            idx = torch.from_numpy(filled).to(dev)
        return result((idx, score), return_tensor)


def fill_popular_tails(indices, clicks, seen, window=None):
    """``indices`` int64 ``[users x k]`` with its -1 tails filled by popularity: per user the most clicked articles (``clicks``,
    ties by index ascending) that are not in the user's ``seen`` row (``(indptr, items)``), lie in the user's ``window`` ``(lo, hi)``
    when one is given and are not in the list already.  A list stays short where no such article is left.  Host code."""
    out = np.array(indices, dtype=np.int64, copy=True)
    clicks = np.asarray(clicks).astype(np.int64)
    xp, xi = seen
    order = np.argsort(-clicks, kind="stable")
    for u in np.flatnonzero((out < 0).any(axis=1)):
        row = out[u]
        have = int((row >= 0).sum())
        cand = order if window is None else order[(order >= int(window[0][u])) & (order < int(window[1][u]))]
        cand = cand[~np.isin(cand, xi[xp[u]:xp[u + 1]]) & ~np.isin(cand, row[:have])][:row.size - have]
        row[have:have + cand.size] = cand
    return out


def covisit_recommend(histories, n_articles, k=10, seen=None, *, window=3, direction="both", normalize="cosine", n_neighbors=50,
                      max_events=None, last=10, position_decay=0.8, candidate_window=None, fill_popular=False, return_tensor=False,
                      device=None):
    """``covisit_neighbors`` of ``histories`` and ``CovisitIndex.recommend`` for the same users in one call (``window`` is the pair
    window of the build; ``candidate_window`` the per-user ``(lo, hi)`` of the recommendation).  Returns ``(indices, scores)``."""
    index = covisit_neighbors(histories, n_articles, window=window, direction=direction, normalize=normalize, n_neighbors=n_neighbors,
                              max_events=max_events, return_tensor=True, device=device)
    return index.recommend(histories, k, seen, last=last, position_decay=position_decay, window=candidate_window,
                           fill_popular=fill_popular, return_tensor=return_tensor, device=device)


def list_overlap(a, b):
    """How much of one neighbour table another one finds.  ``a`` / ``b``: integer ``[n x ka]`` / ``[n x kb]``, -1 where a row is
    short.  Returns ``(per_row float64 [n], mean)``: per row the share of ``a``'s non-negative entries that also appear in ``b``'s
    row (NaN for a row of ``a`` without an entry), and the mean over the rows with at least one entry (NaN without such a row).
    Host code."""
    a, b = _host(a), _host(b)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError(f"a and b must be [n x ka] and [n x kb] (got {a.shape} and {b.shape})")
    ok = a >= 0
    found = np.zeros(a.shape[0], dtype=np.int64)
    for r0 in range(0, a.shape[0], 4096):                               # row blocks: the comparison cube stays small
        r = slice(r0, r0 + 4096)
        found[r] = ((a[r, :, None] == b[r, None, :]) & ok[r, :, None]).any(axis=2).sum(axis=1)
    n = ok.sum(axis=1)
    per = np.where(n > 0, found / np.maximum(n, 1), np.nan)
    return per, float(per[n > 0].mean()) if (n > 0).any() else float("nan")
