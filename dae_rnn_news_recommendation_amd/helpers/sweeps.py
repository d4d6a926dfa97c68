"""The score sweeps over two sets of rows, by the scores of ``pairwise_similarity`` (the reference's helpers.py:11-50) and without
its N x N matrix: ``most_similar`` (top-k), ``target_ranks`` (full rank of one target per row), ``similar_pairs`` (every pair over a
threshold), ``dedup_lists`` (greedy de-duplication of such lists) and ``diversify_lists`` (MMR re-ranking with a de-dup threshold and
a per-label cap); the row filter the first two share (``normalize_exclusions``,
``normalize_shared_exclusions``, ``normalize_window``, ``candidate_windows``); and the start of every sweep: the chunk plan
(``sweep_chunk_rows``, ``sweep_chunk_plan``, ``label_stats_blocks``), ``SweepOperand`` and ``sweep_start``."""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ._device import (container, csr_lists, dense_on_device, device_and_library, device_matrix, matrix_shape, norm_metric, result, row_count,
                      upload, workspace)


def pairwise_similarity(in_df, norm="", metric="cosine", set_diagonal_zero=True, *, return_tensor=False, device=None):
    """Pairwise similarity of the rows of ``in_df`` (ndarray, scipy.sparse matrix, list, or a CUDA float32 tensor).

    norm: '' or sklearn.preprocessing.normalize's 'l1' / 'l2' / 'max', applied first; metric: 'cosine' or
    'linear kernel'; set_diagonal_zero as in the reference.  Returns a float32 ndarray [N x N]
    (``return_tensor=True``: the CUDA tensor view, no copy to the host).

    Sparse input is densified on the device (one fp32 image of the matrix); the reference's sklearn path would return
    a sparse matrix for ``linear kernel`` + sparse input with dense_output left at its default -- here the result is
    always dense, which is what every caller in the reference needs (they index and plot it)."""
    nm = norm_metric(norm, metric)
    torch, lib, dev = device_and_library(device)
    X = device_matrix(torch, in_df, dev)
    N, D = int(X.shape[0]), int(X.shape[1])
    Np = L.pad(N)
    out = torch.empty((Np, Np), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.dae_pairwise_similarity_workspace(N, D))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.call("dae_pairwise_similarity", L.ptr(X), X.stride(0), N, D, *nm, 1 if set_diagonal_zero else 0, L.ptr(out), Np, L.ptr(ws),
               ws_bytes, L.current_stream())
    return result(out[:N, :N], return_tensor)


# chunk_rows="auto": the largest chunk whose operand image stays within this many bytes.  NOT measured: 1 GiB is a round figure
# that keeps two images far below the memory of one device while a chunk still holds thousands of rows at a 50 000-word vocabulary.
SWEEP_AUTO_IMAGE_BYTES = 1 << 30


def sweep_chunk_rows(chunk_rows, n_features):
    """The rows per chunk of a chunked sweep (``most_similar`` / ``label_similarity_stats`` with ``chunk_rows=``): None stays None
    (the one-shot route), an integer >= 1 is rounded up to a multiple of 128 (the tile height: a chunk's image has no padding
    rows inside the operand), and ``"auto"`` is the largest multiple of 128 whose fp32 image of ``n_features`` columns (padded to
    128) is at most ``SWEEP_AUTO_IMAGE_BYTES``, and at least 128.  Host code."""
    if chunk_rows is None:
        return None
    if isinstance(chunk_rows, str):
        if chunk_rows != "auto":
            raise ValueError(f"chunk_rows must be None, a positive integer or 'auto' (got {chunk_rows!r})")
        return max(SWEEP_AUTO_IMAGE_BYTES // (L.pad(max(int(n_features), 1)) * 4) // L.PAD * L.PAD, L.PAD)
    c = int(chunk_rows)
    if c < 1:
        raise ValueError(f"chunk_rows must be None, a positive integer or 'auto' (got {chunk_rows!r})")
    return L.pad(c)


def sweep_chunk_plan(n_rows, chunk_rows):
    """The row ranges ``[(start, stop), ...]`` of ``n_rows`` rows in chunks of ``chunk_rows`` (a multiple of 128, from
    ``sweep_chunk_rows``); the last one may be ragged, and ``chunk_rows >= n_rows`` gives one chunk.  Host code."""
    n, c = int(n_rows), int(chunk_rows)
    if c < 1 or c % L.PAD:
        raise ValueError(f"chunk_rows must be a positive multiple of {L.PAD} (got {chunk_rows})")
    return [(a, min(a + c, n)) for a in range(0, n, c)]


def label_stats_blocks(n_query_chunks, n_corpus_chunks=None):
    """The blocks ``[(a, b, self_mode), ...]`` a chunked ``label_similarity_stats`` sweeps, in the order their sums are added.
    Without candidates (``n_corpus_chunks=None``) the pairs are ``j < i`` of one operand: per query chunk ``a`` the blocks
    ``b < a`` in full (every pair of an earlier chunk lies below the diagonal), then the diagonal block ``(a, a)`` in self mode;
    the blocks ``b > a`` hold no pair and are skipped.  With candidates every ``(a, b)``.  Host code."""
    if n_corpus_chunks is None:
        return [(a, b, b == a) for a in range(int(n_query_chunks)) for b in range(a + 1)]
    return [(a, b, False) for a in range(int(n_query_chunks)) for b in range(int(n_corpus_chunks))]


class SweepOperand:
    """One operand of a sweep, in the form it came in (``_device.container``).  ``dense()`` is the whole operand as one device
    matrix, for the one-shot entries.  For a chunked sweep a scipy.sparse matrix goes up as canonical CSR (``csr``: duplicates
    summed, column ids ascending; uploaded once, at its first use -- no dense array of it exists on either side), a CUDA tensor
    stays as it is, and anything else is a host float32 array whose row slices go up chunk by chunk; ``image`` writes the
    normalised operand image of the rows ``[a0, a1)`` (``dae_sweep_image_csr`` / ``dae_sweep_image_dense``).  ``uploaded`` counts
    the bytes the chunked form has sent to the device."""

    def __init__(self, torch, data, dev):
        self.dev, self.X, self.host, self.uploaded, self._csr = dev, None, None, 0, None
        self.kind, self._m = container(torch, data)
        self.shape = (int(self._m.shape[0]), int(self._m.shape[1]))
        if self.kind == "tensor":
            X = self._m.to(device=dev, dtype=torch.float32)
            self.X = self._m = X if X.stride(1) == 1 or X.shape[1] <= 1 else X.contiguous()
        elif self.kind == "array":
            self.host = self._m

    def dense(self, torch):
        return dense_on_device(torch, self.kind, self._m, self.dev)

    @property
    def csr(self):
        """``(indptr int64, indices int32, data float32)`` on the device, or None for a dense operand."""
        if self._csr is None and self.kind == "scipy":
            m = self._m
            m.sum_duplicates()
            m.sort_indices()
            parts = tuple(np.ascontiguousarray(p) for p in (m.indptr.astype(np.int64), m.indices.astype(np.int32),
                                                            m.data.astype(np.float32, copy=False)))
            self.uploaded = sum(max(p.nbytes, p.itemsize) for p in parts)
            self._csr = tuple(upload(p, self.dev) for p in parts)
        return self._csr

    def image(self, torch, a0, a1, image_p, image_bytes, nm):
        import ctypes
        rows, D = a1 - a0, self.shape[1]
        if self.csr is not None:
            ip, ix, vl = self.csr
            L.call("dae_sweep_image_csr", ctypes.c_void_p(ip.data_ptr() + 8 * a0), L.ptr(ix), L.ptr(vl), rows, D, *nm, image_p, image_bytes,
                   L.current_stream())
            return
        if self.X is not None:
            X = self.X[a0:a1]
        else:
            X = torch.from_numpy(np.ascontiguousarray(self.host[a0:a1])).to(self.dev)
            self.uploaded += X.numel() * 4
        L.call("dae_sweep_image_dense", L.ptr(X), max(int(X.stride(0)), D), rows, D, *nm, image_p, image_bytes, L.current_stream())


def sweep_start(in_df, candidates, norm, metric, device, chunked=False):
    """What ``most_similar``, ``target_ranks``, ``similar_pairs`` and ``label_similarity_stats`` start with: ``norm`` / ``metric``
    checked, the library, the device, and the two operands (None for the second: the corpus is ``in_df`` itself) -- as device
    matrices, or with ``chunked`` as ``SweepOperand``, which must then hold rows, candidates and columns.  Returns ``(torch, lib,
    dev, Q, C, Nq, Nc, D, nm)``; ``nm`` are the two integers of ``norm_metric``."""
    nm = norm_metric(norm, metric)
    torch, lib, dev = device_and_library(device)
    Q = SweepOperand(torch, in_df, dev)
    C = None if candidates is None else SweepOperand(torch, candidates, dev)
    Nq, D = Q.shape
    if C is not None and C.shape[1] != D:
        raise ValueError(f"candidates have {C.shape[1]} columns, in_df has {D}")
    Nc = Nq if C is None else C.shape[0]
    if chunked and (Nq < 1 or Nc < 1 or D < 1):
        raise ValueError(f"a chunked sweep needs rows, candidates and columns (got {Nq} x {D} against {Nc} candidates)")
    if not chunked:
        Q, C = Q.dense(torch), None if C is None else C.dense(torch)
    return torch, lib, dev, Q, C, Nq, Nc, D, nm


def _most_similar_chunked(in_df, candidates, k, norm, metric, flt, chunk_rows, return_tensor, device):
    """``most_similar(chunk_rows=...)``: the outer loop walks the query chunks with one image and one carry (each row's running
    top-k as sorted 64-bit keys), the inner loop the corpus chunks with a second image; ``dae_topk_images`` merges a corpus chunk
    into the carry.  In self mode the diagonal block reuses the query image."""
    import ctypes
    torch, lib, dev, Qo, Co, Nq, Nc, D, nm = sweep_start(in_df, candidates, norm, metric, device, chunked=True)
    k = int(k)
    c = sweep_chunk_rows(chunk_rows, D)
    idx = torch.empty((Nq, max(k, 1)), dtype=torch.int32, device=dev)
    score = torch.empty((Nq, max(k, 1)), dtype=torch.float32, device=dev)
    xp, xi = flt.lists(Nq, Nc)
    xp_d, xi_d = (None, None) if xp is None else (torch.from_numpy(xp).to(dev), upload(xi, dev))
    cq, cc = min(c, L.pad(Nq)), min(c, L.pad(Nc))
    qb, cb = int(lib.dae_sweep_image_bytes(cq, D)), int(lib.dae_sweep_image_bytes(cc, D))
    q_p, q_t = workspace(dev, qb)
    c_p, c_t = workspace(dev, cb)
    carry_p, carry = workspace(dev, int(lib.dae_topk_carry_bytes(cq, max(k, 1))))
    q_plan, c_plan = sweep_chunk_plan(Nq, c), sweep_chunk_plan(Nc, c)
    # a ragged last chunk has fewer query tiles and may get MORE corpus slices than a full one: size the workspace for every block shape
    ws_bytes = max(int(lib.dae_topk_images_workspace(nq, nc, max(k, 1))) for nq in {q_plan[0][1], q_plan[-1][1] - q_plan[-1][0]}
                   for nc in {c_plan[0][1], c_plan[-1][1] - c_plan[-1][0]})
    ws_p, ws = workspace(dev, ws_bytes)
    with torch.cuda.device(dev):
        for q0, q1 in q_plan:
            Qo.image(torch, q0, q1, q_p, qb, nm)
            carry.zero_()                                             # all-zero bytes: an empty carry
            for c0, c1 in c_plan:
                diag = Co is None and c0 == q0
                if not diag:
                    (Qo if Co is None else Co).image(torch, c0, c1, c_p, cb, nm)
                L.call("dae_topk_images", q_p, q1 - q0, q0, None if diag else c_p, c1 - c0, c0, D, k, 1 if flt.exclude_self else 0,
                       None if xp_d is None else ctypes.c_void_p(xp_d.data_ptr() + 8 * q0), L.ptr(xi_d), carry_p,
                       ctypes.c_void_p(idx.data_ptr() + 4 * q0 * idx.stride(0)), ctypes.c_void_p(score.data_ptr() + 4 * q0 * score.stride(0)),
                       idx.stride(0), ws_p, ws_bytes, L.current_stream())
    del q_t, c_t, ws
    return result((idx.long(), score), return_tensor)

def normalize_exclusions(exclude, n_rows, n_candidates):
    """The exclusion lists of ``most_similar`` / ``recommend`` in the form ``dae_topk_similarity_ex`` reads: ``(indptr int64
    [n_rows + 1], items int32)``, every row's items ascending and unique, indices outside ``[0, n_candidates)`` dropped.
    ``exclude``: a list of ``n_rows`` index sequences or an ``(indptr, items)`` tuple.  Host code."""
    indptr, items = csr_lists(exclude, "exclude")
    if indptr.size - 1 != int(n_rows):
        raise ValueError(f"exclude has {indptr.size - 1} rows for {int(n_rows)} queries")
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("exclude must hold integer indices")
    items = items.astype(np.int64)
    rows = np.repeat(np.arange(int(n_rows), dtype=np.int64), np.diff(indptr))
    ok = (items >= 0) & (items < int(n_candidates))
    keys = np.unique(rows[ok] * int(n_candidates) + items[ok])          # sorted by row, then item; duplicates gone
    out_ptr = np.zeros(int(n_rows) + 1, dtype=np.int64)
    if int(n_candidates) > 0:
        out_ptr[1:] = np.cumsum(np.bincount(keys // int(n_candidates), minlength=int(n_rows)))
        return out_ptr, (keys % int(n_candidates)).astype(np.int32)
    return out_ptr, np.zeros(0, dtype=np.int32)


def normalize_shared_exclusions(exclude_shared, n_rows, n_candidates):
    """The shared stamped lists of ``most_similar`` / ``target_ranks`` (``exclude_shared=``) in the form ``dae_topk_similarity_seq``
    reads: ``(indptr int64 [n_lists + 1], items int32, stamps int32, row_list int32 [n_rows], row_limit int32 [n_rows])``.
    ``exclude_shared``: ``(lists, stamps, row_list, row_limit)`` -- ``lists`` a list of index sequences or an ``(indptr, items)``
    tuple, every list ascending and unique with items in ``[0, n_candidates)``; ``stamps`` one integer per item (flat, or in the
    layout of ``lists``); ``row_list`` / ``row_limit`` one integer per query row (a ``row_list`` outside ``[0, n_lists)``: no
    list).  ``ValueError`` for anything else -- the kernel's lookup is a binary search, so the order is checked here.  Host code."""
    if not (isinstance(exclude_shared, (tuple, list)) and len(exclude_shared) == 4):
        raise ValueError("exclude_shared must be (lists, stamps, row_list, row_limit)")
    lists, stamps, row_list, row_limit = exclude_shared
    indptr, items = csr_lists(lists, "exclude_shared")
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("exclude_shared must hold integer indices")
    items = items.astype(np.int64)
    st = csr_lists(stamps, "exclude_shared stamps")[1] if isinstance(stamps, (tuple, list)) else np.asarray(stamps).ravel()
    if st.shape[0] != items.shape[0]:
        raise ValueError(f"{st.shape[0]} stamps for {items.shape[0]} list items")
    if st.size and st.dtype.kind not in "iu":
        raise ValueError("exclude_shared stamps must be integers")
    if items.size and (int(items.min()) < 0 or int(items.max()) >= int(n_candidates)):
        raise ValueError(f"exclude_shared items must be in 0..{int(n_candidates) - 1} (got {int(items.min())}..{int(items.max())})")
    if items.size > 1:
        inner = np.ones(items.size - 1, dtype=bool)
        starts = indptr[1:-1]
        inner[starts[(starts > 0) & (starts < items.size)] - 1] = False     # the step from one list to the next
        if (np.diff(items)[inner] <= 0).any():
            raise ValueError("every list of exclude_shared must be ascending and unique")
    out = []
    for name, r in (("row_list", row_list), ("row_limit", row_limit)):
        if hasattr(r, "detach"):
            r = r.detach().cpu().numpy()
        r = np.asarray(r).ravel()
        if r.shape[0] != int(n_rows):
            raise ValueError(f"exclude_shared {name} has {r.shape[0]} entries for {int(n_rows)} queries")
        if r.size and r.dtype.kind not in "iu":
            raise ValueError(f"exclude_shared {name} must hold integers")
        out.append(np.ascontiguousarray(np.clip(r.astype(np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32)))
    st = np.clip(st.astype(np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    return indptr, np.ascontiguousarray(items.astype(np.int32)), np.ascontiguousarray(st), out[0], out[1]


def normalize_window(window, n_rows, n_candidates):
    """The candidate windows of ``most_similar`` / ``recommend`` / ``target_ranks`` in the form ``dae_topk_similarity_win``
    reads: ``(lo int32 [n_rows], hi int32 [n_rows])``.  ``window``: a pair ``(lo, hi)`` of integer sequences, one entry per query
    row; row i admits the candidates ``lo[i] <= j < hi[i]`` (``lo == hi``: none).  ``ValueError`` for anything else: a wrong
    length, non-integers, ``lo < 0``, ``hi > n_candidates`` or ``lo > hi``.  Host code."""
    if not (isinstance(window, (tuple, list)) and len(window) == 2):
        raise ValueError("window must be a pair (lo, hi) of integer sequences, one entry per query row")
    out = []
    for name, w in zip(("lo", "hi"), window):
        if hasattr(w, "detach"):
            w = w.detach().cpu().numpy()
        w = np.asarray(w).ravel()
        if w.shape[0] != int(n_rows):
            raise ValueError(f"window {name} has {w.shape[0]} entries for {int(n_rows)} queries")
        if w.size and w.dtype.kind not in "iu":
            raise ValueError("window must hold integer indices")
        out.append(w.astype(np.int64))
    lo, hi = out
    if lo.size and int(lo.min()) < 0:
        raise ValueError(f"window lo must not be negative (got {int(lo.min())})")
    if hi.size and int(hi.max()) > int(n_candidates):
        raise ValueError(f"window hi must not exceed the {int(n_candidates)} candidates (got {int(hi.max())})")
    if (lo > hi).any():
        i = int(np.flatnonzero(lo > hi)[0])
        raise ValueError(f"window lo must not exceed hi (row {i}: {int(lo[i])} > {int(hi[i])})")
    return np.ascontiguousarray(lo.astype(np.int32)), np.ascontiguousarray(hi.astype(np.int32))


def _window_order(lo, hi):
    """The stable order of the query rows by ``(lo, hi)``, or None when they are in that order already: neighbours with similar
    windows make the union of a 128-row query tile narrow, and the union is what the kernel walks."""
    perm = np.lexsort((hi, lo))
    return None if (perm == np.arange(perm.size)).all() else perm


def permute_histories(indptr, items, perm):
    """The CSR ``(indptr, items)`` -- histories, exclusion lists -- with its rows in the order ``perm``, which may also be a
    subset of them.  Host code."""
    n = np.diff(indptr)[perm]
    out_ptr = np.zeros(perm.size + 1, dtype=np.int64)
    out_ptr[1:] = np.cumsum(n)
    take = np.repeat(indptr[:-1][perm] - out_ptr[:-1], n) + np.arange(int(out_ptr[-1]), dtype=np.int64)
    return out_ptr, items[take]


class _RowFilter:
    """Which candidates may compete in which query row -- the part ``most_similar`` and ``target_ranks`` share: ``exclude_self``,
    the per-row lists ``(xp, xi)`` of ``normalize_exclusions`` or the shared stamped lists ``shared`` of
    ``normalize_shared_exclusions``, and the pair ``window`` of ``normalize_window`` (each None: no such term), all in the caller's
    row order.  ``place`` hands them to the device, ``entry`` / ``args`` are then the suffix of the entry point that takes them and
    its arguments from ``exclude_self`` to ``win_hi``, and ``restore`` puts a result back in the caller's order."""

    def __init__(self, exclude_self, window, shared, exclude):
        self.exclude_self, self.window, self.shared, self.exclude = bool(exclude_self), window, shared, exclude
        self.xp = self.xi = self.perm_d = None

    def lists(self, Nq, Nc):
        """``(xp, xi)``; a raw ``exclude`` is normalised at the first call, i.e. where its errors have always been raised: behind the
        checks of the operands (and of the targets)."""
        if self.exclude is not None:
            (self.xp, self.xi), self.exclude = normalize_exclusions(self.exclude, Nq, Nc), None
        return self.xp, self.xi

    def place(self, Q, Cm, dev, *per_row):
        """Uploads the filter.  With windows and ``candidates`` (``Cm``) the rows go in the stable order of ``(lo, hi)``
        (``_window_order``): returns ``Q`` and the ``per_row`` device tensors in the order the kernel gets them."""
        import torch
        xp, xi = self.lists(int(Q.shape[0]), int(Q.shape[0]) if Cm is None else int(Cm.shape[0]))
        shared, lo_d, hi_d = self.shared, None, None
        if self.window is not None:
            wlo, whi = self.window
            perm = None if Cm is None else _window_order(wlo, whi)    # the corpus is Q itself: its rows stay where they are
            if perm is not None:
                self.perm_d = torch.from_numpy(perm).to(dev)
                Q, wlo, whi = Q[self.perm_d].contiguous(), wlo[perm], whi[perm]
                per_row = tuple(t[self.perm_d].contiguous() for t in per_row)
                if xp is not None:
                    xp, xi = permute_histories(xp, xi, perm)
                if shared is not None:
                    shared = shared[:3] + (np.ascontiguousarray(shared[3][perm]), np.ascontiguousarray(shared[4][perm]))
            lo_d, hi_d = torch.from_numpy(np.ascontiguousarray(wlo)).to(dev), torch.from_numpy(np.ascontiguousarray(whi)).to(dev)
        if shared is not None:
            d = tuple(upload(a, dev) for a in shared)
            self.entry, lists = "_seq", (L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), int(shared[0].size - 1), L.ptr(d[3]), L.ptr(d[4]))
        else:
            d = (upload(xp, dev), upload(xi, dev))
            self.entry, lists = "_win", (L.ptr(d[0]), L.ptr(d[1]))
        self._device = (d, lo_d, hi_d)                                # the pointers in args stay valid as long as the filter lives
        self.args = (1 if self.exclude_self else 0,) + lists + (L.ptr(lo_d), L.ptr(hi_d))
        return (Q,) + per_row

    def restore(self, *outs):
        """Per-row device results of a call on the rows of ``place``, in the caller's row order."""
        import torch
        if self.perm_d is None:
            return outs
        return tuple(torch.empty_like(t).index_copy_(0, self.perm_d, t) for t in outs)


def _row_filter(in_df, candidates, exclude_self, exclude, exclude_shared, window):
    """The ``_RowFilter`` of the arguments of ``most_similar`` / ``target_ranks``: the default and the error of ``exclude_self``,
    ``exclude`` against ``exclude_shared``, and ``window`` / ``exclude_shared`` normalised -- all before the library is touched."""
    if exclude_self is None:
        exclude_self = candidates is None
    elif exclude_self and candidates is not None:
        raise ValueError("exclude_self=True needs candidates=None (the self pair exists only when the corpus is in_df itself)")
    if exclude is not None and exclude_shared is not None:
        raise ValueError("exclude and exclude_shared do not go together")
    n = lambda: (row_count(in_df), row_count(in_df if candidates is None else candidates))      # noqa: E731
    return _RowFilter(exclude_self, None if window is None else normalize_window(window, *n()),
                      None if exclude_shared is None else normalize_shared_exclusions(exclude_shared, *n()), exclude)


def candidate_windows(query_times, publish_times, max_age=None):
    """Candidate windows of a news feed for a corpus in publication order: for a query at time ``t`` the articles with
    ``t - max_age < publish <= t`` (``max_age=None`` or ``inf``: everything published by ``t``), as the column range
    ``lo = searchsorted(publish, t - max_age, 'right')``, ``hi = searchsorted(publish, t, 'right')``.  A query before the first
    publication gets an empty window.  Returns ``(lo int32 [Nq], hi int32 [Nq])`` for ``window=``.  ``ValueError`` when
    ``publish_times`` decrease (order the corpus first), for non-finite times and for a negative ``max_age``.  Host code."""
    t = np.asarray(query_times, dtype=np.float64).ravel()
    pub = np.asarray(publish_times, dtype=np.float64).ravel()
    if not (np.isfinite(t).all() and np.isfinite(pub).all()):
        raise ValueError("query_times and publish_times must be finite")
    if (np.diff(pub) < 0).any():
        raise ValueError("publish_times decrease: a window is a column range only for a corpus in publication order -- reorder "
                         "the articles by np.argsort(publish_times, kind='stable') first")
    hi = np.searchsorted(pub, t, side="right")
    if max_age is None:
        lo = np.zeros_like(hi)
    else:
        age = float(max_age)
        if not age >= 0.0:
            raise ValueError(f"max_age must not be negative (got {max_age})")
        lo = np.searchsorted(pub, t - age, side="right")                 # age == inf: t - age = -inf, lo = 0
    return lo.astype(np.int32), hi.astype(np.int32)


def most_similar(in_df, k=10, norm="", metric="cosine", exclude_self=None, candidates=None, *, exclude=None, exclude_shared=None,
                 window=None, chunk_rows=None, return_tensor=False, device=None, dedup_threshold=None, dedup_pool=None, dedup_norm="",
                 dedup_metric="cosine"):
    """The ``k`` most similar rows of ``candidates`` (default: ``in_df`` itself) for every row of ``in_df``, by the scores
    ``pairwise_similarity`` would give (same ``norm`` / ``metric``, same exact-fp32 products), without the N x N matrix:
    ``dae_topk_similarity`` keeps a running top-k per row inside the GEMM's epilogue.

    Both inputs take the containers of ``pairwise_similarity`` (ndarray, list, scipy.sparse, CUDA tensor).  ``exclude_self``
    (default: True without ``candidates``, False with them) drops each row's own index -- unlike ``set_diagonal_zero``, which
    keeps the self pair at score 0.  Rows are ordered by score descending, ties by index ascending; with fewer than ``k``
    candidates the tail is index -1, score -inf.  1 <= k <= 128.  Returns ``(indices int64 [N x k], scores float32 [N x k])``
    as ndarrays, or as CUDA tensors with ``return_tensor=True``.

    ``exclude`` (default None: nothing) names, per query row, candidates that must not be returned -- a list of index sequences
    or an ``(indptr, items)`` tuple; it is sorted, de-duplicated and stripped of indices outside the corpus here
    (``normalize_exclusions``).  An excluded candidate is skipped before it can take one of the k slots
    (``dae_topk_similarity_ex``), so a row still gets k results when k others exist.  Allowed together with ``exclude_self``.

    ``window`` (default None: every candidate) is a pair ``(lo, hi)`` of integer sequences, one entry per query row: row i
    admits only the candidates ``lo[i] <= j < hi[i]`` (``normalize_window``; e.g. from ``candidate_windows``), on top of
    ``exclude`` and ``exclude_self`` (``dae_topk_similarity_win``).  An empty window gives a row of -1 / -inf.  The kernel walks
    the union of the windows of 128 neighbouring rows, so with ``candidates`` the rows are handed over in the stable order of
    ``(lo, hi)`` and the result is put back in the caller's order; the order is total, so the result does not depend on it.

    ``exclude_shared = (lists, stamps, row_list, row_limit)`` (instead of ``exclude``) is the form for query rows that are the
    successive states of one user: one list per USER with a stamp per item (``click_prefix_lists``), and per query row the list
    it reads and its stamp limit (``every_click_rows``); row i skips the items of list ``row_list[i]`` whose stamp is at most
    ``row_limit[i]`` (``normalize_shared_exclusions``, ``dae_topk_similarity_seq``).  The result equals, bit for bit, that of
    ``exclude`` with those items listed row by row.

    ``chunk_rows`` (default None: both operands whole, as dense fp32 images -- each must stay below 4 GiB) sweeps the operands a
    bounded number of rows at a time: an integer (rounded up to a multiple of 128) or ``"auto"`` (``sweep_chunk_rows``).  A
    scipy.sparse input then goes to the device once, as CSR, and its images are built chunk by chunk straight from the CSR rows
    (``dae_sweep_image_csr``); dense inputs are cut into row slices.  Each row's running top-k is carried from one corpus chunk
    to the next (``dae_topk_images``), and the result equals that of ``chunk_rows=None`` bit for bit.  ``exclude_self`` and
    ``exclude`` are supported; ``window`` or ``exclude_shared`` with ``chunk_rows`` is a ``ValueError``.

    ``dedup_threshold`` (default None: the call is what it was) de-duplicates every row: ``dedup_pool`` candidates (default
    ``min(128, 4 * k)``; ``k <= dedup_pool <= 128``) are retrieved with every filter above, and ``dedup_lists`` walks them down
    to ``k`` -- a candidate is skipped when its ``dedup_norm`` / ``dedup_metric`` similarity (default cosine) to a candidate
    already selected reaches the threshold.  The scores returned are the retrieval's; a row whose pool runs out ends in -1 / -inf.
    ``chunk_rows`` with ``dedup_threshold`` is a ``ValueError``."""
    if chunk_rows is not None and (window is not None or exclude_shared is not None):
        raise ValueError("chunk_rows does not go with window= or exclude_shared= (the chunked sweep takes exclude_self and exclude only)")
    if dedup_threshold is not None:
        k = int(k)
        pool = min(128, 4 * k) if dedup_pool is None else int(dedup_pool)
        if chunk_rows is not None:
            raise ValueError("chunk_rows does not go with dedup_threshold=")
        if pool < k or pool > 128:
            raise ValueError(f"dedup_pool must be in k..128 = {k}..128 (got {pool})")
        torch, _, dev = device_and_library(device)
        corpus = device_matrix(torch, in_df if candidates is None else candidates, dev)      # once, for both calls
        idx, score = most_similar(corpus if candidates is None else in_df, pool, norm, metric, exclude_self, None if candidates is None else corpus,
                                  exclude=exclude, exclude_shared=exclude_shared, window=window, return_tensor=True, device=device)
        return dedup_lists(idx, corpus, k, dedup_threshold, scores=score, norm=dedup_norm, metric=dedup_metric, return_tensor=return_tensor,
                           device=device)
    flt = _row_filter(in_df, candidates, exclude_self, exclude, exclude_shared, window)
    if chunk_rows is not None:
        return _most_similar_chunked(in_df, candidates, k, norm, metric, flt, chunk_rows, return_tensor, device)
    torch, lib, dev, Q, Cm, Nq, Nc, D, nm = sweep_start(in_df, candidates, norm, metric, device)
    k = int(k)
    idx = torch.empty((Nq, max(k, 1)), dtype=torch.int32, device=dev)
    score = torch.empty((Nq, max(k, 1)), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.dae_topk_similarity_workspace(Nq, Nc, D, k))
    ws_p, ws = workspace(dev, ws_bytes)
    (Q,) = flt.place(Q, Cm, dev)
    if Nq > 0 or (flt.window is None and flt.shared is None):         # without rows only the windowed and the shared call are skipped
        with torch.cuda.device(dev):
            L.call("dae_topk_similarity" + flt.entry, L.ptr(Q), Q.stride(0), Nq, L.ptr(Cm), 0 if Cm is None else Cm.stride(0), Nc, D,
                   *nm, k, *flt.args, L.ptr(idx), L.ptr(score), idx.stride(0), ws_p, ws_bytes, L.current_stream())
    idx, score = flt.restore(idx, score)
    return result((idx.long(), score), return_tensor)


def dedup_lists(indices, embeddings, k, threshold, *, scores=None, norm="", metric="cosine", return_counts=False, return_tensor=False,
                device=None):
    """Greedy de-duplication of recommendation lists on the device (``dae_dedup_lists``).  ``indices`` ``[Nr x L]`` (ndarray or
    CUDA tensor, ``L <= 128``) holds per row candidate rows of ``embeddings``, best first, as ``most_similar`` returns them.
    Each row is walked front to back: a candidate is kept iff no candidate kept before it scores ``>= threshold`` against it,
    by the score ``pairwise_similarity(embeddings, norm, metric)`` gives the two (same normalisation, same exact-fp32
    products); the walk stops after ``k`` kept (``1 <= k <= L``).  Entries < 0 or past the last row of ``embeddings`` are
    skipped.  An index that occurs twice in a row is, under cosine, a duplicate of itself.

    Returns ``(indices int64 [Nr x k], scores)``: the kept candidates in the row's order, -1 where fewer than ``k`` survive;
    ``scores`` (``[Nr x L]``, e.g. the relevance ``most_similar`` returned) are gathered alongside as float32 ``[Nr x k]``
    with a tail of -inf, or None when not given.  With ``return_counts`` a third item ``(n_kept, n_dup_pairs_topk)`` (int64
    ``[Nr]`` each): how many were kept, and how many pairs among the first ``min(k, L)`` candidates reach the threshold -- the
    duplicate pairs the plain top-k would have shown.  ndarrays, or CUDA tensors with ``return_tensor=True``."""
    nm = norm_metric(norm, metric)
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    shape = tuple(indices.shape) if hasattr(indices, "shape") else np.asarray(indices).shape
    if len(shape) != 2:
        raise ValueError("indices must be [n_rows x L]")
    Nr, Ll = int(shape[0]), int(shape[1])
    k = int(k)
    if Ll > 128:
        raise ValueError(f"a list holds at most 128 candidates (got {Ll})")
    if k < 1 or k > Ll:
        raise ValueError(f"k must be in 1..L = 1..{Ll} (got {k})")
    if scores is not None and tuple(scores.shape) != (Nr, Ll):
        raise ValueError(f"scores must have the shape of indices {(Nr, Ll)} (got {tuple(scores.shape)})")
    torch, lib, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev)
    Na, D = int(E.shape[0]), int(E.shape[1])
    lists = _list_table(torch, indices, dev)
    out_idx = torch.empty((Nr, k), dtype=torch.int32, device=dev)
    out_pos = torch.empty((Nr, k), dtype=torch.int32, device=dev)
    counts = torch.empty((Nr, 2), dtype=torch.int32, device=dev)
    if Nr > 0:
        if Na == 0:
            raise ValueError("embeddings has no rows")
        ws_bytes = int(lib.dae_dedup_lists_workspace(Nr, Na, D, Ll))
        ws_p, ws = workspace(dev, ws_bytes)
        with torch.cuda.device(dev):
            L.call("dae_dedup_lists", L.ptr(E), E.stride(0), Na, D, *nm, L.ptr(lists), lists.stride(0), Nr, Ll, k, threshold, L.ptr(out_idx),
                   L.ptr(out_pos), out_idx.stride(0), L.ptr(counts), ws_p, ws_bytes, L.current_stream())
    out_s = None
    if scores is not None:
        s = scores.to(device=dev, dtype=torch.float32) if isinstance(scores, torch.Tensor) else \
            torch.as_tensor(np.asarray(scores, dtype=np.float32)).to(dev)
        pos = out_pos.long()
        out_s = torch.gather(s, 1, pos.clamp(min=0)).masked_fill(pos < 0, float("-inf"))
    out = (out_idx.long(), out_s)
    if return_counts:
        out = out + ((counts[:, 0].long(), counts[:, 1].long()),)
    return result(out, return_tensor)


def _list_table(torch, indices, dev):
    """The int32 device table of a ``[Nr x L]`` index container (an index beyond int32 is beyond every corpus)."""
    if isinstance(indices, torch.Tensor):
        lists = indices.to(device=dev)
    else:
        lists = torch.as_tensor(np.ascontiguousarray(np.asarray(indices))).to(dev)
    return lists.clamp(min=-1, max=torch.iinfo(torch.int32).max).to(torch.int32).contiguous()


def diversify_lists(indices, relevance, embeddings, k, lam=0.7, *, labels=None, max_per_label=None, dedup_threshold=None, norm="",
                    metric="cosine", scale_relevance=None, return_details=False, return_tensor=False, device=None):
    """Re-ranks recommendation lists for diversity on the device (``dae_mmr_lists``): Maximal Marginal Relevance, optionally with
    the de-dup rule and a cap on the articles of one label.  ``indices`` ``[Nr x L]`` (ndarray or CUDA tensor, ``L <= 128``) holds
    per row candidate rows of ``embeddings``, ``relevance`` (same shape) one relevance each -- normally what ``most_similar`` /
    ``recommend`` returned; no order is assumed.  An entry < 0, past the last row of ``embeddings`` or with a non-finite relevance
    is never selected.  Each of at most ``k`` steps (``1 <= k <= L``) selects the candidate with the largest
    ``lam * relevance - (1 - lam) * max(0, similarity to the nearest article already selected)`` (both products and the difference
    rounded to float32 one by one; equal values: the lowest position), the similarity that of
    ``pairwise_similarity(embeddings, norm, metric)``.  ``0 <= lam <= 1``: 1 is the stable sort by relevance, 0 looks at relevance
    for the first pick alone.  ``dedup_threshold`` (default None: off) also drops every candidate whose similarity to a selected
    article reaches it, as ``dedup_lists`` does; ``max_per_label`` (default None: off; needs ``labels``, one integer per row of
    ``embeddings``) lets at most that many articles of one label into a list -- labels < 0 are never capped.

    ``scale_relevance="minmax"`` first rescales each row's relevances (the finite ones of entries inside the corpus) to ``[0, 1]``
    in float32, ``(rel - min) / (max - min)``, a row with ``max == min`` to all 1: the inner product is unbounded while the
    similarity penalty lives in ``[0, 1]``.

    Returns ``(indices int64 [Nr x k], relevance float32 [Nr x k])`` in selection order: the selected articles, -1 where the
    row ran out, and the CALLER's relevance of each, tail -inf.  With ``return_details`` a third item, a dict: ``positions`` (in
    the input row), ``value`` (the criterion at selection), ``nearest`` (the similarity penalty at selection: 0 for the first
    pick), ``n_selected``, ``n_beyond_topk`` (how many of a row's selected are not among its first ``k`` valid entries) and
    ``relevance_used`` (``[Nr x L]``, what the rule saw).  ndarrays, or CUDA tensors with ``return_tensor=True``."""
    nm = norm_metric(norm, metric)
    shape = tuple(indices.shape) if hasattr(indices, "shape") else np.asarray(indices).shape
    if len(shape) != 2:
        raise ValueError("indices must be [n_rows x L]")
    Nr, Ll = int(shape[0]), int(shape[1])
    rshape = tuple(relevance.shape) if hasattr(relevance, "shape") else np.asarray(relevance).shape
    if rshape != (Nr, Ll):
        raise ValueError(f"relevance must have the shape of indices {(Nr, Ll)} (got {rshape})")
    k = int(k)
    if Ll > 128:
        raise ValueError(f"a list holds at most 128 candidates (got {Ll})")
    if k < 1 or k > Ll:
        raise ValueError(f"k must be in 1..L = 1..{Ll} (got {k})")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:                                             # (false for NaN)
        raise ValueError(f"lam must be in [0, 1] (got {lam})")
    threshold = float("inf") if dedup_threshold is None else float(dedup_threshold)
    if threshold != threshold:
        raise ValueError("dedup_threshold is NaN")
    Na, D = matrix_shape(embeddings)
    cap = 0
    if max_per_label is not None:
        cap = int(max_per_label)
        if cap < 1:
            raise ValueError(f"max_per_label must be at least 1 (got {max_per_label})")
        if labels is None:
            raise ValueError("max_per_label needs labels")
    if labels is not None and row_count(labels) < Na:
        raise ValueError(f"labels must hold one entry per row of embeddings ({Na}; got {row_count(labels)})")
    if scale_relevance not in (None, "minmax"):
        raise ValueError(f"scale_relevance must be None or 'minmax' (got {scale_relevance!r})")
    torch, lib, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev)
    lists = _list_table(torch, indices, dev)
    rel = relevance.to(device=dev, dtype=torch.float32) if isinstance(relevance, torch.Tensor) else \
        torch.as_tensor(np.asarray(relevance, dtype=np.float32)).to(dev)
    rel = rel.contiguous()
    used = rel
    if scale_relevance == "minmax" and Nr > 0:
        ok = (lists >= 0) & (lists < Na) & torch.isfinite(rel)
        inf = float("inf")
        lo = rel.masked_fill(~ok, inf).amin(dim=1, keepdim=True)
        hi = rel.masked_fill(~ok, -inf).amax(dim=1, keepdim=True)
        flat = hi == lo
        used = torch.where(ok, torch.where(flat, torch.ones_like(rel), (rel - lo) / (hi - lo).masked_fill(flat, 1.0)), rel).contiguous()
    lab = None
    if labels is not None:
        lab = labels.to(device=dev) if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels)).to(dev)
        lab = lab.reshape(-1).clamp(min=-1, max=torch.iinfo(torch.int32).max).to(torch.int32).contiguous()
    out_idx = torch.empty((Nr, k), dtype=torch.int32, device=dev)
    out_pos = torch.empty((Nr, k), dtype=torch.int32, device=dev)
    out_val = torch.empty((Nr, k), dtype=torch.float32, device=dev)
    out_near = torch.empty((Nr, k), dtype=torch.float32, device=dev)
    counts = torch.empty((Nr, 2), dtype=torch.int32, device=dev)
    if Nr > 0:
        if Na == 0:
            raise ValueError("embeddings has no rows")
        ws_bytes = int(lib.dae_mmr_lists_workspace(Nr, Na, D, Ll))
        ws_p, ws = workspace(dev, ws_bytes)
        with torch.cuda.device(dev):
            L.call("dae_mmr_lists", L.ptr(E), E.stride(0), Na, D, *nm, L.ptr(lists), lists.stride(0), L.ptr(used), used.stride(0), L.ptr(lab),
                   cap, Nr, Ll, k, lam, threshold, L.ptr(out_idx), L.ptr(out_pos), L.ptr(out_val), L.ptr(out_near), out_idx.stride(0),
                   L.ptr(counts), ws_p, ws_bytes, L.current_stream())
    pos = out_pos.long()
    out_r = torch.gather(rel, 1, pos.clamp(min=0)).masked_fill(pos < 0, float("-inf"))
    out = result((out_idx.long(), out_r), return_tensor)
    if return_details:
        details = {"positions": pos, "value": out_val, "nearest": out_near, "n_selected": counts[:, 0].long(),
                   "n_beyond_topk": counts[:, 1].long(), "relevance_used": used}
        out = out + ({name: result(t, return_tensor) for name, t in details.items()},)
    return out


def shared_row_chunks(n, max_pairs=1 << 22):
    """Row ranges ``[a, b)`` whose list lengths ``n`` sum to about ``max_pairs``: the O(sum of L^2) host work goes chunk by chunk."""
    total = np.concatenate([[0], np.cumsum(n)])
    a = 0
    while a < n.size:
        b = max(int(np.searchsorted(total, total[a] + max_pairs, side="right")) - 1, a + 1)
        yield a, min(b, n.size)
        a = min(b, n.size)


def shared_pairs(lp, row_list, a, b):
    """For the query rows ``[a, b)``: every (row, item of the row's shared list) pair as ``(rows int64, places int64)``, ``places``
    pointing into the lists' item / stamp arrays."""
    u = row_list[a:b].astype(np.int64)
    ok = (u >= 0) & (u < lp.size - 1)
    us = np.where(ok, u, 0)
    n = np.where(ok, lp[us + 1] - lp[us], 0)
    start = np.concatenate([[0], np.cumsum(n)])
    rows = np.repeat(np.arange(a, b, dtype=np.int64), n)
    places = np.repeat(lp[us] - start[:-1], n) + np.arange(int(start[-1]), dtype=np.int64)
    return rows, places


def competitors(tgt, Nq, Nc, exclude_self, xp, xi, window, shared=None):
    """The host bookkeeping of ``target_ranks``: ``(n_cand int64 [Nq], barred bool [Nq])`` -- how many candidates compete in each
    row, the target included, and which targets can never be returned.  ``tgt``: int64 targets (negative: none); ``xp, xi``: the
    lists of ``normalize_exclusions`` or None; ``window``: the pair of ``normalize_window``, None meaning ``(0, Nc)`` for every row."""
    tgt = np.asarray(tgt, dtype=np.int64)
    me = np.arange(Nq, dtype=np.int64)
    if window is None:
        wlo, whi = np.zeros(Nq, dtype=np.int64), np.full(Nq, Nc, dtype=np.int64)
    else:
        wlo, whi = (np.asarray(w).astype(np.int64) for w in window)
    n_cand = whi - wlo
    barred = (tgt >= 0) & ~((tgt >= wlo) & (tgt < whi))              # outside its own window: never returned
    self_in = (me >= wlo) & (me < whi) if exclude_self else np.zeros(Nq, dtype=bool)
    if xp is not None:
        rows = np.repeat(me, np.diff(xp))
        it = xi.astype(np.int64)
        is_t = it == tgt[rows]
        barred[rows[is_t]] = True
        inside = (it >= wlo[rows]) & (it < whi[rows])
        n_cand -= np.bincount(rows[inside & ~is_t], minlength=Nq)
        self_in &= np.bincount(rows[(it == rows) & ~is_t], minlength=Nq) == 0      # unless the list took the self column already
    if shared is not None:                                            # the same bookkeeping for the shared stamped lists
        lp, li, ls, row_list, row_limit = shared
        u = row_list.astype(np.int64)
        has = (u >= 0) & (u < lp.size - 1)
        us = np.where(has, u, 0)
        lim = row_limit.astype(np.int64)
        key = np.repeat(np.arange(lp.size - 1, dtype=np.int64), np.diff(lp)) * max(Nc, 1) + li.astype(np.int64)      # ascending

        def listed(col):                                              # is column col[i] barred by row i's list?
            q = us * max(Nc, 1) + np.clip(col, 0, max(Nc - 1, 0))
            at = np.minimum(np.searchsorted(key, q), max(key.size - 1, 0))
            return has & (col >= 0) & (key[at] == q) & (ls[at] <= lim) if key.size else np.zeros(Nq, dtype=bool)
        t_listed = listed(tgt)
        barred |= t_listed
        if window is None:                                            # items up to the limit: one search in the lists' sorted stamps
            smin = int(ls.min()) if ls.size else 0
            span = (int(ls.max()) - smin + 2) if ls.size else 1
            skey = np.sort(np.repeat(np.arange(lp.size - 1, dtype=np.int64), np.diff(lp)) * span + (ls.astype(np.int64) - smin))
            n_list = np.where(has, np.searchsorted(skey, us * span + np.clip(lim - smin, -1, span - 2), side="right") - lp[us], 0)
            n_cand -= n_list - t_listed.astype(np.int64)
        else:
            n_in = np.diff(lp)[us] * has
            for a, b in shared_row_chunks(n_in):
                rows, places = shared_pairs(lp, row_list, a, b)
                it = li[places].astype(np.int64)
                take = (ls[places] <= lim[rows]) & (it >= wlo[rows]) & (it < whi[rows]) & (it != tgt[rows])
                n_cand[a:b] -= np.bincount(rows[take] - a, minlength=b - a)
        self_in &= ~(listed(me) & (me != tgt))                        # unless the list took the self column already
    if exclude_self:
        self_t = tgt == me
        barred |= self_t
        n_cand -= (self_in & ~self_t).astype(np.int64)                # the target is counted even there; the row is not ranked anyway
    return n_cand, barred


def target_ranks(in_df, targets, norm="", metric="cosine", exclude_self=None, candidates=None, *, exclude=None, exclude_shared=None,
                 window=None, return_tensor=False, device=None):
    """The position of one target row of ``candidates`` (default: ``in_df`` itself) per row of ``in_df`` among ALL candidates, by
    the scores and the order of ``most_similar`` (score descending, ties by index ascending), without the N x N matrix:
    ``dae_rank_similarity`` counts the candidates ahead of the target inside the GEMM's epilogue.

    Containers, ``norm``, ``metric``, ``exclude_self`` and ``exclude`` are those of ``most_similar``.  ``targets``: one
    candidate index per row, negative for "no target"; an index >= the number of candidates raises ``ValueError``.

    Returns ``(rank int64 [N], score float32 [N], n_candidates int64 [N])``.  ``rank`` counts from 1 among the candidates that
    ``most_similar`` with the same arguments could return, and ``score`` is the target's score there bit for bit, so for every
    k: ``0 < rank <= k`` exactly when the target is in ``most_similar(..., k, exclude=...)``'s row, at position ``rank - 1``.
    ``rank`` is 0 (``score`` is still the pair's score) for a target that can never be returned: one in its own row's
    ``exclude`` list, or the row itself under ``exclude_self``; and 0 with score -inf for a row without a target.
    ``n_candidates`` is the number of candidates competing in that row, the target included: the corpus size minus the row's
    exclusion items other than the target, minus the row itself when excluded (host code).  ndarrays, or CUDA tensors
    with ``return_tensor=True``.

    With ``window`` (a pair ``(lo, hi)`` as in ``most_similar``; ``dae_rank_similarity_win``) the competitors are the
    candidates inside the row's window, and the sentence about k above holds for ``most_similar(..., window=window)``: a target
    outside its row's window can never be returned and gets ``rank`` 0 (its ``score`` is still the pair's score), and
    ``n_candidates`` is the window's size minus the row's exclusion items inside the window other than the target, minus the
    row itself when it is excluded and lies inside.

    ``exclude_shared = (lists, stamps, row_list, row_limit)`` (instead of ``exclude``; ``dae_rank_similarity_seq``) is the shared
    stamped form of ``most_similar``: every sentence above holds with "row i's exclusion items" read as the items of list
    ``row_list[i]`` whose stamp is at most ``row_limit[i]``, and the result equals that of ``exclude`` with those items bit for
    bit."""
    flt = _row_filter(in_df, candidates, exclude_self, exclude, exclude_shared, window)
    torch, lib, dev, Q, Cm, Nq, Nc, D, nm = sweep_start(in_df, candidates, norm, metric, device)
    tgt = targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    tgt = tgt.ravel()
    if tgt.size and tgt.dtype.kind not in "iu":
        raise ValueError("targets must hold integer indices")
    tgt = tgt.astype(np.int64)
    if tgt.shape[0] != Nq:
        raise ValueError(f"{tgt.shape[0]} targets for {Nq} queries")
    if tgt.size and int(tgt.max()) >= Nc:
        raise ValueError(f"targets must be below {Nc} (got {int(tgt.max())})")
    n_cand, barred = competitors(tgt, Nq, Nc, flt.exclude_self, *flt.lists(Nq, Nc), flt.window, flt.shared)
    rank = torch.empty(Nq, dtype=torch.int32, device=dev)
    score = torch.empty(Nq, dtype=torch.float32, device=dev)
    if Nq == 0:
        return result((rank.long(), score, torch.from_numpy(n_cand).to(dev)), return_tensor)
    ws_bytes = int(lib.dae_rank_similarity_workspace(Nq, Nc, D))
    ws_p, ws = workspace(dev, ws_bytes)
    Q, t_d = flt.place(Q, Cm, dev, torch.from_numpy(np.where(tgt >= 0, tgt, -1).astype(np.int32)).to(dev))
    with torch.cuda.device(dev):
        L.call("dae_rank_similarity" + flt.entry, L.ptr(Q), Q.stride(0), Nq, L.ptr(Cm), 0 if Cm is None else Cm.stride(0), Nc, D,
               *nm, *flt.args, L.ptr(t_d), L.ptr(rank), L.ptr(score), ws_p, ws_bytes, L.current_stream())
    rank, score = flt.restore(rank, score)
    rank = rank.long()
    if barred.any():
        rank[torch.from_numpy(barred).to(dev)] = 0
    return result((rank, score, torch.from_numpy(n_cand).to(dev) if return_tensor else n_cand), return_tensor)

def similar_pairs(in_df, threshold, norm="", metric="cosine", candidates=None, *, max_pairs=None, return_tensor=False, device=None):
    """Every pair (i, j) whose ``pairwise_similarity`` score (same ``norm`` / ``metric``, same exact-fp32 products) is at least
    ``threshold``, without the N x N matrix: ``dae_threshold_pairs`` filters the score tiles in the GEMM's epilogue.

    Without ``candidates`` the corpus is ``in_df`` itself and the strict lower triangle is searched (``j < i``: every unordered
    pair once, never the self pair; the tiles above the diagonal are not computed).  With ``candidates`` every (query row,
    candidate row) pair counts.  Inputs take the containers of ``most_similar``.  A NaN score never qualifies.  The pairs
    are ordered by ``i`` ascending, then ``j`` ascending, bit-identical run to run.

    The result's size is not known beforehand: the library is called with room for ``max(65536, 8 * rows)`` pairs and, when
    more qualify, once more with the exact count.  With ``max_pairs`` set, a count above it raises ``ValueError`` (naming
    the count) instead of allocating.  Returns ``(rows int64, cols int64, scores float32)`` as ndarrays, or as CUDA
    tensors with ``return_tensor=True``."""
    import ctypes
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    torch, lib, dev, Q, Cm, Nq, Nc, D, nm = sweep_start(in_df, candidates, norm, metric, device)
    capacity = max(65536, 8 * Nq)
    if max_pairs is not None:
        capacity = min(capacity, max(int(max_pairs), 0))
    count = ctypes.c_uint64(0)
    for _ in range(2):
        rows = torch.empty(capacity, dtype=torch.int32, device=dev)
        cols = torch.empty(capacity, dtype=torch.int32, device=dev)
        score = torch.empty(capacity, dtype=torch.float32, device=dev)
        ws_bytes = int(lib.dae_threshold_pairs_workspace(Nq, Nc, D, capacity))
        ws_p, ws = workspace(dev, ws_bytes)
        with torch.cuda.device(dev):
            L.call("dae_threshold_pairs", L.ptr(Q), Q.stride(0), Nq, L.ptr(Cm), 0 if Cm is None else Cm.stride(0), Nc, D,
                   *nm, threshold, L.ptr(rows) if capacity else None, L.ptr(cols) if capacity else None,
                   L.ptr(score) if capacity else None, capacity, ctypes.byref(count), ws_p, ws_bytes, L.current_stream())
        del ws
        n = int(count.value)
        if max_pairs is not None and n > int(max_pairs):
            raise ValueError(f"{n} pairs score at least {threshold}, more than max_pairs={int(max_pairs)}")
        if n <= capacity:
            break
        capacity = n                                                  # the count is exact: the second call fits
    else:
        raise RuntimeError(f"dae_threshold_pairs counted {n} pairs after reporting {capacity}")
    return result((rows[:n].long(), cols[:n].long(), score[:n].clone()), return_tensor)

