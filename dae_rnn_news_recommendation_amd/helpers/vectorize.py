"""The stage in front of training (reference ``main_autoencoder.py:206-240``): from a raw count matrix to the pruned vocabulary and
the binary or tf-idf CSR, on the device.  ``column_stats`` (document and term frequency per column), ``limit_features`` /
``limit_features_columns`` / ``select_columns`` (``CountVectorizer._limit_features`` on a count matrix), ``TfidfTransformer``
(sklearn's, fitted on train and applied to validation) and ``binarize`` (``X.data = 1``).

A matrix is a scipy.sparse matrix or a *device CSR dict* with the keys of ``Engine.to_device_csr`` -- ``indptr`` (int64),
``indices`` (int32, ascending and unique within a row), ``values`` (float32, or None: every stored entry is 1), ``n_rows``,
``nnz``, ``n_cols`` -- which is what ``return_device=True`` gives back and ``Engine.upload_csr`` binds without a round trip.

The arithmetic: ``df`` and ``tf`` are integers, added by integer atomics; the idf is computed here in float64 from
``df`` by sklearn's formulas and rounded once to float32; per entry ``v = fl32(t * idf[c])`` with ``t`` the count or
``fl32(1 + log(count))``; the row norm is summed in float64 and the result is ``fl32(v / norm)``.  At the ``max_features`` cut,
columns of equal ``tf`` go to the LOWER column index (sklearn's order among ties is whatever its unstable argsort gives).

The device functions have no CPU implementation.  torch and scipy are imported inside the functions."""
from __future__ import annotations

import numbers

import numpy as np

from .. import _lib as L
from ._device import device_and_library, upload, workspace

NORMS = {None: 0, "l1": 1, "l2": 2}
_MAX_ROWS = (1 << 31) - 2


def _is_device_csr(m):
    return isinstance(m, dict) and "indptr" in m and "indices" in m


def _device_csr(torch, m, dev):
    """The device CSR dict of a scipy.sparse matrix (canonical, float32; uploaded) or of a device CSR dict (checked, as it is)."""
    if _is_device_csr(m):
        if m.get("n_cols") is None:
            raise ValueError("a device CSR dict needs 'n_cols', the number of columns")
        ip, ix, vl = m["indptr"], m["indices"], m.get("values")
        if ip.dtype != torch.int64 or ix.dtype != torch.int32 or (vl is not None and vl.dtype != torch.float32):
            raise ValueError("a device CSR dict holds int64 indptr, int32 indices and float32 values (or None)")
        if not (ip.is_cuda and ix.is_cuda and (vl is None or vl.is_cuda)):
            raise ValueError("a device CSR dict holds CUDA tensors")
        if ip.numel() != int(m["n_rows"]) + 1 or ix.numel() < int(m["nnz"]) or (vl is not None and vl.numel() < int(m["nnz"])):
            raise ValueError("a device CSR dict: indptr has n_rows + 1 entries, indices and values at least nnz")
        return m
    import scipy.sparse as sp
    if not sp.issparse(m):
        raise ValueError("counts must be a scipy.sparse matrix or a device CSR dict")
    m = m.tocsr()
    if not m.has_canonical_format:
        m = m.copy()
        m.sum_duplicates()
        m.sort_indices()
    return dict(indptr=upload(np.ascontiguousarray(m.indptr.astype(np.int64)), dev),
                indices=upload(np.ascontiguousarray(m.indices.astype(np.int32)), dev),
                values=upload(np.ascontiguousarray(m.data.astype(np.float32)), dev),
                n_rows=int(m.shape[0]), nnz=int(m.nnz), n_cols=int(m.shape[1]))


def _device_of(m, device):
    return m["indptr"].device if device is None and _is_device_csr(m) else device


def _shape(m):
    if _is_device_csr(m):
        if m.get("n_cols") is None:
            raise ValueError("a device CSR dict needs 'n_cols', the number of columns")
        return int(m["n_rows"]), int(m["n_cols"])
    return int(m.shape[0]), int(m.shape[1])


def device_csr_to_scipy(d):
    """The host scipy CSR matrix of a device CSR dict (float32; ones for a binary one)."""
    import scipy.sparse as sp
    nnz = int(d["nnz"])
    data = np.ones(nnz, dtype=np.float32) if d["values"] is None else d["values"][:nnz].cpu().numpy()
    return sp.csr_matrix((data, d["indices"][:nnz].cpu().numpy(), d["indptr"].cpu().numpy()), shape=(int(d["n_rows"]), int(d["n_cols"])))


def _indptr_at(d, row):
    import ctypes
    return ctypes.c_void_p(d["indptr"].data_ptr() + 8 * int(row))


def column_stats(counts, *, chunk_rows=None, device=None):
    """``(df, tf)`` of a count matrix, as int64 arrays: the number of stored entries of every column (explicit zeros count, as
    sklearn's ``_document_frequency`` counts them) and the sum of its counts (``dae_csr_column_stats``: integer atomics, exact).
    ``chunk_rows``: rows per call (None: all at once; the sums are the same).  A count that is not an integer in ``[0, 2**24]``
    or a column outside the matrix raises ``ValueError``."""
    import ctypes
    torch, lib, dev = device_and_library(_device_of(counts, device))
    d = _device_csr(torch, counts, dev)
    rows, F = _shape(d)
    if rows > _MAX_ROWS:
        raise ValueError("more than 2**31 - 2 rows")
    df = torch.zeros(max(F, 1), dtype=torch.int64, device=dev)
    tf = torch.zeros(max(F, 1), dtype=torch.int64, device=dev)
    if rows and F and int(d["nnz"]):
        step = rows if chunk_rows is None else int(chunk_rows)
        if step < 1:
            raise ValueError(f"chunk_rows must be positive (got {chunk_rows})")
        ws_bytes = int(lib.dae_csr_column_stats_workspace())
        ws_p, _ws = workspace(dev, ws_bytes)
        rec = (ctypes.c_uint64 * 2)()
        bad = dropped = 0
        for a0 in range(0, rows, step):
            L.call("dae_csr_column_stats", _indptr_at(d, a0), L.ptr(d["indices"]), L.ptr(d["values"]), min(step, rows - a0), F, L.ptr(df),
                   L.ptr(tf), rec, ws_p, ws_bytes, L.current_stream())
            bad, dropped = bad + int(rec[0]), dropped + int(rec[1])
        if dropped:
            raise ValueError(f"{dropped} entries have a column outside 0..{F - 1}")
        if bad:
            raise ValueError(f"{bad} entries are not counts (integers in 0..2**24)")
    return df[:F].cpu().numpy(), tf[:F].cpu().numpy()


def limit_features_columns(df, tf, n_rows, min_df=1, max_df=1.0, max_features=None):
    """The columns ``CountVectorizer(min_df, max_df, max_features)`` keeps, ascending, from the two arrays of ``column_stats`` and
    the number of documents.  A float ``min_df`` / ``max_df`` is a share of the rows, an int an absolute count; a column with
    ``df == 0`` is never kept (such a token would not be in a fitted vocabulary); of the columns left, the ``max_features`` with the
    largest ``tf`` stay, ties going to the lower column index.  Host NumPy."""
    df, tf = np.asarray(df, dtype=np.int64), np.asarray(tf, dtype=np.int64)
    if df.shape != tf.shape or df.ndim != 1:
        raise ValueError("df and tf are two 1-D arrays of one length")
    for name, v in (("min_df", min_df), ("max_df", max_df)):
        if isinstance(v, numbers.Integral):
            if v < 0:
                raise ValueError(f"negative value for {name}")
        elif not 0.0 <= v <= 1.0:
            raise ValueError(f"a float {name} is a share in [0, 1]")
    high = max_df if isinstance(max_df, numbers.Integral) else max_df * n_rows
    low = min_df if isinstance(min_df, numbers.Integral) else min_df * n_rows
    if high < low:
        raise ValueError("max_df corresponds to < documents than min_df")             # sklearn's message
    mask = (df > 0) & (df <= high) & (df >= low)
    if max_features is not None:
        if not isinstance(max_features, numbers.Integral) or max_features < 1:
            raise ValueError("max_features is a positive integer or None")
        if int(mask.sum()) > max_features:
            cand = np.flatnonzero(mask)
            top = np.argsort(-tf[cand], kind="stable")[:int(max_features)]            # stable: equal tf -> the lower column first
            mask = np.zeros_like(mask)
            mask[cand[top]] = True
    kept = np.flatnonzero(mask).astype(np.int64)
    if kept.size == 0:
        raise ValueError("After pruning, no terms remain. Try a lower min_df or a higher max_df.")    # sklearn's message
    return kept


def select_columns(counts, kept_columns, *, return_device=False, device=None):
    """The matrix with the columns ``kept_columns`` (strictly increasing), renumbered ``0 .. len - 1`` -- scipy's
    ``X[:, kept_columns]`` on the device (``dae_csr_select_columns``: count per row, scan, fill).  Returns a scipy CSR matrix
    (float32) or, with ``return_device``, a device CSR dict."""
    import ctypes
    torch, lib, dev = device_and_library(_device_of(counts, device))
    d = _device_csr(torch, counts, dev)
    rows, F = _shape(d)
    kept = np.asarray(kept_columns).ravel()
    if kept.size and kept.dtype.kind not in "iu":
        raise ValueError("kept_columns holds integer column indices")
    kept = kept.astype(np.int64)
    if kept.size and (int(kept.min()) < 0 or int(kept.max()) >= F or (np.diff(kept) <= 0).any()):
        raise ValueError(f"kept_columns must be strictly increasing in 0..{F - 1}")
    if rows > _MAX_ROWS:
        raise ValueError("more than 2**31 - 2 rows")
    nnz, binary = int(d["nnz"]), d["values"] is None
    out_indptr = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    out_indices = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)             # the input's nnz bounds the output's
    out_values = None if binary else torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
    new_nnz = 0
    if rows and F and nnz and kept.size:
        remap = np.full(F, -1, dtype=np.int32)
        remap[kept] = np.arange(kept.size, dtype=np.int32)
        remap_d = upload(remap, dev)
        ws_bytes = int(lib.dae_csr_select_columns_workspace(rows))
        ws_p, _ws = workspace(dev, ws_bytes)
        rec = (ctypes.c_int64 * 2)()
        L.call("dae_csr_select_columns", L.ptr(d["indptr"]), L.ptr(d["indices"]), L.ptr(d["values"]), rows, F, L.ptr(remap_d),
               L.ptr(out_indptr), L.ptr(out_indices), L.ptr(out_values), nnz, rec, ws_p, ws_bytes, L.current_stream())
        if int(rec[1]):
            raise ValueError(f"{int(rec[1])} entries have a column outside 0..{F - 1}")
        new_nnz = int(rec[0])
    out = dict(indptr=out_indptr, indices=out_indices[:new_nnz], values=None if binary else out_values[:new_nnz], n_rows=rows,
               nnz=new_nnz, n_cols=int(kept.size))
    return out if return_device else device_csr_to_scipy(out)


def limit_features(counts, min_df=1, max_df=1.0, max_features=None, *, stats=None, return_device=False):
    """``CountVectorizer._limit_features`` on a count matrix: ``(reduced, kept_columns)``.  ``stats``: the ``(df, tf)`` of
    ``column_stats(counts)`` when they are at hand.  The rule is ``limit_features_columns``'s; ``kept_columns`` applied to other
    rows (validation) is ``select_columns(rows, kept_columns)``."""
    if not _is_device_csr(counts):                                     # one upload for both halves
        torch, _, dev = device_and_library(None)
        counts = _device_csr(torch, counts, dev)
    df, tf = column_stats(counts) if stats is None else stats
    kept = limit_features_columns(df, tf, _shape(counts)[0], min_df, max_df, max_features)
    return select_columns(counts, kept, return_device=return_device), kept


def binarize(counts):
    """The ``X.data = 1`` step (reference main_autoencoder.py:235) on a copy: a scipy matrix with every stored entry 1, or a device
    CSR dict with ``values=None`` (which is how the library takes a binary matrix; the index tensors are shared)."""
    if _is_device_csr(counts):
        return dict(counts, values=None)
    out = counts.copy()
    out.data = np.ones_like(out.data)
    return out


class TfidfTransformer:
    """sklearn's ``TfidfTransformer`` on the device: ``fit`` takes the document frequencies from ``column_stats`` and computes
    ``idf_`` in float64 by sklearn's formulas; ``transform`` runs ``dae_tfidf_transform`` with that idf rounded once to float32."""

    def __init__(self, norm="l2", use_idf=True, smooth_idf=True, sublinear_tf=False):
        if norm not in NORMS:
            raise ValueError(f"'{norm}' is not a supported norm ('l1', 'l2' or None)")
        self.norm, self.use_idf, self.smooth_idf, self.sublinear_tf = norm, bool(use_idf), bool(smooth_idf), bool(sublinear_tf)

    @staticmethod
    def idf_from_df(df, n_samples, smooth_idf=True):
        """``log((n + s) / (df + s)) + 1`` in float64, ``s = int(smooth_idf)`` (sklearn); ``inf`` where that divides by zero."""
        df = np.asarray(df).astype(np.float64) + int(smooth_idf)
        with np.errstate(divide="ignore"):
            return np.log((int(n_samples) + int(smooth_idf)) / df) + 1.0

    def fit(self, X, y=None):
        rows, F = _shape(X)
        self.n_features_in_ = F
        if self.use_idf:
            self.idf_ = self.idf_from_df(column_stats(X)[0], rows, self.smooth_idf)
        return self

    def transform(self, X, return_device=False):
        """The tf-idf matrix of the counts ``X``: a scipy CSR float32 matrix, or with ``return_device`` a device CSR dict (no host
        copy; the index tensors are those of ``X`` when it is a device CSR dict)."""
        import ctypes
        if not hasattr(self, "n_features_in_"):
            raise ValueError("this TfidfTransformer is not fitted")
        torch, lib, dev = device_and_library(_device_of(X, None))
        d = _device_csr(torch, X, dev)
        rows, F = _shape(d)
        if F != self.n_features_in_:
            raise ValueError(f"X has {F} features, but TfidfTransformer is expecting {self.n_features_in_} features as input")
        if rows > _MAX_ROWS:
            raise ValueError("more than 2**31 - 2 rows")
        nnz = int(d["nnz"])
        out = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
        if rows and nnz:
            idf = upload(self.idf_.astype(np.float32), dev) if self.use_idf else None
            ws_bytes = int(lib.dae_tfidf_transform_workspace())
            ws_p, _ws = workspace(dev, ws_bytes)
            rec = (ctypes.c_uint64 * 1)()
            L.call("dae_tfidf_transform", L.ptr(d["indptr"]), L.ptr(d["indices"]), L.ptr(d["values"]), rows, F, L.ptr(idf),
                   int(self.sublinear_tf), NORMS[self.norm], L.ptr(out), rec, ws_p, ws_bytes, L.current_stream())
            if int(rec[0]):
                raise ValueError(f"{int(rec[0])} entries have a column outside 0..{F - 1}")
        res = dict(indptr=d["indptr"], indices=d["indices"][:nnz], values=out[:nnz], n_rows=rows, nnz=nnz, n_cols=F)
        return res if return_device else device_csr_to_scipy(res)

    def fit_transform(self, X, y=None, return_device=False):
        if not _is_device_csr(X):                                      # one upload for both halves
            torch, _, dev = device_and_library(None)
            X = _device_csr(torch, X, dev)
        return self.fit(X).transform(X, return_device=return_device)

    def save(self, path):
        """The parameters, ``n_features_in_`` and ``idf_`` as an ``.npz``."""
        if not hasattr(self, "n_features_in_"):
            raise ValueError("this TfidfTransformer is not fitted")
        np.savez(path, norm=np.str_("" if self.norm is None else self.norm), use_idf=self.use_idf, smooth_idf=self.smooth_idf,
                 sublinear_tf=self.sublinear_tf, n_features_in_=np.int64(self.n_features_in_),
                 idf_=self.idf_ if self.use_idf else np.zeros(0, dtype=np.float64))

    @classmethod
    def load(cls, path):
        with np.load(path) as f:
            t = cls(norm=str(f["norm"]) or None, use_idf=bool(f["use_idf"]), smooth_idf=bool(f["smooth_idf"]),
                    sublinear_tf=bool(f["sublinear_tf"]))
            t.n_features_in_ = int(f["n_features_in_"])
            if t.use_idf:
                t.idf_ = np.asarray(f["idf_"], dtype=np.float64)
        return t
