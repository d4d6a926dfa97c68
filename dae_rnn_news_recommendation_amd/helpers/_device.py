"""What every device call of the package starts and ends with, once: the device and the library, the ``norm`` / ``metric`` check,
the container switch and the matrix intake, uploads, aligned workspaces, the history intake and the result tail.  torch and scipy
are imported inside the functions: importing the package needs numpy alone."""
from __future__ import annotations

import numpy as np

from .. import _lib as L

NORMS = {"": 0, "l1": 1, "l2": 2, "max": 3}
METRICS = {"cosine": 0, "linear kernel": 1}


def device_and_library(device):
    """``(torch, lib, dev)`` of a ``device=`` argument (None: the current CUDA device); the library is loaded first."""
    import torch
    return torch, L.load(), torch.device("cuda" if device is None else device)


def norm_metric(norm, metric):
    """The check of ``norm`` / ``metric``; returns the two integers the C entry points take, ``(norm, metric)``."""
    assert metric in ["cosine", "linear kernel"]                      # helpers.py:34
    if norm not in NORMS:
        raise ValueError(f"'{norm}' is not a supported norm")         # sklearn.preprocessing.normalize's message
    return NORMS[norm], METRICS[metric]


def row_count(data):
    """The number of rows of a container ``device_matrix`` takes, without touching it."""
    shape = getattr(data, "shape", None)
    return int(shape[0]) if shape is not None and len(shape) else len(data)


def matrix_shape(data):
    """``(rows, columns)`` of a container ``device_matrix`` takes, without touching it; ``ValueError`` unless it is 2-D."""
    shape = getattr(data, "shape", None)
    if shape is None:
        shape = np.asarray(data).shape
    if len(shape) != 2:
        raise ValueError("Expected 2D array")
    return int(shape[0]), int(shape[1])


def container(torch, data):
    """The container switch of every matrix argument: ``('tensor', data)``, ``('scipy', a float32 CSR copy)`` or ``('array', a
    float32 ndarray)`` of an ndarray, a list, a scipy.sparse matrix or a tensor; ``ValueError`` unless it is 2-D."""
    if isinstance(data, torch.Tensor):
        matrix_shape(data)
        return "tensor", data
    try:
        import scipy.sparse as sp
        is_sparse = sp.issparse(data)
    except ImportError:                                                # pragma: no cover
        is_sparse = False
    if is_sparse:
        return "scipy", data.tocsr().astype(np.float32)                # astype copies: the caller's matrix is not touched
    a = np.asarray(data, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError("Expected 2D array")
    return "array", a


def dense_on_device(torch, kind, m, dev):
    """The contiguous float32 device matrix of a ``container`` result; a scipy.sparse matrix is densified on the device."""
    if kind == "tensor":
        X = m.to(device=dev, dtype=torch.float32)
    elif kind == "scipy":
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                            # torch: "sparse CSR tensor support is in beta state"
            X = torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int64)),
                                        torch.from_numpy(m.data), size=m.shape).to(dev).to_dense()
    else:
        X = torch.as_tensor(m).to(dev)
    return X.contiguous()


def device_matrix(torch, data, dev, in_place=False):
    """A 2-D contiguous float32 CUDA tensor of ``data`` (ndarray, list, scipy.sparse -- densified on the device -- or tensor).
    ``in_place``: a CUDA float32 view with unit column stride is read where it is, whatever its row stride."""
    kind, m = container(torch, data)
    if in_place and kind == "tensor" and m.is_cuda and m.dtype == torch.float32 and m.stride(1) == 1:
        return m
    return dense_on_device(torch, kind, m, dev)


def upload(a, dev):
    """The host array ``a`` on the device (None stays None).  The library tells "no list" from "an empty list" by the pointer, so
    an empty array goes up as one element (one row, for a 2-D array), never as NULL."""
    import torch
    if a is None:
        return None
    return torch.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], dtype=a.dtype)).to(dev)


def workspace(dev, nbytes):
    """A 256-byte aligned device buffer of ``nbytes`` as ``(c_void_p, tensor)``; the tensor keeps it alive."""
    import ctypes
    import torch
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256), ws


def result(out, return_tensor):
    """The tail of every device function: tensors as they are, or as ndarrays (a tuple item by item; None and ndarrays pass)."""
    if return_tensor:
        return out
    if isinstance(out, tuple):
        return tuple(result(t, False) for t in out)
    return out.cpu().numpy() if hasattr(out, "cpu") else out


def csr_lists(lists, what="histories"):
    """``(indptr int64 [n + 1], items int64 [nnz])`` of a list of index sequences, or of an ``(indptr, items)`` pair -- a *tuple* of
    two arrays; a list is always taken as one sequence per row."""
    if isinstance(lists, tuple) and len(lists) == 2:
        indptr = np.ascontiguousarray(np.asarray(lists[0], dtype=np.int64).ravel())
        items = np.ascontiguousarray(np.asarray(lists[1]).ravel())
        if indptr.size < 1 or indptr[0] != 0 or (np.diff(indptr) < 0).any() or indptr[-1] != items.size:
            raise ValueError(f"{what}: indptr must start at 0, be non-decreasing and end at len(items)")
        return indptr, items
    rows = [np.asarray(r).ravel() for r in lists]
    rows = [r if r.size else r.astype(np.int64) for r in rows]          # an empty row has no dtype of its own
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    items = np.concatenate(rows) if indptr[-1] else np.zeros(0, dtype=np.int64)
    return indptr, items


def event_times(timestamps):
    """Timestamps in the layout of the histories (a list of sequences or an ``(indptr, times)`` tuple), or flat, as one per event."""
    return csr_lists(timestamps, "timestamps")[1] if isinstance(timestamps, (tuple, list)) else timestamps


def check_item_kind(items, what="histories"):
    """Article indices -- history items, sampled negatives -- are integers."""
    if items.size and items.dtype.kind not in "iu":
        raise ValueError(f"{what} must hold integer article indices")


def check_item_range(items, n_articles, lower=True):
    """History items lie in ``[0, n_articles)`` (``lower=False``: only the upper end is looked at -- for the callers whose negative
    items ``click_prefix_lists`` refuses next, in its own words)."""
    if items.size and ((lower and int(items.min()) < 0) or int(items.max()) >= n_articles):
        raise ValueError(f"history items must be in 0..{n_articles - 1} (got {int(items.min())}..{int(items.max())})")


def history_csr(histories, n_articles=None):
    """The history intake: ``(indptr int64, items)`` of ``histories`` (``csr_lists``), the items checked for their kind and, with
    ``n_articles``, for their range.  Where the number of articles is known only later, ``check_item_range`` follows alone."""
    indptr, items = csr_lists(histories)
    check_item_kind(items)
    if n_articles is not None:
        check_item_range(items, n_articles)
    return indptr, items
