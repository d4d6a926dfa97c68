"""Mirror of the parts of the reference's ``helpers.py`` either side of the training path.

* ``save_file`` / ``read_file`` (helpers.py:138-264): the on-disk artefact conventions -- format picked from the file
  extension, writer / reader picked from the container type (ndarray: csv, tsv, npy; scipy.sparse: npz, and csv / tsv
  after densifying; DataFrame: csv, tsv, parquet, pkl; Series: csv, tsv, pkl).  Host code.
* ``pairwise_similarity`` (helpers.py:11-50) -- the evaluation step
``main_autoencoder.py:307-317`` runs six times right after training (embeddings, binary BoW, TF-IDF; train and
validation).  Same name, arguments, assert and return value; the normalisation, the N x N product (exact-fp32 MFMA) and
the diagonal fill run on the MI355X through ``dae_pairwise_similarity``.  No CPU implementation: without the built
library / a GPU this raises.
* ``most_similar`` -- top-k retrieval by the same scores without the N x N matrix (``dae_topk_similarity``), and
  ``label_precision_at_k`` (host code) to score such a result against labels.
* ``similar_pairs`` -- near-duplicate search: every pair scoring at least a threshold, without the N x N matrix
  (``dae_threshold_pairs``); ``duplicate_groups`` and ``duplicate_pair_precision`` (host code) turn the pairs into the
  de-duplication rule "keep the first article of each story" and score them against labels.
* ``label_similarity_stats`` -- the related-vs-unrelated AUROC and box-plot numbers of ``visualize_pairwise_similarity``
  without the N x N matrix: ``dae_pair_hist`` reduces the score tiles into one histogram per class, and
  ``stats_from_histograms`` (host code) derives the AUROC with a bracket that certifies it, and the quartiles.
* ``chunk_rows=`` of ``most_similar`` / ``label_similarity_stats`` -- the same results from operands swept a bounded number of rows
  at a time: a scipy.sparse input stays CSR on the device and its operand images are built chunk by chunk
  (``dae_sweep_image_csr``, ``dae_topk_images``, ``dae_pair_hist_images``); ``sweep_chunk_rows``, ``sweep_chunk_plan`` and
  ``label_stats_blocks`` (host code) are the chunk plan.
* ``user_states`` -- the decaying user model of "Embedding-based News Recommendation for Millions of Users": a decay-weighted
  mean of the embeddings of the articles a user has read (``dae_user_states``); ``recommend`` -- the top-k articles by
  ``user . article`` that the user has not read yet (``most_similar(exclude=...)``, ``dae_topk_similarity_ex``);
  ``next_click_metrics`` (host code) scores such a list against one held-out click per user.
* ``dedup_lists`` -- the pipeline's last stage: walk each recommendation list best first and skip an article whose similarity to
  one already selected reaches a threshold (``dae_dedup_lists``: one 128 x 128 score tile per list); ``recommend`` /
  ``most_similar`` with ``dedup_threshold=`` retrieve a larger pool and run it.
* ``target_ranks`` / ``recommend_ranks`` -- the position of the held-out article among ALL candidates, without the users x
  articles matrix (``dae_rank_similarity``); ``rank_metrics`` (host code) turns the ranks into AUC, mean / median rank,
  untruncated MRR / nDCG and hit / MRR / nDCG at any number of cut-offs from one pass.
* ``fit_user_model`` -- the trained form of that user model: the scaling vector alpha and the decay beta learned from click
  logs by a pairwise ranking loss, whose value and gradients ``user_pair_loss`` gets from one walk of the histories
  (``dae_user_pair_loss``); ``sample_negatives`` and ``decay_factor_derivatives`` (host code) prepare its inputs.
* ``gru_user_states`` -- the recurrent user model of the same paper, inference: the GRU state of every user after every click
  from weights in the layout of ``torch.nn.GRU`` (``GRUUserModel``; ``dae_gru_user_states``, time-major, one exact-fp32 MFMA GEMM
  per step over the users still active); ``gru_schedule`` and ``trim_histories`` (host code) prepare its inputs.
* ``gru_pair_loss`` / ``fit_gru_user_model`` -- the training half of that model: the pairwise ranking loss and, by back-propagation
  through time on the device, the gradients of the four weight arrays (``dae_gru_pair_loss``); mini-batch Adam on top of it.
* ``evaluate_every_click`` -- next-click evaluation at every click of every history, not only the last: ``recommend_every_click`` /
  ``recommend_ranks_every_click`` sweep the ``all_states`` rows against one stamped exclusion list per user, shared by that user's
  rows (``click_prefix_lists``, ``every_click_rows``; ``dae_topk_similarity_seq`` / ``dae_rank_similarity_seq``);
  ``rank_metrics_by_position`` and ``popularity_ranks_every_click`` (host code) give the accuracy-by-history-length table and the
  baseline."""
from __future__ import annotations

import numpy as np

from . import _lib as L

def _container_kind(data):
    import scipy.sparse as sp
    try:
        import pandas as pd
    except ImportError:                                                # pragma: no cover
        pd = None
    if isinstance(data, np.ndarray):
        return "numpy"
    if sp.issparse(data):
        return "scipy"
    if pd is not None and isinstance(data, pd.DataFrame):
        return "pandas_df"
    if pd is not None and isinstance(data, pd.Series):
        return "pandas_series"
    return None


_WRITABLE = {"numpy": ("csv", "tsv", "npy"), "scipy": ("npz",), "pandas_df": ("csv", "tsv", "parquet", "pkl"),
             "pandas_series": ("csv", "tsv", "pkl")}
_READABLE = {"numpy": ("csv", "tsv", "npy"), "scipy": ("csv", "tsv", "npz"), "pandas_df": ("csv", "tsv", "parquet", "pkl"),
             "pandas_series": ("csv", "tsv", "pkl")}


def save_file(data, path, format=None, **savekwargs):
    """Write ``data`` to ``path``; the format is the lower-cased extension unless given (helpers.py:138-199)."""
    import scipy.sparse as sp
    path = str(path)
    if format is None:
        format = path.lower().split(".")[-1]
    if sp.issparse(data) and format in ("csv", "tsv"):                 # text formats of a sparse matrix: densify first (:146-147)
        data = data.toarray()
    kind = _container_kind(data)
    assert kind is not None and format in _WRITABLE[kind], \
        "Shoule be one of following format {}".format(list(_WRITABLE.get(kind, ())))      # the reference's message (:198)
    sep = "," if format == "csv" else "\t"
    if kind == "numpy":
        if format == "npy":
            np.save(path, data, **savekwargs)
        else:
            np.savetxt(path, data, delimiter=sep, **savekwargs)
    elif kind == "scipy":
        sp.save_npz(path, data, **savekwargs)
    elif format in ("csv", "tsv"):
        data.to_csv(path, sep=sep, **savekwargs)
    elif format == "parquet":
        data.to_parquet(path, **savekwargs)
    else:
        data.to_pickle(path, **savekwargs)


def read_file(path, data_type=None, format=None, **readkwargs):
    """Read what ``save_file`` wrote.  ``data_type`` defaults from the format: npy -> 'numpy', npz -> 'scipy', everything
    else -> 'pandas_df' (helpers.py:202-264); pass 'pandas_series' for pickled / csv label vectors as the reference's
    scripts do (main_autoencoder.py:167-170)."""
    import os
    import scipy.sparse as sp
    path = str(path)
    assert os.path.isfile(path), "[Error] {} is not a file".format(path)
    if format is None:
        format = path.lower().split(".")[-1]
    if data_type is None:
        data_type = {"npy": "numpy", "npz": "scipy"}.get(format, "pandas_df")
    assert data_type in _READABLE
    assert format in _READABLE[data_type]
    sep = "," if format == "csv" else "\t"
    if data_type == "numpy":
        return np.load(path, **readkwargs) if format == "npy" else np.loadtxt(path, delimiter=sep, **readkwargs)
    if data_type == "scipy":
        return sp.load_npz(path, **readkwargs) if format == "npz" else sp.csr_matrix(np.loadtxt(path, delimiter=sep, **readkwargs))
    import pandas as pd
    if format == "parquet":
        return pd.read_parquet(path, **readkwargs)
    if format == "pkl":
        return pd.read_pickle(path, **readkwargs)
    if data_type == "pandas_df":
        return pd.read_csv(path, sep=sep, index_col=0, parse_dates=True, **readkwargs)
    # a Series written by to_csv: no header row, first column is the index (the reference asks read_csv for squeeze=True,
    # which current pandas spells .squeeze("columns"))
    return pd.read_csv(path, sep=sep, index_col=0, parse_dates=True, header=None, **readkwargs).squeeze("columns")


_NORMS = {"": 0, "l1": 1, "l2": 2, "max": 3}
_METRICS = {"cosine": 0, "linear kernel": 1}


def _csr_to_dense(torch, m, dev):
    return torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int64)),
                                   torch.from_numpy(m.data), size=m.shape).to(dev).to_dense()


def pairwise_similarity(in_df, norm="", metric="cosine", set_diagonal_zero=True, *, return_tensor=False, device=None):
    """Pairwise similarity of the rows of ``in_df`` (ndarray, scipy.sparse matrix, list, or a CUDA float32 tensor).

    norm: '' or sklearn.preprocessing.normalize's 'l1' / 'l2' / 'max', applied first; metric: 'cosine' or
    'linear kernel'; set_diagonal_zero as in the reference.  Returns a float32 ndarray [N x N]
    (``return_tensor=True``: the CUDA tensor view, no copy to the host).

    Sparse input is densified on the device (one fp32 image of the matrix); the reference's sklearn path would return
    a sparse matrix for ``linear kernel`` + sparse input with dense_output left at its default -- here the result is
    always dense, which is what every caller in the reference needs (they index and plot it)."""
    import torch
    assert metric in ["cosine", "linear kernel"]                      # helpers.py:34
    if norm not in _NORMS:
        raise ValueError(f"'{norm}' is not a supported norm")         # sklearn.preprocessing.normalize's message
    lib = L.load()
    dev = torch.device("cuda" if device is None else device)
    if isinstance(in_df, torch.Tensor):
        X = in_df.to(device=dev, dtype=torch.float32)
    else:
        try:
            import scipy.sparse as sp
            is_sparse = sp.issparse(in_df)
        except ImportError:                                            # pragma: no cover
            is_sparse = False
        if is_sparse:
            import warnings
            m = in_df.tocsr().astype(np.float32)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                        # torch: "sparse CSR tensor support is in beta state"
                X = _csr_to_dense(torch, m, dev)
        else:
            X = torch.as_tensor(np.asarray(in_df, dtype=np.float32)).to(dev)
    if X.dim() != 2:
        raise ValueError("Expected 2D array")
    X = X.contiguous()
    N, D = int(X.shape[0]), int(X.shape[1])
    Np = L.pad(N)
    out = torch.empty((Np, Np), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.dae_pairwise_similarity_workspace(N, D))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.call("dae_pairwise_similarity", L.ptr(X), X.stride(0), N, D, _NORMS[norm], _METRICS[metric], 1 if set_diagonal_zero else 0,
               L.ptr(out), Np, L.ptr(ws), ws_bytes, L.current_stream())
    res = out[:N, :N]
    if return_tensor:
        return res
    return res.cpu().numpy()


def _device_matrix(torch, data, dev):
    """A 2-D contiguous float32 CUDA tensor of ``data`` (ndarray, list, scipy.sparse -- densified on the device -- or tensor)."""
    if isinstance(data, torch.Tensor):
        X = data.to(device=dev, dtype=torch.float32)
    else:
        import scipy.sparse as sp
        if sp.issparse(data):
            import warnings
            m = data.tocsr().astype(np.float32)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                        # torch: "sparse CSR tensor support is in beta state"
                X = _csr_to_dense(torch, m, dev)
        else:
            X = torch.as_tensor(np.asarray(data, dtype=np.float32)).to(dev)
    if X.dim() != 2:
        raise ValueError("Expected 2D array")
    return X.contiguous()


def _sweep_inputs(in_df, candidates, norm, metric, device):
    """What ``most_similar``, ``target_ranks``, ``similar_pairs`` and ``label_similarity_stats`` start with: ``norm`` / ``metric``
    checked, the library, the device, and the two operands as device matrices (``Cm`` None: the corpus is ``in_df`` itself).
    Returns ``(lib, dev, Q, Cm, Nq, Nc, D)``."""
    import torch
    assert metric in ["cosine", "linear kernel"]                      # helpers.py:34
    if norm not in _NORMS:
        raise ValueError(f"'{norm}' is not a supported norm")         # sklearn.preprocessing.normalize's message
    lib = L.load()
    dev = torch.device("cuda" if device is None else device)
    Q = _device_matrix(torch, in_df, dev)
    Cm = None if candidates is None else _device_matrix(torch, candidates, dev)
    Nq, D = int(Q.shape[0]), int(Q.shape[1])
    if Cm is not None and int(Cm.shape[1]) != D:
        raise ValueError(f"candidates have {int(Cm.shape[1])} columns, in_df has {D}")
    return lib, dev, Q, Cm, Nq, Nq if Cm is None else int(Cm.shape[0]), D


def _workspace(dev, nbytes):
    """A 256-byte aligned device workspace of ``nbytes`` as ``(c_void_p, tensor)``; the tensor keeps it alive."""
    import ctypes
    import torch
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256), ws


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


class _SweepOperand:
    """One operand of a chunked sweep on the device, in the form it came in: a scipy.sparse matrix as canonical CSR (duplicates
    summed, column ids ascending), uploaded once -- no dense array of it exists on either side; a CUDA tensor as it is; anything
    else as a host float32 array whose row slices go up chunk by chunk.  ``image`` writes the normalised operand image of the rows
    ``[a0, a1)`` (``dae_sweep_image_csr`` / ``dae_sweep_image_dense``).  ``uploaded`` counts the bytes sent to the device."""

    def __init__(self, torch, data, dev):
        import scipy.sparse as sp
        self.dev, self.csr, self.X, self.host, self.uploaded = dev, None, None, None, 0
        if isinstance(data, torch.Tensor):
            if data.dim() != 2:
                raise ValueError("Expected 2D array")
            X = data.to(device=dev, dtype=torch.float32)
            self.X = X if X.stride(1) == 1 or X.shape[1] <= 1 else X.contiguous()
            self.shape = (int(X.shape[0]), int(X.shape[1]))
        elif sp.issparse(data):
            m = data.tocsr().astype(np.float32)                        # astype copies: the caller's matrix is not touched
            m.sum_duplicates()
            m.sort_indices()
            self.shape = (int(m.shape[0]), int(m.shape[1]))
            parts = (m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float32, copy=False))
            parts = tuple(np.ascontiguousarray(p if p.size else np.zeros(1, dtype=p.dtype)) for p in parts)
            self.uploaded = sum(p.nbytes for p in parts)
            self.csr = tuple(torch.from_numpy(p).to(dev) for p in parts)
        else:
            self.host = np.asarray(data, dtype=np.float32)
            if self.host.ndim != 2:
                raise ValueError("Expected 2D array")
            self.shape = (int(self.host.shape[0]), int(self.host.shape[1]))

    def image(self, torch, a0, a1, image_p, image_bytes, norm, metric):
        import ctypes
        rows, D = a1 - a0, self.shape[1]
        if self.csr is not None:
            ip, ix, vl = self.csr
            L.call("dae_sweep_image_csr", ctypes.c_void_p(ip.data_ptr() + 8 * a0), L.ptr(ix), L.ptr(vl), rows, D, _NORMS[norm],
                   _METRICS[metric], image_p, image_bytes, L.current_stream())
            return
        if self.X is not None:
            X = self.X[a0:a1]
        else:
            X = torch.from_numpy(np.ascontiguousarray(self.host[a0:a1])).to(self.dev)
            self.uploaded += X.numel() * 4
        L.call("dae_sweep_image_dense", L.ptr(X), max(int(X.stride(0)), D), rows, D, _NORMS[norm], _METRICS[metric], image_p, image_bytes,
               L.current_stream())


def _chunked_operands(in_df, candidates, norm, metric, device):
    """The start of a chunked sweep, as ``_sweep_inputs`` is of a one-shot one: ``(lib, dev, Qo, Co, Nq, Nc, D)`` with the operands
    as ``_SweepOperand`` (``Co`` None: the corpus is ``in_df`` itself)."""
    import torch
    assert metric in ["cosine", "linear kernel"]                      # helpers.py:34
    if norm not in _NORMS:
        raise ValueError(f"'{norm}' is not a supported norm")         # sklearn.preprocessing.normalize's message
    lib = L.load()
    dev = torch.device("cuda" if device is None else device)
    Qo = _SweepOperand(torch, in_df, dev)
    Co = None if candidates is None else _SweepOperand(torch, candidates, dev)
    Nq, D = Qo.shape
    if Co is not None and Co.shape[1] != D:
        raise ValueError(f"candidates have {Co.shape[1]} columns, in_df has {D}")
    Nc = Nq if Co is None else Co.shape[0]
    if Nq < 1 or Nc < 1 or D < 1:
        raise ValueError(f"a chunked sweep needs rows, candidates and columns (got {Nq} x {D} against {Nc} candidates)")
    return lib, dev, Qo, Co, Nq, Nc, D


def _most_similar_chunked(in_df, candidates, k, norm, metric, flt, chunk_rows, return_tensor, device):
    """``most_similar(chunk_rows=...)``: the outer loop walks the query chunks with one image and one carry (each row's running
    top-k as sorted 64-bit keys), the inner loop the corpus chunks with a second image; ``dae_topk_images`` merges a corpus chunk
    into the carry.  In self mode the diagonal block reuses the query image."""
    import ctypes
    import torch
    lib, dev, Qo, Co, Nq, Nc, D = _chunked_operands(in_df, candidates, norm, metric, device)
    k = int(k)
    c = sweep_chunk_rows(chunk_rows, D)
    idx = torch.empty((Nq, max(k, 1)), dtype=torch.int32, device=dev)
    score = torch.empty((Nq, max(k, 1)), dtype=torch.float32, device=dev)
    xp, xi = flt.lists(Nq, Nc)
    xp_d = xi_d = None
    if xp is not None:
        xp_d = torch.from_numpy(xp).to(dev)
        xi_d = torch.from_numpy(xi if xi.size else np.zeros(1, dtype=np.int32)).to(dev)
    cq, cc = min(c, L.pad(Nq)), min(c, L.pad(Nc))
    qb, cb = int(lib.dae_sweep_image_bytes(cq, D)), int(lib.dae_sweep_image_bytes(cc, D))
    q_p, q_t = _workspace(dev, qb)
    c_p, c_t = _workspace(dev, cb)
    carry_bytes = int(lib.dae_topk_carry_bytes(cq, max(k, 1)))
    carry = torch.empty(carry_bytes + 256, dtype=torch.uint8, device=dev)
    carry_p = ctypes.c_void_p(carry.data_ptr() + (-carry.data_ptr()) % 256)
    q_plan, c_plan = sweep_chunk_plan(Nq, c), sweep_chunk_plan(Nc, c)
    # a ragged last chunk has fewer query tiles and may get MORE corpus slices than a full one: size the workspace for every block shape
    ws_bytes = max(int(lib.dae_topk_images_workspace(nq, nc, max(k, 1))) for nq in {q_plan[0][1], q_plan[-1][1] - q_plan[-1][0]}
                   for nc in {c_plan[0][1], c_plan[-1][1] - c_plan[-1][0]})
    ws_p, ws = _workspace(dev, ws_bytes)
    with torch.cuda.device(dev):
        for q0, q1 in q_plan:
            Qo.image(torch, q0, q1, q_p, qb, norm, metric)
            carry.zero_()                                             # all-zero bytes: an empty carry
            for c0, c1 in c_plan:
                diag = Co is None and c0 == q0
                if not diag:
                    (Qo if Co is None else Co).image(torch, c0, c1, c_p, cb, norm, metric)
                L.call("dae_topk_images", q_p, q1 - q0, q0, None if diag else c_p, c1 - c0, c0, D, k, 1 if flt.exclude_self else 0,
                       None if xp_d is None else ctypes.c_void_p(xp_d.data_ptr() + 8 * q0), L.ptr(xi_d), carry_p,
                       ctypes.c_void_p(idx.data_ptr() + 4 * q0 * idx.stride(0)), ctypes.c_void_p(score.data_ptr() + 4 * q0 * score.stride(0)),
                       idx.stride(0), ws_p, ws_bytes, L.current_stream())
    del q_t, c_t, ws
    idx = idx.long()
    if return_tensor:
        return idx, score
    return idx.cpu().numpy(), score.cpu().numpy()


def _csr_lists(lists, what="histories"):
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


def normalize_exclusions(exclude, n_rows, n_candidates):
    """The exclusion lists of ``most_similar`` / ``recommend`` in the form ``dae_topk_similarity_ex`` reads: ``(indptr int64
    [n_rows + 1], items int32)``, every row's items ascending and unique, indices outside ``[0, n_candidates)`` dropped.
    ``exclude``: a list of ``n_rows`` index sequences or an ``(indptr, items)`` tuple.  Host code."""
    indptr, items = _csr_lists(exclude, "exclude")
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
    indptr, items = _csr_lists(lists, "exclude_shared")
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("exclude_shared must hold integer indices")
    items = items.astype(np.int64)
    st = _csr_lists(stamps, "exclude_shared stamps")[1] if isinstance(stamps, (tuple, list)) else np.asarray(stamps).ravel()
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


def _n_rows(data):
    """The number of rows of a container ``_device_matrix`` takes, without touching it."""
    shape = getattr(data, "shape", None)
    return int(shape[0]) if shape is not None and len(shape) else len(data)


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


def _permute_csr(indptr, items, perm):
    """The CSR ``(indptr, items)`` with its rows in the order ``perm``."""
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
                    xp, xi = _permute_csr(xp, xi, perm)
                if shared is not None:
                    shared = shared[:3] + (np.ascontiguousarray(shared[3][perm]), np.ascontiguousarray(shared[4][perm]))
            lo_d, hi_d = torch.from_numpy(np.ascontiguousarray(wlo)).to(dev), torch.from_numpy(np.ascontiguousarray(whi)).to(dev)
        # the library tells "no lists" from "empty lists" by the pointers: an empty array still goes up as one element, never as NULL
        up = lambda a: None if a is None else torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(dev)      # noqa: E731
        if shared is not None:
            d = tuple(up(a) for a in shared)
            self.entry, lists = "_seq", (L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), int(shared[0].size - 1), L.ptr(d[3]), L.ptr(d[4]))
        else:
            d = (up(xp), up(xi))
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
    n = lambda: (_n_rows(in_df), _n_rows(in_df if candidates is None else candidates))      # noqa: E731
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
    import torch
    if chunk_rows is not None and (window is not None or exclude_shared is not None):
        raise ValueError("chunk_rows does not go with window= or exclude_shared= (the chunked sweep takes exclude_self and exclude only)")
    if dedup_threshold is not None:
        k = int(k)
        pool = min(128, 4 * k) if dedup_pool is None else int(dedup_pool)
        if chunk_rows is not None:
            raise ValueError("chunk_rows does not go with dedup_threshold=")
        if pool < k or pool > 128:
            raise ValueError(f"dedup_pool must be in k..128 = {k}..128 (got {pool})")
        dev = torch.device("cuda" if device is None else device)
        corpus = _device_matrix(torch, in_df if candidates is None else candidates, dev)      # once, for both calls
        idx, score = most_similar(corpus if candidates is None else in_df, pool, norm, metric, exclude_self, None if candidates is None else corpus,
                                  exclude=exclude, exclude_shared=exclude_shared, window=window, return_tensor=True, device=device)
        return dedup_lists(idx, corpus, k, dedup_threshold, scores=score, norm=dedup_norm, metric=dedup_metric, return_tensor=return_tensor,
                           device=device)
    flt = _row_filter(in_df, candidates, exclude_self, exclude, exclude_shared, window)
    if chunk_rows is not None:
        return _most_similar_chunked(in_df, candidates, k, norm, metric, flt, chunk_rows, return_tensor, device)
    lib, dev, Q, Cm, Nq, Nc, D = _sweep_inputs(in_df, candidates, norm, metric, device)
    k = int(k)
    idx = torch.empty((Nq, max(k, 1)), dtype=torch.int32, device=dev)
    score = torch.empty((Nq, max(k, 1)), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.dae_topk_similarity_workspace(Nq, Nc, D, k))
    ws_p, ws = _workspace(dev, ws_bytes)
    (Q,) = flt.place(Q, Cm, dev)
    if Nq > 0 or (flt.window is None and flt.shared is None):         # without rows only the windowed and the shared call are skipped
        with torch.cuda.device(dev):
            L.call("dae_topk_similarity" + flt.entry, L.ptr(Q), Q.stride(0), Nq, L.ptr(Cm), 0 if Cm is None else Cm.stride(0), Nc, D,
                   _NORMS[norm], _METRICS[metric], k, *flt.args, L.ptr(idx), L.ptr(score), idx.stride(0), ws_p, ws_bytes,
                   L.current_stream())
    idx, score = flt.restore(idx, score)
    idx = idx.long()
    if return_tensor:
        return idx, score
    return idx.cpu().numpy(), score.cpu().numpy()


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
    import torch
    indptr, items = _csr_lists(histories)
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("histories must hold integer article indices")
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta must be in [0, 1] (got {beta})")
    decay = None if timestamps is None else decay_factors(indptr, _csr_lists(timestamps, "timestamps")[1]
                                                          if isinstance(timestamps, (tuple, list)) else timestamps, beta, time_unit)
    L.load()
    dev = torch.device("cuda" if device is None else device)
    E = _device_matrix(torch, embeddings, dev) if not (isinstance(embeddings, torch.Tensor) and embeddings.is_cuda
                                                       and embeddings.dtype == torch.float32 and embeddings.dim() == 2
                                                       and embeddings.stride(1) == 1) else embeddings      # a strided view is read in place
    Na, H = int(E.shape[0]), int(E.shape[1])
    if items.size and (int(items.min()) < 0 or int(items.max()) >= Na):
        raise ValueError(f"history items must be in 0..{Na - 1} (got {int(items.min())}..{int(items.max())})")
    M, nnz = int(indptr.size - 1), int(items.size)
    rows = nnz if all_states else M
    U = torch.empty((rows, H), dtype=torch.float32, device=dev)
    if rows == 0 or H == 0:
        return U if return_tensor else U.cpu().numpy()
    ip_d = torch.from_numpy(indptr).to(dev)
    it_d = torch.from_numpy(items.astype(np.int32) if nnz else np.zeros(1, dtype=np.int32)).to(dev)
    dc_d = None if decay is None else torch.from_numpy(decay if nnz else np.zeros(1, dtype=np.float32)).to(dev)
    with torch.cuda.device(dev):
        L.call("dae_user_states", L.ptr(E), E.stride(0), Na, H, L.ptr(ip_d), L.ptr(it_d), M, nnz, beta, L.ptr(dc_d),
               1 if all_states else 0, L.ptr(U), U.stride(0), L.current_stream())
    if return_tensor:
        return U
    return U.cpu().numpy()


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
    indptr, items = _csr_lists(histories)
    k = int(max_events)
    if k < 0:
        raise ValueError(f"max_events must not be negative (got {max_events})")
    n = np.minimum(np.diff(indptr), k)
    out = np.zeros(indptr.size, dtype=np.int64)
    out[1:] = np.cumsum(n)
    start = indptr[1:] - n                                              # first kept event of every user
    pos = np.repeat(start - out[:-1], n) + np.arange(int(out[-1]), dtype=np.int64)
    return out, items[pos]


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
    import torch
    if not isinstance(model, GRUUserModel):
        raise TypeError("model must be a GRUUserModel (GRUUserModel.load / from_torch)")
    if max_events is not None and all_states:
        raise ValueError("max_events and all_states do not go together: the rows of all_states are the caller's events")
    if int(batch_users) < 1:
        raise ValueError(f"batch_users must be positive (got {batch_users})")
    indptr, items = _csr_lists(histories)
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("histories must hold integer article indices")
    if max_events is not None:
        indptr, items = trim_histories((indptr, items), max_events)
    H, D = model.hidden_size, model.input_size
    M, nnz = int(indptr.size - 1), int(items.size)
    if not isinstance(embeddings, torch.Tensor):
        shape = getattr(embeddings, "shape", None)
        if shape is None:
            shape = np.asarray(embeddings).shape
        if len(shape) != 2:
            raise ValueError("Expected 2D array")
        if int(shape[1]) != D:
            raise ValueError(f"embeddings have {int(shape[1])} columns, the model's weight_ih has {D}")
        if items.size and (int(items.min()) < 0 or int(items.max()) >= int(shape[0])):
            raise ValueError(f"history items must be in 0..{int(shape[0]) - 1} (got {int(items.min())}..{int(items.max())})")
    if initial is not None and not isinstance(initial, torch.Tensor):
        initial = np.asarray(initial, dtype=np.float32)
    if initial is not None and tuple(initial.shape) != (M, H):
        raise ValueError(f"initial must be [users x H] = [{M} x {H}] (got {tuple(initial.shape)})")
    lib = L.load()
    dev = torch.device("cuda" if device is None else device)
    E = _fit_embeddings(torch, embeddings, dev)
    Na = int(E.shape[0])
    if int(E.shape[1]) != D:
        raise ValueError(f"embeddings have {int(E.shape[1])} columns, the model's weight_ih has {D}")
    if items.size and (int(items.min()) < 0 or int(items.max()) >= Na):
        raise ValueError(f"history items must be in 0..{Na - 1} (got {int(items.min())}..{int(items.max())})")
    rows = nnz if all_states else M
    U = torch.empty((rows, H), dtype=torch.float32, device=dev)
    if rows == 0:
        return U if return_tensor else U.cpu().numpy()
    if Na == 0:
        raise ValueError("embeddings hold no articles")
    h0 = None
    if initial is not None:
        h0 = (initial.to(device=dev, dtype=torch.float32) if isinstance(initial, torch.Tensor)
              else torch.as_tensor(np.asarray(initial, dtype=np.float32)).to(dev)).contiguous()
    w = [torch.from_numpy(getattr(model, n)).to(dev) for n in GRUUserModel.NAMES]
    it_d = torch.from_numpy(items.astype(np.int32) if nnz else np.zeros(1, dtype=np.int32)).to(dev)
    chunk = min(int(batch_users), M)
    ws_bytes = int(lib.dae_gru_user_states_workspace(Na, D, H, chunk))
    ws_ptr, ws = _workspace(dev, ws_bytes)
    import ctypes
    with torch.cuda.device(dev):
        for c0 in range(0, M, chunk):
            c1 = min(c0 + chunk, M)
            e0, e1 = int(indptr[c0]), int(indptr[c1])
            ip = np.ascontiguousarray(indptr[c0:c1 + 1] - e0)
            order, active = gru_schedule(ip)
            ip_d, or_d = torch.from_numpy(ip).to(dev), torch.from_numpy(order).to(dev)
            Uc = U[e0:e1] if all_states else U[c0:c1]
            h0c = None if h0 is None else h0[c0:c1]
            L.call("dae_gru_user_states", L.ptr(E), E.stride(0), Na, D, H, L.ptr(w[0]), D, L.ptr(w[1]), H, L.ptr(w[2]), L.ptr(w[3]),
                   L.ptr(ip_d), ctypes.c_void_p(it_d.data_ptr() + 4 * e0), L.ptr(or_d), c1 - c0, e1 - e0, int(active.size),
                   active.ctypes.data_as(ctypes.c_void_p), L.ptr(h0c), H, 1 if all_states else 0,
                   ctypes.c_void_p(Uc.data_ptr()), U.stride(0), ws_ptr, ws_bytes, L.current_stream())
    del ws
    if return_tensor:
        return U
    return U.cpu().numpy()


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


def _fit_embeddings(torch, embeddings, dev):
    """The embeddings as a float32 device matrix; a CUDA float32 view with unit column stride is read in place."""
    if (isinstance(embeddings, torch.Tensor) and embeddings.is_cuda and embeddings.dtype == torch.float32 and embeddings.dim() == 2
            and embeddings.stride(1) == 1):
        return embeddings
    return _device_matrix(torch, embeddings, dev)


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
        ws_ptr, ws = _workspace(dev, ws_bytes)
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
    if neg.size and neg.dtype.kind not in "iu":
        raise ValueError("negatives must hold integer article indices")
    if neg.size and int(neg.max()) >= Na:
        raise ValueError(f"negatives must be below {Na}, or negative for no pair (got {int(neg.max())})")
    return np.ascontiguousarray(np.maximum(neg, -1).astype(np.int32))


def _event_times(timestamps):
    return _csr_lists(timestamps, "timestamps")[1] if isinstance(timestamps, (tuple, list)) else timestamps


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
    import torch
    indptr, items = _csr_lists(histories)
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("histories must hold integer article indices")
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta must be in [0, 1] (got {beta})")
    decay = ddecay = None
    if timestamps is not None:
        t = _event_times(timestamps)
        decay = decay_factors(indptr, t, beta, time_unit)
        ddecay = decay_factor_derivatives(indptr, t, beta, time_unit) if beta > 0.0 else None      # beta = 0: factors in {0, 1}, dbeta = 0
    L.load()
    dev = torch.device("cuda" if device is None else device)
    E = _fit_embeddings(torch, embeddings, dev)
    Na, H = int(E.shape[0]), int(E.shape[1])
    alpha = np.asarray(alpha, dtype=np.float64).ravel()
    if alpha.size != H:
        raise ValueError(f"alpha has {alpha.size} entries for {H} embedding dimensions")
    if not 1 <= H <= 1024:
        raise ValueError(f"the embedding dimension must be in 1..1024 (got {H})")
    if items.size and (int(items.min()) < 0 or int(items.max()) >= Na):
        raise ValueError(f"history items must be in 0..{Na - 1} (got {int(items.min())}..{int(items.max())})")
    M, nnz = int(indptr.size - 1), int(items.size)
    neg = _check_negatives(negatives, nnz, Na)
    n_neg = int(neg.shape[1])
    one = lambda a, dt: torch.from_numpy(a if a.size else np.zeros(1, dtype=dt)).to(dev)      # never a NULL pointer
    return _pair_loss_call(torch, E, torch.from_numpy(indptr).to(dev), one(items.astype(np.int32), np.int32),
                           torch.from_numpy(neg if nnz else np.zeros((1, n_neg), dtype=np.int32)).to(dev), M, nnz, n_neg, alpha, beta,
                           None if decay is None else one(decay, np.float32), None if ddecay is None else one(ddecay, np.float32),
                           margins=return_margins)


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
        return U if return_tensor else U.cpu().numpy()


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
    import torch
    indptr, items = _csr_lists(histories)
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("histories must hold integer article indices")
    beta = float(beta0)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta0 must be in [0, 1] (got {beta0})")
    if int(epochs) < 0 or not float(lr) > 0.0:
        raise ValueError("epochs must not be negative and lr must be positive")
    t = None if timestamps is None else np.asarray(_event_times(timestamps), dtype=np.float64).ravel()
    L.load()
    dev = torch.device("cuda" if device is None else device)
    E = _fit_embeddings(torch, embeddings, dev)
    Na, H = int(E.shape[0]), int(E.shape[1])
    if not 1 <= H <= 1024:
        raise ValueError(f"the embedding dimension must be in 1..1024 (got {H})")
    if items.size and (int(items.min()) < 0 or int(items.max()) >= Na):
        raise ValueError(f"history items must be in 0..{Na - 1} (got {int(items.min())}..{int(items.max())})")
    M, nnz = int(indptr.size - 1), int(items.size)
    step_users = M if batch_users is None else int(batch_users)
    if batch_users is not None and step_users < 1:
        raise ValueError(f"batch_users must be positive (got {batch_users})")
    if fit_beta:
        beta = min(max(beta, 1e-6), 1.0 - 1e-6)                             # theta is finite
    x = np.concatenate([np.ones(H), [np.log(beta / (1.0 - beta)) if fit_beta else 0.0]])      # (alpha, theta)
    m1, m2, step = np.zeros(H + 1), np.zeros(H + 1), 0
    history = []
    it_d = torch.from_numpy(items.astype(np.int32) if nnz else np.zeros(1, dtype=np.int32)).to(dev)
    for epoch in range(int(epochs)):
        neg = sample_negatives(indptr, items, Na, n_neg, int(seed) + epoch, window=window)
        ng_d = torch.from_numpy(neg if nnz else np.zeros((1, int(n_neg)), dtype=np.int32)).to(dev)
        for u0 in range(0, M, max(step_users, 1)):
            u1 = min(u0 + step_users, M)
            a, b = int(indptr[u0]), int(indptr[u1])
            if fit_beta:
                beta = 1.0 / (1.0 + np.exp(-x[H]))
            beta32 = float(np.float32(beta))
            dc_d = dd_d = None
            if t is not None:
                ip = indptr[u0:u1 + 1] - a
                dc_d = torch.from_numpy(decay_factors(ip, t[a:b], beta32, time_unit) if b > a else np.zeros(1, np.float32)).to(dev)
                if fit_beta:
                    dd_d = torch.from_numpy(decay_factor_derivatives(ip, t[a:b], beta32, time_unit) if b > a
                                            else np.zeros(1, np.float32)).to(dev)
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


def _embedding_shape(embeddings):
    shape = getattr(embeddings, "shape", None)
    if shape is None:
        shape = np.asarray(embeddings).shape
    if len(shape) != 2:
        raise ValueError("Expected 2D array")
    return int(shape[0]), int(shape[1])


def _gru_fit_checks(embeddings, H, D, items):
    """The host-side refusals of ``gru_pair_loss`` / ``fit_gru_user_model``, before any device work: ``(articles, H)``."""
    Na, De = _embedding_shape(embeddings)
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("histories must hold integer article indices")
    if De != D:
        raise ValueError(f"embeddings have {De} columns, the model's weight_ih has {D}")
    if D != H:
        raise ValueError(f"training scores the state against the embeddings: the hidden size ({H}) must equal the embedding size D = {D}")
    if items.size and (int(items.min()) < 0 or int(items.max()) >= Na):
        raise ValueError(f"history items must be in 0..{Na - 1} (got {int(items.min())}..{int(items.max())})")
    if Na == 0:
        raise ValueError("embeddings hold no articles")
    return Na, H


def _gru_pair_loss_call(torch, E, w, indptr, it_d, ng_d, n_neg, grads, scal, margins=None):
    """One ``dae_gru_pair_loss`` on device operands, nothing read back.  ``indptr``: host int64 [M + 1] starting at 0; ``it_d``
    int32 [nnz], ``ng_d`` int32 [nnz x n_neg]; ``w`` / ``grads``: the four float32 weight tensors and their gradients (contiguous);
    ``scal``: float64 [2] that receives the loss and the bits of the int64 pair count; ``margins``: float32 [nnz x n_neg] or None."""
    import ctypes
    dev = E.device
    lib = L.load()
    Na, H = int(E.shape[0]), int(E.shape[1])
    M, nnz = int(indptr.size - 1), int(indptr[-1])
    order, active = gru_schedule(indptr)
    T = int(active.size)
    ip_d = torch.from_numpy(np.array(indptr, dtype=np.int64)).to(dev)
    or_d = torch.from_numpy(order if M else np.zeros(1, dtype=np.int32)).to(dev)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.dae_gru_pair_loss_workspace(Na, H, M, nnz, T, n_neg))
        ws_ptr, ws = _workspace(dev, ws_bytes)
        L.call("dae_gru_pair_loss", L.ptr(E), E.stride(0), Na, H, L.ptr(w[0]), H, L.ptr(w[1]), H, L.ptr(w[2]), L.ptr(w[3]), L.ptr(ip_d),
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
    import torch
    if not isinstance(model, GRUUserModel):
        raise TypeError("model must be a GRUUserModel (GRUUserModel.load / from_torch)")
    indptr, items = _csr_lists(histories)
    Na, H = _gru_fit_checks(embeddings, model.hidden_size, model.input_size, items)
    nnz = int(items.size)
    neg = _check_negatives(negatives, nnz, Na)
    n_neg = int(neg.shape[1])
    L.load()
    dev = torch.device("cuda" if device is None else device)
    E = _fit_embeddings(torch, embeddings, dev)
    w = [torch.from_numpy(getattr(model, n)).to(dev) for n in GRUUserModel.NAMES]
    grads = [torch.empty_like(a) for a in w]
    scal = torch.zeros(2, dtype=torch.float64, device=dev)
    mg = torch.empty((max(nnz, 1), n_neg), dtype=torch.float32, device=dev) if return_margins else None
    it_d = torch.from_numpy(items.astype(np.int32) if nnz else np.zeros(1, dtype=np.int32)).to(dev)
    ng_d = torch.from_numpy(neg if nnz else np.zeros((1, n_neg), dtype=np.int32)).to(dev)
    _gru_pair_loss_call(torch, E, w, indptr, it_d, ng_d, n_neg, grads, scal, mg)
    host = scal.cpu().numpy()
    res = {"loss": float(host[0]), "n_pairs": int(host[1:].view(np.int64)[0])}
    for name, g in zip(GRUUserModel.NAMES, grads):
        res[name] = g.cpu().numpy()
    if return_margins:
        res["margins"] = mg[:nnz].cpu().numpy()
    return res


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
    import torch
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
    if init is not None and not isinstance(init, GRUUserModel):
        raise TypeError("init must be a GRUUserModel")
    indptr, items = _csr_lists(histories)
    D = _embedding_shape(embeddings)[1]
    H = D if init is None else init.hidden_size
    Na, H = _gru_fit_checks(embeddings, H, D if init is None else init.input_size, items)
    indptr, items = trim_histories((indptr, items), max_events)
    n_neg, batch_users = int(n_neg), int(batch_users)
    rng = np.random.default_rng(seed)
    if init is None:
        k = 1.0 / np.sqrt(H)
        start = [rng.uniform(-k, k, s).astype(np.float32) for s in ((3 * H, H), (3 * H, H), (3 * H,), (3 * H,))]
    else:
        start = [getattr(init, n) for n in GRUUserModel.NAMES]
    L.load()
    dev = torch.device("cuda" if device is None else device)
    E = _fit_embeddings(torch, embeddings, dev)
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
            _gru_pair_loss_call(torch, E, w, ip, it_d, ng_d, n_neg, grads, scal)
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
            m = evaluate_every_click(validation, E, GRUUserModel(*host), device=device)["metrics"]
            m["epoch"] = epoch + 1
            scored.append(m)
            if keep_best and m["mrr"] == m["mrr"] and (best is None or m["mrr"] > best):      # NaN (no click to score): never the best
                best, best_w = m["mrr"], host
    final = best_w if keep_best and best_w is not None else [a.cpu().numpy() for a in w]
    return GRUUserModel(*final, history=np.asarray(history, dtype=np.float64), validation=scored if validation is not None else None)


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
    import torch
    assert metric in ["cosine", "linear kernel"]                      # helpers.py:34
    if norm not in _NORMS:
        raise ValueError(f"'{norm}' is not a supported norm")
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
    lib = L.load()
    dev = torch.device("cuda" if device is None else device)
    E = _device_matrix(torch, embeddings, dev)
    Na, D = int(E.shape[0]), int(E.shape[1])
    if isinstance(indices, torch.Tensor):
        lists = indices.to(device=dev)
    else:
        lists = torch.as_tensor(np.ascontiguousarray(np.asarray(indices))).to(dev)
    big = torch.iinfo(torch.int32).max
    lists = lists.clamp(min=-1, max=big).to(torch.int32).contiguous()           # (an index beyond int32 is beyond every corpus)
    out_idx = torch.empty((Nr, k), dtype=torch.int32, device=dev)
    out_pos = torch.empty((Nr, k), dtype=torch.int32, device=dev)
    counts = torch.empty((Nr, 2), dtype=torch.int32, device=dev)
    if Nr > 0:
        if Na == 0:
            raise ValueError("embeddings has no rows")
        ws_bytes = int(lib.dae_dedup_lists_workspace(Nr, Na, D, Ll))
        ws_p, ws = _workspace(dev, ws_bytes)
        with torch.cuda.device(dev):
            L.call("dae_dedup_lists", L.ptr(E), E.stride(0), Na, D, _NORMS[norm], _METRICS[metric], L.ptr(lists), lists.stride(0), Nr, Ll, k,
                   threshold, L.ptr(out_idx), L.ptr(out_pos), out_idx.stride(0), L.ptr(counts), ws_p, ws_bytes, L.current_stream())
    out_s = None
    if scores is not None:
        s = scores.to(device=dev, dtype=torch.float32) if isinstance(scores, torch.Tensor) else \
            torch.as_tensor(np.asarray(scores, dtype=np.float32)).to(dev)
        pos = out_pos.long()
        out_s = torch.gather(s, 1, pos.clamp(min=0)).masked_fill(pos < 0, float("-inf"))
    out = (out_idx.long(), out_s)
    if return_counts:
        out = out + ((counts[:, 0].long(), counts[:, 1].long()),)
    if return_tensor:
        return out
    host = lambda t: None if t is None else t.cpu().numpy()
    return (host(out[0]), host(out[1])) + (((host(out[2][0]), host(out[2][1])),) if return_counts else ())


def recommend(user_vectors, embeddings, k=10, seen=None, norm="", metric="linear kernel", *, window=None, return_tensor=False,
              device=None, dedup_threshold=None, dedup_pool=None, dedup_norm="", dedup_metric="cosine"):
    """The ``k`` articles (rows of ``embeddings``) with the largest relevance to every user vector (e.g. from ``user_states``)
    among those the user has not read: ``most_similar(user_vectors, candidates=embeddings, exclude=seen)``.  ``seen``: per
    user the indices already read (a list of sequences or an ``(indptr, items)`` tuple -- a history as given to ``user_states``
    will do; order and repeats do not matter), or None.  The default ``metric`` is the paper's relevance, the inner product;
    ``'cosine'`` and ``norm`` are those of ``most_similar``, and so is ``window``: per user the range of articles that may be
    shown at all (``candidate_windows``: those published by the time of the click, and not too long before).  Returns
    ``(indices, scores)`` as ``most_similar`` does.

    ``dedup_threshold`` (default None: no de-duplication, the call is what it was) drops near-duplicates from every list:
    ``dedup_pool`` unseen, in-window candidates (default ``min(128, 4 * k)``) are retrieved and ``dedup_lists`` walks them down
    to ``k``, skipping an article whose ``dedup_norm`` / ``dedup_metric`` similarity (default cosine) to one already selected
    reaches the threshold.  ``dedup_pool < k`` or ``> 128`` is a ``ValueError``."""
    return most_similar(user_vectors, k=k, norm=norm, metric=metric, candidates=embeddings, exclude=seen, window=window,
                        return_tensor=return_tensor, device=device, dedup_threshold=dedup_threshold, dedup_pool=dedup_pool,
                        dedup_norm=dedup_norm, dedup_metric=dedup_metric)


def next_click_metrics(indices, targets):
    """Scores a recommendation list against one held-out article per query: hit@k (the target is in the list), MRR@k
    (``1 / rank``) and nDCG@k (``1 / log2(1 + rank)``; one relevant item, so the ideal DCG is 1), rank counted from 1, each 0
    when the target is not in the list; averaged over the queries with a target >= 0.  An index of -1 matches nothing.  Host
    code.  Returns ``{'hit', 'mrr', 'ndcg', 'n'}``; the three are NaN when no query counts."""
    idx = np.asarray(indices)
    if idx.ndim != 2:
        raise ValueError("indices must be [n_queries x k]")
    tgt = np.asarray(targets).ravel().astype(np.int64)
    if tgt.shape[0] != idx.shape[0]:
        raise ValueError(f"{tgt.shape[0]} targets for {idx.shape[0]} queries")
    ok = tgt >= 0
    n = int(ok.sum())
    if n == 0 or idx.shape[1] == 0:
        nan = float("nan")
        return {"hit": nan if n == 0 else 0.0, "mrr": nan if n == 0 else 0.0, "ndcg": nan if n == 0 else 0.0, "n": n}
    match = (idx[ok] == tgt[ok][:, None]) & (idx[ok] >= 0)
    hit = match.any(axis=1)
    rank = np.where(hit, match.argmax(axis=1) + 1, 1).astype(np.float64)      # the first occurrence
    return {"hit": float(hit.mean()), "mrr": float(np.where(hit, 1.0 / rank, 0.0).mean()),
            "ndcg": float(np.where(hit, 1.0 / np.log2(1.0 + rank), 0.0).mean()), "n": n}


def _shared_row_chunks(n, max_pairs=1 << 22):
    """Row ranges ``[a, b)`` whose list lengths ``n`` sum to about ``max_pairs``: the O(sum of L^2) host work goes chunk by chunk."""
    total = np.concatenate([[0], np.cumsum(n)])
    a = 0
    while a < n.size:
        b = max(int(np.searchsorted(total, total[a] + max_pairs, side="right")) - 1, a + 1)
        yield a, min(b, n.size)
        a = min(b, n.size)


def _shared_pairs(lp, row_list, a, b):
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


def _competitors(tgt, Nq, Nc, exclude_self, xp, xi, window, shared=None):
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
            for a, b in _shared_row_chunks(n_in):
                rows, places = _shared_pairs(lp, row_list, a, b)
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
    import torch
    flt = _row_filter(in_df, candidates, exclude_self, exclude, exclude_shared, window)
    lib, dev, Q, Cm, Nq, Nc, D = _sweep_inputs(in_df, candidates, norm, metric, device)
    tgt = targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    tgt = tgt.ravel()
    if tgt.size and tgt.dtype.kind not in "iu":
        raise ValueError("targets must hold integer indices")
    tgt = tgt.astype(np.int64)
    if tgt.shape[0] != Nq:
        raise ValueError(f"{tgt.shape[0]} targets for {Nq} queries")
    if tgt.size and int(tgt.max()) >= Nc:
        raise ValueError(f"targets must be below {Nc} (got {int(tgt.max())})")
    n_cand, barred = _competitors(tgt, Nq, Nc, flt.exclude_self, *flt.lists(Nq, Nc), flt.window, flt.shared)
    rank = torch.empty(Nq, dtype=torch.int32, device=dev)
    score = torch.empty(Nq, dtype=torch.float32, device=dev)
    if Nq == 0:
        out = (rank.long(), score, torch.from_numpy(n_cand).to(dev))
        return out if return_tensor else tuple(t.cpu().numpy() for t in out)
    ws_bytes = int(lib.dae_rank_similarity_workspace(Nq, Nc, D))
    ws_p, ws = _workspace(dev, ws_bytes)
    Q, t_d = flt.place(Q, Cm, dev, torch.from_numpy(np.where(tgt >= 0, tgt, -1).astype(np.int32)).to(dev))
    with torch.cuda.device(dev):
        L.call("dae_rank_similarity" + flt.entry, L.ptr(Q), Q.stride(0), Nq, L.ptr(Cm), 0 if Cm is None else Cm.stride(0), Nc, D,
               _NORMS[norm], _METRICS[metric], *flt.args, L.ptr(t_d), L.ptr(rank), L.ptr(score), ws_p, ws_bytes, L.current_stream())
    rank, score = flt.restore(rank, score)
    rank = rank.long()
    if barred.any():
        rank[torch.from_numpy(barred).to(dev)] = 0
    if return_tensor:
        return rank, score, torch.from_numpy(n_cand).to(dev)
    return rank.cpu().numpy(), score.cpu().numpy(), n_cand


def recommend_ranks(user_vectors, embeddings, targets, seen=None, norm="", metric="linear kernel", *, window=None, return_tensor=False,
                    device=None):
    """The rank of each user's held-out article among all the articles the user has not read: the full-rank twin of
    ``recommend`` -- ``target_ranks(user_vectors, targets, candidates=embeddings, exclude=seen)``.  Returns ``(rank, score,
    n_candidates)`` as ``target_ranks`` does; ``rank`` is 0 for a target the user has already seen, and, with ``window`` (as in
    ``recommend``), for one outside the user's window."""
    return target_ranks(user_vectors, targets, norm=norm, metric=metric, candidates=embeddings, exclude=seen, window=window,
                        return_tensor=return_tensor, device=device)


def rank_metrics(rank, n_candidates, targets, ks=(1, 5, 10, 50, 100)):
    """Scores full ranks (``target_ranks`` / ``recommend_ranks``) against one held-out article per query.  Host code.

    Over the ``n`` queries with a target >= 0, a rank of 0 (the target can never be recommended) counting as a miss: ``hit@k``,
    ``mrr@k`` (``1 / rank``) and ``ndcg@k`` (``1 / log2(1 + rank)``) for every k of ``ks`` -- equal to ``next_click_metrics`` on
    the k-list of ``recommend`` -- and the untruncated ``mrr`` and ``ndcg``.  Over the ``n_ranked`` queries with rank > 0:
    ``mean_rank``, ``median_rank`` and ``auc``, the mean of ``(n_candidates - rank) / (n_candidates - 1)`` (the share of the other
    candidates the target beats; queries with a single candidate are skipped).  A value is NaN where no query counts."""
    r = np.asarray(rank).ravel().astype(np.int64)
    nc = np.asarray(n_candidates).ravel().astype(np.int64)
    tgt = np.asarray(targets).ravel().astype(np.int64)
    if not (r.shape[0] == nc.shape[0] == tgt.shape[0]):
        raise ValueError(f"{r.shape[0]} ranks, {nc.shape[0]} candidate counts and {tgt.shape[0]} targets")
    ok = tgt >= 0
    r, nc = r[ok], nc[ok]
    n = int(ok.sum())
    nan = float("nan")
    out = {"n": n, "n_ranked": int((r > 0).sum())}
    rf = np.where(r > 0, r, 1).astype(np.float64)
    for k in ks:
        k = int(k)
        hit = (r > 0) & (r <= k)
        out[f"hit@{k}"] = float(hit.mean()) if n else nan
        out[f"mrr@{k}"] = float(np.where(hit, 1.0 / rf, 0.0).mean()) if n else nan
        out[f"ndcg@{k}"] = float(np.where(hit, 1.0 / np.log2(1.0 + rf), 0.0).mean()) if n else nan
    out["mrr"] = float(np.where(r > 0, 1.0 / rf, 0.0).mean()) if n else nan
    out["ndcg"] = float(np.where(r > 0, 1.0 / np.log2(1.0 + rf), 0.0).mean()) if n else nan
    ranked = r > 0
    out["mean_rank"] = float(r[ranked].mean()) if ranked.any() else nan
    out["median_rank"] = float(np.median(r[ranked])) if ranked.any() else nan
    a = ranked & (nc > 1)
    out["auc"] = float(((nc[a] - r[a]) / (nc[a] - 1.0)).mean()) if a.any() else nan
    return out


def popularity_ranks(histories, n_articles, targets, seen=None, *, window=None):
    """Full ranks of the popularity baseline (``popularity_recommend``'s order: click count descending, index ascending, the
    user's ``seen`` articles -- default: the own history -- skipped).  Host code.  Returns ``(rank int64 [users],
    n_candidates int64 [users])`` with the conventions of ``target_ranks``: rank 0 without a target or for a seen one.  With
    ``window`` (a pair ``(lo, hi)`` per user, as in ``recommend``) only the articles ``lo <= a < hi`` compete, in the same order,
    and a target outside the window has rank 0."""
    indptr, items = _csr_lists(histories)
    M = indptr.size - 1
    if window is not None:
        window = normalize_window(window, M, n_articles)
    xp, xi = normalize_exclusions((indptr, items) if seen is None else seen, M, n_articles)
    order = np.argsort(-np.bincount(items.astype(np.int64), minlength=int(n_articles)), kind="stable")
    pos = np.empty(int(n_articles), dtype=np.int64)
    pos[order] = np.arange(int(n_articles))
    tgt = np.asarray(targets).ravel().astype(np.int64)
    if tgt.shape[0] != M:
        raise ValueError(f"{tgt.shape[0]} targets for {M} users")
    rank = np.zeros(M, dtype=np.int64)
    n_cand = np.full(M, int(n_articles), dtype=np.int64)
    if window is not None:
        for u in range(M):
            lo, hi = int(window[0][u]), int(window[1][u])
            mine = xi[xp[u]:xp[u + 1]]
            mine = mine[(mine >= lo) & (mine < hi)]
            t = tgt[u]
            n_cand[u] = hi - lo - (mine.size - int(t >= 0 and (mine == t).any()))
            if t < 0 or not lo <= t < hi or (mine == t).any():
                continue
            rank[u] = 1 + int((pos[lo:hi] < pos[t]).sum()) - int((pos[mine] < pos[t]).sum())
        return rank, n_cand
    for u in range(M):
        mine = xi[xp[u]:xp[u + 1]]
        t = tgt[u]
        n_cand[u] -= mine.size - int(t >= 0 and (mine == t).any())
        if t < 0 or (mine == t).any():
            continue
        rank[u] = 1 + pos[t] - int((pos[mine] < pos[t]).sum())
    return rank, n_cand


def popularity_recommend(histories, n_articles, k, seen=None, *, window=None):
    """The baseline a recommender has to beat: for every user the ``k`` most-clicked articles (over all ``histories``; ties by
    index ascending) that are not in the user's ``seen`` list (default: the user's own history).  Host code.  Returns
    int64 ``[users x k]``, -1 where fewer than k articles remain.  With ``window`` (a pair ``(lo, hi)`` per user, as in
    ``recommend``) only the articles ``lo <= a < hi`` are eligible, in the same order."""
    indptr, items = _csr_lists(histories)
    M = indptr.size - 1
    if window is not None:
        window = normalize_window(window, M, n_articles)
    xp, xi = normalize_exclusions((indptr, items) if seen is None else seen, M, n_articles)
    order = np.argsort(-np.bincount(items.astype(np.int64), minlength=int(n_articles)), kind="stable")
    out = np.full((M, int(k)), -1, dtype=np.int64)
    if window is not None:
        for u in range(M):
            lo, hi = int(window[0][u]), int(window[1][u])
            mine = xi[xp[u]:xp[u + 1]]
            cand = order[(order >= lo) & (order < hi)]                     # the window's articles, most clicked first
            keep = cand[~np.isin(cand, mine)][:int(k)]
            out[u, :keep.size] = keep
        return out
    for u in range(M):
        mine = xi[xp[u]:xp[u + 1]]
        head = order[:int(k) + mine.size]                                  # enough to survive the removal of `mine`
        keep = head[~np.isin(head, mine)][:int(k)]
        out[u, :keep.size] = keep
    return out


def click_prefix_lists(histories):
    """One exclusion list per user for the every-click protocol, shared by all of that user's rows: ``(indptr int64 [users + 1],
    items int32, stamps int32)`` -- per user the distinct articles of the history, ascending, each with the 0-based position of
    its FIRST click.  The state after click e must skip exactly the items with ``stamp <= e`` (``exclude_shared=``,
    ``dae_topk_similarity_seq``): the lists are no larger than the click log, where one materialised prefix per event would be
    sum of L (L + 1) / 2 items.  ``ValueError`` for a negative article index.  Host code, no per-user loop."""
    indptr, items = _csr_lists(histories)
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("histories must hold integer article indices")
    items = items.astype(np.int64)
    if items.size and int(items.min()) < 0:
        raise ValueError(f"history items must not be negative (got {int(items.min())})")
    M = indptr.size - 1
    users = np.repeat(np.arange(M, dtype=np.int64), np.diff(indptr))
    span = int(items.max()) + 1 if items.size else 1
    key, first = np.unique(users * span + items, return_index=True)      # by user, then article; the index of the first occurrence
    out = np.zeros(M + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.bincount(key // span, minlength=M))
    return out, (key % span).astype(np.int32), (first - indptr[:-1][key // span]).astype(np.int32)


def every_click_rows(histories, timestamps=None):
    """The query rows of the every-click protocol, one per event e in the order of ``user_states(all_states=True)``, as a dict:
    ``targets`` int64 (the user's next article, -1 at the user's last event), ``row_list`` int32 (the user: the list of
    ``click_prefix_lists`` the row reads), ``row_limit`` int32 (the event's 0-based position within the user: the row skips the
    items stamped at most that), ``positions`` int64 (the number of clicks seen, ``row_limit + 1``) and, with ``timestamps`` (one per
    event), ``query_times`` float64: the time of the NEXT click, which is what ``candidate_windows`` wants (at a user's last
    event, which has no target, the event's own time).  Host code."""
    indptr, items = _csr_lists(histories)
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("histories must hold integer article indices")
    nnz, n = int(items.size), np.diff(indptr)
    users = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), n)
    pos = np.arange(nnz, dtype=np.int64) - indptr[:-1][users]
    last = np.zeros(nnz, dtype=bool)
    last[indptr[1:][n > 0] - 1] = True
    nxt = np.minimum(np.arange(nnz, dtype=np.int64) + 1, max(nnz - 1, 0))
    out = {"targets": np.where(last, -1, items.astype(np.int64)[nxt] if nnz else np.zeros(0, np.int64)).astype(np.int64),
           "row_list": users.astype(np.int32), "row_limit": pos.astype(np.int32), "positions": pos + 1}
    if timestamps is not None:
        t = np.asarray(_event_times(timestamps), dtype=np.float64).ravel()
        if t.size != nnz:
            raise ValueError(f"{t.size} timestamps for {nnz} events")
        out["query_times"] = np.where(last, t, t[nxt] if nnz else t)
    return out


def _every_click_chunks(states, embeddings, histories, window, batch_rows, device):
    """What the two every-click sweeps share: the checked inputs, and per chunk of ``batch_rows`` rows the arguments of the sweep.
    Returns ``(rows dict, E, chunks)``; a chunk is ``(a, b, states[a:b], exclude_shared, window or None)``."""
    import torch
    if int(batch_rows) < 1:
        raise ValueError(f"batch_rows must be positive (got {batch_rows})")
    indptr, items = _csr_lists(histories)
    rows = every_click_rows((indptr, items))
    nnz = int(items.size)
    if _n_rows(states) != nnz:
        raise ValueError(f"{_n_rows(states)} state rows for {nnz} events (states is the all_states=True output for these histories)")
    Na = _n_rows(embeddings)
    if items.size and int(items.max()) >= Na:
        raise ValueError(f"history items must be in 0..{Na - 1} (got {int(items.min())}..{int(items.max())})")
    lists = click_prefix_lists((indptr, items))
    if window is not None:
        window = normalize_window(window, nnz, Na)
    L.load()
    dev = torch.device("cuda" if device is None else device)
    E = _fit_embeddings(torch, embeddings, dev)

    def chunks():
        for a in range(0, nnz, int(batch_rows)):
            b = min(a + int(batch_rows), nnz)
            yield (a, b, states[a:b], ((lists[0], lists[1]), lists[2], rows["row_list"][a:b], rows["row_limit"][a:b]),
                   None if window is None else (window[0][a:b], window[1][a:b]))
    return rows, E, chunks()


def recommend_every_click(states, embeddings, histories, k=10, *, window=None, batch_rows=1 << 20, norm="", metric="linear kernel",
                          return_tensor=False, device=None):
    """``recommend`` at every click: for the state after each event e of every history -- ``states`` [events x H], the
    ``all_states=True`` output of ``user_states`` / ``gru_user_states`` for the same ``histories`` -- the ``k`` articles with the
    largest relevance among those the user had not clicked by then (positions <= e).  The seen articles are one stamped list
    per user, shared by that user's rows (``click_prefix_lists``, ``most_similar(exclude_shared=...)``, ``dae_topk_similarity_seq``).

    ``window``: a pair ``(lo, hi)`` per EVENT, e.g. ``candidate_windows(every_click_rows(histories, t)['query_times'], publish,
    max_age)``.  The rows go through the sweep in chunks of ``batch_rows`` (an operand image must stay below 4 GiB); the chunking
    does not change a bit.  Returns ``(indices int64 [events x k], scores float32 [events x k], targets int64 [events])``:
    ``targets[e]`` is the user's next click, -1 at a user's last event."""
    import torch
    rows, E, chunks = _every_click_chunks(states, embeddings, histories, window, batch_rows, device)
    idx, score = [], []
    for a, b, S, shared, win in chunks:
        i, s = most_similar(S, k=k, norm=norm, metric=metric, candidates=E, exclude_shared=shared, window=win, return_tensor=True,
                            device=device)
        idx.append(i)
        score.append(s)
    if not idx:
        idx = [torch.empty((0, max(int(k), 1)), dtype=torch.int64, device=E.device)]
        score = [torch.empty((0, max(int(k), 1)), dtype=torch.float32, device=E.device)]
    idx, score = torch.cat(idx), torch.cat(score)
    if return_tensor:
        return idx, score, torch.from_numpy(rows["targets"]).to(idx.device)
    return idx.cpu().numpy(), score.cpu().numpy(), rows["targets"]


def recommend_ranks_every_click(states, embeddings, histories, *, window=None, batch_rows=1 << 20, norm="", metric="linear kernel",
                                return_tensor=False, device=None):
    """``recommend_ranks`` at every click, the full-rank twin of ``recommend_every_click`` (same arguments and chunking;
    ``target_ranks(exclude_shared=...)``, ``dae_rank_similarity_seq``): the rank of every next click among all the articles the
    user had not clicked by then.  Returns ``(rank, score, n_candidates, targets)`` with the conventions of ``target_ranks``:
    ``rank`` is 0 at a user's last event (no target), for a re-click of an article already seen, and for a target outside its
    event's window."""
    import torch
    rows, E, chunks = _every_click_chunks(states, embeddings, histories, window, batch_rows, device)
    out = [[], [], []]
    for a, b, S, shared, win in chunks:
        r = target_ranks(S, rows["targets"][a:b], norm=norm, metric=metric, candidates=E, exclude_shared=shared, window=win,
                         return_tensor=True, device=device)
        for o, x in zip(out, r):
            o.append(x)
    if not out[0]:
        out = [[torch.empty(0, dtype=dt, device=E.device)] for dt in (torch.int64, torch.float32, torch.int64)]
    rank, score, n_cand = (torch.cat(o) for o in out)
    if return_tensor:
        return rank, score, n_cand, torch.from_numpy(rows["targets"]).to(rank.device)
    return rank.cpu().numpy(), score.cpu().numpy(), n_cand.cpu().numpy(), rows["targets"]


def evaluate_every_click(histories, embeddings, model, *, timestamps=None, time_unit=None, window=None, batch_users=4096,
                         ks=(1, 5, 10, 50, 100), device=None):
    """Next-click evaluation at EVERY click of every history (the per-position protocol of session-based recommendation), where
    the last-click protocol scores one click per user: the state after each event is ranked against the event that follows,
    among all the articles the user had not clicked by then (``recommend_ranks_every_click``).

    ``model``: a ``GRUUserModel`` (states of ``gru_user_states``), a fitted ``UserModel`` (``alpha *`` the states of ``user_states``
    with its ``beta`` and ``time_unit``, as ``UserModel.states`` applies them) or a float ``beta`` (``user_states``; ``time_unit``
    as there).  ``timestamps`` (one per event) drive the decay of the two decay forms; ``window`` is a pair ``(lo, hi)`` per EVENT.
    The states are produced for ``batch_users`` users at a time and ranked at once, so [events x H] never exists whole.

    Returns a dict: the per-event arrays ``rank``, ``score``, ``n_candidates``, ``targets``, ``positions`` (clicks seen, for
    ``rank_metrics_by_position``) and ``metrics`` = ``rank_metrics`` over all events with a target."""
    import torch
    if int(batch_users) < 1:
        raise ValueError(f"batch_users must be positive (got {batch_users})")
    indptr, items = _csr_lists(histories)
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("histories must hold integer article indices")
    M, nnz = int(indptr.size - 1), int(items.size)
    t = None if timestamps is None else np.asarray(_event_times(timestamps), dtype=np.float64).ravel()
    if t is not None and t.size != nnz:
        raise ValueError(f"{t.size} timestamps for {nnz} events")
    if window is not None:
        window = normalize_window(window, nnz, _n_rows(embeddings))
    if not isinstance(model, (GRUUserModel, UserModel)):
        model = float(model)
    L.load()
    dev = torch.device("cuda" if device is None else device)
    E = _fit_embeddings(torch, embeddings, dev)
    alpha = torch.from_numpy(model.alpha.astype(np.float32)).to(dev) if isinstance(model, UserModel) else None
    out = [[], [], []]
    for u0 in range(0, M, int(batch_users)):
        u1 = min(u0 + int(batch_users), M)
        a, b = int(indptr[u0]), int(indptr[u1])
        if b == a:
            continue
        hist = (indptr[u0:u1 + 1] - a, items[a:b])
        tb = None if t is None else t[a:b]
        if isinstance(model, GRUUserModel):
            S = gru_user_states(hist, E, model, all_states=True, return_tensor=True, device=device)
        elif isinstance(model, UserModel):
            S = user_states(hist, E, model.beta, timestamps=tb, time_unit=model.time_unit, all_states=True, return_tensor=True,
                            device=device) * alpha
        else:
            S = user_states(hist, E, model, timestamps=tb, time_unit=time_unit, all_states=True, return_tensor=True, device=device)
        r = recommend_ranks_every_click(S, E, hist, window=None if window is None else (window[0][a:b], window[1][a:b]), device=device)
        for o, x in zip(out, r[:3]):
            o.append(x)
        del S
    rows = every_click_rows((indptr, items))
    rank, score, n_cand = (np.concatenate(o) if o else np.zeros(0, dtype=dt) for o, dt in zip(out, (np.int64, np.float32, np.int64)))
    return {"rank": rank, "score": score, "n_candidates": n_cand, "targets": rows["targets"], "positions": rows["positions"],
            "metrics": rank_metrics(rank, n_cand, rows["targets"], ks=ks)}


def rank_metrics_by_position(rank, n_candidates, targets, positions, edges=(1, 2, 3, 5, 10, 20, 50), ks=(1, 5, 10, 50, 100)):
    """``rank_metrics`` per bucket of clicks seen: the accuracy-against-history-length table of the every-click protocol.  Host code.

    ``positions``: per row the number of clicks the state has seen (``every_click_rows``).  The buckets are ``[edges[i], edges[i + 1])``
    and ``[edges[-1], inf)``, plus a leading bucket for the rows below ``edges[0]`` when there are any: every row is in exactly one,
    and pooling them gives ``rank_metrics`` of all rows.  Returns a list of dicts, one per bucket in order: ``lo``, ``hi`` (None: open
    end) and the entries of ``rank_metrics`` over the bucket's rows."""
    r, nc, tgt, pos = (np.asarray(x).ravel() for x in (rank, n_candidates, targets, positions))
    if not (r.shape[0] == nc.shape[0] == tgt.shape[0] == pos.shape[0]):
        raise ValueError(f"{r.shape[0]} ranks, {nc.shape[0]} candidate counts, {tgt.shape[0]} targets and {pos.shape[0]} positions")
    edges = [int(e) for e in edges]
    if not edges or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError("edges must be a non-empty increasing sequence")
    which = np.searchsorted(np.asarray(edges, dtype=np.int64), pos.astype(np.int64), side="right")      # 0: below edges[0]
    out = []
    for b in range(0 if (which == 0).any() else 1, len(edges) + 1):
        m = which == b
        out.append(dict(lo=None if b == 0 else edges[b - 1], hi=None if b == len(edges) else edges[b], **rank_metrics(r[m], nc[m], tgt[m], ks=ks)))
    return out


def popularity_ranks_every_click(histories, n_articles, *, window=None):
    """Full ranks of the popularity baseline under the every-click protocol: ``popularity_ranks``' order (click count over all
    ``histories`` descending, index ascending), per event e the articles the user clicked at positions <= e skipped, the target
    the user's next click.  ``window``: a pair ``(lo, hi)`` per EVENT.  Host code (chunked, O(sum of L^2)).  Returns ``(rank int64
    [events], n_candidates int64 [events], targets int64 [events])`` with the conventions of ``target_ranks``: rank 0 without a
    target, for a seen one and for one outside the window."""
    indptr, items = _csr_lists(histories)
    Na, nnz = int(n_articles), int(items.size)
    if items.size and int(items.max()) >= Na:
        raise ValueError(f"history items must be in 0..{Na - 1} (got {int(items.min())}..{int(items.max())})")
    rows = every_click_rows((indptr, items))
    lp, li, ls = click_prefix_lists((indptr, items))
    tgt = rows["targets"]
    if window is not None:
        window = normalize_window(window, nnz, Na)
    n_cand, barred = _competitors(tgt, nnz, Na, False, None, None, window, (lp, li, ls, rows["row_list"], rows["row_limit"]))
    order = np.argsort(-np.bincount(items.astype(np.int64), minlength=Na), kind="stable")
    pos = np.empty(Na, dtype=np.int64)
    pos[order] = np.arange(Na)
    ok = (tgt >= 0) & ~barred
    pt = pos[np.where(ok, tgt, 0)]
    if window is None:
        ahead = pt.copy()                                                   # every article before the target in the order
    else:
        ahead = np.array([int((pos[window[0][e]:window[1][e]] < pt[e]).sum()) if ok[e] else 0 for e in range(nnz)], dtype=np.int64)
    lim = rows["row_limit"].astype(np.int64)
    n_in = np.diff(lp)[rows["row_list"]] if nnz else np.zeros(0, dtype=np.int64)
    for a, b in _shared_row_chunks(n_in):                                   # minus the seen ones among them
        r, places = _shared_pairs(lp, rows["row_list"], a, b)
        it = li[places].astype(np.int64)
        take = (ls[places] <= lim[r]) & (pos[it] < pt[r])
        if window is not None:
            take &= (it >= window[0][r]) & (it < window[1][r])
        ahead[a:b] -= np.bincount(r[take] - a, minlength=b - a)
    return np.where(ok, 1 + ahead, 0).astype(np.int64), n_cand, tgt


def _label_keys(labels):
    """Labels as float64 (numeric) with a validity mask: negative / NaN labels are missing, as in visualize_pairwise_similarity."""
    lab = np.asarray(labels)
    lab = lab.reshape(lab.shape[0], -1)[:, 0] if lab.ndim > 1 else lab
    if lab.dtype.kind in "biuf":
        v = lab.astype(np.float64)
        return v, np.isfinite(v) & (v >= 0)
    return lab, np.array([x is not None for x in lab], dtype=bool)


def label_precision_at_k(indices, labels, candidate_labels=None):
    """Precision@k of a retrieval result: the mean, over the queries, of the fraction of each query's ``k`` returned indices
    whose label equals the query's label.  ``labels`` are the query labels; ``candidate_labels`` those of the corpus the
    indices point into (default: ``labels``, i.e. the corpus is the query set).  Queries whose label is negative or NaN
    are skipped; an index of -1 (fewer than k candidates) or a candidate with a missing label counts as a miss.  Host code.
    Returns ``(precision, number of queries counted)``; precision is NaN when no query counts."""
    idx = np.asarray(indices)
    if idx.ndim != 2:
        raise ValueError("indices must be [n_queries x k]")
    ql, qv = _label_keys(labels)
    cl, cv = (ql, qv) if candidate_labels is None else _label_keys(candidate_labels)
    if ql.shape[0] != idx.shape[0]:
        raise ValueError(f"{ql.shape[0]} labels for {idx.shape[0]} queries")
    if idx.shape[1] == 0 or not qv.any():
        return float("nan"), 0
    safe = np.where(idx >= 0, idx, 0)
    hit = (idx >= 0) & cv[safe] & (cl[safe] == ql[:, None])
    frac = hit[qv].mean(axis=1)
    return float(frac.mean()), int(qv.sum())


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
    import torch
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    lib, dev, Q, Cm, Nq, Nc, D = _sweep_inputs(in_df, candidates, norm, metric, device)
    capacity = max(65536, 8 * Nq)
    if max_pairs is not None:
        capacity = min(capacity, max(int(max_pairs), 0))
    count = ctypes.c_uint64(0)
    for _ in range(2):
        rows = torch.empty(capacity, dtype=torch.int32, device=dev)
        cols = torch.empty(capacity, dtype=torch.int32, device=dev)
        score = torch.empty(capacity, dtype=torch.float32, device=dev)
        ws_bytes = int(lib.dae_threshold_pairs_workspace(Nq, Nc, D, capacity))
        ws_p, ws = _workspace(dev, ws_bytes)
        with torch.cuda.device(dev):
            L.call("dae_threshold_pairs", L.ptr(Q), Q.stride(0), Nq, L.ptr(Cm), 0 if Cm is None else Cm.stride(0), Nc, D,
                   _NORMS[norm], _METRICS[metric], threshold, L.ptr(rows) if capacity else None, L.ptr(cols) if capacity else None,
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
    rows, cols, score = rows[:n].long(), cols[:n].long(), score[:n].clone()
    if return_tensor:
        return rows, cols, score
    return rows.cpu().numpy(), cols.cpu().numpy(), score.cpu().numpy()


def duplicate_groups(rows, cols, n):
    """Connected components of the pair graph over ``n`` items (``rows[p]`` -- ``cols[p]`` are its edges, e.g. the result of
    ``similar_pairs``).  Returns ``(group, keep)``: ``group`` (int64 ``[n]``) is the smallest index of the item's
    component, so an item with no partner is its own group; ``keep`` (bool ``[n]``) is true for exactly that smallest
    index -- the de-duplication rule "keep the first article of each story".  Host code."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = int(n)
    r = np.asarray(rows, dtype=np.int64).ravel()
    c = np.asarray(cols, dtype=np.int64).ravel()
    if r.shape != c.shape:
        raise ValueError(f"{r.shape[0]} rows for {c.shape[0]} cols")
    if r.size and (min(r.min(), c.min()) < 0 or max(r.max(), c.max()) >= n):
        raise ValueError(f"pair indices must be in 0..{n - 1}")
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    graph = coo_matrix((np.ones(r.size, np.int8), (r, c)), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    first = np.full(int(comp.max()) + 1, n, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n, dtype=np.int64))
    group = first[comp]
    return group, group == np.arange(n)


def duplicate_pair_precision(rows, cols, labels, candidate_labels=None):
    """The share of the pairs ``(rows[p], cols[p])`` whose two labels are equal.  ``labels`` are those of the rows;
    ``candidate_labels`` those of the corpus the cols point into (default: ``labels``, i.e. the corpus is the query set).
    Pairs with a missing label (negative or NaN, the rule of ``label_precision_at_k``) are skipped.  Host code.  Returns
    ``(precision, number of pairs counted)``; precision is NaN when no pair counts."""
    r = np.asarray(rows, dtype=np.int64).ravel()
    c = np.asarray(cols, dtype=np.int64).ravel()
    if r.shape != c.shape:
        raise ValueError(f"{r.shape[0]} rows for {c.shape[0]} cols")
    lab, valid = _label_keys(labels)
    clab, cvalid = (lab, valid) if candidate_labels is None else _label_keys(candidate_labels)
    ok = valid[r] & cvalid[c]
    if not ok.any():
        return float("nan"), 0
    return float((lab[r[ok]] == clab[c[ok]]).mean()), int(ok.sum())


_STAT_KEYS = ("auroc","n_related", "n_unrelated", "mean_related", "mean_unrelated")


def visualize_pairwise_similarity(labels, pairwise_similarity_metrics, plot='boxplot', title=None, figsize=(16, 9), save_path=None,
                                  **plot_kwargs):
    """The numbers behind the reference's ROC + box plot figure (helpers.py:79-135), computed on the device.

    Same arguments and asserts.  Pairs (i, j), j < i, with both labels >= 0 are 'related' when the labels are equal,
    'unrelated' otherwise; returns a dict with the AUROC of related-vs-unrelated scores (what ``roc_curve`` + ``auc`` give
    the reference), the population sizes, means and the box-plot five-number summaries.  Nothing is drawn (matplotlib is
    not part of this stack): with ``save_path`` the dict is written as JSON next to where the figure would have gone
    (``.png`` -> ``.json``).  ``pairwise_similarity_metrics`` may be an ndarray or a CUDA tensor (e.g. from
    ``pairwise_similarity(..., return_tensor=True)``)."""
    import ctypes
    import json
    import torch
    labels = np.asarray(labels)
    assert labels.shape[0] == pairwise_similarity_metrics.shape[0]
    assert pairwise_similarity_metrics.shape[0] == pairwise_similarity_metrics.shape[1]
    assert plot in ['scatter', 'boxplot']
    lib = L.load()
    S = pairwise_similarity_metrics
    if not isinstance(S, torch.Tensor):
        S = torch.as_tensor(np.asarray(S, dtype=np.float32))
    S = S.to(device="cuda" if not S.is_cuda else S.device, dtype=torch.float32)
    if S.stride(1) != 1:
        S = S.contiguous()
    N = int(S.shape[0])
    lab = np.asarray(labels).reshape(N, -1)[:, 0]
    if lab.dtype.kind == 'f':                      # NaN / inf 'missing' labels: the reference filters them with labels >= 0
        lab = np.where(np.isfinite(lab), lab, -1.0)
    lab = np.ascontiguousarray(lab.astype(np.int32))
    ws_bytes = int(lib.dae_pair_stats_workspace(N))
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=S.device)
    off = (-ws.data_ptr()) % 256
    out = (ctypes.c_double * 16)()
    with torch.cuda.device(S.device):
        L.call("dae_pair_stats", L.ptr(S), S.stride(0), lab.ctypes.data_as(ctypes.c_void_p), N, ctypes.cast(out, ctypes.c_void_p),
               ctypes.c_void_p(ws.data_ptr() + off), ws_bytes, L.current_stream())
    v = [float(x) for x in out]
    res = dict(zip(_STAT_KEYS, v[:5]))
    res["n_related"], res["n_unrelated"] = int(v[1]), int(v[2])
    res["related"] = dict(zip(("min", "q1", "median", "q3", "max"), v[5:10]))
    res["unrelated"] = dict(zip(("min", "q1", "median", "q3", "max"), v[10:15]))
    res["title"] = title
    if save_path is not None:
        path = str(save_path)
        path = path[:-4] + ".json" if path.lower().endswith(".png") else path + ".json"
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
    return res


def _label_ids(labels, n):
    """int32 labels by the missing-label rule of visualize_pairwise_similarity: negative, NaN and inf labels are missing (-1)."""
    lab = np.asarray(labels)
    if lab.shape[0] != n:
        raise ValueError(f"{lab.shape[0]} labels for {n} rows")
    lab = lab.reshape(n, -1)[:, 0]
    if lab.dtype.kind == 'f':
        lab = np.where(np.isfinite(lab), lab, -1.0)
    return np.ascontiguousarray(np.where(lab < 0, -1, lab).astype(np.int32))


def stats_from_histograms(hist_related, hist_unrelated, score_range, *, min_related=None, max_related=None, min_unrelated=None,
                          max_unrelated=None, sum_related=None, sum_unrelated=None):
    """AUROC and box-plot numbers of two score populations known only through their histograms over the same ``bins``
    equal-width bins of ``score_range = (lo, hi)`` (bin of ``s``: ``clamp(floor((s - lo) * bins / (hi - lo)), 0, bins - 1)``, so
    the two end bins also hold whatever lies outside the range).  Host code, integer arithmetic on the counts.

    * ``auroc``: pairs (related, unrelated) in different bins are ordered by their bins, pairs sharing a bin count as ties (1/2).
      ``auroc_low`` / ``auroc_high`` = ``auroc`` -/+ half the share of pairs sharing a bin: binning is monotone, so the exact
      tie-aware AUROC of the scores lies inside whatever their distribution -- a certificate, not an error estimate.
    * ``related`` / ``unrelated``: ``min``, ``q1``, ``median``, ``q3``, ``max`` at numpy's positions ``q * (n - 1)``: the two order
      statistics either side of the position are each represented by the midpoint of the bin that holds them (clipped to
      ``[min, max]``) and interpolated linearly as numpy does, so the error is at most half a bin, and a bin holding one
      distinct value at its centre (integer scores in unit bins) gives the exact quartile.  ``related_bounds`` /
      ``unrelated_bounds`` give, per quartile, the bracket (lower edge of the lower statistic's bin, upper edge of the upper
      one's) clipped to ``[min, max]``, which the exact quartile lies in; the edges are widened by the few fp32 roundings of the
      bin index.
    * ``min`` / ``max`` / ``sum`` of a class, when known exactly, are passed in; otherwise the outer edges of its first / last
      occupied bin and the midpoint sum stand in.  An empty class gives NaN, as ``visualize_pairwise_similarity`` does."""
    rel = [int(x) for x in np.asarray(hist_related).ravel()]
    un = [int(x) for x in np.asarray(hist_unrelated).ravel()]
    bins = len(rel)
    if len(un) != bins or bins < 1:
        raise ValueError("the two histograms must have the same, non-zero number of bins")
    lo, hi = float(np.float32(score_range[0])), float(np.float32(score_range[1]))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("score_range must be finite with lo < hi")
    if min(rel) < 0 or min(un) < 0:
        raise ValueError("negative count")
    span = float(np.float32(hi) - np.float32(lo))
    slack = 4.0 * 2.0 ** -24 * max(abs(lo), abs(hi), span)               # roundings of s - lo, * bins, / span, in score units
    nan = float("nan")
    n_rel, n_un = sum(rel), sum(un)
    res = {"auroc": nan, "n_related": n_rel, "n_unrelated": n_un, "mean_related": nan, "mean_unrelated": nan,
           "auroc_low": nan, "auroc_high": nan}
    if n_rel and n_un:
        below = wins2 = ties = 0                                         # wins2 = 2 * (wins + ties / 2)
        for b in range(bins):
            wins2 += rel[b] * (2 * below + un[b])
            ties += rel[b] * un[b]
            below += un[b]
        den = 2 * n_rel * n_un
        res["auroc"] = wins2 / den
        res["auroc_low"] = (wins2 - ties) / den
        res["auroc_high"] = (wins2 + ties) / den

    def edge(b):
        return lo + b * span / bins

    def one_class(h, n, vmin, vmax, vsum):
        five = dict.fromkeys(("min", "q1", "median", "q3", "max"), nan)
        bounds = {k: (nan, nan) for k in ("q1", "median", "q3")}
        if n == 0:
            return nan, five, bounds
        cum = np.cumsum(np.asarray(h, dtype=np.int64))
        first, last = int(np.searchsorted(cum, 0, side="right")), int(np.searchsorted(cum, n - 1, side="right"))
        vmin = edge(first) if vmin is None else float(vmin)
        vmax = edge(last + 1) if vmax is None else float(vmax)
        if vsum is None:
            vsum = float(sum(c * min(max(edge(b) + 0.5 * span / bins, vmin), vmax) for b, c in enumerate(h) if c))
        five["min"], five["max"] = vmin, vmax

        def clip(v):
            return min(max(v, vmin), vmax)
        for name, q in (("q1", 0.25), ("median", 0.5), ("q3", 0.75)):
            pos = q * (n - 1)
            r0, r1 = int(np.floor(pos)), int(np.ceil(pos))
            b0, b1 = int(np.searchsorted(cum, r0, side="right")), int(np.searchsorted(cum, r1, side="right"))
            v0, v1 = clip(edge(b0) + 0.5 * span / bins), clip(edge(b1) + 0.5 * span / bins)
            five[name] = v0 + (v1 - v0) * (pos - r0)
            # the end bins also hold whatever the clamp put there: their outer edges are min / max
            bounds[name] = (vmin if b0 == 0 else clip(edge(b0) - slack), vmax if b1 == bins - 1 else clip(edge(b1 + 1) + slack))
        return float(vsum) / n, five, bounds

    res["mean_related"], res["related"], res["related_bounds"] = one_class(rel, n_rel, min_related, max_related, sum_related)
    res["mean_unrelated"], res["unrelated"], res["unrelated_bounds"] = one_class(un, n_un, min_unrelated, max_unrelated, sum_unrelated)
    return res


def _label_stats_chunked(in_df, labels, candidates, candidate_labels, norm, metric, bins, chunk_rows, device):
    """``label_similarity_stats(chunk_rows=...)``: returns ``sweep(lo, hi) -> (out16 as a list, hist uint64 [2 x bins])``, the
    numbers one ``dae_pair_hist`` call returns, summed over the blocks of ``label_stats_blocks`` (``dae_pair_hist_images``; one
    query image and one corpus image at a time).  Histograms, counts and ``n_nan`` add as integers, min / max combine, the fp64
    sums add in block order.  The automatic range of the linear kernel is rebuilt from the largest squared row norm of every
    chunk image (``dae_sweep_image_norm2_max``; a maximum does not depend on the chunking), with ``dae_pair_hist``'s arithmetic."""
    import ctypes
    import math
    import torch
    lib, dev, Qo, Co, Nq, Nc, D = _chunked_operands(in_df, candidates, norm, metric, device)
    lq = _label_ids(labels, Nq)
    lc = lq if Co is None else _label_ids(candidate_labels, Nc)
    c = sweep_chunk_rows(chunk_rows, D)
    cq, cc = min(c, L.pad(Nq)), min(c, L.pad(Nc))
    qb, cb = int(lib.dae_sweep_image_bytes(cq, D)), int(lib.dae_sweep_image_bytes(cc, D))
    q_p, q_t = _workspace(dev, qb)
    c_p, c_t = _workspace(dev, cb)
    ws_bytes = max(int(lib.dae_pair_hist_images_workspace(cq, cc, bins)), int(lib.dae_sweep_image_norm2_max_workspace()))
    ws_p, ws = _workspace(dev, ws_bytes)
    q_plan, c_plan = sweep_chunk_plan(Nq, c), sweep_chunk_plan(Nc, c)
    blocks = label_stats_blocks(len(q_plan), None if Co is None else len(c_plan))
    auto = {}

    def norm2_max(op, plan, image_p, image_bytes):
        best, out = 0.0, ctypes.c_double()
        for a0, a1 in plan:
            op.image(torch, a0, a1, image_p, image_bytes, norm, metric)
            L.call("dae_sweep_image_norm2_max", image_p, a1 - a0, D, ctypes.byref(out), ws_p, ws_bytes, L.current_stream())
            best = max(best, float(out.value))
        return best

    def auto_range():
        if metric == "cosine":
            return -1.0, 1.0
        if not auto:
            mq = norm2_max(Qo, q_plan, q_p, qb)
            mc = mq if Co is None else norm2_max(Co, c_plan, c_p, cb)
            M = math.sqrt(mq) * math.sqrt(mc) * (1.0 + 1.0 / 1048576.0)
            with np.errstate(over="ignore"):
                Mf = np.float32(M)
            if float(Mf) < M:
                Mf = np.nextafter(Mf, np.float32(np.inf))
            if not (Mf > 0 and np.isfinite(Mf)):
                Mf = np.float32(1.0)                                      # all-zero rows (every score is 0) / overflowing norms
            auto["M"] = float(Mf)
        return -auto["M"], auto["M"]

    def sweep(lo, hi):
        if lo >= hi:
            lo, hi = auto_range()
        total = np.zeros((2, bins), dtype=np.uint64)
        hist = np.zeros((2, bins), dtype=np.uint64)
        out = (ctypes.c_double * 16)()
        nan = float("nan")
        n, n_nan, sums, mins, maxs, tiles, rng = [0, 0], 0, [0.0, 0.0], [nan, nan], [nan, nan], 0.0, (lo, hi)
        have = None
        with torch.cuda.device(dev):
            for a, b, self_mode in blocks:
                q0, q1 = q_plan[a]
                if have != a:
                    Qo.image(torch, q0, q1, q_p, qb, norm, metric)
                    have = a
                if self_mode:
                    c0, c1 = q0, q1
                else:
                    c0, c1 = c_plan[b]
                    (Qo if Co is None else Co).image(torch, c0, c1, c_p, cb, norm, metric)
                lqa, lcb = np.ascontiguousarray(lq[q0:q1]), np.ascontiguousarray(lc[c0:c1])
                L.call("dae_pair_hist_images", q_p, q1 - q0, lqa.ctypes.data_as(ctypes.c_void_p), None if self_mode else c_p, c1 - c0,
                       lcb.ctypes.data_as(ctypes.c_void_p), D, lo, hi, bins, hist.ctypes.data_as(ctypes.c_void_p),
                       ctypes.cast(out, ctypes.c_void_p), ws_p, ws_bytes, L.current_stream())
                v = [float(x) for x in out]
                total += hist
                n_nan += int(v[2])
                tiles += v[12]
                rng = (v[9], v[10])
                for cls in range(2):
                    if v[cls] > 0:
                        n[cls] += int(v[cls])
                        sums[cls] += v[3 + cls]
                        mins[cls] = v[5 + 2 * cls] if mins[cls] != mins[cls] else min(mins[cls], v[5 + 2 * cls])
                        maxs[cls] = v[6 + 2 * cls] if maxs[cls] != maxs[cls] else max(maxs[cls], v[6 + 2 * cls])
        v = [nan] * 16
        v[0], v[1], v[2] = float(n[0]), float(n[1]), float(n_nan)
        for cls in range(2):
            if n[cls]:
                v[3 + cls], v[5 + 2 * cls], v[6 + 2 * cls] = sums[cls], mins[cls], maxs[cls]
        v[9], v[10], v[11], v[12] = rng[0], rng[1], float(len(blocks)), tiles
        return v, total

    sweep.keep = (q_t, c_t, ws)
    return sweep


def label_similarity_stats(in_df, labels, norm="", metric="cosine", candidates=None, candidate_labels=None, *, bins=2048,
                           score_range=None, refine=False, return_histograms=False, save_path=None, title=None, chunk_rows=None,
                           device=None):
    """The numbers of ``visualize_pairwise_similarity(labels, pairwise_similarity(in_df, norm, metric))`` without the N x N matrix:
    ``dae_pair_hist`` bins every pair's score (same ``norm`` / ``metric``, same exact-fp32 products as ``similar_pairs``) into one
    histogram per class inside the GEMM's epilogue, and ``stats_from_histograms`` derives the statistics.

    Pairs and classes as there: without ``candidates`` the pairs ``j < i`` of ``in_df``; with ``candidates`` (and their
    ``candidate_labels``) every (row, candidate) pair; a pair counts when both labels are present (negative, NaN and inf labels
    are missing) and is related when they are equal.  Inputs take the containers of ``similar_pairs``.

    Returns the dict of ``visualize_pairwise_similarity`` -- ``auroc``, ``n_related``, ``n_unrelated``, ``mean_related``,
    ``mean_unrelated``, the ``related`` / ``unrelated`` five-number dicts, ``title`` -- plus ``auroc_low`` / ``auroc_high`` (a bracket
    that is certain to hold the exact tie-aware AUROC of the same scores; its width is the share of pairs sharing a bin),
    ``related_bounds`` / ``unrelated_bounds`` (brackets of the quartiles), ``score_range``, ``bins``, ``n_nan`` (pairs with a NaN
    score: in no bin and in no count).  ``min``, ``max`` and the means are exact (fp32 values; fp64 sums); the counts are
    integers and the sums are reduced in a fixed shape, so the result is bit-identical run to run.

    ``bins`` <= 2048.  ``score_range=None`` is the automatic range: [-1, 1] for cosine, the Cauchy-Schwarz bound of the row norms
    for the linear kernel.  ``refine=True`` calls the library a second time over ``(min, max)`` of the scores seen in the first
    call, which narrows the brackets when the automatic range is much wider than the data (raw linear-kernel scores with one
    long row); the first call's bracket is kept under ``first_pass``.  ``return_histograms=True`` adds ``hist_related``,
    ``hist_unrelated`` (uint64) and ``bin_edges`` (float64, bins + 1): enough to draw the ROC curve and the box plot.
    ``save_path`` writes the dict (without the arrays) as JSON with the ``.png`` -> ``.json`` rule of
    ``visualize_pairwise_similarity``.

    ``chunk_rows`` (default None: both operands whole, as dense fp32 images -- each must stay below 4 GiB) as in ``most_similar``:
    the operands are swept in blocks of that many rows, a scipy.sparse input as CSR (``_label_stats_chunked``).  Histograms,
    counts, ``n_nan``, ``min``, ``max`` and the score range equal those of ``chunk_rows=None`` exactly; the fp64 score sums are added
    block by block, so the means agree to rounding (1e-12 relative), not bit for bit."""
    import ctypes
    import json
    import torch
    lib = L.load()
    bins = int(bins)
    if not 2 <= bins <= int(lib.dae_pair_hist_max_bins()):
        raise ValueError(f"bins must be in 2..{int(lib.dae_pair_hist_max_bins())} (got {bins})")
    if (candidates is None) != (candidate_labels is None):
        raise ValueError("candidates and candidate_labels go together")
    if score_range is None:
        lo, hi = 0.0, 0.0                                             # lo >= hi: the library's automatic range
    else:
        lo, hi = float(score_range[0]), float(score_range[1])
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError("score_range must be finite with lo < hi")
    if chunk_rows is not None:
        sweep = _label_stats_chunked(in_df, labels, candidates, candidate_labels, norm, metric, bins, chunk_rows, device)
    else:
        lib, dev, Q, Cm, Nq, Nc, D = _sweep_inputs(in_df, candidates, norm, metric, device)
        lq = _label_ids(labels, Nq)
        lc = None if Cm is None else _label_ids(candidate_labels, Nc)
        ws_bytes = int(lib.dae_pair_hist_workspace(Nq, Nc, D, bins))
        ws_p, ws = _workspace(dev, ws_bytes)

        def sweep(lo, hi):
            hist = np.zeros((2, bins), dtype=np.uint64)
            out = (ctypes.c_double * 16)()
            with torch.cuda.device(dev):
                L.call("dae_pair_hist", L.ptr(Q), Q.stride(0), Nq, lq.ctypes.data_as(ctypes.c_void_p), L.ptr(Cm),
                       0 if Cm is None else Cm.stride(0), Nc, None if lc is None else lc.ctypes.data_as(ctypes.c_void_p), D, _NORMS[norm],
                       _METRICS[metric], lo, hi, bins, hist.ctypes.data_as(ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p),
                       ws_p, ws_bytes, L.current_stream())
            return [float(x) for x in out], hist

    def run(lo, hi):
        v, hist = sweep(lo, hi)
        have_r, have_u = v[0] > 0, v[1] > 0
        st = stats_from_histograms(hist[0], hist[1], (v[9], v[10]),
                                   min_related=v[5] if have_r else None, max_related=v[6] if have_r else None,
                                   min_unrelated=v[7] if have_u else None, max_unrelated=v[8] if have_u else None,
                                   sum_related=v[3] if have_r else None, sum_unrelated=v[4] if have_u else None)
        st["score_range"] = (v[9], v[10])
        st["bins"] = bins
        st["n_nan"] = int(v[2])
        return st, hist

    res, hist = run(lo, hi)
    if refine:
        seen = [res[c][k] for c, n in (("related", "n_related"), ("unrelated", "n_unrelated")) if res[n] for k in ("min", "max")]
        if seen and np.isfinite(min(seen)) and np.isfinite(max(seen)) and min(seen) < max(seen):
            first = {k: res[k] for k in ("auroc", "auroc_low", "auroc_high", "score_range")}
            res, hist = run(min(seen), max(seen))
            res["first_pass"] = first
    res["title"] = title
    if save_path is not None:
        path = str(save_path)
        path = path[:-4] + ".json" if path.lower().endswith(".png") else path + ".json"
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
    if return_histograms:
        lo_, hi_ = res["score_range"]
        span = float(np.float32(hi_) - np.float32(lo_))
        res["hist_related"], res["hist_unrelated"] = hist[0].copy(), hist[1].copy()
        res["bin_edges"] = lo_ + np.arange(bins + 1, dtype=np.float64) * span / bins
    return res
