"""Scoring similarities against labels.  ``visualize_pairwise_similarity`` (the reference's helpers.py:79-135): the AUROC and the
box-plot numbers of related against unrelated pairs, from an N x N score matrix; ``label_similarity_stats``: the same numbers
without that matrix (``dae_pair_hist`` reduces the score tiles to one histogram per class, ``stats_from_histograms`` derives the
statistics and the brackets that certify them), one-shot or in chunks.  Host code on top of the other sweeps: ``label_precision_at_k``
(of a ``most_similar`` result), ``duplicate_groups`` and ``duplicate_pair_precision`` (of a ``similar_pairs`` result)."""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ._device import workspace
from .sweeps import label_stats_blocks, sweep_chunk_plan, sweep_chunk_rows, sweep_start


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
    lab = _label_ids(labels, N)                    # NaN / inf / negative labels are missing: the reference filters with labels >= 0
    ws_bytes = int(lib.dae_pair_stats_workspace(N))
    ws_p, ws = workspace(S.device, ws_bytes)
    out = (ctypes.c_double * 16)()
    with torch.cuda.device(S.device):
        L.call("dae_pair_stats", L.ptr(S), S.stride(0), lab.ctypes.data_as(ctypes.c_void_p), N, ctypes.cast(out, ctypes.c_void_p),
               ws_p, ws_bytes, L.current_stream())
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


# The slots of the 16 doubles ``dae_pair_hist`` / ``dae_pair_hist_images`` return beside the histograms; the pairs are indexed by
# class (0: related, 1: unrelated).  The slots not named here stay NaN.
_N, _N_NAN, _SUM, _MIN, _MAX, _LO, _HI, _GRID, _TILES = (0, 1), 2, (3, 4), (5, 7), (6, 8), 9, 10, 11, 12


def _label_stats_chunked(in_df, labels, candidates, candidate_labels, norm, metric, bins, chunk_rows, device):
    """``label_similarity_stats(chunk_rows=...)``: returns ``sweep(lo, hi) -> (out16 as a list, hist uint64 [2 x bins])``, the
    numbers one ``dae_pair_hist`` call returns, summed over the blocks of ``label_stats_blocks`` (``dae_pair_hist_images``; one
    query image and one corpus image at a time).  Histograms, counts and ``n_nan`` add as integers, min / max combine, the fp64
    sums add in block order.  The automatic range of the linear kernel is rebuilt from the largest squared row norm of every
    chunk image (``dae_sweep_image_norm2_max``; a maximum does not depend on the chunking), with ``dae_pair_hist``'s arithmetic."""
    import ctypes
    import math
    torch, lib, dev, Qo, Co, Nq, Nc, D, nm = sweep_start(in_df, candidates, norm, metric, device, chunked=True)
    lq = _label_ids(labels, Nq)
    lc = lq if Co is None else _label_ids(candidate_labels, Nc)
    c = sweep_chunk_rows(chunk_rows, D)
    cq, cc = min(c, L.pad(Nq)), min(c, L.pad(Nc))
    qb, cb = int(lib.dae_sweep_image_bytes(cq, D)), int(lib.dae_sweep_image_bytes(cc, D))
    q_p, q_t = workspace(dev, qb)
    c_p, c_t = workspace(dev, cb)
    ws_bytes = max(int(lib.dae_pair_hist_images_workspace(cq, cc, bins)), int(lib.dae_sweep_image_norm2_max_workspace()))
    ws_p, ws = workspace(dev, ws_bytes)
    q_plan, c_plan = sweep_chunk_plan(Nq, c), sweep_chunk_plan(Nc, c)
    blocks = label_stats_blocks(len(q_plan), None if Co is None else len(c_plan))
    auto = {}

    def norm2_max(op, plan, image_p, image_bytes):
        best, out = 0.0, ctypes.c_double()
        for a0, a1 in plan:
            op.image(torch, a0, a1, image_p, image_bytes, nm)
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
                    Qo.image(torch, q0, q1, q_p, qb, nm)
                    have = a
                if self_mode:
                    c0, c1 = q0, q1
                else:
                    c0, c1 = c_plan[b]
                    (Qo if Co is None else Co).image(torch, c0, c1, c_p, cb, nm)
                lqa, lcb = np.ascontiguousarray(lq[q0:q1]), np.ascontiguousarray(lc[c0:c1])
                L.call("dae_pair_hist_images", q_p, q1 - q0, lqa.ctypes.data_as(ctypes.c_void_p), None if self_mode else c_p, c1 - c0,
                       lcb.ctypes.data_as(ctypes.c_void_p), D, lo, hi, bins, hist.ctypes.data_as(ctypes.c_void_p),
                       ctypes.cast(out, ctypes.c_void_p), ws_p, ws_bytes, L.current_stream())
                v = [float(x) for x in out]
                total += hist
                n_nan += int(v[_N_NAN])
                tiles += v[_TILES]
                rng = (v[_LO], v[_HI])
                for cls in range(2):
                    if v[_N[cls]] > 0:
                        n[cls] += int(v[_N[cls]])
                        sums[cls] += v[_SUM[cls]]
                        mins[cls] = v[_MIN[cls]] if mins[cls] != mins[cls] else min(mins[cls], v[_MIN[cls]])
                        maxs[cls] = v[_MAX[cls]] if maxs[cls] != maxs[cls] else max(maxs[cls], v[_MAX[cls]])
        v = [nan] * 16
        v[_N_NAN], v[_LO], v[_HI], v[_GRID], v[_TILES] = float(n_nan), rng[0], rng[1], float(len(blocks)), tiles
        for cls in range(2):
            v[_N[cls]] = float(n[cls])
            if n[cls]:
                v[_SUM[cls]], v[_MIN[cls]], v[_MAX[cls]] = sums[cls], mins[cls], maxs[cls]
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
        torch, lib, dev, Q, Cm, Nq, Nc, D, nm = sweep_start(in_df, candidates, norm, metric, device)
        lq = _label_ids(labels, Nq)
        lc = None if Cm is None else _label_ids(candidate_labels, Nc)
        ws_bytes = int(lib.dae_pair_hist_workspace(Nq, Nc, D, bins))
        ws_p, ws = workspace(dev, ws_bytes)

        def sweep(lo, hi):
            hist = np.zeros((2, bins), dtype=np.uint64)
            out = (ctypes.c_double * 16)()
            with torch.cuda.device(dev):
                L.call("dae_pair_hist", L.ptr(Q), Q.stride(0), Nq, lq.ctypes.data_as(ctypes.c_void_p), L.ptr(Cm),
                       0 if Cm is None else Cm.stride(0), Nc, None if lc is None else lc.ctypes.data_as(ctypes.c_void_p), D, *nm, lo, hi,
                       bins, hist.ctypes.data_as(ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p), ws_p, ws_bytes, L.current_stream())
            return [float(x) for x in out], hist

    def run(lo, hi):
        v, hist = sweep(lo, hi)
        exact = {f"{what}_{name}": v[slot[cls]] if v[_N[cls]] > 0 else None for cls, name in enumerate(("related", "unrelated"))
                 for what, slot in (("min", _MIN), ("max", _MAX), ("sum", _SUM))}
        st = stats_from_histograms(hist[0], hist[1], (v[_LO], v[_HI]), **exact)
        st["score_range"] = (v[_LO], v[_HI])
        st["bins"] = bins
        st["n_nan"] = int(v[_N_NAN])
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
