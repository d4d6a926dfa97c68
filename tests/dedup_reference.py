"""The greedy de-duplication of recommendation lists (include/dae_hip.h: dae_dedup_lists) as a short NumPy function.

A row of ``lists`` holds candidate indices, best first.  Walking it front to back, the entry at position p is kept iff no entry
kept at a position q < p has S[lists[p], lists[q]] >= threshold; the walk stops after k kept.  Entries < 0 or >= S.shape[0] are
skipped and never kept.  ``S`` is any score matrix: float64 from the oracle for the tests against exact arithmetic, or the
library's own float32 pairwise_similarity for the bit contract.  The comparison is made in S's dtype against ``threshold`` as
given (pass a numpy float32 to compare in float32).

tests/test_dedup_cpu.py pins it on hand-made cases; tests/test_hip_dedup.py compares the kernel with it.
"""
import numpy as np


def dedup_reference(lists, S, k, threshold):
    """Returns (out_idx [Nr x k], out_pos [Nr x k], counts [Nr x 2]) as int64; -1 where fewer than k survive.
    counts[:, 0]: the number kept; counts[:, 1]: the pairs q < p < min(k, L) of valid entries with S >= threshold."""
    lists = np.asarray(lists)
    S = np.asarray(S)
    Nr, L = lists.shape
    Na = S.shape[0]
    assert 1 <= k <= L
    out_idx = np.full((Nr, k), -1, np.int64)
    out_pos = np.full((Nr, k), -1, np.int64)
    counts = np.zeros((Nr, 2), np.int64)
    for i in range(Nr):
        row = lists[i].astype(np.int64)
        valid = (row >= 0) & (row < Na)
        safe = np.where(valid, row, 0)
        dup = (S[np.ix_(safe, safe)] >= threshold) & valid[:, None] & valid[None, :]       # dup[p, q]
        kept = []
        for p in range(L):
            if len(kept) == k:
                break
            if valid[p] and not dup[p, kept].any():
                kept.append(p)
        out_idx[i, :len(kept)] = row[kept]
        out_pos[i, :len(kept)] = kept
        b = min(k, L)
        counts[i] = len(kept), int(np.tril(dup[:b, :b], -1).sum())
    return out_idx, out_pos, counts


def near_tie_rows(lists, S, threshold, tol):
    """Rows of ``lists`` with a pair q < p of valid entries whose score lies within ``tol`` of the threshold (bool [Nr]): the rows
    whose decisions fp32 arithmetic may take either way."""
    lists = np.asarray(lists)
    S = np.asarray(S)
    Na = S.shape[0]
    out = np.zeros(lists.shape[0], bool)
    for i, row in enumerate(lists.astype(np.int64)):
        v = row[(row >= 0) & (row < Na)]
        near = np.abs(S[np.ix_(v, v)] - threshold) <= tol
        out[i] = np.tril(near, -1).any()
    return out
