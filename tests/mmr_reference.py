"""The diversification of recommendation lists (include/dae_hip.h: dae_mmr_lists) as a short NumPy function.

A row of ``lists`` holds candidate indices, ``rel`` one relevance each.  Position p is valid iff 0 <= list[p] < S.shape[0] and
rel[p] is finite.  m = 0 everywhere, alive = valid; each of at most k steps computes, for the alive positions,
v = lam * rel - (1 - lam) * m with a separate multiply and subtract, selects the largest v (the lowest position among equals),
records (index, position, v, m), then m = fmax(m, S[list[selected], list[candidate]]), drops the candidates whose score to the
selected reaches a finite ``threshold`` and, with ``max_per_label`` > 0, every candidate of the selected's label (if >= 0) once that
many carry it.

Everything is computed in S's dtype: with float32 ``S``, ``rel`` and ``lam`` (the library's own pairwise_similarity) every
operation is one correctly rounded fp32 operation and the result is the bit contract; with the oracle's float64 ``S`` it is exact
arithmetic.  tests/test_mmr_cpu.py pins it on hand-made cases; tests/test_hip_mmr.py compares the kernel with it.
"""
import numpy as np


def _steps(row, rel_row, S, k, lam, lab, cap, threshold):
    """One row; yields per step (position, v of it, m of it, gap to the runner-up or inf, the scores of the selected to the alive)."""
    dt = S.dtype.type
    L = row.size
    Na = S.shape[0]
    with np.errstate(invalid="ignore"):
        r = rel_row.astype(dt)
        valid = (row >= 0) & (row < Na) & np.isfinite(r)
    safe = np.where(valid, row, 0)
    lam, one = dt(lam), dt(1)
    oml = one - lam
    m = np.zeros(L, dt)
    alive = valid.copy()
    picked = []
    while len(picked) < k and alive.any():
        with np.errstate(invalid="ignore", over="ignore"):
            v = lam * r - oml * m                               # two roundings each side: numpy never fuses
        best = np.fmax.reduce(np.where(alive, v, dt(-np.inf)))
        eq = alive & (v == best)
        p = int(np.flatnonzero(eq if eq.any() else alive)[0])   # the lowest position; (every alive v NaN: the lowest alive)
        others = np.sort(v[alive])
        gap = float(others[-1] - others[-2]) if others.size > 1 else np.inf
        alive[p] = False
        picked.append(p)
        s = S[safe[p], safe]
        yield p, v[p], m[p], gap, s[alive]
        m = np.fmax(m, s)
        if np.isfinite(threshold):
            with np.errstate(invalid="ignore"):
                alive &= ~(s >= dt(threshold))
        if cap > 0 and lab is not None and valid[p] and lab[p] >= 0:
            if sum(lab[q] == lab[p] for q in picked) >= cap:
                alive &= lab != lab[p]


def mmr_reference(lists, rel, S, k, lam, labels=None, max_per_label=0, threshold=np.inf):
    """Returns (out_idx, out_pos int64 [Nr x k], tail -1; out_val, out_near in S's dtype [Nr x k], tail -inf; counts int64
    [Nr x 2]: the number selected, and how many of the selected are not among the first k valid positions)."""
    lists = np.asarray(lists).astype(np.int64)
    rel = np.asarray(rel)
    S = np.asarray(S)
    Nr, L = lists.shape
    assert 1 <= k <= L and rel.shape == lists.shape
    labels = None if labels is None else np.asarray(labels).astype(np.int64)
    out_idx = np.full((Nr, k), -1, np.int64)
    out_pos = np.full((Nr, k), -1, np.int64)
    out_val = np.full((Nr, k), -np.inf, S.dtype)
    out_near = np.full((Nr, k), -np.inf, S.dtype)
    counts = np.zeros((Nr, 2), np.int64)
    for i in range(Nr):
        row = lists[i]
        inside = (row >= 0) & (row < S.shape[0])
        with np.errstate(invalid="ignore"):
            valid = inside & np.isfinite(rel[i].astype(S.dtype))
        lab = None if labels is None else np.where(inside, labels[np.where(inside, row, 0)], -1)
        first_k = set(np.flatnonzero(valid)[:k].tolist())
        for t, (p, v, m, _, _) in enumerate(_steps(row, rel[i], S, k, lam, lab, int(max_per_label), threshold)):
            out_idx[i, t], out_pos[i, t], out_val[i, t], out_near[i, t] = row[p], p, v, m
            counts[i, 0] += 1
            counts[i, 1] += p not in first_k
    return out_idx, out_pos, out_val, out_near, counts


def near_tie_rows_mmr(lists, rel, S, k, lam, band, labels=None, max_per_label=0, threshold=np.inf, tol=0.0):
    """Rows whose selection fp32 arithmetic may take either way (bool [Nr]): some step of the run on ``S`` (the oracle's float64)
    has a gap 0 < v_best - v_second <= band, or -- with a finite threshold -- a score of the selected to an alive candidate within
    ``tol`` of the threshold."""
    lists = np.asarray(lists).astype(np.int64)
    rel = np.asarray(rel)
    S = np.asarray(S)
    labels = None if labels is None else np.asarray(labels).astype(np.int64)
    out = np.zeros(lists.shape[0], bool)
    for i, row in enumerate(lists):
        inside = (row >= 0) & (row < S.shape[0])
        lab = None if labels is None else np.where(inside, labels[np.where(inside, row, 0)], -1)
        for _, _, _, gap, s in _steps(row, rel[i], S, k, lam, lab, int(max_per_label), threshold):
            if 0 < gap <= band or (np.isfinite(threshold) and s.size and (np.abs(s - threshold) <= tol).any()):
                out[i] = True
                break
    return out
