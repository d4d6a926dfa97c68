"""The word-based user model in NumPy: the rules of include/dae_hip.h (dae_word_profiles / dae_word_topk / dae_word_rank) restated
with np.float32 arithmetic, one operation per rounding, so that the device result can be compared bit for bit.  Test
infrastructure: plain loops, no attempt at speed."""
import numpy as np

F32 = np.float32


def csr_parts(articles):
    """``(indptr int64, indices int64, values float32 or None)`` of a scipy CSR matrix or of a ``(indptr, indices, values)`` tuple."""
    if isinstance(articles, tuple):
        ip, ix, vl = articles
        return np.asarray(ip, dtype=np.int64), np.asarray(ix, dtype=np.int64), None if vl is None else np.asarray(vl, dtype=F32)
    m = articles.tocsr()
    return m.indptr.astype(np.int64), m.indices.astype(np.int64), m.data.astype(F32)


def profiles_reference(indptr, items, articles, V, max_events=None):
    """The profiles as a boolean array ``[users x V]``: word w of user u is set when some article among the user's last
    ``max_events`` clicks stores column w.  Items and columns out of range are dropped."""
    ip, ix, _ = csr_parts(articles)
    Na = ip.size - 1
    indptr, items = np.asarray(indptr, dtype=np.int64), np.asarray(items, dtype=np.int64)
    P = np.zeros((indptr.size - 1, int(V)), dtype=bool)
    for u in range(indptr.size - 1):
        h = items[indptr[u]:indptr[u + 1]]
        if max_events is not None:
            h = h[max(h.size - int(max_events), 0):]
        for a in h:
            if 0 <= a < Na:
                c = ix[ip[a]:ip[a + 1]]
                P[u, c[(c >= 0) & (c < V)]] = True
    return P


def entry_weights_reference(articles, V, term_weights=None):
    """One float32 weight per stored entry: the value (1 without values), times the column's term weight in one fp32 rounding;
    +0 for a column out of range."""
    ip, ix, vl = csr_parts(articles)
    x = np.ones(ix.size, dtype=F32) if vl is None else vl
    ok = (ix >= 0) & (ix < V)
    if term_weights is None:
        e = x.copy()
    else:
        tw = np.asarray(term_weights, dtype=F32)
        e = tw[np.where(ok, ix, 0)] * x                                 # float32 * float32: one rounding
    return np.where(ok, e, F32(0)).astype(F32)


def scores_reference(P, articles, term_weights=None):
    """``R [users x Na]`` float32: per pair the sequential fp32 sum, in storage order, of the article's entry weights over the words
    in the user's profile, from +0 (an absent word adds +0)."""
    ip, ix, _ = csr_parts(articles)
    M, V = P.shape
    e = entry_weights_reference(articles, V, term_weights)
    Na = ip.size - 1
    R = np.zeros((M, Na), dtype=F32)
    zero = np.zeros(M, dtype=F32)
    for a in range(Na):
        s = np.zeros(M, dtype=F32)
        for p in range(ip[a], ip[a + 1]):
            c = ix[p]
            if 0 <= c < V:
                s = (s + np.where(P[:, c], e[p], zero)).astype(F32)     # one fp32 add per entry, all users at once
        R[:, a] = s
    return R


def _admitted(R, u, seen, window):
    Na = R.shape[1]
    ok = np.ones(Na, dtype=bool)
    if window is not None:
        lo, hi = int(window[0][u]), int(window[1][u])
        ok[:max(lo, 0)] = False
        ok[max(hi, 0):] = False
    if seen is not None:
        s = np.asarray(seen[u], dtype=np.int64)
        ok[s[(s >= 0) & (s < Na)]] = False
    return ok


def topk_reference(R, k, seen=None, window=None):
    """``(indices int64 [users x k], scores float32 [users x k])``: score descending, index ascending, -0 and +0 one score, after
    the exclusion lists ``seen`` (a list of sequences) and the windows ``(lo, hi)``; tails -1 / -inf."""
    M, Na = R.shape
    idx = np.full((M, k), -1, dtype=np.int64)
    sc = np.full((M, k), -np.inf, dtype=F32)
    for u in range(M):
        cand = np.flatnonzero(_admitted(R, u, seen, window))
        s = R[u, cand] + F32(0)                                          # -0 + +0 = +0
        order = np.lexsort((cand, -s.astype(np.float64)))[:k]
        idx[u, :order.size] = cand[order]
        sc[u, :order.size] = s[order]
    return idx, sc


def ranks_reference(R, targets, seen=None, window=None):
    """``(rank int64, target_score float32)``: 1 + the admitted articles other than the target whose (score, index) pair is ahead
    of the target's; 0 / -inf without a target.  The target is ranked whether or not it is admitted itself."""
    M, Na = R.shape
    rank = np.zeros(M, dtype=np.int64)
    ts = np.full(M, -np.inf, dtype=F32)
    for u in range(M):
        t = int(targets[u])
        if t < 0:
            continue
        ok = _admitted(R, u, seen, window)
        ok[t] = False
        s = R[u].astype(np.float64)
        ahead = (s > s[t]) | ((s == s[t]) & (np.arange(Na) < t))
        rank[u] = 1 + int((ahead & ok).sum())
        ts[u] = R[u, t]
    return rank, ts
