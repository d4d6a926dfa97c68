"""The co-visitation model in NumPy: the rules of include/dae_hip.h (dae_covisit_neighbors / dae_covisit_recommend) restated with
np.float32 arithmetic, one operation per rounding, so that the device result can be compared bit for bit.  Test infrastructure:
plain loops, no attempt at speed."""
import numpy as np

F32 = np.float32


def covisit_records(indptr, items, window, both):
    """Every record ``(a, b)`` of the log as an int64 ``[R x 2]`` array, in the order of the rules: users ascending, ``p`` ascending,
    ``q`` ascending, with ``both`` the mirrored record right behind."""
    indptr, items = np.asarray(indptr, dtype=np.int64), np.asarray(items, dtype=np.int64)
    rec = []
    for u in range(indptr.size - 1):
        h = items[indptr[u]:indptr[u + 1]]
        for p in range(h.size):
            for q in range(p + 1, min(p + int(window), h.size - 1) + 1):
                a, b = int(h[p]), int(h[q])
                if a != b:
                    rec.append((a, b))
                    if both:
                        rec.append((b, a))
    return np.asarray(rec, dtype=np.int64).reshape(-1, 2)


def covisit_reference(indptr, items, Na, window, both, cosine, K):
    """The neighbour table: a dict of ``nbr`` int32 / ``sim`` float32 / ``cnt`` int32 ``[Na x K]`` (tails -1 / 0 / 0), ``degree``,
    ``clicks`` int32 ``[Na]``, ``n_records`` and ``n_pairs``."""
    Na, K = int(Na), int(K)
    items = np.asarray(items, dtype=np.int64)
    rec = covisit_records(indptr, items, window, both)
    clicks = np.bincount(items, minlength=Na).astype(np.int32)
    nbr = np.full((Na, K), -1, dtype=np.int32)
    sim = np.zeros((Na, K), dtype=F32)
    cnt = np.zeros((Na, K), dtype=np.int32)
    degree = np.zeros(Na, dtype=np.int32)
    keys, c = np.unique(rec[:, 0] * Na + rec[:, 1], return_counts=True)
    a_of, b_of = keys // Na, keys % Na
    if cosine:
        prod = clicks[a_of].astype(F32) * clicks[b_of].astype(F32)      # one fp32 rounding
        s = c.astype(F32) / np.sqrt(prod)                               # fp32 sqrt and fp32 division, each correctly rounded
    else:
        s = c.astype(F32)
    assert s.dtype == F32
    for a in np.unique(a_of):
        sel = np.flatnonzero(a_of == a)
        degree[a] = sel.size
        order = sel[np.lexsort((b_of[sel], -s[sel].astype(np.float64)))][:K]      # s descending, b ascending
        nbr[a, :order.size], sim[a, :order.size], cnt[a, :order.size] = b_of[order], s[order], c[order]
    return {"nbr": nbr, "sim": sim, "cnt": cnt, "degree": degree, "clicks": clicks, "n_records": int(rec.shape[0]),
            "n_pairs": int(keys.size)}


def covisit_recommend_reference(nbr, sim, indptr, items, seen_indptr, seen_items, age_weight, last, k, window=None):
    """The recommendation lists from a table: ``(indices int32 [M x k], scores float32 [M x k])``, tails -1 / -inf.  ``seen_*`` is a
    CSR of the users' seen articles (any order); ``window``: None or a pair ``(lo, hi)`` of per-user arrays."""
    indptr, items = np.asarray(indptr, dtype=np.int64), np.asarray(items, dtype=np.int64)
    seen_indptr, seen_items = np.asarray(seen_indptr, dtype=np.int64), np.asarray(seen_items, dtype=np.int64)
    w = np.asarray(age_weight, dtype=F32)
    M, last, k = indptr.size - 1, int(last), int(k)
    idx = np.full((M, k), -1, dtype=np.int32)
    score = np.full((M, k), -np.inf, dtype=F32)
    for u in range(M):
        h = items[indptr[u]:indptr[u + 1]]
        n = min(last, h.size)
        acc = {}
        for o in range(n):                                               # the sources, oldest first
            x, age = int(h[h.size - n + o]), n - 1 - o
            for t in range(nbr.shape[1]):
                c = int(nbr[x, t])
                if c < 0:
                    continue
                acc[c] = F32(acc.get(c, F32(0)) + F32(w[age] * F32(sim[x, t])))
        mine = set(int(v) for v in seen_items[seen_indptr[u]:seen_indptr[u + 1]])
        cand = [(c, s) for c, s in acc.items() if c not in mine
                and (window is None or int(window[0][u]) <= c < int(window[1][u]))]
        cand.sort(key=lambda cs: (-float(cs[1]), cs[0]))                 # -0.0 and +0.0 compare equal here, as on the device
        for t, (c, s) in enumerate(cand[:k]):
            idx[u, t], score[u, t] = c, s
    return idx, score
