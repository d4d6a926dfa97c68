"""Seeded synthetic inputs of the shapes BASELINE.json names (the UCI-news blob is missing from the
reference checkout: .MISSING_LARGE_BLOBS:2).  Recipe from SURVEY.md section 8(d): row nnz ~ clipped
Poisson(lambda), columns Zipf(s~1.1) without replacement per row, values 1.0 (binary,
main_autoencoder.py:235) or L2-normalised tf-idf-like weights; 4-class labels with the UCI category
skew (b/t/e/m ~ .27/.26/.36/.11) or power-law "story" ids."""
from __future__ import annotations

import numpy as np
from scipy import sparse


def synthetic_csr(n_rows, n_features, *, nnz_per_row=200, seed=1234, tfidf=False, zipf_s=1.1):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_features + 1) ** zipf_s
    p /= p.sum()
    counts = np.clip(rng.poisson(nnz_per_row, n_rows), 1, min(n_features, 4 * nnz_per_row))
    # Zipf columns without replacement per row: Gumbel top-k on log p (vectorised in row blocks)
    logp = np.log(p)
    indptr = np.zeros(n_rows + 1, np.int64)
    indptr[1:] = np.cumsum(counts)
    indices = np.empty(indptr[-1], np.int32)
    blk = max(1, (1 << 24) // n_features)
    for r0 in range(0, n_rows, blk):
        r1 = min(n_rows, r0 + blk)
        g = logp[None, :] + rng.gumbel(size=(r1 - r0, n_features))
        kmax = int(counts[r0:r1].max())
        top = np.argpartition(-g, kmax - 1, axis=1)[:, :kmax]
        # order the kmax candidates by score so that the first counts[i] are the true top-k
        order = np.argsort(-np.take_along_axis(g, top, axis=1), axis=1)
        top = np.take_along_axis(top, order, axis=1)
        for i in range(r0, r1):
            c = np.sort(top[i - r0, :counts[i]])
            indices[indptr[i]:indptr[i + 1]] = c
    if tfidf:
        data = rng.random(indptr[-1]).astype(np.float32) * 0.9 + 0.1
        m = sparse.csr_matrix((data, indices, indptr), shape=(n_rows, n_features))
        norms = np.sqrt(np.asarray(m.multiply(m).sum(axis=1))).ravel()
        m = sparse.diags(1.0 / np.maximum(norms, 1e-12)).dot(m).tocsr().astype(np.float32)
        m.sort_indices()
        return m
    data = np.ones(indptr[-1], np.float32)
    return sparse.csr_matrix((data, indices, indptr), shape=(n_rows, n_features))


def synthetic_labels(n_rows, *, kind="category", seed=1234):
    rng = np.random.default_rng(seed + 1)
    if kind == "category":
        return rng.choice(4, size=n_rows, p=[0.27, 0.26, 0.36, 0.11]).astype(np.int64)
    n_story = max(2, n_rows // 6)
    w = 1.0 / np.arange(1, n_story + 1) ** 0.8
    return rng.choice(n_story, size=n_rows, p=w / w.sum()).astype(np.int64)


def synthetic_sessions(n_users, labels, *, mean_len, seed, n_preferred=2, p_preferred=0.9):
    """Seeded click logs over the articles ``labels`` describes (one label per article): every user prefers ``n_preferred``
    label classes drawn uniformly, reads a geometric number of articles (at least 1, mean ``mean_len``), and each click is, with probability
    ``p_preferred``, a uniformly drawn article of one of the preferred classes, else a uniformly drawn article of the whole
    corpus.  An article may repeat within a user.  Returns the history CSR ``(indptr int64 [n_users + 1], items int32)``,
    oldest click first; deterministic per seed."""
    rng = np.random.default_rng(seed)
    lab = np.asarray(labels).ravel()
    classes, inv = np.unique(lab, return_inverse=True)
    order = np.argsort(inv, kind="stable")                                  # articles grouped by class
    start = np.zeros(classes.size + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(inv, minlength=classes.size))
    n_pref = min(int(n_preferred), classes.size)
    pref = np.argsort(rng.random((int(n_users), classes.size)), axis=1)[:, :n_pref]      # distinct classes per user
    lens = rng.geometric(1.0 / max(float(mean_len), 1.0), int(n_users)).astype(np.int64)      # >= 1, mean mean_len
    indptr = np.zeros(int(n_users) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    nnz = int(indptr[-1])
    user = np.repeat(np.arange(int(n_users)), lens)
    cls = pref[user, rng.integers(0, n_pref, nnz)]
    within = start[cls] + (rng.random(nnz) * (start[cls + 1] - start[cls])).astype(np.int64)
    items = np.where(rng.random(nnz) < p_preferred, order[within], rng.integers(0, lab.size, nnz))
    return indptr, items.astype(np.int32)


def synthetic_timed_sessions(n_users, labels, *, mean_len, seed, span_hours=720.0, mean_delay_hours=6.0, n_preferred=2,
                             p_preferred=0.9):
    """``synthetic_sessions`` on a timeline: the articles are published at seeded uniform times over ``span_hours``, in the order
    of their index (``publish_times`` does not decrease, so the corpus is in publication order and a window of time is a range
    of indices), and a user clicks the articles of the session in publication order, each an exponential delay of mean
    ``mean_delay_hours`` after it appeared but never before the previous click: ``t = running max of (publish[item] + delay)``.
    So most clicks fall within a few ``mean_delay_hours`` of publication, every click is at or after its article's publication,
    and a user's timestamps do not decrease.  Returns ``(indptr int64 [n_users + 1], items int32, timestamps float64 [clicks],
    publish_times float64 [articles])`` in hours, oldest click first; deterministic per seed."""
    indptr, items = synthetic_sessions(n_users, labels, mean_len=mean_len, seed=seed, n_preferred=n_preferred, p_preferred=p_preferred)
    rng = np.random.default_rng([int(seed), 0x71AE])
    n_articles = np.asarray(labels).ravel().size
    publish = np.sort(rng.random(n_articles) * float(span_hours))
    delay = rng.exponential(float(mean_delay_hours), items.size)
    items = items.copy()
    times = np.empty(items.size, dtype=np.float64)
    for u in range(int(n_users)):
        a, b = int(indptr[u]), int(indptr[u + 1])
        it = np.sort(items[a:b], kind="stable")                             # index order is publication order
        items[a:b] = it
        times[a:b] = np.maximum.accumulate(publish[it] + delay[a:b])
    return indptr, items, times, publish


def xavier_uniform(n_features, n_components, const=1, seed=42):
    """U(+-const*sqrt(6/(F+H))) (autoencoder/utils.py:16-26) from a NumPy Generator: the reference's
    tf.random_uniform stream is not reproducible without TensorFlow, so parity runs inject this W0."""
    b = const * np.sqrt(6.0 / (n_features + n_components))
    return np.random.default_rng(seed).uniform(-b, b, (n_features, n_components)).astype(np.float32)
