"""Spherical k-means (helpers.kmeans; include/dae_hip.h: dae_kmeans_assign / dae_kmeans_update) as a short float64 NumPy
restatement of its rules: normalise, arg-max with ties to the lower id, update, relocation, stopping.  Beside the result, every
iteration reports how close its decisions were: the smallest gap between a row's best and second-best score, and the smallest gap
between the scores that decide a relocation -- a test compares a float32 device run with this only where those gaps exceed the
float32 error of a score."""
import numpy as np


def normalize(X):
    X = np.asarray(X, dtype=np.float64)
    n = np.sqrt((X * X).sum(axis=1, keepdims=True))
    return X / np.where(n == 0, 1.0, n)


def blobs(N, K, D, noise, seed):
    """Planted unit-norm blobs: ``X = normalize(centre[y] + noise * randn)`` as float32, ``y``, and the unit centres."""
    rng = np.random.RandomState(seed)
    centres = normalize(rng.randn(K, D))
    y = rng.randint(0, K, N)
    X = normalize(centres[y] + noise * rng.randn(N, D)).astype(np.float32)
    return X, y, centres


def assign(Xn, Cn):
    """``(labels, scores, smallest top-2 gap, per-row gaps)`` of unit rows against unit centroids; ties go to the lower id."""
    S = Xn @ Cn.T
    labels = S.argmax(axis=1)                                         # the first of equal maxima
    scores = S[np.arange(S.shape[0]), labels]
    if S.shape[1] > 1:
        T = S.copy()
        T[np.arange(S.shape[0]), labels] = -np.inf
        gaps = scores - T.max(axis=1)
    else:
        gaps = np.full(S.shape[0], np.inf)
    return labels, scores, (float(gaps.min()) if gaps.size else np.inf), gaps


def update(Xn, labels, K, C):
    """The centroids after one update (a cluster without members, or whose sum is zero, keeps its row) and the counts."""
    C = C.copy()
    counts = np.bincount(labels[(labels >= 0) & (labels < K)], minlength=K)
    for c in np.flatnonzero(counts):
        s = Xn[labels == c].sum(axis=0)
        n2 = float(s @ s)
        if n2 > 0:
            C[c] = s / np.sqrt(n2)
    return C, counts


def relocation(scores, labels, counts):
    """``(rows, gap)``: the rows that become the centroids of the empty clusters, ascending cluster id -- lowest score first, ties
    to the lower row id, rows that are their cluster's only member left out -- and the smallest gap between neighbouring scores
    among those rows and the first row not taken (inf without a decision)."""
    E = int((counts == 0).sum())
    order = sorted(range(len(scores)), key=lambda i: (scores[i], i))
    cand = [i for i in order if counts[labels[i]] > 1]
    rows = np.array(cand[:E], dtype=np.int64)
    decided = np.array([scores[i] for i in cand[:E + 1]])
    gap = float(np.diff(decided).min()) if E and decided.size > 1 else np.inf
    return rows, gap


def lloyd(X, init, max_iter=50, tol=1e-4, empty="relocate"):
    """The run of ``helpers.kmeans(X, K, init=init, ...)`` in float64.  Returns a dict: ``labels`` (the final ones), ``all_labels``
    (those of every assignment), ``history`` (``(mean score, changed)`` per assignment), ``centroids``, ``counts`` (of the final
    labels), ``n_iter``, ``relocated``, ``gaps`` (per assignment, the smallest top-2 gap) and ``relocation_gaps`` (per update)."""
    Xn, C = normalize(X), normalize(init)
    N, K = Xn.shape[0], C.shape[0]
    prev, prev_mean, n_iter, relocated = None, None, 0, 0
    all_labels, history, gaps, rgaps = [], [], [], []
    while True:
        labels, scores, gap, _ = assign(Xn, normalize(C))
        mean = float(scores.sum() / N)
        changed = N if prev is None else int((labels != prev).sum())
        all_labels.append(labels); history.append((mean, changed)); gaps.append(gap)
        if prev is not None and changed == 0:
            break
        if tol > 0 and prev_mean is not None and mean - prev_mean < tol * abs(prev_mean):
            break
        if n_iter >= max_iter:
            break
        C, counts = update(Xn, labels, K, C)
        n_iter += 1
        prev_mean = mean
        if empty == "relocate" and (counts == 0).any():
            rows, rgap = relocation(scores, labels, counts)
            rgaps.append(rgap)
            if rows.size:
                C[np.flatnonzero(counts == 0)[:rows.size]] = Xn[rows]
                relocated += int(rows.size)
                prev_mean = None
        else:
            rgaps.append(np.inf)
        prev = labels
    return dict(labels=labels, all_labels=all_labels, history=history, centroids=C, counts=np.bincount(labels, minlength=K), n_iter=n_iter,
                relocated=relocated, gaps=gaps, relocation_gaps=rgaps)
