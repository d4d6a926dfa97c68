"""Clustering of the embeddings the project trains, and retrieval through the clusters.  ``kmeans`` / ``kmeans_assign``: spherical
k-means by Lloyd iterations on the device -- the assignment is the exact-fp32 score sweep of ``most_similar`` with an arg-max for an
epilogue (``dae_kmeans_assign``), the update a stable sort of the rows by label and fixed-order fp64 sums (``dae_kmeans_update``).
``cluster_label_scores``: purity, NMI and ARI of a clustering against labels (host code).  ``ClusterIndex``: the corpus stored in
cluster order, so that one probe of a query is one windowed call of ``most_similar`` (``merge_probe_lists`` joins the probes)."""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ._device import METRICS, device_and_library, device_matrix, result, row_count, upload, workspace
from .label_stats import _label_keys
from .sweeps import SweepOperand, most_similar, normalize_exclusions


class _Image:
    """The sweep image of a whole operand: ``p`` the aligned pointer, ``rows`` its ``[pad(n) x pad(D)]`` float32 view."""

    def __init__(self, torch, lib, dev, n, D):
        self.n, self.D, self.bytes = n, D, int(lib.dae_sweep_image_bytes(n, D))
        if self.bytes == 0 or L.pad(n) * L.pad(D) * 4 >= 1 << 32:
            raise ValueError(f"the operand image of {n} x {D} must hold rows and columns and stay below 4 GiB")
        self.p, self._t = workspace(dev, self.bytes)
        off = (-self._t.data_ptr()) % 256
        self.rows = self._t[off:off + L.pad(n) * L.pad(D) * 4].view(torch.float32).view(L.pad(n), L.pad(D))

    def fill(self, torch, operand, nm):
        operand.image(torch, 0, self.n, self.p, self.bytes, nm)
        return self


def _assign(lib, img_x, img_c, prev, labels, scores, ws, rec):
    ws_p, ws_bytes = ws
    L.call("dae_kmeans_assign", img_x.p, img_x.n, img_c.p, img_c.n, img_x.D, L.ptr(prev), L.ptr(labels), L.ptr(scores), rec, ws_p, ws_bytes,
           L.current_stream())
    return rec[0], int(rec[1])


def kmeans_assign(X, centroids, metric="cosine", *, return_tensor=False, device=None):
    """The nearest centroid of every row of ``X``: ``labels[i]`` is the row ``j`` of ``centroids`` with the largest score, ties to the
    lower ``j``, and ``scores[i]`` that score -- the scores ``pairwise_similarity(X, '', metric)`` would give against the centroids
    (``'cosine'``: both sides L2-normalised, an all-zero row stays zero, scores 0 everywhere and so lands in cluster 0; ``'linear
    kernel'``: the plain dot product).  On finite scores the result equals ``most_similar(X, 1, '', metric, candidates=centroids)``
    bit for bit; a row whose scores are all -inf or NaN (possible only with non-finite input) gets label -1 and score -inf, where
    ``most_similar`` returns a column.
    Both inputs take the containers of ``most_similar`` (ndarray, list, scipy.sparse -- whose image is built straight from the CSR rows,
    never densified on the host -- and CUDA tensor).  Returns ``(labels int64 [N], scores float32 [N])``."""
    import ctypes
    if metric not in METRICS:
        raise ValueError(f"metric must be 'cosine' or 'linear kernel' (got {metric!r})")
    nm = (0, METRICS[metric])
    torch, lib, dev = device_and_library(device)
    Xo, Co = SweepOperand(torch, X, dev), SweepOperand(torch, centroids, dev)
    (N, D), (K, Dc) = Xo.shape, Co.shape
    if Dc != D:
        raise ValueError(f"centroids have {Dc} columns, X has {D}")
    if K < 1 or D < 1:
        raise ValueError(f"kmeans_assign needs centroids and columns (got {K} x {D})")
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    scores = torch.empty(N, dtype=torch.float32, device=dev)
    if N > 0:
        with torch.cuda.device(dev):
            img_x = _Image(torch, lib, dev, N, D).fill(torch, Xo, nm)
            img_c = _Image(torch, lib, dev, K, D).fill(torch, Co, nm)
            ws_bytes = int(lib.dae_kmeans_assign_workspace(N, K))
            ws_p, ws = workspace(dev, ws_bytes)
            _assign(lib, img_x, img_c, None, labels, scores, (ws_p, ws_bytes), (ctypes.c_double * 4)())
            del ws
    return result((labels.long(), scores), return_tensor)


class KMeansResult:
    """What ``kmeans`` returns.  ``labels`` int64 [N] and ``scores`` float32 [N]: the final assignment against ``centroids`` float32
    [K x D] (unit rows); ``counts`` int64 [K]; ``mean_score``: the fp64 sum of the scores / N; ``n_iter``: centroid updates done;
    ``history``: one ``(mean score, changed labels)`` per assignment; ``order`` int64 [N]: the row ids sorted by (label, row id);
    ``offsets`` int64 [K + 1]: cluster c is ``order[offsets[c]:offsets[c + 1]]``; ``relocated``: empty clusters given a new centroid;
    ``seed``: the seed of the run kept.  ``predict(X)`` assigns other rows to the centroids; ``predict`` of the training rows equals
    ``labels`` bit for bit."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def predict(self, X, *, return_tensor=False, device=None):
        return kmeans_assign(X, self.centroids, "cosine", return_tensor=return_tensor, device=device)[0]


def relocation_rows(scores, labels, counts):
    """The rows that become the centroids of the empty clusters (``counts == 0``), one per empty cluster in ascending cluster id: the
    rows with the lowest assignment score, ordered by score ascending and ties by the lower row id, without the rows that are the
    only member of their cluster (and without rows that have no label).  Fewer rows than empty clusters may qualify.  Host code."""
    scores, labels, counts = np.asarray(scores), np.asarray(labels).astype(np.int64), np.asarray(counts).astype(np.int64)
    n_empty = int((counts == 0).sum())
    by_score = np.lexsort((np.arange(scores.size), scores))
    lab = labels[by_score]
    ok = (lab >= 0) & (lab < counts.size)
    ok[ok] = counts[lab[ok]] > 1
    return by_score[ok][:n_empty]


def _fit(torch, lib, dev, img_x, C, max_iter, tol, relocate):
    """One run of Lloyd iterations from the centroids ``C`` (float32 [K x D] on the device, updated in place)."""
    import ctypes
    N, D, K = img_x.n, img_x.D, int(C.shape[0])
    i32 = dict(dtype=torch.int32, device=dev)
    labels, prev, scores = torch.empty(N, **i32), torch.empty(N, **i32), torch.empty(N, dtype=torch.float32, device=dev)
    counts, order, offsets = torch.empty(K, **i32), torch.empty(N, **i32), torch.empty(K + 1, dtype=torch.int64, device=dev)
    img_c = _Image(torch, lib, dev, K, D)
    aws_bytes, uws_bytes = int(lib.dae_kmeans_assign_workspace(N, K)), int(lib.dae_kmeans_update_workspace(N, K, D))
    (aws_p, aws), (uws_p, uws) = workspace(dev, aws_bytes), workspace(dev, uws_bytes)
    rec, rec_u = (ctypes.c_double * 4)(), (ctypes.c_double * 4)()

    def update(centroids):
        L.call("dae_kmeans_update", img_x.p, N, D, L.ptr(labels), K, L.ptr(centroids), 0 if centroids is None else centroids.stride(0),
               L.ptr(counts), L.ptr(order), L.ptr(offsets), rec_u, uws_p, uws_bytes, L.current_stream())

    history, n_iter, relocated, have_prev, prev_mean, sorted_labels = [], 0, 0, False, None, False
    while True:
        L.call("dae_sweep_image_dense", L.ptr(C), C.stride(0), K, D, 0, 0, img_c.p, img_c.bytes, L.current_stream())
        total, changed = _assign(lib, img_x, img_c, prev if have_prev else None, labels, scores, (aws_p, aws_bytes), rec)
        mean = total / N
        history.append((mean, changed))
        if have_prev and changed == 0:
            sorted_labels = True                                      # the last update sorted these very labels
            break
        if tol > 0 and prev_mean is not None and mean - prev_mean < tol * abs(prev_mean):
            break
        if n_iter >= max_iter:
            break
        update(C)
        n_iter += 1
        prev_mean = mean
        if relocate and rec_u[1] > 0:
            rows = relocation_rows(scores.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy())
            if rows.size:
                empties = torch.nonzero(counts == 0).ravel()[:rows.size]
                C[empties] = img_x.rows[torch.from_numpy(rows).to(dev), :D]
                relocated += int(rows.size)
                prev_mean = None                                      # the mean may fall after a relocation: no tol test on it
        labels, prev, have_prev = prev, labels, True
    if not sorted_labels:
        update(None)
    del aws, uws
    return dict(labels=labels.long(), centroids=C, counts=counts.long(), scores=scores, mean_score=history[-1][0], n_iter=n_iter,
                history=history, order=order.long(), offsets=offsets, relocated=relocated)


def kmeans(X, n_clusters, *, max_iter=50, tol=1e-4, init="random", n_init=1, seed=0, empty="relocate", return_tensor=False, device=None):
    """Spherical k-means of the rows of ``X`` (ndarray, list, scipy.sparse or CUDA tensor) into ``n_clusters`` clusters by Lloyd
    iterations on the device.  Rows and centroids are L2-normalised and a row goes to the centroid of the largest cosine, ties to
    the lower cluster id; an all-zero row stays zero, scores 0 against every centroid and so lands in cluster 0.  A centroid is the
    normalised sum of its rows, added in fp64 in a fixed order: the run is bit-identical from call to call.

    ``init``: ``'random'`` takes the rows ``np.random.RandomState(seed).choice(N, n_clusters, replace=False)``; or a ``[K x D]`` array
    of starting centroids.  ``n_init > 1`` restarts with the seeds ``seed, seed + 1, ...`` and keeps the run with the largest mean
    score (the first of equals).  The iterations stop when no label changed, when the mean score improved by less than ``tol``
    relative (``tol=0``: never for that reason), or after ``max_iter`` centroid updates; the labels returned are always those of an
    assignment against the centroids returned.  ``empty='relocate'``: after an update that leaves E clusters without members, the E
    rows with the lowest assignment score (``relocation_rows``) become their centroids, in ascending cluster id; ``'keep'`` leaves
    such a centroid where it was.  Every assignment and every update returns host numbers, i.e. synchronises.

    Returns a ``KMeansResult`` (arrays as ndarrays, or as CUDA tensors with ``return_tensor=True``)."""
    if empty not in ("relocate", "keep"):
        raise ValueError(f"empty must be 'relocate' or 'keep' (got {empty!r})")
    K, max_iter, n_init = int(n_clusters), int(max_iter), int(n_init)
    if max_iter < 0 or n_init < 1 or not float(tol) >= 0:
        raise ValueError("kmeans needs max_iter >= 0, n_init >= 1 and tol >= 0")
    torch, lib, dev = device_and_library(device)
    Xo = SweepOperand(torch, X, dev)
    N, D = Xo.shape
    if not 1 <= K <= N or D < 1:
        raise ValueError(f"n_clusters must be in 1..{N} rows, and the rows need columns (got {K} clusters for {N} x {D})")
    given = not isinstance(init, str)
    if not given and init != "random":
        raise ValueError(f"init must be 'random' or a [K x D] array (got {init!r})")
    best = None
    with torch.cuda.device(dev):
        img_x = _Image(torch, lib, dev, N, D).fill(torch, Xo, (0, 0))
        if given:
            Io = SweepOperand(torch, init, dev)
            if Io.shape != (K, D):
                raise ValueError(f"init must be [{K} x {D}] (got {Io.shape[0]} x {Io.shape[1]})")
            start = _Image(torch, lib, dev, K, D).fill(torch, Io, (0, 0)).rows[:K, :D]
        for run in range(1 if given else n_init):
            if given:
                C = start.clone()
            else:
                C = img_x.rows[torch.from_numpy(np.random.RandomState(seed + run).choice(N, K, replace=False)).to(dev), :D].clone()
            fit = _fit(torch, lib, dev, img_x, C, max_iter, float(tol), empty == "relocate")
            fit["seed"] = None if given else seed + run
            if best is None or fit["mean_score"] > best["mean_score"]:
                best = fit
    return KMeansResult(**{name: result(v, return_tensor) for name, v in best.items()})


def cluster_label_scores(pred, true):
    """A clustering ``pred`` against the labels ``true``, from one contingency table: ``purity`` (every cluster votes for its most
    frequent label), ``nmi`` (mutual information over the arithmetic mean of the two entropies:
    ``sklearn.metrics.normalized_mutual_info_score``) and ``ari`` (``adjusted_rand_score``), with ``n`` rows counted, ``n_clusters``
    and ``n_labels`` among them.  Rows whose true label is negative or NaN are skipped, as in ``label_precision_at_k``.  Host code."""
    p = np.asarray(pred).ravel()
    t, valid = _label_keys(true)
    if p.shape[0] != t.shape[0]:
        raise ValueError(f"{p.shape[0]} cluster ids for {t.shape[0]} labels")
    p, t = p[valid], t[valid]
    n = int(p.size)
    out = {"purity": float("nan"), "nmi": float("nan"), "ari": float("nan"), "n": n, "n_clusters": 0, "n_labels": 0}
    if n == 0:
        return out
    pu, pi = np.unique(p, return_inverse=True)
    tu, ti = np.unique(t, return_inverse=True)
    table = np.bincount(ti.ravel() * pu.size + pi.ravel(), minlength=tu.size * pu.size).reshape(tu.size, pu.size)
    out["n_clusters"], out["n_labels"] = int(pu.size), int(tu.size)
    out["purity"] = float(table.max(axis=0).sum() / n)
    nt, npred = table.sum(axis=1), table.sum(axis=0)
    # nmi
    if pu.size == 1 and tu.size == 1:
        out["nmi"] = 1.0
    else:
        i, j = np.nonzero(table)
        nij = table[i, j].astype(np.float64)
        mi = float(np.sum(nij / n * (np.log(nij) - np.log(n)) + nij / n * (np.log(n) * 2 - np.log(nt[i]) - np.log(npred[j]))))
        mi = max(mi, 0.0)
        entropy = lambda c: float(-np.sum(c[c > 0] / n * (np.log(c[c > 0]) - np.log(n))))      # noqa: E731
        denom = 0.5 * (entropy(nt) + entropy(npred))
        out["nmi"] = 0.0 if mi < np.finfo(np.float64).eps else mi / max(denom, np.finfo(np.float64).eps)
    # ari, from the pair counts
    sq = sum(int(v) ** 2 for v in table.ravel())
    fp = sum(int(v) ** 2 for v in npred) - sq
    fn = sum(int(v) ** 2 for v in nt) - sq
    tp = sq - n
    tn = n * n - fp - fn - sq
    out["ari"] = 1.0 if fp == 0 and fn == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    return out


def merge_probe_lists(indices, scores, order, k):
    """The per-probe top-k lists of ``ClusterIndex.search`` as one: ``indices`` / ``scores`` are one ``[Nq x k']`` tensor per probe
    (positions in the cluster-ordered corpus, -1 / -inf tails), ``order`` int64 maps a position to the caller's id.  The candidates
    of a row are mapped back, sorted by score descending and then by the caller's id ascending, and cut to ``k``; the tail is
    -1 / -inf.  Different probes of a row are different clusters, so no candidate repeats.  Runs on whatever device the tensors
    are on."""
    import torch
    idx, sc = torch.cat(list(indices), dim=1), torch.cat(list(scores), dim=1)
    valid = idx >= 0
    big = torch.iinfo(torch.int64).max
    orig = torch.where(valid, order[idx.clamp_min(0)], torch.full_like(idx, big))
    sc = torch.where(valid, sc, torch.full_like(sc, float("-inf")))
    by_id = torch.argsort(orig, dim=1, stable=True)
    orig, sc = torch.gather(orig, 1, by_id), torch.gather(sc, 1, by_id)
    by_score = torch.argsort(sc, dim=1, descending=True, stable=True)      # stable: equal scores stay in id order
    orig, sc = torch.gather(orig, 1, by_score)[:, :k], torch.gather(sc, 1, by_score)[:, :k]
    orig = torch.where(orig == big, torch.full_like(orig, -1), orig)
    if orig.shape[1] < k:
        pad = k - orig.shape[1]
        orig = torch.cat([orig, orig.new_full((orig.shape[0], pad), -1)], dim=1)
        sc = torch.cat([sc, sc.new_full((sc.shape[0], pad), float("-inf"))], dim=1)
    return orig, sc


class ClusterIndex:
    """An inverted file over a k-means clustering: the corpus in cluster order (``corpus``: row p is the caller's row ``order[p]``;
    the sort is stable, so inside a cluster the caller's order is kept), ``offsets`` (cluster c is the rows ``offsets[c] ..
    offsets[c + 1]``), the ``centroids`` and the inverse permutation ``inverse``.  ``search`` scores a query only against the
    members of its ``n_probe`` nearest clusters; the scores are those of ``most_similar`` for the same pair."""

    def __init__(self, corpus, order, offsets, centroids, norm="", metric="cosine"):
        if metric not in METRICS:
            raise ValueError(f"metric must be 'cosine' or 'linear kernel' (got {metric!r})")
        self.corpus, self.norm, self.metric = corpus, norm, metric
        self.order = np.ascontiguousarray(np.asarray(order, dtype=np.int64))
        self.offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
        self.centroids = np.ascontiguousarray(np.asarray(centroids, dtype=np.float32))
        n = row_count(corpus)
        if self.order.size != n or self.offsets.size != self.centroids.shape[0] + 1 or int(self.offsets[-1]) > n:
            raise ValueError("order must hold one id per corpus row, and offsets one entry per centroid and one more")
        self.inverse = np.empty(n, dtype=np.int64)
        self.inverse[self.order] = np.arange(n, dtype=np.int64)

    n_clusters = property(lambda self: int(self.centroids.shape[0]))

    @classmethod
    def build(cls, embeddings, n_clusters, norm="", metric="cosine", **kmeans_kwargs):
        """k-means of ``embeddings`` (``kmeans_kwargs``: ``max_iter``, ``seed``, ...) and the index of the result."""
        kmeans_kwargs["return_tensor"] = False
        return cls.from_kmeans(embeddings, kmeans(embeddings, n_clusters, **kmeans_kwargs), norm, metric)

    @classmethod
    def from_kmeans(cls, embeddings, result, norm="", metric="cosine"):
        """The index of a ``KMeansResult`` of ``embeddings`` (ndarray, list, scipy.sparse or tensor)."""
        to_np = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)      # noqa: E731
        order, offsets = to_np(result.order).astype(np.int64), to_np(result.offsets)
        if int(offsets[-1]) != order.size:
            raise ValueError(f"{order.size - int(offsets[-1])} rows have no cluster (label -1: non-finite embeddings); an index could "
                             "never return them")
        if hasattr(embeddings, "detach"):
            import torch
            corpus = embeddings[torch.from_numpy(order).to(embeddings.device)]
        elif hasattr(embeddings, "tocsr"):
            corpus = embeddings.tocsr()[order]
        else:
            corpus = np.asarray(embeddings, dtype=np.float32)[order]
        return cls(corpus, order, offsets, to_np(result.centroids), norm, metric)

    def save(self, path):
        """The index as one ``.npz`` (dense corpora only)."""
        if hasattr(self.corpus, "tocsr"):
            raise ValueError("save takes a dense corpus")
        corpus = self.corpus.cpu().numpy() if hasattr(self.corpus, "cpu") else self.corpus
        np.savez(path, corpus=np.asarray(corpus, dtype=np.float32), order=self.order, offsets=self.offsets, centroids=self.centroids,
                 norm=np.array(self.norm), metric=np.array(self.metric))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["corpus"], z["order"], z["offsets"], z["centroids"], str(z["norm"]), str(z["metric"]))

    def search(self, Q, k=10, n_probe=8, *, exclude=None, return_tensor=False, device=None, window=None, exclude_shared=None):
        """The top ``k`` of every row of ``Q`` among the members of its ``n_probe`` nearest clusters, in the caller's ids:
        ``(indices int64 [Nq x k], scores float32 [Nq x k])``, ordered as ``most_similar`` orders them.  The clusters are the
        ``n_probe`` best centroids by cosine for a cosine index; for ``'linear kernel'`` by ``q . centroid``, where the choice is a
        heuristic (a far cluster may hold a long row).  Every probe rank is one windowed ``most_similar`` call on the cluster-ordered
        corpus, with its own image builds and host work, so the index pays off at small ``n_probe`` (``tools/ann_bench.py``);
        ``n_probe = n_clusters`` returns what ``most_similar`` returns, bit for bit.  ``exclude`` as in ``most_similar``, in
        the caller's ids.  ``window`` / ``exclude_shared`` are not supported; ``k <= 128`` and ``n_probe <= 128``."""
        if window is not None or exclude_shared is not None:
            raise ValueError("ClusterIndex.search does not take window= or exclude_shared=")
        k, P = int(k), min(int(n_probe), self.n_clusters)
        if not 1 <= P <= 128:
            raise ValueError(f"n_probe, cut to the number of clusters, must be in 1..128 (got {n_probe} for {self.n_clusters} clusters)")
        if not 1 <= k <= 128:
            raise ValueError(f"k must be in 1..128 (got {k})")
        torch, _, dev = device_and_library(device)
        Qd = device_matrix(torch, Q, dev)
        corpus = device_matrix(torch, self.corpus, dev)
        Nq, n = int(Qd.shape[0]), int(corpus.shape[0])
        if exclude is not None:
            xp, xi = normalize_exclusions(exclude, Nq, n)
            exclude = (xp, self.inverse[xi])
        probes, _ = most_similar(Qd, P, "", self.metric, candidates=upload(self.centroids, dev), return_tensor=True, device=dev)
        offsets = upload(self.offsets, dev)
        idx, sc = [], []
        for p in range(P):
            c = probes[:, p].clamp_min(0)
            lo = torch.where(probes[:, p] >= 0, offsets[c], offsets[c + 1])      # no such cluster: an empty window
            i, s = most_similar(Qd, k, self.norm, self.metric, candidates=corpus, exclude=exclude, window=(lo, offsets[c + 1]),
                                return_tensor=True, device=dev)
            idx.append(i)
            sc.append(s)
        return result(merge_probe_lists(idx, sc, upload(self.order, dev), k), return_tensor)

    def probed_fraction(self, Q, n_probe=8, *, device=None):
        """The share of the corpus scored per query row at ``n_probe``: the members of its probed clusters over the corpus rows."""
        torch, _, dev = device_and_library(device)
        P = min(int(n_probe), self.n_clusters)
        probes, _ = most_similar(Q, P, "", self.metric, candidates=upload(self.centroids, dev), return_tensor=True, device=dev)
        sizes = upload(np.diff(self.offsets), dev)
        return float(sizes[probes.clamp_min(0)].sum(dim=1).double().mean().item() / max(self.order.size, 1))
