"""Recommendation and its evaluation on top of the sweeps and the user models: ``recommend`` / ``recommend_ranks`` (a user's unseen
articles by relevance; the full rank of the held-out one) with ``next_click_metrics`` and ``rank_metrics``; ``recommend_diverse``
(retrieval, then the MMR re-rank of ``diversify_lists``) with ``list_diversity``; the popularity
baseline (``popularity_recommend``, ``popularity_ranks``); and the every-click protocol -- ``click_prefix_lists``,
``every_click_rows``, ``recommend_every_click``, ``recommend_ranks_every_click``, ``evaluate_every_click``,
``rank_metrics_by_position``, ``popularity_ranks_every_click``."""
from __future__ import annotations

import numpy as np

from ._device import check_item_range, csr_lists, device_and_library, device_matrix, event_times, history_csr, result, row_count
from .sweeps import (competitors, diversify_lists, most_similar, normalize_exclusions, normalize_window, shared_pairs, shared_row_chunks,
                     target_ranks)
from .user_models import GRUUserModel, LSTMUserModel, RNNUserModel, UserModel, user_states


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


def recommend_diverse(user_vectors, embeddings, k=10, seen=None, lam=0.7, pool=None, norm="", metric="linear kernel", *, window=None,
                      labels=None, max_per_label=None, dedup_threshold=None, diversity_norm="", diversity_metric="cosine",
                      scale_relevance="minmax", return_details=False, return_tensor=False, device=None):
    """``recommend`` followed by ``diversify_lists``: per user ``pool`` unseen, in-window candidates (default ``min(128, 4 * k)``;
    ``k <= pool <= 128``) are retrieved by relevance (``norm`` / ``metric``, as in ``recommend``) and re-ranked down to ``k`` by
    Maximal Marginal Relevance with weight ``lam``, the similarity between articles by ``diversity_norm`` / ``diversity_metric``
    (default cosine), optionally with ``dedup_threshold`` and ``labels`` / ``max_per_label``.  The relevance is rescaled per list
    to ``[0, 1]`` by default (``scale_relevance``): the inner product is unbounded, the similarity penalty is not.  The corpus
    goes to the device once for both calls.  Returns what ``diversify_lists`` returns; the relevance is the retrieval's."""
    k = int(k)
    pool = min(128, 4 * k) if pool is None else int(pool)
    if pool < k or pool > 128:
        raise ValueError(f"pool must be in k..128 = {k}..128 (got {pool})")
    if not 0.0 <= float(lam) <= 1.0:
        raise ValueError(f"lam must be in [0, 1] (got {lam})")
    if max_per_label is not None and (int(max_per_label) < 1 or labels is None):
        raise ValueError("max_per_label must be at least 1 and needs labels")
    if scale_relevance not in (None, "minmax"):
        raise ValueError(f"scale_relevance must be None or 'minmax' (got {scale_relevance!r})")
    torch, _, dev = device_and_library(device)
    corpus = device_matrix(torch, embeddings, dev)                       # once, for both calls
    idx, score = most_similar(user_vectors, k=pool, norm=norm, metric=metric, candidates=corpus, exclude=seen, window=window,
                              return_tensor=True, device=device)
    return diversify_lists(idx, score, corpus, k, lam, labels=labels, max_per_label=max_per_label, dedup_threshold=dedup_threshold,
                           norm=diversity_norm, metric=diversity_metric, scale_relevance=scale_relevance, return_details=return_details,
                           return_tensor=return_tensor, device=device)


def list_diversity(indices, nearest=None, labels=None):
    """How diverse recommendation lists are.  Host code.  ``indices`` ``[n x k]``, -1 where a list is short; ``nearest`` (same
    shape, e.g. ``diversify_lists(..., return_details=True)['nearest']``): per entry the similarity to the nearest entry before
    it; ``labels``: one integer per article.  Returns a dict with, per list (``[n]`` arrays) and averaged over the lists where
    the figure exists (NaN where none does): ``nearest`` / ``mean_nearest`` -- the mean of ``nearest`` over a list's entries from
    the second on (NaN for a list of fewer than two); ``n_labels`` / ``mean_n_labels`` -- the number of distinct labels;
    ``max_label_share`` / ``mean_max_label_share`` -- the largest share of a list one label holds (NaN for an empty list).  The
    first pair needs ``nearest``, the other two ``labels``; what cannot be computed is left out."""
    idx = np.asarray(indices)
    if idx.ndim != 2:
        raise ValueError("indices must be [n_lists x k]")
    ok = idx >= 0
    out = {}

    def mean(x):
        x = x[~np.isnan(x)]
        return float(x.mean()) if x.size else float("nan")

    if nearest is not None:
        near = np.asarray(nearest, dtype=np.float64)
        if near.shape != idx.shape:
            raise ValueError(f"nearest must have the shape of indices {idx.shape} (got {near.shape})")
        later = ok & (np.cumsum(ok, axis=1) > 1)                          # a list's selected entries from the second on
        n = later.sum(axis=1)
        per = np.where(n > 0, np.where(later, near, 0.0).sum(axis=1) / np.maximum(n, 1), np.nan)
        out["nearest"], out["mean_nearest"] = per, mean(per)
    if labels is not None:
        lab = np.asarray(labels).ravel()
        if idx.size and ok.any() and int(idx.max()) >= lab.size:
            raise ValueError(f"labels holds {lab.size} entries, the lists name article {int(idx.max())}")
        n_labels = np.zeros(idx.shape[0], dtype=np.int64)
        share = np.full(idx.shape[0], np.nan)
        for i in range(idx.shape[0]):
            row = lab[idx[i][ok[i]]]
            if row.size:
                _, c = np.unique(row, return_counts=True)
                n_labels[i], share[i] = c.size, c.max() / row.size
        out["n_labels"], out["mean_n_labels"] = n_labels, float(n_labels.mean()) if n_labels.size else float("nan")
        out["max_label_share"], out["mean_max_label_share"] = share, mean(share)
    return out


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
    indptr, items = csr_lists(histories)
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
    indptr, items = csr_lists(histories)
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
    indptr, items = history_csr(histories)
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
    indptr, items = history_csr(histories)
    nnz, n = int(items.size), np.diff(indptr)
    users = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), n)
    pos = np.arange(nnz, dtype=np.int64) - indptr[:-1][users]
    last = np.zeros(nnz, dtype=bool)
    last[indptr[1:][n > 0] - 1] = True
    nxt = np.minimum(np.arange(nnz, dtype=np.int64) + 1, max(nnz - 1, 0))
    out = {"targets": np.where(last, -1, items.astype(np.int64)[nxt] if nnz else np.zeros(0, np.int64)).astype(np.int64),
           "row_list": users.astype(np.int32), "row_limit": pos.astype(np.int32), "positions": pos + 1}
    if timestamps is not None:
        t = np.asarray(event_times(timestamps), dtype=np.float64).ravel()
        if t.size != nnz:
            raise ValueError(f"{t.size} timestamps for {nnz} events")
        out["query_times"] = np.where(last, t, t[nxt] if nnz else t)
    return out


def _every_click_chunks(states, embeddings, histories, window, batch_rows, device):
    """What the two every-click sweeps share: the checked inputs, and per chunk of ``batch_rows`` rows the arguments of the sweep.
    Returns ``(rows dict, E, chunks)``; a chunk is ``(a, b, states[a:b], exclude_shared, window or None)``."""
    if int(batch_rows) < 1:
        raise ValueError(f"batch_rows must be positive (got {batch_rows})")
    indptr, items = history_csr(histories)
    rows = every_click_rows((indptr, items))
    nnz = int(items.size)
    if row_count(states) != nnz:
        raise ValueError(f"{row_count(states)} state rows for {nnz} events (states is the all_states=True output for these histories)")
    Na = row_count(embeddings)
    check_item_range(items, Na, lower=False)
    lists = click_prefix_lists((indptr, items))
    if window is not None:
        window = normalize_window(window, nnz, Na)
    torch, _, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev, in_place=True)

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
    return result((idx, score, torch.from_numpy(rows["targets"]).to(idx.device) if return_tensor else rows["targets"]), return_tensor)


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
    return result((rank, score, n_cand, torch.from_numpy(rows["targets"]).to(rank.device) if return_tensor else rows["targets"]),
                  return_tensor)


_RECURRENT = (GRUUserModel, LSTMUserModel, RNNUserModel)


def evaluate_every_click(histories, embeddings, model, *, timestamps=None, time_unit=None, window=None, batch_users=4096,
                         ks=(1, 5, 10, 50, 100), device=None):
    """Next-click evaluation at EVERY click of every history (the per-position protocol of session-based recommendation), where
    the last-click protocol scores one click per user: the state after each event is ranked against the event that follows,
    among all the articles the user had not clicked by then (``recommend_ranks_every_click``).

    ``model``: a ``GRUUserModel``, ``LSTMUserModel`` or ``RNNUserModel`` (the ``all_states`` rows of its ``.states``), a fitted ``UserModel`` (``alpha *`` the states of ``user_states``
    with its ``beta`` and ``time_unit``, as ``UserModel.states`` applies them) or a float ``beta`` (``user_states``; ``time_unit``
    as there).  ``timestamps`` (one per event) drive the decay of the two decay forms; ``window`` is a pair ``(lo, hi)`` per EVENT.
    The states are produced for ``batch_users`` users at a time and ranked at once, so [events x H] never exists whole.

    Returns a dict: the per-event arrays ``rank``, ``score``, ``n_candidates``, ``targets``, ``positions`` (clicks seen, for
    ``rank_metrics_by_position``) and ``metrics`` = ``rank_metrics`` over all events with a target."""
    if int(batch_users) < 1:
        raise ValueError(f"batch_users must be positive (got {batch_users})")
    indptr, items = history_csr(histories)
    M, nnz = int(indptr.size - 1), int(items.size)
    t = None if timestamps is None else np.asarray(event_times(timestamps), dtype=np.float64).ravel()
    if t is not None and t.size != nnz:
        raise ValueError(f"{t.size} timestamps for {nnz} events")
    if window is not None:
        window = normalize_window(window, nnz, row_count(embeddings))
    if not isinstance(model, _RECURRENT + (UserModel,)):
        model = float(model)
    torch, _, dev = device_and_library(device)
    E = device_matrix(torch, embeddings, dev, in_place=True)
    alpha = torch.from_numpy(model.alpha.astype(np.float32)).to(dev) if isinstance(model, UserModel) else None
    out = [[], [], []]
    for u0 in range(0, M, int(batch_users)):
        u1 = min(u0 + int(batch_users), M)
        a, b = int(indptr[u0]), int(indptr[u1])
        if b == a:
            continue
        hist = (indptr[u0:u1 + 1] - a, items[a:b])
        tb = None if t is None else t[a:b]
        if isinstance(model, _RECURRENT):
            S = model.states(hist, E, all_states=True, return_tensor=True, device=device)
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
    indptr, items = csr_lists(histories)
    Na, nnz = int(n_articles), int(items.size)
    check_item_range(items, Na, lower=False)
    rows = every_click_rows((indptr, items))
    lp, li, ls = click_prefix_lists((indptr, items))
    tgt = rows["targets"]
    if window is not None:
        window = normalize_window(window, nnz, Na)
    n_cand, barred = competitors(tgt, nnz, Na, False, None, None, window, (lp, li, ls, rows["row_list"], rows["row_limit"]))
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
    for a, b in shared_row_chunks(n_in):                                   # minus the seen ones among them
        r, places = shared_pairs(lp, rows["row_list"], a, b)
        it = li[places].astype(np.int64)
        take = (ls[places] <= lim[r]) & (pos[it] < pt[r])
        if window is not None:
            take &= (it >= window[0][r]) & (it < window[1][r])
        ahead[a:b] -= np.bincount(r[take] - a, minlength=b - a)
    return np.where(ok, 1 + ahead, 0).astype(np.int64), n_cand, tgt

