"""The word-based user model, the baseline of "Embedding-based News Recommendation for Millions of Users" (section 5.1): an article
is the set of its words, a user is the set of the words of everything they have browsed, and the relevance is a weighted count of
the words the two share.  ``word_profiles`` builds the users' word sets on the device as bitmaps (``dae_word_profiles``) and returns
a ``WordProfiles``; ``word_recommend`` is the top-k of the relevance without a users x articles matrix and without a dense
users x vocabulary one (``dae_word_topk``: about one select-and-add per stored word of the article per pair); ``word_ranks`` is
its full-rank twin (``dae_word_rank``) in the form ``rank_metrics`` takes; ``idf_weights`` gives sklearn's smooth idf as term
weights.  The rules of the model are stated in include/dae_hip.h.

Articles are a scipy.sparse matrix or a device CSR dict ``[n_articles x n_words]``, as ``helpers.vectorize`` takes them (columns
ascending and unique per row, ``values`` float32 or None for all ones).  The device functions have no CPU implementation.  torch
and scipy are imported inside the functions."""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ._device import device_and_library, history_csr, result, upload, workspace
from .sweeps import _window_order, competitors, normalize_exclusions, normalize_window, permute_histories
from .vectorize import TfidfTransformer, _device_csr, _device_of, _is_device_csr, _shape, binarize, column_stats

TILE = 128                 # users per bitmap tile
DEFAULT_BATCH_USERS = 32768


class WordProfiles:
    """What ``word_profiles`` returns: ``bitmaps``, the users' word sets as a device tensor int32 ``[ceil(n_users / 128) x n_words
    x 4]`` -- bit ``u & 31`` of word ``(u & 127) >> 5`` of cell ``(u >> 7, w)`` says "user u has word w" -- ``n_users``, ``n_words``
    and ``sizes`` int32 ``[n_users]``, the number of distinct words of every profile."""

    def __init__(self, bitmaps, n_users, n_words, sizes):
        self.bitmaps, self.n_users, self.n_words, self.sizes = bitmaps, int(n_users), int(n_words), sizes

    def to_scipy(self):
        """The profiles as a host scipy CSR matrix of booleans ``[n_users x n_words]`` (for tests and benchmarks)."""
        import scipy.sparse as sp
        M, V = self.n_users, self.n_words
        if M == 0:
            return sp.csr_matrix((0, V), dtype=bool)
        raw = self.bitmaps.cpu().numpy().view(np.uint32)
        rows = []
        for t in range(raw.shape[0]):
            bits = np.unpackbits(np.ascontiguousarray(raw[t]).view(np.uint8).reshape(V, 16), axis=1, bitorder="little")    # [V x 128]
            rows.append(sp.csr_matrix(bits.T.astype(bool)))
        return sp.vstack(rows, format="csr")[:M]


def _check_k(k):
    k = int(k)
    if not 1 <= k <= 128:
        raise ValueError(f"k must be in 1..128 (got {k})")
    return k


def _check_max_events(max_events):
    if max_events is None:
        return 0
    if int(max_events) < 1:
        raise ValueError(f"max_events must be at least 1, or None for every click (got {max_events})")
    return min(int(max_events), 2 ** 31 - 1)


def _check_batch(batch_users):
    if int(batch_users) < 1:
        raise ValueError(f"batch_users must be positive (got {batch_users})")
    return (int(batch_users) + TILE - 1) // TILE * TILE


def _check_weights(term_weights, V):
    if term_weights is None:
        return None
    w = term_weights.detach().cpu().numpy() if hasattr(term_weights, "detach") else np.asarray(term_weights)
    w = w.ravel().astype(np.float32)
    if w.shape[0] != V:
        raise ValueError(f"{w.shape[0]} term_weights for {V} words")
    if not np.isfinite(w).all():
        raise ValueError("term_weights must be finite")
    return np.ascontiguousarray(w)


def _users(users, Na, V, max_events):
    """The user argument of ``word_recommend`` / ``word_ranks``: ``(profiles or None, history CSR or None, n_users)``, checked."""
    if isinstance(users, WordProfiles):
        if users.n_words != V:
            raise ValueError(f"the profiles are over {users.n_words} words, the articles over {V}")
        if max_events is not None:
            raise ValueError("max_events belongs to word_profiles: these profiles are built already")
        return users, None, users.n_users
    indptr, items = history_csr(users, Na)
    return None, (indptr, items), int(indptr.size - 1)


def _build(torch, dev, d, indptr, items, max_events):
    """``(bitmaps int32 [tiles x V x 4], sizes int32 [M])`` of the history CSR over the device CSR ``d``; M >= 1."""
    M, (Na, V) = int(indptr.size - 1), _shape(d)
    tiles = (M + TILE - 1) // TILE
    bitmaps = torch.empty((tiles, V, 4), dtype=torch.int32, device=dev)
    sizes = torch.empty(M, dtype=torch.int32, device=dev)
    hp, hi = upload(np.ascontiguousarray(indptr, dtype=np.int64), dev), upload(np.ascontiguousarray(items.astype(np.int32)), dev)
    with torch.cuda.device(dev):
        L.call("dae_word_profiles", L.ptr(hp), L.ptr(hi), int(items.size), M, max_events, L.ptr(d["indptr"]), L.ptr(d["indices"]),
               int(d["nnz"]), Na, V, L.ptr(bitmaps), bitmaps.numel() * 4, L.ptr(sizes), L.current_stream())
    return bitmaps, sizes


def word_profiles(histories, articles, *, max_events=None, return_tensor=False, device=None):
    """The word sets of the users of ``histories`` (a list of index sequences or an ``(indptr, items)`` tuple, oldest click
    first) over ``articles`` ``[n_articles x n_words]``: word w is in user u's profile when some article among the user's last
    ``max_events`` clicks (None: all) stores column w.  Explicit zeros count; repeated clicks change nothing.  Built on the device
    with integer atomics (``dae_word_profiles``): exact, whatever the order of the users.  Returns a ``WordProfiles``; ``sizes`` is
    an ndarray, or a CUDA tensor with ``return_tensor=True``.  The bitmaps take ``ceil(n_users / 128) * n_words * 16`` bytes."""
    Na, V = _shape(articles)
    me = _check_max_events(max_events)
    indptr, items = history_csr(histories, Na)
    M = int(indptr.size - 1)
    torch, lib, dev = device_and_library(_device_of(articles, device))
    if M == 0 or V == 0 or Na == 0:
        return WordProfiles(torch.zeros(((M + TILE - 1) // TILE, V, 4), dtype=torch.int32, device=dev), M, V,
                            result(torch.zeros(M, dtype=torch.int32, device=dev), return_tensor))
    bitmaps, sizes = _build(torch, dev, _device_csr(torch, articles, dev), indptr, items, me)
    return WordProfiles(bitmaps, M, V, result(sizes, return_tensor))


def idf_weights(articles):
    """sklearn's smooth idf of the columns of ``articles`` as term weights: ``log((1 + n) / (1 + df)) + 1`` in float64 on the host
    from the document frequencies of ``column_stats`` (stored entries per column, explicit zeros included), rounded once to
    float32 ``[n_words]``."""
    n, V = _shape(articles)
    if _is_device_csr(articles):
        structure = binarize(articles)
    else:
        structure = articles.tocsr().astype(np.float32)
        structure.data = np.ones_like(structure.data)
    df = column_stats(structure)[0] if n and V else np.zeros(V, dtype=np.int64)
    return TfidfTransformer.idf_from_df(df, n, True).astype(np.float32)


class _Sweep:
    """What ``word_recommend`` and ``word_ranks`` share: the arguments checked before the device is touched, the users in window
    order, the entry weights computed once, and the loop over batches of users whose bitmaps exist at a time."""

    def __init__(self, users, articles, seen, term_weights, max_events, window, batch_users, device):
        self.Na, self.V = _shape(articles)
        self.me = _check_max_events(max_events)
        self.batch = _check_batch(batch_users)
        self.tw = _check_weights(term_weights, self.V)
        self.profiles, self.hist, self.M = _users(users, self.Na, self.V, max_events)
        M, Na = self.M, self.Na
        self.seen = None if seen is None else normalize_exclusions(seen, M, Na)
        self.window = None if window is None else normalize_window(window, M, Na)
        self.articles, self.device = articles, device
        # with windows the users go in the stable order of (lo, hi), as in most_similar: the union of a tile's windows stays narrow
        self.perm = _window_order(*self.window) if self.window is not None and self.hist is not None else None

    def batch_sizes(self):
        """The distinct numbers of users ``run`` hands to one call (the corpus split, and so the workspace, depends on it)."""
        return {n for n in (min(self.M, self.batch), self.M % self.batch) if n > 0}

    def run(self, torch, dev, d, call, *per_user):
        """``call(bitmap_pointer_tensor, users a .. b, n, xp_d, xi_d, lo_d, hi_d, weights, per_user slices)`` for every batch, the
        users in the order ``self.perm``."""
        M, V, perm = self.M, self.V, self.perm
        hist, seen, window = self.hist, self.seen, self.window
        if perm is not None:
            hist = permute_histories(*hist, perm)
            seen = None if seen is None else permute_histories(*seen, perm)
            window = (window[0][perm], window[1][perm])
            per_user = tuple(a[perm] for a in per_user)
        nnz = int(d["nnz"])
        weights = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
        tw_d = upload(self.tw, dev)
        with torch.cuda.device(dev):
            L.call("dae_word_entry_weights", L.ptr(d["indices"]), L.ptr(d["values"]), nnz, V, L.ptr(tw_d), L.ptr(weights), L.current_stream())
        for a in range(0, M, self.batch):
            b = min(a + self.batch, M)
            if self.profiles is not None:
                bits = self.profiles.bitmaps[a // TILE:(b + TILE - 1) // TILE]
            else:
                p0, p1 = int(hist[0][a]), int(hist[0][b])
                bits, _ = _build(torch, dev, d, hist[0][a:b + 1] - p0, hist[1][p0:p1], self.me)
            xp_d = xi_d = lo_d = hi_d = None
            if seen is not None:
                s0, s1 = int(seen[0][a]), int(seen[0][b])
                xp_d, xi_d = upload(np.ascontiguousarray(seen[0][a:b + 1] - s0), dev), upload(np.ascontiguousarray(seen[1][s0:s1]), dev)
            if window is not None:
                lo_d, hi_d = upload(np.ascontiguousarray(window[0][a:b]), dev), upload(np.ascontiguousarray(window[1][a:b]), dev)
            call(bits, a, b, xp_d, xi_d, lo_d, hi_d, weights, *(x[a:b] for x in per_user))

    def restore(self, torch, dev, *outs):
        if self.perm is None:
            return outs
        perm_d = torch.from_numpy(self.perm).to(dev)
        return tuple(torch.empty_like(t).index_copy_(0, perm_d, t) for t in outs)


def word_recommend(users, articles, k=10, seen=None, *, term_weights=None, max_events=None, window=None, batch_users=DEFAULT_BATCH_USERS,
                   return_tensor=False, device=None):
    """For every user the ``k`` articles with the largest word-based relevance.  ``users``: histories (as ``word_profiles`` takes
    them; ``max_events`` as there) or a ``WordProfiles`` over the same vocabulary.  The relevance of article a to user u is the
    float32 sum, in ascending column order, of a's entry weights over the words in u's profile; an entry's weight is its stored
    value (1 for a binary matrix), times ``term_weights[column]`` -- None or ``n_words`` finite floats, e.g. ``idf_weights`` --
    rounded once to float32.  Without values and weights that is the number of words the two share.

    Order and filters are those of ``most_similar``: score descending, then index ascending; ``seen`` (default None: nothing) names
    per user the articles that must not be returned -- an excluded article never takes one of the k slots; ``window`` is a pair
    ``(lo, hi)`` per user.  1 <= k <= 128.  Returns ``(indices int64 [users x k], scores float32 [users x k])`` with -1 / -inf where
    fewer than ``k`` candidates exist, as ndarrays or, with ``return_tensor=True``, CUDA tensors.

    The users go through ``batch_users`` at a time (rounded up to a multiple of 128), so the bitmaps built from histories stay
    bounded; with ``window`` and histories the users are handed over in window order and the result is put back.  The result is
    bit-identical from run to run and does not depend on ``batch_users`` or on the order of the users."""
    k = _check_k(k)
    sw = _Sweep(users, articles, seen, term_weights, max_events, window, batch_users, device)
    M, Na, V = sw.M, sw.Na, sw.V
    torch, lib, dev = device_and_library(_device_of(articles, device) if sw.profiles is None else sw.profiles.bitmaps.device)
    idx = torch.full((M, k), -1, dtype=torch.int32, device=dev)
    score = torch.full((M, k), -np.inf, dtype=torch.float32, device=dev)
    if M == 0 or Na == 0 or V == 0:
        return result((idx.long(), score), return_tensor)
    d = _device_csr(torch, articles, dev)
    ws_bytes = max(int(lib.dae_word_topk_workspace(n, Na, k)) for n in sw.batch_sizes())
    ws_p, ws = workspace(dev, ws_bytes)

    def call(bits, a, b, xp_d, xi_d, lo_d, hi_d, weights):
        with torch.cuda.device(dev):
            L.call("dae_word_topk", L.ptr(bits), b - a, V, L.ptr(d["indptr"]), L.ptr(d["indices"]), L.ptr(weights), int(d["nnz"]), Na, k,
                   L.ptr(xp_d), L.ptr(xi_d), L.ptr(lo_d), L.ptr(hi_d), L.ptr(idx[a:b]), L.ptr(score[a:b]), idx.stride(0), ws_p, ws_bytes,
                   L.current_stream())
    sw.run(torch, dev, d, call)
    idx, score = sw.restore(torch, dev, idx, score)
    return result((idx.long(), score), return_tensor)


def word_ranks(users, articles, targets, seen=None, *, term_weights=None, max_events=None, window=None, batch_users=DEFAULT_BATCH_USERS,
               return_tensor=False, device=None):
    """The full-rank twin of ``word_recommend`` (same arguments): the position of one target article per user (negative: none)
    among all the articles ``word_recommend`` could return for that user, by its scores and its order.  Returns ``(rank int64,
    target_score float32, n_candidates int64)`` as ``recommend_ranks`` returns them, so ``rank_metrics`` takes them unchanged.
    ``rank`` counts from 1 and ``target_score`` is the pair's score bit for bit: when the target is in ``word_recommend``'s list it
    stands at position ``rank - 1`` with that score.  The target itself is ranked even when ``seen`` or the window holds it out --
    the rank is then the place it would take among the user's candidates; ``rank`` is 0 (score -inf) only without a target.
    ``n_candidates`` is the number of articles competing for the user, the target included (host code)."""
    sw = _Sweep(users, articles, seen, term_weights, max_events, window, batch_users, device)
    M, Na, V = sw.M, sw.Na, sw.V
    tgt = targets.detach().cpu().numpy() if hasattr(targets, "detach") else np.asarray(targets)
    tgt = tgt.ravel()
    if tgt.size and tgt.dtype.kind not in "iu":
        raise ValueError("targets must hold integer indices")
    tgt = tgt.astype(np.int64)
    if tgt.shape[0] != M:
        raise ValueError(f"{tgt.shape[0]} targets for {M} users")
    if tgt.size and int(tgt.max()) >= Na:
        raise ValueError(f"targets must be below {Na} (got {int(tgt.max())})")
    xp, xi = (None, None) if sw.seen is None else sw.seen
    n_cand, _ = competitors(tgt, M, Na, False, xp, xi, sw.window)
    if sw.window is not None:                                           # a target outside its window still stands among the window's articles
        n_cand = n_cand + ((tgt >= 0) & ~((tgt >= sw.window[0]) & (tgt < sw.window[1]))).astype(np.int64)
    torch, lib, dev = device_and_library(_device_of(articles, device) if sw.profiles is None else sw.profiles.bitmaps.device)
    rank = torch.zeros(M, dtype=torch.int32, device=dev)
    score = torch.full((M,), -np.inf, dtype=torch.float32, device=dev)
    if M and Na and V:
        d = _device_csr(torch, articles, dev)
        ws_bytes = max(int(lib.dae_word_rank_workspace(n)) for n in sw.batch_sizes())
        ws_p, ws = workspace(dev, ws_bytes)
        t_host = np.where(tgt >= 0, tgt, -1).astype(np.int32)

        def call(bits, a, b, xp_d, xi_d, lo_d, hi_d, weights, t):
            t_d = upload(np.ascontiguousarray(t), dev)
            with torch.cuda.device(dev):
                L.call("dae_word_rank", L.ptr(bits), b - a, V, L.ptr(d["indptr"]), L.ptr(d["indices"]), L.ptr(weights), int(d["nnz"]), Na,
                       L.ptr(xp_d), L.ptr(xi_d), L.ptr(lo_d), L.ptr(hi_d), L.ptr(t_d), L.ptr(rank[a:b]), L.ptr(score[a:b]), ws_p, ws_bytes,
                       L.current_stream())
        sw.run(torch, dev, d, call, t_host)
        rank, score = sw.restore(torch, dev, rank, score)
    return result((rank.long(), score, torch.from_numpy(n_cand).to(dev) if return_tensor else n_cand), return_tensor)
