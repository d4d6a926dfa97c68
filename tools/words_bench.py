#!/usr/bin/env python3
"""The word-based user model (helpers.word_profiles / word_recommend / word_ranks: bitmap profiles, sparse on both sides) against the
route that existed before it: the users x vocabulary profile matrix built on the host with scipy and handed to
``most_similar(profiles, candidates=articles, metric="linear kernel", exclude=seen, chunk_rows="auto")``, which densifies both
operands chunk by chunk and spends 2 V MFMA flops per (user, article) pair.

Shape (defaults): 100 000 articles over V = 10 000 words, about 100 words per article drawn from a Zipf law, 65 536 users with
``synthetic_sessions`` histories, k = 10, every user's own history as the seen list.  Both routes run in this process on the same
device, their repetitions interleaved (new, old, new, old, ...), every call timed from launch to a device synchronisation; the
report gives every repetition, not only a mean.  Also: the peak device memory of each route (torch's allocator above what was
allocated before the call), the windowed case (a window of n_articles / 16 per user), which the old route cannot run, and
``word_ranks``.  With ``--topk-trees A,B`` (two built checkouts, e.g. the parent commit and this one) ``tools/topk_bench.py`` of each
is run as a child process, four rounds in the orders A B, A B, B A, B A (a gap that follows the position and not the tree shows as
such), and the report says per shape whether B's slowest run lies above the spread of A's: the top-k kernels share their epilogue with the
word kernels, so their time is part of this measurement.  Without the option the report says that the comparison was not run.

  python tools/words_bench.py                              # writes profiles/words_bench.txt
  python tools/words_bench.py --articles 20000 --users 8192 --reps 2 --out /tmp/words.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def zipf_articles(n_articles, n_words, per_article, seed):
    """A CSR matrix [n_articles x n_words] float32 with about ``per_article`` distinct Zipf-distributed columns per row and
    tf-idf-like values."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(n_words) + 10.0)
    p /= p.sum()
    draws = int(per_article * 1.35)                                       # duplicates go: about per_article stay
    cols = np.sort(rng.choice(n_words, size=(n_articles, draws), p=p), axis=1)
    keep = np.ones(cols.shape, dtype=bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    indptr = np.zeros(n_articles + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(keep.sum(axis=1))
    indices = cols[keep].astype(np.int32)
    data = rng.uniform(0.02, 0.5, indices.size).astype(np.float32)
    return sp.csr_matrix((data, indices, indptr), shape=(n_articles, n_words))


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_bytes(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - base)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", type=int, default=100000)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--per-article", type=int, default=100)
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-old", action="store_true", help="do not run the dense route")
    ap.add_argument("--topk-trees", default="", help="two built checkouts A,B whose tools/topk_bench.py are run interleaved")
    ap.add_argument("--topk-names", default="", help="what the two checkouts are, for the report: NAME_A,NAME_B")
    ap.add_argument("--topk-shapes", default="8000x500x10,8000x500x100")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "words_bench.txt"))
    a = ap.parse_args(argv)
    import scipy.sparse as sp
    import torch
    from dae_rnn_news_recommendation_amd import helpers
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
    assert torch.cuda.is_available(), "words_bench needs a GPU"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    Na, V, M, k = a.articles, a.vocab, a.users, a.k
    A = zipf_articles(Na, V, a.per_article, a.seed)
    labels = np.random.default_rng(a.seed + 1).integers(0, 40, Na)
    indptr, items = synthetic_sessions(M, labels, mean_len=12, seed=a.seed + 2)
    hist = (np.asarray(indptr, dtype=np.int64), np.asarray(items, dtype=np.int64))
    say("words_bench on %s: %d articles x %d words, %.1f words per article, %d users, %.1f clicks per user, k = %d" % (
        torch.cuda.get_device_name(0), Na, V, A.nnz / Na, M, items.size / M, k))
    d = dict(indptr=torch.from_numpy(A.indptr.astype(np.int64)).cuda(), indices=torch.from_numpy(A.indices.astype(np.int32)).cuda(),
             values=torch.from_numpy(A.data).cuda(), n_rows=Na, nnz=int(A.nnz), n_cols=V)
    targets = np.random.default_rng(a.seed + 3).integers(0, Na, M)
    lo = np.random.default_rng(a.seed + 4).integers(0, Na - Na // 16 + 1, M)
    window = (lo, lo + Na // 16)

    t0 = time.perf_counter()
    H = sp.csr_matrix((np.ones(items.size, dtype=np.float32), hist[1], hist[0]), shape=(M, Na))
    P = (H @ (A != 0).astype(np.float32)).tocsr()
    P.data[:] = 1.0
    P.sort_indices()
    say("host: scipy profiles %.0f ms, %.1f words per profile (the old route's input; not part of its device time)" % (
        (time.perf_counter() - t0) * 1e3, P.nnz / M))

    new_profiles = lambda: helpers.word_profiles(hist, d, return_tensor=True)                                       # noqa: E731
    new_recommend = lambda: helpers.word_recommend(hist, d, k, seen=hist, return_tensor=True)                       # noqa: E731
    new_window = lambda: helpers.word_recommend(hist, d, k, seen=hist, window=window, return_tensor=True)           # noqa: E731
    new_ranks = lambda: helpers.word_ranks(hist, d, targets, seen=hist, return_tensor=True)                         # noqa: E731
    old = lambda: helpers.most_similar(P, k, norm="", metric="linear kernel", candidates=A, exclude=hist, chunk_rows="auto",   # noqa: E731
                                       return_tensor=True)
    prof = new_profiles()
    same = bool((prof.sizes.cpu().numpy() == np.diff(P.indptr)).all())
    if M * V <= 1 << 28:
        same = same and (prof.to_scipy() != P.astype(bool)).nnz == 0
    say("device profiles equal the scipy profiles (%s): %s; bitmaps %.1f MiB" % (
        "bit for bit" if M * V <= 1 << 28 else "profile sizes", same, prof.bitmaps.numel() * 4 / 2 ** 20))
    routes = [("word_profiles", new_profiles), ("word_recommend", new_recommend), ("word_recommend window n/16", new_window),
              ("word_ranks", new_ranks)]
    if not a.skip_old:
        routes.append(("most_similar dense chunked", old))
    for name, fn in routes:                                               # warm-up: the first call of every kernel
        ms, _ = timed(torch, fn)
        say("warm-up %-28s %10.1f ms" % (name, ms))
    times = {name: [] for name, _ in routes}
    for r in range(a.reps):                                               # interleaved repetitions
        for name, fn in routes:
            times[name].append(timed(torch, fn)[0])
    for name, _ in routes:
        t = times[name]
        say("%-36s median %10.1f ms   all %s" % (name, float(np.median(t)), " ".join("%.1f" % x for x in t)))
    for name, fn in routes:
        say("peak device memory %-28s %10.1f MiB" % (name, peak_bytes(torch, fn) / 2 ** 20))
    if not a.skip_old:
        got, want = new_recommend(), old()
        agree = float((got[0] == want[0]).float().mean())
        say("lists of the two routes agree in %.4f of the slots (fp32 sums in different orders: near-ties may swap)" % agree)
        say("word_recommend is %.1fx the dense route (median over median)" % (
            np.median(times["most_similar dense chunked"]) / np.median(times["word_recommend"])))
    trees = [t for t in a.topk_trees.split(",") if t]
    if not trees:
        say("top-k comparison not run: it needs --topk-trees A,B, two built checkouts (the parent commit and this one)")
    else:
        assert len(trees) == 2, "--topk-trees takes two checkouts"
        names = dict(zip("AB", (a.topk_names.split(",") + ["the first of --topk-trees", "the second"])[:2]))
        say("tools/topk_bench.py (most_similar, ms per call) of two built checkouts, one child process per run: A = %s, B = %s" % (names["A"], names["B"]))
        ms = {}
        for r, order in enumerate(("AB", "AB", "BA", "BA")):          # both orders: a gap that follows the position is not the tree's
            for pos, tag in enumerate(order):
                run = subprocess.run([sys.executable, os.path.join(trees["AB".index(tag)], "tools", "topk_bench.py"), "--shapes", a.topk_shapes],
                                     capture_output=True, text=True, timeout=900)
                assert run.returncode == 0, run.stderr[-2000:]
                for l in run.stdout.splitlines():
                    if l.startswith("{"):
                        j = json.loads(l)
                        shape = "N %d D %d k %d" % (j["N"], j["D"], j["k"])
                        ms.setdefault(shape, {"A": [], "B": []})[tag].append((j["most_similar"]["ms"], pos))
                        say("topk_bench round %d order %s, %s runs %s: %s most_similar %.4f ms, pairwise %.4f ms" % (
                            r, order, tag, "first" if pos == 0 else "second", shape, j["most_similar"]["ms"], j["pairwise"]["ms"]))
        for shape, t in ms.items():
            A_, B_ = [x for x, _ in t["A"]], [x for x, _ in t["B"]]
            first = [x for v in t.values() for x, pos in v if pos == 0]
            second = [x for v in t.values() for x, pos in v if pos == 1]
            say("topk %s: A %.4f .. %.4f (median %.4f), B %.4f .. %.4f (median %.4f), B / A %.4f; B above A's spread: %s (B's slowest run "
                "against A's slowest); run first %.4f, run second %.4f (medians over both trees)" % (
                    shape, min(A_), max(A_), float(np.median(A_)), min(B_), max(B_), float(np.median(B_)),
                    float(np.median(B_)) / float(np.median(A_)), "yes" if max(B_) > max(A_) else "no", float(np.median(first)),
                    float(np.median(second))))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
