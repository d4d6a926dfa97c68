#!/usr/bin/env python3
"""Cluster-probed top-k (helpers.ClusterIndex.search) against the exact sweep (helpers.most_similar) on planted blobs.

One JSON line for the index build (k-means: iterations, mean score, ms) and the exact sweep, then one per n_probe: wall
milliseconds per call (host clock around a synchronised call, best of --repeats after a warm-up), recall@k against the exact lists,
and the share of the corpus a query is scored against (the members of its probed clusters; the kernel walks whole 128-column
tiles of them).  Recall depends on the data: the blobs here overlap (--noise), so a row's neighbours spill into other clusters.

  python tools/ann_bench.py                                      # 200000 articles, 20000 queries, H = 500, 1024 clusters
  python tools/ann_bench.py --articles 50000 --clusters 256 --probes 1,2,4,8
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.recommend_bench import device_record  # noqa: E402


def best_ms(torch, fn, repeats):
    out = fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return round(best, 3), out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", type=int, default=200000)
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--H", type=int, default=500)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--topics", type=int, default=2000, help="planted blobs")
    ap.add_argument("--noise", type=float, default=0.08)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--probes", default="1,4,16,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "ann_bench needs a GPU"
    print(json.dumps(device_record(torch)), flush=True)
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    centres = torch.nn.functional.normalize(torch.randn(a.topics, a.H, device=dev, generator=g), dim=1)

    def draw(n):
        y = torch.randint(0, a.topics, (n,), device=dev, generator=g)
        return torch.nn.functional.normalize(centres[y] + a.noise * torch.randn(n, a.H, device=dev, generator=g), dim=1).contiguous()
    E, Q = draw(a.articles), draw(a.queries)
    t0 = time.perf_counter()
    res = helpers.kmeans(E, a.clusters, max_iter=a.iters, seed=a.seed, return_tensor=True)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    ix = helpers.ClusterIndex.from_kmeans(E, res)
    sizes = res.counts.cpu().numpy()
    print(json.dumps({"job": "build", "articles": a.articles, "H": a.H, "clusters": a.clusters, "kmeans_ms": round(build_ms, 1),
                      "n_iter": res.n_iter, "mean_score": round(res.mean_score, 6), "relocated": res.relocated,
                      "largest_cluster": int(sizes.max()), "smallest_cluster": int(sizes.min())}), flush=True)
    exact_ms, (want, _) = best_ms(torch, lambda: helpers.most_similar(Q, a.k, candidates=E, return_tensor=True), a.repeats)
    print(json.dumps({"job": "exact", "queries": a.queries, "k": a.k, "ms": exact_ms}), flush=True)
    for n_probe in (int(p) for p in a.probes.split(",")):
        ms, (got, _) = best_ms(torch, lambda: ix.search(Q, a.k, n_probe=n_probe, return_tensor=True), a.repeats)
        hits = (got.unsqueeze(2) == want.unsqueeze(1)).any(dim=2) & (got >= 0)
        print(json.dumps({"job": "probed", "n_probe": n_probe, "ms": ms, "ms_over_exact": round(ms / exact_ms, 3),
                          "recall_at_k": round(float(hits.double().sum().item() / want.numel()), 5),
                          "corpus_share_scored": round(ix.probed_fraction(Q, n_probe), 5)}), flush=True)


if __name__ == "__main__":
    main()
