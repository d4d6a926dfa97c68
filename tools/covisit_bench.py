#!/usr/bin/env python3
"""The co-visitation build and its recommendation at the workload's own shape, against what a user would write without them.

  build      dae_covisit_neighbors (emit, rocprim sort, run-length, select) against the torch route on the same device: the record
             keys by tensor ops (one shifted comparison per window offset), torch.unique(return_counts=True) for the pair counts, and
             a composite sort -- by similarity within the article -- for the cut to K per row.  Both tables are compared.
  recommend  dae_covisit_recommend over all users against a NumPy loop over a sample of them (the lists are compared).

The log is seeded: geometric history lengths, articles drawn from a Zipf law (so hub articles with thousands of distinct neighbours
exist beside a median of tens).  Buffers and workspaces are allocated beforehand; a timing is a host clock around one call ending in
a synchronise, the median and the minimum over --rounds after a warm-up call.  Reported per route: ms, records / s, GB / s of key
bytes sorted (8 bytes per record over the whole build), the share of the build's kernel time spent in rocprim's sort (one profiled
call, kernels told apart by name), and the peak device memory above the inputs.  No pass mark: the figures are what they are.

  python tools/covisit_bench.py                                  # 100000 articles, 1000000 users, mean length 12, window 3
  python tools/covisit_bench.py --articles 20000 --users 100000 --rounds 9
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.recommend_bench import device_record  # noqa: E402


def zipf_log(np, users, articles, mean_len, seed, s=1.0):
    rng = np.random.default_rng(seed)
    lens = rng.geometric(1.0 / mean_len, users).astype(np.int64)
    indptr = np.zeros(users + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    p = 1.0 / np.arange(1, articles + 1) ** s
    items = rng.permutation(articles)[np.searchsorted(np.cumsum(p / p.sum()), rng.random(int(indptr[-1]))).clip(0, articles - 1)]
    return indptr, items.astype(np.int32)


def torch_route(torch, d_ptr, d_items, Na, window, K):
    """The table by tensor ops; returns (nbr int64 [Na x K], sim, n_records, n_pairs)."""
    dev = d_items.device
    nnz = d_items.numel()
    it = d_items.long()
    user = torch.repeat_interleave(torch.arange(d_ptr.numel() - 1, device=dev), d_ptr[1:] - d_ptr[:-1])
    keys = []
    for d in range(1, window + 1):
        if d >= nnz:
            break
        a, b = it[:-d], it[d:]
        ok = (user[:-d] == user[d:]) & (a != b)
        a, b = a[ok], b[ok]
        keys += [a * Na + b, b * Na + a]
    keys = torch.cat(keys)
    uniq, c = torch.unique(keys, return_counts=True)
    a, b = uniq // Na, uniq % Na
    clicks = torch.bincount(it, minlength=Na).float()
    s = c.float() / torch.sqrt(clicks[a] * clicks[b])
    order = torch.argsort(s, descending=True, stable=True)                # b ascending already (uniq is sorted): stable keeps it
    order = order[torch.argsort(a[order], stable=True)]
    a, b, s = a[order], b[order], s[order]
    start = torch.searchsorted(a, torch.arange(Na, device=dev))
    rank = torch.arange(a.numel(), device=dev) - start[a]
    keep = rank < K
    nbr = torch.full((Na, K), -1, dtype=torch.int64, device=dev)
    sim = torch.zeros((Na, K), dtype=torch.float32, device=dev)
    nbr[a[keep], rank[keep]] = b[keep]
    sim[a[keep], rank[keep]] = s[keep]
    return nbr, sim, int(keys.numel()), int(uniq.numel())


def numpy_recommend(np, nbr, sim, indptr, items, users, w, last, k):
    out = np.full((len(users), k), -1, dtype=np.int64)
    for r, u in enumerate(users):
        h = items[indptr[u]:indptr[u + 1]]
        n = min(last, h.size)
        acc = {}
        for o in range(n):
            x, wt = int(h[h.size - n + o]), w[n - 1 - o]
            row, srow = nbr[x], sim[x]
            for t in range(int((row >= 0).sum())):
                c = int(row[t])
                acc[c] = np.float32(acc.get(c, np.float32(0)) + np.float32(wt * srow[t]))
        mine = set(h.tolist())
        cand = sorted(((c, s) for c, s in acc.items() if c not in mine), key=lambda cs: (-float(cs[1]), cs[0]))[:k]
        out[r, :len(cand)] = [c for c, _ in cand]
    return out


def timed(torch, fn, rounds):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def peak_of(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, int(torch.cuda.max_memory_allocated() - before)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", type=int, default=100000)
    ap.add_argument("--users", type=int, default=1000000)
    ap.add_argument("--mean-len", type=float, default=12.0)
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--neighbors", type=int, default=50)
    ap.add_argument("--last", type=int, default=10)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--sample", type=int, default=200, help="users of the NumPy recommendation loop")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    from dae_rnn_news_recommendation_amd.helpers._device import workspace
    assert torch.cuda.is_available(), "covisit_bench needs a GPU"
    lib, dev = L.load(), torch.device("cuda")
    print(json.dumps(device_record(torch)), flush=True)
    Na, M, K, w = a.articles, a.users, a.neighbors, a.window
    indptr, items = zipf_log(np, M, Na, a.mean_len, a.seed)
    nnz = int(items.size)
    host = indptr.ctypes.data_as(ctypes.c_void_p)
    bound = int(lib.dae_covisit_record_bound(host, M, w, 1))
    ws_bytes = int(lib.dae_covisit_neighbors_workspace(bound, Na, K))
    d_ptr, d_items = torch.from_numpy(indptr).to(dev), torch.from_numpy(items).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    nbr, cnt, sim = torch.empty((Na, K), **i32), torch.empty((Na, K), **i32), torch.empty((Na, K), dtype=torch.float32, device=dev)
    degree, clicks, totals = torch.empty(Na, **i32), torch.empty(Na, **i32), torch.empty(2, dtype=torch.int64, device=dev)
    ws_p, ws = workspace(dev, ws_bytes)
    stream = L.current_stream()

    def build():
        L.call("dae_covisit_neighbors", L.ptr(d_ptr), L.ptr(d_items), host, M, nnz, Na, w, 1, 1, K, L.ptr(nbr), L.ptr(sim), L.ptr(cnt), K,
               L.ptr(degree), L.ptr(clicks), L.ptr(totals), ws_p, ws_bytes, stream)

    t_build = timed(torch, build, a.rounds)
    records, pairs = (int(v) for v in totals.cpu().numpy())
    deg = degree.cpu().numpy()
    sort_share = None
    try:                                                                  # one profiled call: the sort's share of the kernel time
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            build()
            torch.cuda.synchronize()
        ev = [(e.key, getattr(e, "device_time_total", 0) or getattr(e, "cuda_time_total", 0)) for e in prof.key_averages()]
        total = sum(t for _, t in ev)
        sort_share = round(sum(t for n, t in ev if "sort" in n.lower() or "onesweep" in n.lower() or "histogram" in n.lower()) / total, 4) if total else None
        kernels = sorted(ev, key=lambda e: -e[1])[:8]
    except Exception as exc:                                              # the figure is optional; say why it is missing
        kernels = [("profiler unavailable: %r" % (exc,), 0)]
    (t_nbr, t_sim, t_rec, t_pairs), torch_peak = peak_of(torch, lambda: torch_route(torch, d_ptr, d_items, Na, w, K))
    t_torch = timed(torch, lambda: torch_route(torch, d_ptr, d_items, Na, w, K), max(1, a.rounds // 2))
    same_nbr = float((t_nbr == nbr.long()).double().mean().item())
    same_sim = float((t_sim.view(torch.int32) == sim.view(torch.int32)).double().mean().item())
    out = {"articles": Na, "users": M, "clicks": nnz, "window": w, "neighbors": K, "records": records, "record_bound": bound, "pairs": pairs,
           "degree": {"median": float(np.median(deg)), "p99": float(np.percentile(deg, 99)), "max": int(deg.max()),
                      "rows_over_256": int((deg > 256).sum())},
           "build_ms": t_build, "build_records_per_s": round(records / t_build["median"] * 1e3), "build_key_GBps": round(records * 8 / t_build["median"] * 1e-6, 2),
           "build_sort_share_of_kernel_time": sort_share, "build_top_kernels_us": [(n[:60], round(t)) for n, t in kernels],
           "build_workspace_bytes": ws_bytes, "torch_ms": t_torch, "torch_peak_bytes": torch_peak, "torch_records": t_rec, "torch_pairs": t_pairs,
           "speedup_over_torch": round(t_torch["median"] / t_build["median"], 2), "neighbors_equal_share": round(same_nbr, 6),
           "sims_bit_equal_share": round(same_sim, 6)}
    print(json.dumps(out), flush=True)
    del t_nbr, t_sim
    torch.cuda.empty_cache()
    # recommend
    xp, xi = helpers.normalize_exclusions((indptr, items), M, Na)
    age = (np.float64(0.8) ** np.arange(a.last)).astype(np.float32)
    d_xp, d_xi, d_age = torch.from_numpy(xp).to(dev), torch.from_numpy(xi).to(dev), torch.from_numpy(age).to(dev)
    idx, score = torch.empty((M, a.k), **i32), torch.empty((M, a.k), dtype=torch.float32, device=dev)

    def rec():
        L.call("dae_covisit_recommend", L.ptr(nbr), L.ptr(sim), K, Na, K, L.ptr(d_ptr), L.ptr(d_items), M, L.ptr(d_xp), L.ptr(d_xi), None, None,
               L.ptr(d_age), a.last, a.k, L.ptr(idx), L.ptr(score), a.k, stream)

    t_rec_ms = timed(torch, rec, a.rounds)
    users = np.random.default_rng(a.seed + 1).choice(M, min(a.sample, M), replace=False)
    h_nbr, h_sim = nbr.cpu().numpy(), sim.cpu().numpy()
    t0 = time.perf_counter()
    want = numpy_recommend(np, h_nbr, h_sim, indptr, items, users, age, a.last, a.k)
    np_ms = (time.perf_counter() - t0) * 1e3
    got = idx.cpu().numpy()[users]
    print(json.dumps({"recommend_users": M, "last": a.last, "k": a.k, "recommend_ms": t_rec_ms,
                      "recommend_users_per_s": round(M / t_rec_ms["median"] * 1e3), "numpy_sample_users": int(users.size),
                      "numpy_ms_per_user": round(np_ms / users.size, 3), "numpy_ms_all_users_extrapolated": round(np_ms / users.size * M),
                      "lists_equal": bool(np.array_equal(got, want))}), flush=True)


if __name__ == "__main__":
    main()
