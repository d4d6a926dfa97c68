#!/usr/bin/env python3
"""One Lloyd iteration of spherical k-means at a few (N, K, D): the dedicated entries against top-k at k = 1 and against torch.

  (k) centroid image + dae_kmeans_assign + dae_kmeans_update       what helpers.kmeans runs per iteration (the row image is built once)
  (a) dae_topk_similarity with k = 1 + dae_kmeans_update           most_similar(k = 1), the route a user had: it builds both images
                                                                   inside the call (the N x pad(D) row image is written and read again)
  (i) centroid image + dae_topk_images with k = 1                  the LDS-tile epilogue of top-k on the SAME prebuilt row image as (k):
                                                                   the two differ in the epilogue (and the carry top-k keeps) alone
  (b) torch: normalised X @ C.T -> argmax -> index_add_ -> normalise     the N x K score matrix in memory, fp32 sums by atomics

Buffers and workspaces are allocated beforehand; a timing is a host clock around --min-ms worth of back-to-back calls (at least
one; the count is fixed per route after the warm-up round), each ending in a synchronise as the entries return host numbers, so a
figure holds one launch sequence and one synchronise per call.  The routes run interleaved, --rounds times after one warm-up round,
in one process: per route the median and the minimum over the rounds of the time per call, the TFLOP/s of the assignment
(2 N K D over its median) and the peak device memory above the operands.  The labels of the routes are compared ((k), (a) and (i)
must agree exactly; torch's matmul rounds differently).

  python tools/kmeans_bench.py                                   # 200000x1024x500, 50000x256x500, 20000x4096x500, 2000x8192x500
  python tools/kmeans_bench.py --shapes 100000x512x128 --rounds 9
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

DEFAULT_SHAPES = "200000x1024x500,50000x256x500,20000x4096x500,2000x8192x500"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated N x K x D")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=20.0, help="length of one timed window")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd.helpers._device import workspace
    assert torch.cuda.is_available(), "kmeans_bench needs a GPU"
    lib = L.load()
    dev = torch.device("cuda")
    print(json.dumps(device_record(torch)), flush=True)
    for shape in a.shapes.split(","):
        N, K, D = (int(v) for v in shape.lower().split("x"))
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        cent = torch.nn.functional.normalize(torch.randn(K, D, device=dev, generator=g), dim=1)
        y = torch.randint(0, K, (N,), device=dev, generator=g)
        X = torch.nn.functional.normalize(cent[y] + 0.3 * torch.randn(N, D, device=dev, generator=g), dim=1).contiguous()
        C = X[torch.randperm(N, device=dev, generator=g)[:K]].clone()      # full-range random data, rows as centroids
        stream = L.current_stream()
        xb, cb = int(lib.dae_sweep_image_bytes(N, D)), int(lib.dae_sweep_image_bytes(K, D))
        (xi_p, xi), (ci_p, ci) = workspace(dev, xb), workspace(dev, cb)
        L.call("dae_sweep_image_dense", L.ptr(X), X.stride(0), N, D, 0, 0, xi_p, xb, stream)
        aws_b, uws_b, tws_b = int(lib.dae_kmeans_assign_workspace(N, K)), int(lib.dae_kmeans_update_workspace(N, K, D)), \
            int(lib.dae_topk_similarity_workspace(N, K, D, 1))
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        (aws_p, aws), (uws_p, uws) = workspace(dev, aws_b), workspace(dev, uws_b)
        i32 = dict(dtype=torch.int32, device=dev)
        labels, scores = torch.empty(N, **i32), torch.empty(N, dtype=torch.float32, device=dev)
        counts, order, offsets = torch.empty(K, **i32), torch.empty(N, **i32), torch.empty(K + 1, dtype=torch.int64, device=dev)
        C_new = torch.empty_like(C)
        rec = (ctypes.c_double * 4)()

        def assign_k():
            L.call("dae_sweep_image_dense", L.ptr(C), C.stride(0), K, D, 0, 0, ci_p, cb, stream)
            L.call("dae_kmeans_assign", xi_p, N, ci_p, K, D, None, L.ptr(labels), L.ptr(scores), rec, aws_p, aws_b, stream)

        def update_k(lab=None):
            L.call("dae_kmeans_update", xi_p, N, D, L.ptr(labels if lab is None else lab), K, L.ptr(C_new), C_new.stride(0), L.ptr(counts),
                   L.ptr(order), L.ptr(offsets), rec, uws_p, uws_b, stream)

        assign_k()
        update_k()
        own_peak = torch.cuda.max_memory_allocated() - base
        tws_p, tws = workspace(dev, tws_b)
        idx1, sc1 = torch.empty((N, 1), **i32), torch.empty((N, 1), dtype=torch.float32, device=dev)

        def assign_a():
            L.call("dae_topk_similarity", L.ptr(X), X.stride(0), N, L.ptr(C), C.stride(0), K, D, 0, 0, 1, 0, L.ptr(idx1), L.ptr(sc1), 1, tws_p,
                   tws_b, stream)
            torch.cuda.synchronize()

        iws_b, carry_b = int(lib.dae_topk_images_workspace(N, K, 1)), int(lib.dae_topk_carry_bytes(N, 1))
        (iws_p, iws), (carry_p, carry) = workspace(dev, iws_b), workspace(dev, carry_b)
        idx2, sc2 = torch.empty((N, 1), **i32), torch.empty((N, 1), dtype=torch.float32, device=dev)

        def assign_i():
            L.call("dae_sweep_image_dense", L.ptr(C), C.stride(0), K, D, 0, 0, ci_p, cb, stream)
            carry.zero_()                                              # an empty carry
            L.call("dae_topk_images", xi_p, N, 0, ci_p, K, 0, D, 1, 0, None, None, carry_p, L.ptr(idx2), L.ptr(sc2), 1, iws_p, iws_b, stream)
            torch.cuda.synchronize()

        t_state = {}

        def assign_b():
            t_state["lab"] = (X @ torch.nn.functional.normalize(C, dim=1).T).argmax(dim=1)
            torch.cuda.synchronize()

        def update_b():
            s = torch.zeros(K, D, device=dev).index_add_(0, t_state["lab"], X)
            t_state["C"] = torch.nn.functional.normalize(s, dim=1)
            torch.cuda.synchronize()

        routes = {"kmeans_assign": assign_k, "kmeans_update": update_k, "topk1_assign": assign_a, "topk1_images_assign": assign_i, "torch_assign": assign_b,
                  "torch_update": update_b}
        times = {name: [] for name in routes}
        peaks, reps = {}, {}
        for rnd in range(a.rounds + 1):
            for name, fn in routes.items():
                if rnd == 0:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    fn()                                               # first use: code objects, attributes, allocator
                    peaks[name] = int(torch.cuda.max_memory_allocated() - before)
                n = reps.get(name, 3)
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                ms = (time.perf_counter() - t0) * 1e3 / n
                if rnd == 0:
                    reps[name] = max(1, int(round(a.min_ms / max(ms, 1e-3))))
                else:
                    times[name].append(ms)
        flop = 2.0 * N * K * D
        same_a = bool(torch.equal(labels, idx1[:, 0]) and torch.equal(scores, sc1[:, 0]))
        same_i = bool(torch.equal(labels, idx2[:, 0]) and torch.equal(scores, sc2[:, 0]))
        same_b = float((labels.long() == t_state["lab"]).double().mean().item())
        out = {"N": N, "K": K, "D": D, "rounds": a.rounds, "labels_equal_topk1": same_a, "labels_equal_topk1_images": same_i, "calls_per_window": reps,
               "labels_equal_torch_share": round(same_b, 6), "workspace_bytes": {"kmeans_assign": aws_b, "kmeans_update": uws_b, "topk1": tws_b},
               "peak_bytes_first_call": peaks, "own_buffers_bytes": int(own_peak)}
        for name, ts in times.items():
            out[name + "_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
            if name.endswith("assign"):
                out[name + "_tflops"] = round(flop / statistics.median(ts) * 1e-9, 2)
        out["iteration_ms"] = {"kmeans": round(out["kmeans_assign_ms"]["median"] + out["kmeans_update_ms"]["median"], 3),
                               "topk1_then_update": round(out["topk1_assign_ms"]["median"] + out["kmeans_update_ms"]["median"], 3),
                               "torch": round(out["torch_assign_ms"]["median"] + out["torch_update_ms"]["median"], 3)}
        print(json.dumps(out), flush=True)
        del xi, ci, aws, uws, tws, iws, carry, X, C, t_state
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
