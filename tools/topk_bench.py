#!/usr/bin/env python3
"""Top-k retrieval timing: helpers.most_similar (fused similarity + top-k, dae_topk_similarity) against the materialised
path, pairwise_similarity(return_tensor=True) alone and followed by torch.topk.

Every path is warmed up on every shape, then timed with HIP events over windows of at least --window-ms (the repetition count
doubles until a window is long enough); the time per call is the window over the repetitions.  One JSON line per shape:
times, achieved TFLOP/s (2 Nq Nc D / time) and their share of the fp32 MFMA peak of the MI355X (157.3 TF/s), and the peak
device memory each path allocates (torch.cuda.max_memory_allocated above what was allocated before the call).

  python tools/topk_bench.py                         # N = 8000 at k = 10 and 100, N = 64000 at k = 100; D = 500
  python tools/topk_bench.py --shapes 20000x500x100
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3
DEFAULT_SHAPES = "8000x500x10,8000x500x100,64000x500x100"


def timed_ms(torch, fn, window_ms):
    reps = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= window_ms:
            return ms / reps, reps
        reps *= 2


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
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated N x D x k (queries = corpus = N rows)")
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "topk_bench needs a GPU"
    for shape in a.shapes.split(","):
        N, D, k = (int(v) for v in shape.lower().split("x"))
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        X = torch.randn((N, D), device="cuda", generator=g)
        paths = {
            "most_similar": lambda: helpers.most_similar(X, k=k, return_tensor=True),
            "pairwise": lambda: helpers.pairwise_similarity(X, return_tensor=True),
            "pairwise_topk": lambda: torch.topk(helpers.pairwise_similarity(X, return_tensor=True), k, dim=1),
        }
        for fn in paths.values():                          # warm-up: library load, kernel attributes, allocator
            fn()
        torch.cuda.synchronize()
        flop = 2.0 * N * N * D
        rec = {"N": N, "D": D, "k": k, "flop": flop}
        for name, fn in paths.items():
            ms, reps = timed_ms(torch, fn, a.window_ms)
            rec[name] = {"ms": round(ms, 4), "reps": reps, "tflops": round(flop / ms * 1e-9, 2),
                         "peak_frac": round(flop / ms * 1e-9 / PEAK_FP32_MFMA_TFLOPS, 4), "peak_mem_bytes": peak_bytes(torch, fn)}
        rec["most_similar_over_pairwise"] = round(rec["most_similar"]["ms"] / rec["pairwise"]["ms"], 3)
        rec["most_similar_over_pairwise_topk"] = round(rec["most_similar"]["ms"] / rec["pairwise_topk"]["ms"], 3)
        print(json.dumps(rec), flush=True)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
