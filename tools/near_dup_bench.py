#!/usr/bin/env python3
"""Near-duplicate search timing: helpers.similar_pairs in self mode (fused similarity + threshold filter, dae_threshold_pairs,
only the tiles on or below the diagonal) against the materialised route, pairwise_similarity(return_tensor=True) alone and
followed by torch.nonzero(torch.tril(S >= T, -1)).

The rows are standard-normal with planted duplicates: the last --dup-frac of them are earlier rows plus 0.05 x noise (cosine
about 0.9988), so the result is not empty at T = 0.9.  Every path is warmed up on every shape, then timed with HIP events
over windows of at least --window-ms (the repetition count doubles until a window is long enough); the time per call is
the window over the repetitions.  One JSON line per shape: times, achieved TFLOP/s by useful FLOPs (similar_pairs: the strict
lower triangle, N (N - 1) D; the matrix paths: the whole square, 2 N N D) and their share of the fp32 MFMA peak of the MI355X
(157.3 TF/s), the peak device memory each path allocates (torch.cuda.max_memory_allocated above what was allocated before the call) and the pair
count.  Shapes whose matrix would not fit --matrix-limit-gb run similar_pairs alone.

  python tools/near_dup_bench.py                         # 8000 x 500, 20000 x 500, 64000 x 500 (similar_pairs alone); T = 0.9
  python tools/near_dup_bench.py --shapes 20000x500 --threshold 0.95 --out profiles/near_dup_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3
DEFAULT_SHAPES = "8000x500,20000x500,64000x500"


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
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated N x D (the corpus is searched against itself)")
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--dup-frac", type=float, default=0.05, help="share of the rows that are noisy copies of earlier rows")
    ap.add_argument("--matrix-limit-gb", type=float, default=8.0, help="skip the materialised paths when N x N x 4 bytes exceed this")
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    import torch
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "near_dup_bench needs a GPU"
    T = a.threshold
    lines = []
    for shape in a.shapes.split(","):
        N, D = (int(v) for v in shape.lower().split("x"))
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        X = torch.randn((N, D), device="cuda", generator=g)
        n_dup = int(N * a.dup_frac)
        if n_dup:
            src = torch.randint(0, N - n_dup, (n_dup,), device="cuda", generator=g)
            X[N - n_dup:] = X[src] + 0.05 * torch.randn((n_dup, D), device="cuda", generator=g)
        paths = {"similar_pairs": lambda: helpers.similar_pairs(X, T, return_tensor=True)}
        if N * N * 4 <= a.matrix_limit_gb * 1e9:
            paths["pairwise"] = lambda: helpers.pairwise_similarity(X, set_diagonal_zero=False, return_tensor=True)
            paths["pairwise_nonzero"] = lambda: torch.nonzero(torch.tril(
                helpers.pairwise_similarity(X, set_diagonal_zero=False, return_tensor=True) >= T, -1))
        counts = {}
        for name, fn in paths.items():                      # warm-up: library load, kernel attributes, allocator
            out = fn()
            if name != "pairwise":                          # rows of similar_pairs / index pairs of torch.nonzero
                counts[name] = int((out[0] if isinstance(out, tuple) else out).shape[0])
            del out
        torch.cuda.synchronize()
        flops = {"similar_pairs": 1.0 * N * (N - 1) * D, "pairwise": 2.0 * N * N * D, "pairwise_nonzero": 2.0 * N * N * D}
        rec = {"N": N, "D": D, "threshold": T, "planted": n_dup, "pairs": counts["similar_pairs"]}
        if "pairwise_nonzero" in counts:
            rec["pairs_pairwise_nonzero"] = counts["pairwise_nonzero"]
        for name, fn in paths.items():
            ms, reps = timed_ms(torch, fn, a.window_ms)
            flop = flops[name]
            rec[name] = {"ms": round(ms, 4), "reps": reps, "flop": flop, "tflops": round(flop / ms * 1e-9, 2),
                         "peak_frac": round(flop / ms * 1e-9 / PEAK_FP32_MFMA_TFLOPS, 4), "peak_mem_bytes": peak_bytes(torch, fn)}
        if "pairwise" in rec:
            rec["similar_pairs_over_pairwise"] = round(rec["similar_pairs"]["ms"] / rec["pairwise"]["ms"], 3)
            rec["similar_pairs_over_pairwise_nonzero"] = round(rec["similar_pairs"]["ms"] / rec["pairwise_nonzero"]["ms"], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del X
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
