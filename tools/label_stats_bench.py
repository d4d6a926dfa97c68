#!/usr/bin/env python3
"""Label statistics timing: helpers.label_similarity_stats (fused similarity + per-class score histograms, dae_pair_hist, only the
tiles on or below the diagonal) against
  * the matrix route, pairwise_similarity(return_tensor=True) + visualize_pairwise_similarity (dae_pair_stats: copies the lower
    triangle into key arrays and sorts them) -- left out, with the reason, where the matrix and that workspace exceed
    --matrix-limit-gb;
  * similar_pairs with a threshold nothing reaches: the same tiles and K loop with an empty epilogue.

The rows are class centre + noise (20 classes, 5 % of the labels missing).  Every path is warmed up on every shape, then timed
with HIP events over windows of at least --window-ms (the repetition count doubles until a window is long enough).  One JSON line
per shape: ms, achieved TFLOP/s by the triangle's useful FLOPs N (N - 1) D and the share of the fp32 MFMA peak of the MI355X
(157.3 TF/s), the peak device memory each path allocates, the AUROC bracket and its width, and the ratios.  ``pair_hist_abi`` is the
library call alone (no host derivation of the statistics).

  python tools/label_stats_bench.py --out profiles/label_stats_bench.json     # 8000 x 500, 20000 x 500, 64000 x 500
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.near_dup_bench import PEAK_FP32_MFMA_TFLOPS, peak_bytes, timed_ms  # noqa: E402

DEFAULT_SHAPES = "8000x500,20000x500,64000x500"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated N x D")
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--centre", type=float, default=0.15, help="weight of the class centre in a row")
    ap.add_argument("--bins", type=int, default=2048)
    ap.add_argument("--matrix-limit-gb", type=float, default=24.0,
                    help="leave the matrix route out when N x N x 4 bytes + dae_pair_stats_workspace(N) exceed this")
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "label_stats_bench needs a GPU"
    lib = L.load()
    lines = []
    for shape in a.shapes.split(","):
        N, D = (int(v) for v in shape.lower().split("x"))
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        lab = torch.randint(0, a.classes, (N,), device="cuda", generator=g)
        X = a.centre * torch.randn((a.classes, D), device="cuda", generator=g)[lab] + torch.randn((N, D), device="cuda", generator=g)
        lab[torch.rand((N,), device="cuda", generator=g) < 0.05] = -1
        labels = lab.cpu().numpy()
        lab32 = np.ascontiguousarray(labels.astype(np.int32))
        ws_bytes = int(lib.dae_pair_hist_workspace(N, N, D, a.bins))
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
        off = (-ws.data_ptr()) % 256
        hist = np.zeros((2, a.bins), dtype=np.uint64)
        out16 = (ctypes.c_double * 16)()

        def abi_call():
            L.call("dae_pair_hist", L.ptr(X), X.stride(0), N, lab32.ctypes.data_as(ctypes.c_void_p), None, 0, N, None, D, 0, 0, 0.0, 0.0,
                   a.bins, hist.ctypes.data_as(ctypes.c_void_p), ctypes.cast(out16, ctypes.c_void_p), ctypes.c_void_p(ws.data_ptr() + off),
                   ws_bytes, L.current_stream())

        paths = {"label_similarity_stats": lambda: helpers.label_similarity_stats(X, labels, bins=a.bins),
                 "pair_hist_abi": abi_call,
                 "similar_pairs_empty": lambda: helpers.similar_pairs(X, 2.0, return_tensor=True)}
        matrix_bytes = N * N * 4 + int(lib.dae_pair_stats_workspace(N))
        rec = {"N": N, "D": D, "classes": a.classes, "bins": a.bins}
        if matrix_bytes <= a.matrix_limit_gb * 1e9:
            paths["matrix_route"] = lambda: helpers.visualize_pairwise_similarity(labels, helpers.pairwise_similarity(X, return_tensor=True))
        else:
            rec["matrix_route"] = {"left_out": "N x N x 4 bytes + dae_pair_stats_workspace(N) = %.1f GB exceed --matrix-limit-gb %.1f"
                                               % (matrix_bytes / 1e9, a.matrix_limit_gb)}
        res = {name: fn() for name, fn in paths.items()}        # warm-up: library load, kernel attributes, allocator
        torch.cuda.synchronize()
        st = res["label_similarity_stats"]
        assert res["similar_pairs_empty"][0].shape[0] == 0
        rec.update(auroc=st["auroc"], auroc_low=st["auroc_low"], auroc_high=st["auroc_high"],
                   bracket_width=st["auroc_high"] - st["auroc_low"], n_related=st["n_related"], n_unrelated=st["n_unrelated"],
                   workgroups=int(out16[11]), tiles=int(out16[12]))
        if "matrix_route" in res:
            rec["auroc_matrix_route"] = res["matrix_route"]["auroc"]
        del res
        flop = 1.0 * N * (N - 1) * D
        for name, fn in paths.items():
            ms, reps = timed_ms(torch, fn, a.window_ms)
            rec[name] = {"ms": round(ms, 4), "reps": reps, "tflops": round(flop / ms * 1e-9, 2),
                         "peak_frac": round(flop / ms * 1e-9 / PEAK_FP32_MFMA_TFLOPS, 4)}
            if name != "pair_hist_abi":
                rec[name]["peak_mem_bytes"] = peak_bytes(torch, fn)
        rec["pair_hist_workspace_bytes"] = ws_bytes
        rec["stats_over_empty_epilogue"] = round(rec["label_similarity_stats"]["ms"] / rec["similar_pairs_empty"]["ms"], 3)
        rec["abi_over_empty_epilogue"] = round(rec["pair_hist_abi"]["ms"] / rec["similar_pairs_empty"]["ms"], 3)
        if "ms" in rec.get("matrix_route", {}):
            rec["stats_over_matrix_route"] = round(rec["label_similarity_stats"]["ms"] / rec["matrix_route"]["ms"], 4)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del X, ws
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
