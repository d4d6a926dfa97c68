#!/usr/bin/env python3
"""Sparse operands of top-k and label statistics: the densified one-shot route (helpers.most_similar / label_similarity_stats with
chunk_rows=None: the scipy matrix goes up as CSR, is densified on the device and copied into padded operand images) against the
chunked CSR route (chunk_rows=N: the CSR stays CSR, dae_sweep_image_csr builds one chunk's image at a time, dae_topk_images /
dae_pair_hist_images sweep pairs of chunks).

One JSON line per shape and route: wall milliseconds per call (host timer around a synchronised call, best of --repeats after one
warm-up: the chunked route has host work between its launches, which device events alone would not see), the peak device memory
the call allocates (torch.cuda.max_memory_allocated above what was allocated before it) and the bytes uploaded (CSR arrays; the
densified route uploads the same CSR, with int64 column ids).  The one-shot route is skipped, and says so, where an operand image
would reach 4 GiB.  One more line per shape times the two image kernels on one chunk.  Every chunked result is compared with the one-shot result (array_equal).

  python tools/sparse_sweep_bench.py                          # 8000 x 10000, 20000 x 50000 and 24000 x 50000 (past the 4 GiB image) at 1 %, k = 10
  python tools/sparse_sweep_bench.py --shapes 4096x20000 --chunks 256,1024,auto
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_SHAPES = "8000x10000,20000x50000,24000x50000"


def measure(torch, fn, repeats):
    fn()                                                   # warm-up: library load, kernel attributes, allocator
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    best, out = None, None
    for _ in range(repeats):
        out = None
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return round(best, 3), int(torch.cuda.max_memory_allocated() - base), out


def image_line(torch, L, helpers, m, rows):
    """One JSON line: the image of the first `rows` rows by csr_row_normalize_kernel and, from the densified rows, by
    row_normalize_kernel (cosine, no norm; HIP events around 5 launches each), and the bytes of the image they write."""
    lib = L.load()
    F = m.shape[1]
    op = helpers.SweepOperand(torch, m[:rows], torch.device("cuda"))
    X = torch.from_numpy(m[:rows].toarray()).cuda()
    nb = int(lib.dae_sweep_image_bytes(rows, F))
    img = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ip, ix, vl = op.csr

    def timed(fn, reps=5):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return round(e0.elapsed_time(e1) / reps, 4)
    csr_ms = timed(lambda: L.call("dae_sweep_image_csr", L.ptr(ip), L.ptr(ix), L.ptr(vl), rows, F, 0, 0, L.ptr(img), nb, L.current_stream()))
    dense_ms = timed(lambda: L.call("dae_sweep_image_dense", L.ptr(X), X.stride(0), rows, F, 0, 0, L.ptr(img), nb, L.current_stream()))
    print(json.dumps({"job": "image", "rows": rows, "F": F, "nnz": int(m[:rows].nnz), "image_bytes": nb, "csr_kernel_ms": csr_ms,
                      "csr_kernel_write_GBps": round(nb / csr_ms * 1e-6, 1), "dense_kernel_ms": dense_ms,
                      "dense_kernel_read_write_GBps": round((nb + X.numel() * 4) / dense_ms * 1e-6, 1)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated N x F (rows x vocabulary)")
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunks", default="1024,4096,auto", help="comma-separated chunk_rows values")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--labels", type=int, default=20, help="label classes of the label-statistics runs (0: top-k only)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from scipy import sparse
    from dae_rnn_news_recommendation_amd import _lib as L, helpers
    assert torch.cuda.is_available(), "sparse_sweep_bench needs a GPU"
    chunks = [c if c == "auto" else int(c) for c in a.chunks.split(",")]
    for shape in a.shapes.split(","):
        N, F = (int(v) for v in shape.lower().split("x"))
        m = sparse.random(N, F, density=a.density, random_state=np.random.RandomState(a.seed), format="csr", dtype=np.float32)
        lab = np.random.default_rng(a.seed).integers(0, max(a.labels, 1), N)
        csr_bytes = m.indptr.size * 8 + m.nnz * 8
        fits = L.pad(N) * L.pad(F) * 4 < 1 << 32
        image_line(torch, L, helpers, m, min(N, 4096))
        jobs = [("top_k", lambda c: helpers.most_similar(m, k=a.k, chunk_rows=c, return_tensor=True))]
        if a.labels > 0:
            jobs.append(("label_stats", lambda c: helpers.label_similarity_stats(m, lab, chunk_rows=c, return_histograms=True)))
        for job, fn in jobs:
            base = {"job": job, "N": N, "F": F, "nnz": int(m.nnz), "k": a.k if job == "top_k" else None}
            ref, ref_ms = None, None
            if fits:
                ref_ms, peak, ref = measure(torch, lambda: fn(None), a.repeats)
                print(json.dumps(dict(base, route="densified", chunk_rows=None, ms=ref_ms, peak_mem_bytes=peak,
                                      uploaded_bytes=csr_bytes + m.nnz * 4)), flush=True)
            else:
                print(json.dumps(dict(base, route="densified", chunk_rows=None, skipped="an operand image would reach 4 GiB")), flush=True)
            for c in chunks:
                ms, peak, out = measure(torch, lambda: fn(c), a.repeats)
                rec = dict(base, route="chunked_csr", chunk_rows=c, chunk_rows_used=helpers.sweep_chunk_rows(c, F), ms=ms,
                           peak_mem_bytes=peak, uploaded_bytes=csr_bytes)
                if ref is not None:
                    if job == "top_k":
                        rec["equals_densified"] = bool(torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]))
                    else:
                        rec["equals_densified"] = bool(np.array_equal(out["hist_related"], ref["hist_related"])
                                                       and np.array_equal(out["hist_unrelated"], ref["hist_unrelated"]))
                    rec["ms_over_densified"] = round(ms / ref_ms, 3)
                print(json.dumps(rec), flush=True)
                del out
            del ref
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
