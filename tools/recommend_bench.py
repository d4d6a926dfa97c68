#!/usr/bin/env python3
"""User-state and seen-aware recommendation timing, all paths in one process.

Users: --users browsing histories with geometric lengths (mean --mean-len, capped at --max-len) over Na articles of H columns.

  * dae_user_states, last states and all states, against the only library route there is today: torch.sparse.mm of a
    host-built normalised weight CSR [users x Na] (weight of event e = the product of the later decay factors / z; repeated
    articles summed) with E -- last states only; the all-states form has no library counterpart short of materialising
    nnz x H products.  ms, gathered GB/s (nnz * H * 4 bytes per call), peak device memory.  `user_states_sorted` is the same
    call with the users ordered by history length, longest first (what a length-sorted schedule would buy).
  * dae_topk_similarity_ex with the histories as exclusion lists against dae_topk_similarity on the same operands, for each k:
    ms and the ratio.  The library calls are timed on operands prepared beforehand (the exclusion CSR normalised and uploaded
    once); `recommend_helper_s` is one wall-clock call of helpers.recommend, host preparation and copies included.

Every path is warmed up, then timed with HIP events over windows of at least --window-ms (the repetition count doubles until a
window is long enough).  One JSON line per shape, preceded by one line describing the device (name, CUs, clocks).

  python tools/recommend_bench.py --out profiles/recommend_bench.json     # Na 8000 and 64000, H 500, 100 000 users, k 10 and 100
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.near_dup_bench import peak_bytes, timed_ms  # noqa: E402


def device_record(torch):
    p = torch.cuda.get_device_properties(0)
    rec = {"device": p.name, "compute_units": p.multi_processor_count, "total_memory_bytes": p.total_memory}
    for key in ("clock_rate", "memory_clock_rate", "memory_bus_width", "gcnArchName"):
        if hasattr(p, key):
            rec[key] = getattr(p, key)                                    # clocks in kHz
    try:                                                                  # the clocks as the driver reports them right now (read only)
        import subprocess
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        rec["rocm_smi_clocks"] = json.loads(out)
    except Exception as e:                                                # noqa: BLE001
        rec["rocm_smi_clocks"] = "unavailable: %s" % type(e).__name__
    rec["torch"] = torch.__version__
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", default="8000,64000")
    ap.add_argument("--H", type=int, default=500)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--mean-len", type=float, default=50.0)
    ap.add_argument("--max-len", type=int, default=1000)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--beta", type=float, default=0.9)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from scipy import sparse
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "recommend_bench needs a GPU"
    lib = L.load()
    lines = [json.dumps(device_record(torch))]
    print(lines[0], flush=True)
    M, H, beta = a.users, a.H, a.beta
    for Na in (int(v) for v in a.articles.split(",")):
        rng = np.random.default_rng(a.seed)
        lens = np.minimum(rng.geometric(1.0 / a.mean_len, M), a.max_len).astype(np.int64)
        indptr = np.zeros(M + 1, np.int64)
        indptr[1:] = np.cumsum(lens)
        nnz = int(indptr[-1])
        items = rng.integers(0, Na, nnz).astype(np.int32)
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        E = torch.randn((Na, H), device="cuda", generator=g)
        ip_d, it_d = torch.from_numpy(indptr).cuda(), torch.from_numpy(items).cuda()
        order = np.argsort(-lens, kind="stable")                         # users by history length, longest first
        ip_s = np.zeros(M + 1, np.int64)
        ip_s[1:] = np.cumsum(lens[order])
        it_s = np.concatenate([items[indptr[u]:indptr[u + 1]] for u in order])
        ip_sd, it_sd = torch.from_numpy(ip_s).cuda(), torch.from_numpy(it_s).cuda()
        rec = {"Na": Na, "H": H, "users": M, "nnz": nnz, "mean_len": round(nnz / M, 2), "max_len": int(lens.max()), "beta": beta}

        def states(all_states, ip=ip_d, it=it_d):
            U = torch.empty((nnz if all_states else M, H), dtype=torch.float32, device="cuda")
            L.call("dae_user_states", L.ptr(E), E.stride(0), Na, H, L.ptr(ip), L.ptr(it), M, nnz, beta, None, 1 if all_states else 0,
                   L.ptr(U), U.stride(0), L.current_stream())
            return U

        # the SpMM route: weight of event e of a user with n events at position p: beta ** (n - 1 - p) / z_n, z_n = sum of beta ** j
        pos = np.arange(nnz) - np.repeat(indptr[:-1], lens)
        n_of = np.repeat(lens, lens)
        z = np.cumsum(beta ** np.arange(a.max_len + 1, dtype=np.float64))
        w = beta ** (n_of - 1 - pos).astype(np.float64) / z[n_of - 1]
        t0 = time.perf_counter()
        Wc = sparse.csr_matrix((w.astype(np.float32), items, indptr), shape=(M, Na))
        Wc.sum_duplicates()
        rec["spmm_host_build_s"] = round(time.perf_counter() - t0, 3)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                              # torch: "sparse CSR tensor support is in beta state"
            Wt = torch.sparse_csr_tensor(torch.from_numpy(Wc.indptr.astype(np.int64)), torch.from_numpy(Wc.indices.astype(np.int64)),
                                         torch.from_numpy(Wc.data), size=(M, Na)).cuda()
        paths = {"user_states_last": lambda: states(0), "user_states_all": lambda: states(1),
                 "user_states_last_sorted": lambda: states(0, ip_sd, it_sd), "spmm_last": lambda: torch.sparse.mm(Wt, E)}
        res = {name: fn() for name, fn in paths.items()}                 # warm-up
        torch.cuda.synchronize()
        rec["spmm_max_abs_diff"] = float((res["user_states_last"] - res["spmm_last"]).abs().max())
        assert rec["spmm_max_abs_diff"] < 1e-4
        ends = torch.from_numpy(indptr[1:] - 1).cuda()
        assert torch.equal(res["user_states_all"][ends], res["user_states_last"])
        assert torch.equal(res["user_states_last_sorted"], res["user_states_last"][torch.from_numpy(order).cuda()])
        U = res["user_states_last"]
        del res
        for name, fn in paths.items():
            ms, reps = timed_ms(torch, fn, a.window_ms)
            rec[name] = {"ms": round(ms, 4), "reps": reps, "gathered_gbs": round(nnz * H * 4 / ms * 1e-6, 1),
                         "peak_mem_bytes": peak_bytes(torch, fn)}
        rec["user_states_over_spmm"] = round(rec["user_states_last"]["ms"] / rec["spmm_last"]["ms"], 3)
        rec["sorted_over_given_order"] = round(rec["user_states_last_sorted"]["ms"] / rec["user_states_last"]["ms"], 3)
        del Wt

        # ---- ranking: histories as exclusion lists against the plain top-k on the same operands ----
        t0 = time.perf_counter()
        xp, xi = helpers.normalize_exclusions((indptr, items), M, Na)
        rec["normalize_exclusions_host_s"] = round(time.perf_counter() - t0, 3)
        rec["excluded_entries"] = int(xi.size)
        xp_d, xi_d = torch.from_numpy(xp).cuda(), torch.from_numpy(xi).cuda()
        for k in (int(v) for v in a.ks.split(",")):
            ws_bytes = int(lib.dae_topk_similarity_ex_workspace(M, Na, H, k))
            ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
            wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
            idx = torch.empty((M, k), dtype=torch.int32, device="cuda")
            sc = torch.empty((M, k), dtype=torch.float32, device="cuda")

            def plain():
                L.call("dae_topk_similarity", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, k, 0, L.ptr(idx), L.ptr(sc), k,
                       wp, ws_bytes, L.current_stream())

            def seen():
                L.call("dae_topk_similarity_ex", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, k, 0, L.ptr(xp_d),
                       L.ptr(xi_d), L.ptr(idx), L.ptr(sc), k, wp, ws_bytes, L.current_stream())

            plain(); seen()
            torch.cuda.synchronize()
            row = torch.arange(M, device="cuda").repeat_interleave(torch.from_numpy(np.diff(xp)).cuda())
            hit = torch.zeros((M, Na), dtype=torch.bool, device="cuda") if M * Na <= 1 << 33 else None
            if hit is not None:                                           # no seen article in any list
                hit[row, xi_d.long()] = True
                assert not torch.gather(hit, 1, idx.long().clamp(min=0)).any()
                del hit
            r = {}
            for name, fn in (("most_similar_abi", plain), ("recommend_abi", seen)):
                ms, reps = timed_ms(torch, fn, a.window_ms)
                r[name] = {"ms": round(ms, 4), "reps": reps, "tflops": round(2.0 * M * Na * H / ms * 1e-9, 2)}
            r["recommend_over_most_similar"] = round(r["recommend_abi"]["ms"] / r["most_similar_abi"]["ms"], 3)
            r["workspace_bytes"] = ws_bytes
            del ws
            t0 = time.perf_counter()
            helpers.recommend(U, E, k=k, seen=(indptr, items), return_tensor=True)
            torch.cuda.synchronize()
            r["recommend_helper_s"] = round(time.perf_counter() - t0, 3)
            rec["k%d" % k] = r
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del E, U
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
