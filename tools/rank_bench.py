#!/usr/bin/env python3
"""Full-rank evaluation timing, all routes in one process.

Users: --users browsing histories with geometric lengths (mean --mean-len, capped at --max-len) over Na articles of H columns
(the shapes of tools/recommend_bench.py); user vectors N(0, 1), one random target per user.

  * rank_abi           dae_rank_similarity with the histories as exclusion lists (helpers.recommend_ranks' kernel path)
  * recommend_abi      dae_topk_similarity_ex, k = 10, same lists -- the yardstick: the same GEMM, and an epilogue that does
                       strictly more per candidate that beats the threshold.  rank_over_recommend = rank ms / recommend ms.
  * most_similar_abi   dae_topk_similarity, k = 10, no lists
  * matrix route       where the users x articles block fits: torch matmul in row blocks of --block users, the seen entries
                       set to -inf, compare with the target's score and sum; with its peak device memory.  torch's GEMM
                       rounds differently and the route has no index tie-break, so the share of rows with the kernel's rank
                       is reported, not asserted.

Every path is warmed up, then timed with HIP events over windows of at least --window-ms.  One JSON line per shape, preceded by
one line describing the device.

  python tools/rank_bench.py --out profiles/rank_bench.json     # Na 8000 and 64000, H 500, 100 000 users
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
from tools.recommend_bench import device_record  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", default="8000,64000")
    ap.add_argument("--H", type=int, default=500)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--mean-len", type=float, default=50.0)
    ap.add_argument("--max-len", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--block", type=int, default=8192, help="users per block of the matrix route")
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "rank_bench needs a GPU"
    lib = L.load()
    lines = [json.dumps(device_record(torch))]
    print(lines[0], flush=True)
    M, H, k = a.users, a.H, a.k
    for Na in (int(v) for v in a.articles.split(",")):
        rng = np.random.default_rng(a.seed)
        lens = np.minimum(rng.geometric(1.0 / a.mean_len, M), a.max_len).astype(np.int64)
        indptr = np.zeros(M + 1, np.int64)
        indptr[1:] = np.cumsum(lens)
        items = rng.integers(0, Na, int(indptr[-1])).astype(np.int32)
        targets = rng.integers(0, Na, M).astype(np.int32)
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        E = torch.randn((Na, H), device="cuda", generator=g)
        U = torch.randn((M, H), device="cuda", generator=g)
        xp, xi = helpers.normalize_exclusions((indptr, items), M, Na)
        xp_d, xi_d, t_d = torch.from_numpy(xp).cuda(), torch.from_numpy(xi).cuda(), torch.from_numpy(targets).cuda()
        rec = {"Na": Na, "H": H, "users": M, "excluded_entries": int(xi.size), "k": k}

        ws_bytes = max(int(lib.dae_rank_similarity_workspace(M, Na, H)), int(lib.dae_topk_similarity_ex_workspace(M, Na, H, k)))
        rec["rank_workspace_bytes"] = int(lib.dae_rank_similarity_workspace(M, Na, H))
        rec["topk_workspace_bytes"] = int(lib.dae_topk_similarity_ex_workspace(M, Na, H, k))
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
        wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
        rank = torch.empty(M, dtype=torch.int32, device="cuda")
        tsc = torch.empty(M, dtype=torch.float32, device="cuda")
        idx = torch.empty((M, k), dtype=torch.int32, device="cuda")
        sc = torch.empty((M, k), dtype=torch.float32, device="cuda")

        def ranks():
            L.call("dae_rank_similarity", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, 0, L.ptr(xp_d), L.ptr(xi_d),
                   L.ptr(t_d), L.ptr(rank), L.ptr(tsc), wp, ws_bytes, L.current_stream())

        def ranks_plain():
            L.call("dae_rank_similarity", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, 0, None, None,
                   L.ptr(t_d), L.ptr(rank), L.ptr(tsc), wp, ws_bytes, L.current_stream())

        def seen():
            L.call("dae_topk_similarity_ex", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, k, 0, L.ptr(xp_d),
                   L.ptr(xi_d), L.ptr(idx), L.ptr(sc), k, wp, ws_bytes, L.current_stream())

        def plain():
            L.call("dae_topk_similarity", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, k, 0, L.ptr(idx), L.ptr(sc), k,
                   wp, ws_bytes, L.current_stream())

        row_of = torch.arange(M, device="cuda").repeat_interleave(torch.from_numpy(np.diff(xp)).cuda())
        out_m = torch.empty(M, dtype=torch.int64, device="cuda")
        fits = a.block * Na * 4 * 3 < torch.cuda.get_device_properties(0).total_memory // 2

        def matrix():
            for b0 in range(0, M, a.block):
                b1 = min(M, b0 + a.block)
                S = U[b0:b1] @ E.T
                ts = S.gather(1, t_d[b0:b1].long()[:, None])
                e0, e1 = int(xp[b0]), int(xp[b1])
                S[row_of[e0:e1] - b0, xi_d[e0:e1].long()] = float("-inf")
                out_m[b0:b1] = 1 + (S > ts).sum(dim=1)

        ranks(); seen(); plain(); ranks_plain()
        ranks()
        torch.cuda.synchronize()
        # agreement with the top-k call: a target inside the k-list sits at position rank - 1
        seen()
        torch.cuda.synchronize()
        pos = (idx.long() == t_d.long()[:, None])
        inside = pos.any(dim=1)
        in_list = torch.zeros(M, dtype=torch.bool, device="cuda")           # seen targets: ranked by the kernel, never in the list
        hit = xi_d.long() == t_d.long()[row_of]
        in_list[row_of[hit]] = True
        assert torch.equal(pos.float().argmax(dim=1)[inside] + 1, rank.long()[inside])
        assert torch.equal(inside, (rank <= k) & ~in_list)
        rec["targets_in_top_k"] = int(inside.sum())
        for name, fn in (("rank_abi", ranks), ("rank_abi_no_lists", ranks_plain), ("recommend_abi", seen), ("most_similar_abi", plain)):
            ms, reps = timed_ms(torch, fn, a.window_ms)
            rec[name] = {"ms": round(ms, 4), "reps": reps, "tflops": round(2.0 * M * Na * H / ms * 1e-9, 2)}
        rec["rank_over_recommend"] = round(rec["rank_abi"]["ms"] / rec["recommend_abi"]["ms"], 3)
        rec["rank_over_most_similar"] = round(rec["rank_abi"]["ms"] / rec["most_similar_abi"]["ms"], 3)
        if fits:
            ranks()
            matrix()
            torch.cuda.synchronize()
            rec["matrix_equal_rank_share"] = round(float((out_m == rank.long())[~in_list].float().mean()), 6)
            ms, reps = timed_ms(torch, matrix, a.window_ms)
            rec["matrix_route"] = {"ms": round(ms, 4), "reps": reps, "tflops": round(2.0 * M * Na * H / ms * 1e-9, 2), "block": a.block,
                                   "peak_mem_bytes": peak_bytes(torch, matrix), "full_matrix_bytes": M * Na * 4}
            rec["rank_over_matrix"] = round(rec["rank_abi"]["ms"] / rec["matrix_route"]["ms"], 3)
        t0 = time.perf_counter()
        helpers.recommend_ranks(U, E, targets, seen=(indptr, items), return_tensor=True)
        torch.cuda.synchronize()
        rec["recommend_ranks_helper_s"] = round(time.perf_counter() - t0, 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del E, U, ws
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
