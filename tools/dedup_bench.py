#!/usr/bin/env python3
"""De-duplication of recommendation lists: what the last stage costs beside the retrieval it follows, all paths in one process.

--users user vectors against Na articles of H columns, a share --dup-frac of which are noisy copies of earlier ones; every user
has a history of --hist seen articles.  Timed, on operands prepared beforehand (exclusion CSR normalised and uploaded once):

  (a) recommend at k = --k            dae_topk_similarity_ex
  (b) recommend at k = --pool         dae_topk_similarity_ex
  (c) (b) + dae_dedup_lists           the pool walked down to k, cosine >= --threshold
  (d) the host route                  gather [R, L, D] on the device, torch.bmm, threshold, copy to the host, greedy loop in NumPy
                                      (one wall-clock run; (b) not included)

ms per call, the ratio (c) / (b), the share of the de-dup call in (c), the MACs of both (users x Na x H against users x 128^2 x
pad128(H)) and the bytes the gather moves, workspace / peak device memory.  The device paths are warmed up, then timed with HIP
events over windows of at least --window-ms.  The de-dup result is checked against the host route first (rows whose decisions
both routes take alike: the host route multiplies in another order, so a score within 1e-5 of the threshold may fall either way).
One JSON line per shape, preceded by one line describing the device.

  python tools/dedup_bench.py --out profiles/dedup_bench.txt
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

from tools.near_dup_bench import timed_ms  # noqa: E402
from tools.recommend_bench import device_record  # noqa: E402


def host_greedy(dup, valid, k):
    """The greedy walk on the host: dup [R, L, L] bool (dup[r, p, q]: the pair reaches the threshold), valid [R, L].  Returns the
    kept positions [R, k], -1 padded."""
    import numpy as np
    R, Ll = valid.shape
    out = np.full((R, k), -1, np.int64)
    for r in range(R):
        kept = []
        d, v = dup[r], valid[r]
        for p in range(Ll):
            if v[p] and not d[p, kept].any():
                kept.append(p)
                if len(kept) == k:
                    break
        out[r, :len(kept)] = kept
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", default="8000,64000")
    ap.add_argument("--H", type=int, default=500)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--hist", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--pool", type=int, default=40)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--dup-frac", type=float, default=0.25)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "dedup_bench needs a GPU"
    lib = L.load()
    lines = [json.dumps(device_record(torch))]
    print(lines[0], flush=True)
    M, H, k, pool, T = a.users, a.H, a.k, a.pool, a.threshold
    for Na in (int(v) for v in a.articles.split(",")):
        rng = np.random.default_rng(a.seed)
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        n_dup = int(Na * a.dup_frac)
        E = torch.randn((Na, H), device="cuda", generator=g)
        src = torch.randint(0, Na - n_dup, (n_dup,), device="cuda", generator=g)
        E[Na - n_dup:] = E[src] + 0.05 * torch.randn((n_dup, H), device="cuda", generator=g)      # cosine ~ 0.9988
        items = rng.integers(0, Na, (M, a.hist)).astype(np.int32)
        U = E[torch.from_numpy(items.astype(np.int64)).cuda()].mean(dim=1).contiguous()            # a user likes what it has read
        xp, xi = helpers.normalize_exclusions([row for row in items], M, Na)
        xp_d, xi_d = torch.from_numpy(xp).cuda(), torch.from_numpy(xi).cuda()
        Hp = L.pad(H)
        rec = {"Na": Na, "H": H, "users": M, "k": k, "pool": pool, "threshold": T, "dup_frac": a.dup_frac,
               "sweep_macs": M * Na * H, "dedup_macs": M * 128 * 128 * Hp, "dedup_gather_bytes": 2 * M * 128 * Hp * 4}

        def topk(kk):
            ws_bytes = int(lib.dae_topk_similarity_ex_workspace(M, Na, H, kk))
            ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
            wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
            idx = torch.empty((M, kk), dtype=torch.int32, device="cuda")
            sc = torch.empty((M, kk), dtype=torch.float32, device="cuda")

            def run():
                L.call("dae_topk_similarity_ex", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, kk, 0, L.ptr(xp_d), L.ptr(xi_d),
                       L.ptr(idx), L.ptr(sc), kk, wp, ws_bytes, L.current_stream())
            return run, idx, sc, ws, ws_bytes

        run_a, _, _, ws_a, rec["topk_k_workspace_bytes"] = topk(k)
        run_b, idx_b, sc_b, ws_b, rec["topk_pool_workspace_bytes"] = topk(pool)
        dws_bytes = int(lib.dae_dedup_lists_workspace(M, Na, H, pool))
        dws = torch.empty(dws_bytes + 256, dtype=torch.uint8, device="cuda")
        dwp = ctypes.c_void_p(dws.data_ptr() + (-dws.data_ptr()) % 256)
        oi = torch.empty((M, k), dtype=torch.int32, device="cuda")
        op = torch.empty((M, k), dtype=torch.int32, device="cuda")
        cnt = torch.empty((M, 2), dtype=torch.int32, device="cuda")
        rec["dedup_workspace_bytes"] = dws_bytes

        def run_dedup():
            L.call("dae_dedup_lists", L.ptr(E), E.stride(0), Na, H, 0, 0, L.ptr(idx_b), idx_b.stride(0), M, pool, k, T, L.ptr(oi), L.ptr(op), k,
                   L.ptr(cnt), dwp, dws_bytes, L.current_stream())

        def run_c():
            run_b()
            run_dedup()

        run_a(); run_c()
        torch.cuda.synchronize()
        rec["dup_pairs_in_top_k"] = round(float(cnt[:, 1].float().mean()), 4)
        rec["kept_per_list"] = round(float(cnt[:, 0].float().mean()), 4)

        # (d) the host route, once, wall clock; in chunks of users so that [R, L, D] stays at 1 GiB
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        En = torch.nn.functional.normalize(E, dim=1)
        step = max(1, (1 << 30) // (pool * H * 4))
        pos_h = np.empty((M, k), np.int64)
        near = np.zeros(M, bool)
        t_loop = 0.0
        for r0 in range(0, M, step):
            li = idx_b[r0:r0 + step].long()
            G = En[li.clamp(min=0)]
            S = torch.bmm(G, G.transpose(1, 2))
            dup = (S >= T).cpu().numpy()
            near[r0:r0 + step] = (((S - T).abs() <= 1e-5).tril(-1).any(dim=2).any(dim=1)).cpu().numpy()
            t1 = time.perf_counter()
            pos_h[r0:r0 + step] = host_greedy(dup, (li >= 0).cpu().numpy(), k)
            t_loop += time.perf_counter() - t1
        rec["host_route"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "greedy_loop_ms": round(t_loop * 1e3, 1),
                             "peak_mem_bytes": int(torch.cuda.max_memory_allocated() - base)}
        same = (op.cpu().numpy().astype(np.int64) == pos_h).all(axis=1)
        rec["rows_near_threshold"] = int(near.sum())
        assert same[~near].all(), "the device and the host route disagree on a row without a score near the threshold"
        del En, G, S

        for name, fn in (("a_recommend_k", run_a), ("b_recommend_pool", run_b), ("c_recommend_pool_dedup", run_c), ("dedup_alone", run_dedup)):
            ms, reps = timed_ms(torch, fn, a.window_ms)
            rec[name] = {"ms": round(ms, 4), "reps": reps}
        rec["c_over_b"] = round(rec["c_recommend_pool_dedup"]["ms"] / rec["b_recommend_pool"]["ms"], 4)
        rec["dedup_share_of_c"] = round(rec["dedup_alone"]["ms"] / rec["c_recommend_pool_dedup"]["ms"], 4)
        rec["dedup_tflops"] = round(2.0 * rec["dedup_macs"] / rec["dedup_alone"]["ms"] * 1e-9, 2)
        rec["dedup_gather_gbs"] = round(rec["dedup_gather_bytes"] / rec["dedup_alone"]["ms"] * 1e-6, 1)
        t0 = time.perf_counter()
        helpers.recommend(U, E, k=k, seen=(xp, xi), dedup_threshold=T, dedup_pool=pool, return_tensor=True)
        torch.cuda.synchronize()
        rec["recommend_dedup_helper_s"] = round(time.perf_counter() - t0, 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del E, U, ws_a, ws_b, dws
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
