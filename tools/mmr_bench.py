#!/usr/bin/env python3
"""Diversification of recommendation lists: what the MMR re-rank costs beside the retrieval it follows and beside de-duplication,
which runs the same gather and the same K loop on the same tile.  All paths in one process, the set-up of tools/dedup_bench.py.

--users user vectors against Na articles of H columns, a share --dup-frac of which are noisy copies of earlier ones, --classes
labels; every user has a history of --hist seen articles.  Timed, on operands prepared beforehand (exclusion CSR normalised and
uploaded once; the pool's relevance rescaled per list to [0, 1] once):

  (b) recommend at k = --pool          dae_topk_similarity_ex
  (c) (b) + dae_dedup_lists            the pool walked down to k, cosine >= --threshold
  (m) (b) + dae_mmr_lists              the pool re-ranked down to k at --lam
  (n) (b) + dae_mmr_lists              with the threshold and --cap articles per label on top
  (d) the host route                   gather [R, L, D] on the device, torch.bmm, copy to the host, the k-step MMR loop in NumPy,
                                       vectorised over the lists (one wall-clock run; (b) not included)

ms per call, the ratios (m) / (b) and mmr / dedup alone -- the comparison that matters: both pay the gather and the whole tile --
workspace / peak device memory.  The library has no stamped-event profile for these entries, so the share of dae_mmr_lists spent
after the K loop is read from the step count instead: the call at k = 1, k = --k and k = --pool runs the same gather and K loop and
1, k and pool selection steps; "selection_ms_per_step" is the slope, "selection_share" its part of the call at k = --k.  The device
paths are warmed up, then timed with HIP events over windows of at least --window-ms.  "rows_equal_host": the share of lists on
which the device and the host route select the same positions (the host route multiplies in another order, so near-ties may fall
either way).  One JSON line per shape, preceded by one line describing the device.

  python tools/mmr_bench.py --out profiles/mmr_bench.txt
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


def host_mmr(S, rel, valid, k, lam):
    """The k-step MMR loop on the host, vectorised over the lists: S [R, L, L] float32 (S[r, q, p]), rel / valid [R, L].  Returns
    the selected positions [R, k], -1 padded."""
    import numpy as np
    R, Ll = rel.shape
    lam = np.float32(lam)
    oml = np.float32(1) - lam
    m = np.zeros((R, Ll), np.float32)
    alive = valid.copy()
    out = np.full((R, k), -1, np.int64)
    rows = np.arange(R)
    lr = lam * rel
    for t in range(k):
        v = np.where(alive, lr - oml * m, -np.inf)
        p = v.argmax(axis=1)                                        # the first of equals
        ok = alive[rows, p]
        out[ok, t] = p[ok]
        alive[rows, p] = False
        m = np.fmax(m, S[rows, p])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", default="8000,64000")
    ap.add_argument("--H", type=int, default=500)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--hist", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--pool", type=int, default=40)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--cap", type=int, default=3)
    ap.add_argument("--classes", type=int, default=30)
    ap.add_argument("--dup-frac", type=float, default=0.25)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "mmr_bench needs a GPU"
    lib = L.load()
    lines = [json.dumps(device_record(torch))]
    print(lines[0], flush=True)
    M, H, k, pool, T, lam = a.users, a.H, a.k, a.pool, a.threshold, a.lam
    inf = float("inf")
    for Na in (int(v) for v in a.articles.split(",")):
        rng = np.random.default_rng(a.seed)
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        n_dup = int(Na * a.dup_frac)
        E = torch.randn((Na, H), device="cuda", generator=g)
        src = torch.randint(0, Na - n_dup, (n_dup,), device="cuda", generator=g)
        E[Na - n_dup:] = E[src] + 0.05 * torch.randn((n_dup, H), device="cuda", generator=g)      # cosine ~ 0.9988
        labels = torch.randint(0, a.classes, (Na,), device="cuda", generator=g, dtype=torch.int32)
        labels[Na - n_dup:] = labels[src]
        items = rng.integers(0, Na, (M, a.hist)).astype(np.int32)
        U = E[torch.from_numpy(items.astype(np.int64)).cuda()].mean(dim=1).contiguous()            # a user likes what it has read
        xp, xi = helpers.normalize_exclusions([row for row in items], M, Na)
        xp_d, xi_d = torch.from_numpy(xp).cuda(), torch.from_numpy(xi).cuda()
        Hp = L.pad(H)
        rec = {"Na": Na, "H": H, "users": M, "k": k, "pool": pool, "lam": lam, "threshold": T, "cap": a.cap, "dup_frac": a.dup_frac,
               "sweep_macs": M * Na * H, "tile_macs": M * 128 * 128 * Hp, "gather_bytes": 2 * M * 128 * Hp * 4}

        ws_bytes = int(lib.dae_topk_similarity_ex_workspace(M, Na, H, pool))
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
        wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
        idx_b = torch.empty((M, pool), dtype=torch.int32, device="cuda")
        sc_b = torch.empty((M, pool), dtype=torch.float32, device="cuda")

        def run_b():
            L.call("dae_topk_similarity_ex", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, pool, 0, L.ptr(xp_d), L.ptr(xi_d),
                   L.ptr(idx_b), L.ptr(sc_b), pool, wp, ws_bytes, L.current_stream())

        run_b()
        torch.cuda.synchronize()
        lo, hi = sc_b.amin(dim=1, keepdim=True), sc_b.amax(dim=1, keepdim=True)
        rel = ((sc_b - lo) / (hi - lo).clamp(min=1e-30)).contiguous()                              # the pool is full: every entry valid
        lws_bytes = int(lib.dae_mmr_lists_workspace(M, Na, H, pool))
        assert lws_bytes == int(lib.dae_dedup_lists_workspace(M, Na, H, pool))
        lws = torch.empty(lws_bytes + 256, dtype=torch.uint8, device="cuda")
        lwp = ctypes.c_void_p(lws.data_ptr() + (-lws.data_ptr()) % 256)
        oi = torch.empty((M, pool), dtype=torch.int32, device="cuda")
        op = torch.empty((M, pool), dtype=torch.int32, device="cuda")
        ov = torch.empty((M, pool), dtype=torch.float32, device="cuda")
        on = torch.empty((M, pool), dtype=torch.float32, device="cuda")
        cnt = torch.empty((M, 2), dtype=torch.int32, device="cuda")
        rec["topk_pool_workspace_bytes"], rec["list_workspace_bytes"] = ws_bytes, lws_bytes

        def run_dedup():
            L.call("dae_dedup_lists", L.ptr(E), E.stride(0), Na, H, 0, 0, L.ptr(idx_b), idx_b.stride(0), M, pool, k, T, L.ptr(oi), L.ptr(op),
                   pool, L.ptr(cnt), lwp, lws_bytes, L.current_stream())

        def mmr(kk, cap=0, thr=inf):
            def run():
                L.call("dae_mmr_lists", L.ptr(E), E.stride(0), Na, H, 0, 0, L.ptr(idx_b), idx_b.stride(0), L.ptr(rel), rel.stride(0),
                       L.ptr(labels), cap, M, pool, kk, lam, thr, L.ptr(oi), L.ptr(op), L.ptr(ov), L.ptr(on), pool, L.ptr(cnt), lwp,
                       lws_bytes, L.current_stream())
            return run

        run_mmr, run_mmr_side = mmr(k), mmr(k, a.cap, T)

        def run_c():
            run_b(); run_dedup()

        def run_m():
            run_b(); run_mmr()

        def run_n():
            run_b(); run_mmr_side()

        run_c(); run_n(); run_m()
        torch.cuda.synchronize()
        pos_d = op[:, :k].cpu().numpy().astype(np.int64)
        rec["beyond_topk_per_list"] = round(float(cnt[:, 1].float().mean()), 4)
        rec["mean_nearest"] = round(float(on[:, 1:k].mean()), 4)

        # (d) the host route, once, wall clock; in chunks of users so that [R, L, D] stays at 1 GiB
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        En = torch.nn.functional.normalize(E, dim=1)
        step = max(1, (1 << 30) // (pool * H * 4))
        pos_h = np.empty((M, k), np.int64)
        t_loop = 0.0
        for r0 in range(0, M, step):
            li = idx_b[r0:r0 + step].long()
            G = En[li.clamp(min=0)]
            S = torch.bmm(G, G.transpose(1, 2)).cpu().numpy()
            t1 = time.perf_counter()
            pos_h[r0:r0 + step] = host_mmr(S, rel[r0:r0 + step].cpu().numpy(), (li >= 0).cpu().numpy(), k, lam)
            t_loop += time.perf_counter() - t1
        rec["host_route"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "mmr_loop_ms": round(t_loop * 1e3, 1),
                             "peak_mem_bytes": int(torch.cuda.max_memory_allocated() - base)}
        rec["rows_equal_host"] = round(float((pos_d == pos_h).all(axis=1).mean()), 4)
        del En, G, S

        for name, fn in (("b_recommend_pool", run_b), ("c_recommend_pool_dedup", run_c), ("m_recommend_pool_mmr", run_m),
                         ("n_recommend_pool_mmr_threshold_cap", run_n), ("dedup_alone", run_dedup), ("mmr_alone", run_mmr),
                         ("mmr_threshold_cap_alone", run_mmr_side), ("mmr_alone_k1", mmr(1)), ("mmr_alone_kpool", mmr(pool))):
            ms, reps = timed_ms(torch, fn, a.window_ms)
            rec[name] = {"ms": round(ms, 4), "reps": reps}
        rec["m_over_b"] = round(rec["m_recommend_pool_mmr"]["ms"] / rec["b_recommend_pool"]["ms"], 4)
        rec["c_over_b"] = round(rec["c_recommend_pool_dedup"]["ms"] / rec["b_recommend_pool"]["ms"], 4)
        rec["mmr_over_dedup"] = round(rec["mmr_alone"]["ms"] / rec["dedup_alone"]["ms"], 4)
        per_step = (rec["mmr_alone_kpool"]["ms"] - rec["mmr_alone_k1"]["ms"]) / max(pool - 1, 1)
        rec["selection_ms_per_step"] = round(per_step, 5)
        rec["selection_share"] = round(per_step * k / rec["mmr_alone"]["ms"], 4)
        rec["mmr_tflops"] = round(2.0 * rec["tile_macs"] / rec["mmr_alone"]["ms"] * 1e-9, 2)
        t0 = time.perf_counter()
        helpers.recommend_diverse(U, E, k=k, seen=(xp, xi), lam=lam, pool=pool, return_tensor=True)
        torch.cuda.synchronize()
        rec["recommend_diverse_helper_s"] = round(time.perf_counter() - t0, 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del E, U, ws, lws
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
