#!/usr/bin/env python3
"""GRU user-state timing (dae_gru_user_states), all paths in one process.

Users and articles: those of tools/recommend_bench.py -- --users browsing histories with geometric lengths (mean --mean-len,
capped at --max-len) over Na articles of H columns (D = H), N(0, 1) embeddings; the weights are torch.nn.GRU's default
initialisation (seeded), or --weights (a helpers.GRUUserModel .npz, e.g. from tools/gru_fit_torch.py).

  * dae_gru_user_states, last states and all states, on a schedule prepared beforehand (helpers.gru_schedule, uploaded once).
  * the same schedule written with torch: the input projection of every article once (one addmm), then per step one
    torch.addmm (h W_hh^T + b_hh over the users still active) plus pointwise ops, states updated in place; all states are
    scattered to their event rows.  fp32 (torch's default GEMM precision).
  * off by default (--torch-gru): torch.nn.GRU on packed sequences -- MIOpen's first-use kernel search has not been measured.

Per path: ms, events/s, TFLOP/s counting 6 H^2 per event plus the projection 6 Na D H, peak device memory.
`tail_share`: the share of the library call's time spent in the steps with fewer than 128 active users (less than one row
tile), measured as 1 - (the call truncated to the steps with at least 128) / (the whole call).

Every path is warmed up, then timed with HIP events over windows of at least --window-ms.  One JSON line per shape, preceded
by one line describing the device.  Nothing is gated on these numbers.

  python tools/gru_bench.py --out profiles/gru_bench.json
"""
import argparse
import ctypes
import json
import os
import sys

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
    ap.add_argument("--weights", default="", help="helpers.GRUUserModel .npz (default: torch.nn.GRU's initialisation, seeded)")
    ap.add_argument("--torch-gru", action="store_true", help="also time torch.nn.GRU on packed sequences (last states)")
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "gru_bench needs a GPU"
    lib = L.load()
    lines = [json.dumps(device_record(torch))]
    print(lines[0], flush=True)
    M, H = a.users, a.H
    D = H
    if a.weights:
        model = helpers.GRUUserModel.load(a.weights)
        assert (model.input_size, model.hidden_size) == (D, H), "--weights: sizes %d, %d" % (model.input_size, model.hidden_size)
    else:
        torch.manual_seed(a.seed)
        model = helpers.GRUUserModel.from_torch(torch.nn.GRU(D, H))
    w_ih, w_hh, b_ih, b_hh = (torch.from_numpy(getattr(model, n)).cuda() for n in helpers.GRUUserModel.NAMES)
    for Na in (int(v) for v in a.articles.split(",")):
        rng = np.random.default_rng(a.seed)
        lens = np.minimum(rng.geometric(1.0 / a.mean_len, M), a.max_len).astype(np.int64)
        indptr = np.zeros(M + 1, np.int64)
        indptr[1:] = np.cumsum(lens)
        nnz = int(indptr[-1])
        items = rng.integers(0, Na, nnz).astype(np.int32)
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        E = torch.randn((Na, D), device="cuda", generator=g)
        order, active = helpers.gru_schedule(indptr)
        T = int(active.size)
        T128 = int((active >= 128).sum())
        ip_d, it_d, or_d = torch.from_numpy(indptr).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(order).cuda()
        ws_bytes = int(lib.dae_gru_user_states_workspace(Na, D, H, M))
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
        wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
        flops = 6.0 * H * H * nnz + 6.0 * Na * D * H
        rec = {"Na": Na, "D": D, "H": H, "users": M, "nnz": nnz, "mean_len": round(nnz / M, 2), "steps": T, "steps_with_128_active": T128,
               "events_in_steps_below_128": int(active[T128:].sum()), "workspace_bytes": ws_bytes, "gflop": round(flops * 1e-9, 1)}

        def states(all_states, steps=T):
            U = torch.empty((nnz if all_states else M, H), dtype=torch.float32, device="cuda")
            L.call("dae_gru_user_states", L.ptr(E), E.stride(0), Na, D, H, L.ptr(w_ih), D, L.ptr(w_hh), H, L.ptr(b_ih), L.ptr(b_hh),
                   L.ptr(ip_d), L.ptr(it_d), L.ptr(or_d), M, nnz, steps, active.ctypes.data_as(ctypes.c_void_p), None, 0,
                   1 if all_states else 0, L.ptr(U), U.stride(0), wp, ws_bytes, L.current_stream())
            return U

        # the torch route on the same schedule: per step the items and the event rows of the active users (sorted positions 0 .. active[t])
        start = indptr[:-1][order]
        step_events = [torch.from_numpy(start[:int(active[t])] + t).cuda() for t in range(T)]
        step_items = [it_d[ev].long() for ev in step_events]
        inv = torch.from_numpy(np.argsort(order)).cuda()
        w_hh_t, w_ih_t = w_hh.t().contiguous(), w_ih.t().contiguous()

        def torch_route(all_states):
            P = torch.addmm(b_ih, E, w_ih_t)                              # [Na x 3H]
            S = torch.zeros((M, H), dtype=torch.float32, device="cuda")
            U = torch.empty((nnz, H), dtype=torch.float32, device="cuda") if all_states else None
            for t in range(T):
                n_act = int(active[t])
                h = S[:n_act]
                gh = torch.addmm(b_hh, h, w_hh_t)
                gi = P[step_items[t]]
                rz = torch.sigmoid(gi[:, :2 * H] + gh[:, :2 * H])
                n = torch.tanh(torch.addcmul(gi[:, 2 * H:], rz[:, :H], gh[:, 2 * H:]))
                z = rz[:, H:]
                h.copy_(torch.lerp(n, h, z))                              # (1 - z) n + z h
                if all_states:
                    U[step_events[t]] = h
            return U if all_states else S[inv]

        paths = {"gru_last": lambda: states(0), "gru_all": lambda: states(1), "gru_last_128": lambda: states(0, T128),
                 "torch_steps_last": lambda: torch_route(False), "torch_steps_all": lambda: torch_route(True)}
        if a.torch_gru:
            gru = torch.nn.GRU(D, H, batch_first=True).cuda()
            with torch.no_grad():
                for p, v in zip((gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0), (w_ih, w_hh, b_ih, b_hh)):
                    p.copy_(v)
            keep = order[lens[order] > 0]
            seqs = [E[it_d[indptr[u]:indptr[u + 1]].long()] for u in keep]

            def packed():
                with torch.no_grad():
                    return gru(torch.nn.utils.rnn.pack_sequence(seqs, enforce_sorted=True))[1][0]
            paths["torch_gru_packed_last"] = packed
        res = {name: fn() for name, fn in paths.items()}                 # warm-up
        torch.cuda.synchronize()
        ends = torch.from_numpy(indptr[1:] - 1).cuda()
        assert torch.equal(res["gru_all"][ends], res["gru_last"])        # geometric lengths: no empty history
        rec["torch_max_abs_diff_last"] = float((res["gru_last"] - res["torch_steps_last"]).abs().max())
        rec["torch_max_abs_diff_all"] = float((res["gru_all"] - res["torch_steps_all"]).abs().max())
        assert rec["torch_max_abs_diff_last"] < 1e-3 and rec["torch_max_abs_diff_all"] < 1e-3
        del res
        for name, fn in paths.items():
            ms, reps = timed_ms(torch, fn, a.window_ms)
            ev = int(active[:T128].sum()) if name == "gru_last_128" else nnz
            fl = 6.0 * H * H * ev + 6.0 * Na * D * H
            rec[name] = {"ms": round(ms, 3), "reps": reps, "events_per_s": round(ev / ms * 1e3), "tflops": round(fl / ms * 1e-9, 2),
                         "peak_mem_bytes": peak_bytes(torch, fn)}
        rec["tail_share"] = round(1.0 - rec["gru_last_128"]["ms"] / rec["gru_last"]["ms"], 4)
        rec["gru_over_torch_last"] = round(rec["gru_last"]["ms"] / rec["torch_steps_last"]["ms"], 3)
        rec["gru_over_torch_all"] = round(rec["gru_all"]["ms"] / rec["torch_steps_all"]["ms"], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del E, ws, step_events, step_items
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
