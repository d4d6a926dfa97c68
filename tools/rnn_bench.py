#!/usr/bin/env python3
"""LSTM and plain-RNN user-state timing (dae_lstm_user_states, dae_rnn_user_states), all paths in one process.

Users and articles: those of tools/gru_bench.py -- --users browsing histories with geometric lengths (mean --mean-len, capped at
--max-len) over --articles articles of H columns (D = H), N(0, 1) embeddings; the weights are torch.nn.LSTM's / torch.nn.RNN's
default initialisation (seeded).  Per cell:

  * the library call, last states and all states, on a schedule prepared beforehand (helpers.gru_schedule, uploaded once);
  * `torch steps`: the same schedule written with torch -- the input projection of every article once (one addmm), then per step
    one torch.addmm (P[item] + h W_hh^T over the users still active) plus pointwise ops, states updated in place; all states are
    scattered to their event rows.  fp32 (torch's default GEMM precision);
  * `torch module`: torch.nn.LSTM / torch.nn.RNN on padded batches -- the users sorted by length, --module-batch at a time, every
    batch padded to its longest history; the last states are gathered from the padded output, "all" also compacts the padded
    output to one row per event (in the sorted order).  Skipped with --no-module.

Per path: ms, events/s, TFLOP/s counting 2 G H^2 per event plus the projection 2 G Na D H (G = 4 gates for the LSTM, 1 for the
RNN), peak device memory.  `steps < 128`: the share of the schedule's steps with fewer than 128 active users (less than one row
tile); `tail share`: the share of the library call's time spent in them, measured as 1 - (the call truncated to the steps with
at least 128) / (the whole call).

Every path is warmed up, then timed with HIP events over windows of at least --window-ms.  Plain text, one block per cell,
preceded by one line describing the device.  Nothing is gated on these numbers.

  python tools/rnn_bench.py --out profiles/rnn_bench.txt
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
    ap.add_argument("--articles", type=int, default=8000)
    ap.add_argument("--H", type=int, default=500)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--mean-len", type=float, default=50.0)
    ap.add_argument("--max-len", type=int, default=1000)
    ap.add_argument("--cells", default="lstm,rnn")
    ap.add_argument("--module-batch", type=int, default=2048, help="users per padded batch of the torch.nn module route")
    ap.add_argument("--no-module", action="store_true", help="skip torch.nn.LSTM / torch.nn.RNN on padded batches")
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the text to this file")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "rnn_bench needs a GPU"
    lib = L.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                                       # rewritten as it grows: a run that is cut short leaves what it measured
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say(json.dumps(device_record(torch)))
    M, H, Na = a.users, a.H, a.articles
    D = H
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
    say("Na %d  D = H %d  users %d  events %d (mean %.2f, longest %d)  steps %d, of which %d (%.1f %%) have fewer than 128 active users and hold %d events"
        % (Na, H, M, nnz, nnz / M, T, T, T - T128, 100.0 * (T - T128) / max(T, 1), int(active[T128:].sum())))
    # the torch routes' index lists: per step the items and the event rows of the active users (sorted positions 0 .. active[t])
    start = indptr[:-1][order]
    step_events = [torch.from_numpy(start[:int(active[t])] + t).cuda() for t in range(T)]
    step_items = [it_d[ev].long() for ev in step_events]
    inv = torch.from_numpy(np.argsort(order)).cuda()
    ends = torch.from_numpy(indptr[1:] - 1).cuda()
    for cell in a.cells.split(","):
        G = {"lstm": 4, "rnn": 1}[cell]
        cls = helpers.LSTMUserModel if cell == "lstm" else helpers.RNNUserModel
        torch.manual_seed(a.seed)
        module = (torch.nn.LSTM if cell == "lstm" else torch.nn.RNN)(D, H, batch_first=True).cuda()
        model = cls.from_torch(module)
        w_ih, w_hh, b_ih, b_hh = (torch.from_numpy(getattr(model, n)).cuda() for n in cls.NAMES)
        ws_bytes = int(getattr(lib, "dae_%s_user_states_workspace" % cell)(Na, D, H, M))
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
        wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)

        def states(all_states, steps=T):
            U = torch.empty((nnz if all_states else M, H), dtype=torch.float32, device="cuda")
            head = (L.ptr(E), E.stride(0), Na, D, H, L.ptr(w_ih), D, L.ptr(w_hh), H, L.ptr(b_ih), L.ptr(b_hh), L.ptr(ip_d), L.ptr(it_d),
                    L.ptr(or_d), M, nnz, steps, active.ctypes.data_as(ctypes.c_void_p), None, 0)
            if cell == "lstm":
                L.call("dae_lstm_user_states", *head, None, 0, 1 if all_states else 0, L.ptr(U), U.stride(0), None, 0, wp, ws_bytes,
                       L.current_stream())
            else:
                L.call("dae_rnn_user_states", *head, 1 if all_states else 0, L.ptr(U), U.stride(0), wp, ws_bytes, L.current_stream())
            return U

        w_hh_t, w_ih_t, bias = w_hh.t().contiguous(), w_ih.t().contiguous(), b_ih + b_hh

        def torch_steps(all_states):
            P = torch.addmm(bias, E, w_ih_t)                              # [Na x G H]
            S = torch.zeros((M, H), dtype=torch.float32, device="cuda")
            C = torch.zeros((M, H), dtype=torch.float32, device="cuda") if cell == "lstm" else None
            U = torch.empty((nnz, H), dtype=torch.float32, device="cuda") if all_states else None
            for t in range(T):
                n_act = int(active[t])
                h = S[:n_act]
                pre = torch.addmm(P[step_items[t]], h, w_hh_t)
                if cell == "lstm":
                    c = C[:n_act]
                    ifo = torch.sigmoid(pre)
                    c.mul_(ifo[:, H:2 * H]).addcmul_(ifo[:, :H], torch.tanh(pre[:, 2 * H:3 * H]))
                    torch.mul(ifo[:, 3 * H:], torch.tanh(c), out=h)
                else:
                    torch.tanh(pre, out=h)
                if all_states:
                    U[step_events[t]] = h
            return U if all_states else S[inv]

        paths = {"library  last": lambda: states(0), "library  all": lambda: states(1), "library  last, steps >= 128 only": lambda: states(0, T128),
                 "torch steps  last": lambda: torch_steps(False), "torch steps  all": lambda: torch_steps(True)}
        if not a.no_module:
            batches = []
            for b0 in range(0, M, a.module_batch):
                ub = order[b0:b0 + a.module_batch]
                ub = ub[lens[ub] > 0]
                if ub.size:
                    ln = torch.from_numpy(lens[ub]).cuda()
                    Tb = int(lens[ub].max())
                    pos = torch.arange(Tb, device="cuda")[None, :]
                    mask = pos < ln[:, None]
                    idx = torch.zeros((ub.size, Tb), dtype=torch.long, device="cuda")
                    idx[mask] = torch.from_numpy(np.concatenate([items[indptr[u]:indptr[u + 1]] for u in ub]).astype(np.int64)).cuda()
                    batches.append((torch.from_numpy(ub.astype(np.int64)).cuda(), ln, mask, idx))

            def torch_module(all_states):
                last = torch.zeros((M, H), dtype=torch.float32, device="cuda")
                rows = []
                with torch.no_grad():
                    for ub, ln, mask, idx in batches:
                        out = module(E[idx])[0]                            # [batch x Tb x H], the padding computed too
                        last[ub] = out[torch.arange(ub.numel(), device="cuda"), ln - 1]
                        if all_states:
                            rows.append(out[mask])
                return torch.cat(rows) if all_states else last
            paths["torch module  last"] = lambda: torch_module(False)
            paths["torch module  all"] = lambda: torch_module(True)
        res = {name: fn() for name, fn in paths.items()}                 # warm-up
        torch.cuda.synchronize()
        assert torch.equal(res["library  all"][ends], res["library  last"])   # geometric lengths: no empty history
        diffs = {"torch steps": (float((res["library  last"] - res["torch steps  last"]).abs().max()),
                                 float((res["library  all"] - res["torch steps  all"]).abs().max()))}
        if not a.no_module:
            diffs["torch module"] = (float((res["library  last"] - res["torch module  last"]).abs().max()),)
        assert all(v < 1e-3 for d in diffs.values() for v in d), diffs
        del res
        flop_event, flop_proj = 2.0 * G * H * H, 2.0 * G * Na * D * H
        say("")
        say("%s  (dae_%s_user_states; workspace %.1f MB; %.1f GFLOP)" % (cell.upper(), cell, ws_bytes / 1e6, (flop_event * nnz + flop_proj) * 1e-9))
        say("  %-36s %10s %14s %9s %12s" % ("path", "ms", "events/s", "TFLOP/s", "peak MB"))
        ms_of = {}
        for name, fn in paths.items():
            ms, reps = timed_ms(torch, fn, a.window_ms)
            ev = int(active[:T128].sum()) if "only" in name else nnz
            ms_of[name] = ms
            say("  %-36s %10.3f %14d %9.2f %12.1f" % (name, ms, round(ev / ms * 1e3), (flop_event * ev + flop_proj) / ms * 1e-9,
                                                      peak_bytes(torch, fn) / 1e6))
        say("  tail share (time in the steps with fewer than 128 active users): %.4f"
            % (1.0 - ms_of["library  last, steps >= 128 only"] / ms_of["library  last"]))
        say("  library / torch steps: last %.3f, all %.3f" % (ms_of["library  last"] / ms_of["torch steps  last"],
                                                                ms_of["library  all"] / ms_of["torch steps  all"]))
        if not a.no_module:
            say("  library / torch module: last %.3f, all %.3f" % (ms_of["library  last"] / ms_of["torch module  last"],
                                                                     ms_of["library  all"] / ms_of["torch module  all"]))
        say("  max |library - torch|: " + ", ".join("%s %s" % (k, " / ".join("%.2e" % x for x in v)) for k, v in diffs.items()))
        del ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
