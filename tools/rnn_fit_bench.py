#!/usr/bin/env python3
"""One mini-batch training step of the LSTM and plain-RNN user models: dae_lstm_pair_loss / dae_rnn_pair_loss against torch
autograd, in one process.  The form of tools/gru_fit_bench.py, once per cell.

Batch: --users browsing histories with geometric lengths (mean --mean-len), trimmed to their --max-len most recent events, over
--articles articles of H columns (D = H), N(0, 1) embeddings; --n-neg negatives per click from helpers.sample_negatives; the
weights are torch.nn.LSTM's / torch.nn.RNN's default initialisation (seeded).

  * library: one dae_{cell}_pair_loss call on a schedule prepared beforehand (loss, pair count and the four gradients; forward,
    loss, backward through time and the weight-gradient GEMMs).
  * torch: the same batch through the forward of tools/gru_fit_torch.py --cell (the torch.nn module on the padded batch without
    its last column, the einsum margins, softplus) plus backward(), on the same device.

Per cell and path: ms, events/s, peak device memory; the library's workspace; `library_over_torch`, the ratio of the two times.
Both are warmed up, then timed with HIP events over windows of at least --window-ms.  Nothing is gated on these numbers.

  python tools/rnn_fit_bench.py --out profiles/rnn_fit_bench.txt
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
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--mean-len", type=float, default=50.0)
    ap.add_argument("--max-len", type=int, default=50)
    ap.add_argument("--n-neg", type=int, default=4)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cells", default="lstm,rnn", help="comma-separated: lstm, rnn")
    ap.add_argument("--no-torch", action="store_true", help="time the library alone")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "rnn_fit_bench needs a GPU"
    lib = L.load()
    lines = [json.dumps(device_record(torch))]
    print(lines[0], flush=True)
    M, H, Na, n_neg = a.users, a.H, a.articles, a.n_neg
    rng = np.random.default_rng(a.seed)
    lens = rng.geometric(1.0 / a.mean_len, M).astype(np.int64)
    indptr = np.zeros(M + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    indptr, items = helpers.trim_histories((indptr, rng.integers(0, Na, int(indptr[-1]))), a.max_len)
    lens = np.diff(indptr)
    nnz = int(indptr[-1])
    neg = helpers.sample_negatives(indptr, items, Na, n_neg, a.seed)
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    E = torch.randn((Na, H), device="cuda", generator=g)
    order, active = helpers.gru_schedule(indptr)
    T = int(active.size)
    scal = torch.zeros(2, dtype=torch.float64, device="cuda")
    ip_d, or_d = torch.from_numpy(indptr).cuda(), torch.from_numpy(order).cuda()
    it_d, ng_d = torch.from_numpy(items.astype(np.int32)).cuda(), torch.from_numpy(neg).cuda()
    # the padded batch of tools/gru_fit_torch.py
    it = np.zeros((M, T), np.int64)
    ng = np.full((M, T, n_neg), -1, np.int64)
    for r in range(M):
        s, e = indptr[r], indptr[r + 1]
        it[r, :e - s] = items[s:e]
        ng[r, :e - s] = neg[s:e]
    it_t, ng_t = torch.from_numpy(it).cuda(), torch.from_numpy(ng).cuda()
    for cell in a.cells.split(","):
        cls = {"lstm": helpers.LSTMUserModel, "rnn": helpers.RNNUserModel}[cell]
        torch.manual_seed(a.seed)
        net = {"lstm": torch.nn.LSTM, "rnn": torch.nn.RNN}[cell](H, H, batch_first=True).cuda()
        model = cls.from_torch(net)
        w = [torch.from_numpy(getattr(model, n)).cuda() for n in cls.NAMES]
        grads = [torch.empty_like(x) for x in w]
        ws_bytes = int(getattr(lib, "dae_%s_pair_loss_workspace" % cell)(Na, H, M, nnz, T, n_neg))
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
        wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
        rec = {"cell": cell, "Na": Na, "H": H, "users": M, "nnz": nnz, "mean_len": round(nnz / M, 2), "steps": T, "n_neg": n_neg,
               "scored_events": int(np.maximum(lens - 1, 0).sum()), "workspace_bytes": ws_bytes}

        def library():
            L.call("dae_%s_pair_loss" % cell, L.ptr(E), E.stride(0), Na, H, L.ptr(w[0]), H, L.ptr(w[1]), H, L.ptr(w[2]), L.ptr(w[3]),
                   L.ptr(ip_d), L.ptr(it_d), L.ptr(or_d), M, nnz, T, active.ctypes.data_as(ctypes.c_void_p), L.ptr(ng_d), n_neg,
                   ctypes.c_void_p(scal.data_ptr()), ctypes.c_void_p(scal.data_ptr() + 8), L.ptr(grads[0]), H, L.ptr(grads[1]), H,
                   L.ptr(grads[2]), L.ptr(grads[3]), None, wp, ws_bytes, L.current_stream())
            return scal

        def torch_route():
            net.zero_grad(set_to_none=True)
            states, _ = net(E[it_t[:, :-1]])
            pos, ngn = E[it_t[:, 1:]], ng_t[:, 1:]
            valid = ngn >= 0
            x = (states * pos).sum(-1, keepdim=True) - torch.einsum("uth,utnh->utn", states, E[ngn.clamp(min=0)])
            loss = (torch.nn.functional.softplus(-x) * valid).sum()
            loss.backward()
            return loss.detach()

        paths = {"library": library}
        if not a.no_torch:
            paths["torch"] = torch_route
        res = {name: fn().clone() for name, fn in paths.items()}          # warm-up
        torch.cuda.synchronize()
        host = scal.cpu().numpy()
        rec["loss_per_pair"] = float(host[0]) / max(int(host[1:].view(np.int64)[0]), 1)
        rec["n_pairs"] = int(host[1:].view(np.int64)[0])
        if "torch" in res:
            rec["torch_loss_rel_diff"] = abs(float(res["torch"]) - float(host[0])) / abs(float(host[0]))
            rec["torch_grad_rel_diff"] = {n: float((gr - p.grad).abs().max() / p.grad.abs().max()) for n, gr, p in
                                          zip(cls.NAMES, grads, (net.weight_ih_l0, net.weight_hh_l0, net.bias_ih_l0, net.bias_hh_l0))}
        for name, fn in paths.items():
            ms, reps = timed_ms(torch, fn, a.window_ms)
            rec[name] = {"ms": round(ms, 3), "reps": reps, "events_per_s": round(nnz / ms * 1e3), "peak_mem_bytes": peak_bytes(torch, fn)}
        if "torch" in rec:
            rec["library_over_torch"] = round(rec["library"]["ms"] / rec["torch"]["ms"], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del ws, net
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
