#!/usr/bin/env python3
"""Timing of the training step of the decay user model, all paths in one process.

Users: --users browsing histories with geometric lengths (mean --mean-len, capped at --max-len) over Na articles of H columns,
--n-neg uniform negatives per click (helpers.sample_negatives).

  (a) dae_user_pair_loss: loss, dalpha and dbeta in one walk of the histories (no margins written).
  (b) dae_user_states, last states, at the same shape: it gathers one row per event where (a) gathers 1 + n_neg, so (a) / (b)
      near 1 + n_neg means (a) gathers as efficiently as (b); a clearly larger ratio points at the reductions or the tail.
  (c) at --torch-users users only (the matrix of all states is 2 GB there): the route that existed before --
      helpers.user_states(all_states=True), then torch gathers, products and autograd for the loss and dalpha (no dbeta: that
      route has no second recurrence).  Its loss and dalpha are compared with (a)'s on the same users.

Every path is warmed up, then timed with HIP events over windows of at least --window-ms (the repetition count doubles until a
window is long enough); peak device memory is that of one call.  One JSON line per Na, preceded by one line describing the
device.

  python tools/user_fit_bench.py --out profiles/user_fit_bench.json      # Na 8000 and 64000, H 500, 100 000 users, n_neg 4
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
    ap.add_argument("--torch-users", type=int, default=20000)
    ap.add_argument("--mean-len", type=float, default=50.0)
    ap.add_argument("--max-len", type=int, default=1000)
    ap.add_argument("--n-neg", type=int, default=4)
    ap.add_argument("--beta", type=float, default=0.9)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "user_fit_bench needs a GPU"
    lib = L.load()
    lines = [json.dumps(device_record(torch))]
    print(lines[0], flush=True)
    M, H, beta, n_neg = a.users, a.H, a.beta, a.n_neg
    for Na in (int(v) for v in a.articles.split(",")):
        rng = np.random.default_rng(a.seed)
        lens = np.minimum(rng.geometric(1.0 / a.mean_len, M), a.max_len).astype(np.int64)
        indptr = np.zeros(M + 1, np.int64)
        indptr[1:] = np.cumsum(lens)
        nnz = int(indptr[-1])
        items = rng.integers(0, Na, nnz).astype(np.int32)
        neg = helpers.sample_negatives(indptr, items, Na, n_neg, a.seed)
        g = torch.Generator(device="cuda").manual_seed(a.seed)
        E = torch.randn((Na, H), device="cuda", generator=g)
        alpha = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)
        al_d = torch.from_numpy(alpha).cuda()
        ip_d, it_d, ng_d = torch.from_numpy(indptr).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(neg).cuda()
        rec = {"Na": Na, "H": H, "users": M, "nnz": nnz, "n_neg": n_neg, "mean_len": round(nnz / M, 2), "max_len": int(lens.max()),
               "beta": beta, "valid_pairs": int((neg >= 0).sum())}

        def pair_loss(m=M, n=nnz, ip=ip_d):
            out = torch.empty(H + 3, dtype=torch.float64, device="cuda")
            ws_bytes = int(lib.dae_user_pair_loss_workspace(m, H))
            ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
            base = out.data_ptr()
            L.call("dae_user_pair_loss", L.ptr(E), E.stride(0), Na, H, L.ptr(ip), L.ptr(it_d), m, n, beta, None, None, L.ptr(al_d),
                   L.ptr(ng_d), n_neg, ctypes.c_void_p(base + 8 * H), ctypes.c_void_p(base), ctypes.c_void_p(base + 8 * (H + 1)),
                   ctypes.c_void_p(base + 8 * (H + 2)), None, ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256), ws_bytes,
                   L.current_stream())
            return out, ws

        def last_states():
            U = torch.empty((M, H), dtype=torch.float32, device="cuda")
            L.call("dae_user_states", L.ptr(E), E.stride(0), Na, H, L.ptr(ip_d), L.ptr(it_d), M, nnz, beta, None, 0, L.ptr(U), U.stride(0),
                   L.current_stream())
            return U

        # (c): the first --torch-users users; event e > first is predicted by the all_states row e - 1
        m = min(a.torch_users, M)
        nz = int(indptr[m])
        ip_m = torch.from_numpy(indptr[:m + 1].copy()).cuda()
        first = np.zeros(nz, bool)
        first[indptr[:m][lens[:m] > 0]] = True
        ev = torch.from_numpy(np.flatnonzero(~first)).cuda()
        ok = torch.from_numpy(neg[:nz][~first] >= 0).cuda()
        ng_c = ng_d[:nz][ev].clamp(min=0).long()
        it_l = it_d[:nz][ev].long()

        def torch_route():
            al = al_d.clone().requires_grad_(True)
            U = helpers.user_states((indptr[:m + 1], items[:nz]), E, beta, all_states=True, return_tensor=True)
            au = U[ev - 1] * al
            pos = (au * E[it_l]).sum(1)
            loss = torch.zeros((), dtype=torch.float64, device="cuda")
            for j in range(n_neg):
                x = pos - (au * E[ng_c[:, j]]).sum(1)
                loss = loss + (torch.nn.functional.softplus(-x) * ok[:, j]).double().sum()
            loss.backward()
            return loss.detach(), al.grad

        got = pair_loss()[0].cpu().numpy()
        last_states()
        sub = pair_loss(m, nz, ip_m)[0].cpu().numpy()
        t_loss, t_grad = torch_route()
        torch.cuda.synchronize()
        assert int(got[H + 2:].view(np.int64)[0]) == rec["valid_pairs"]
        rec["torch_users"], rec["torch_nnz"] = m, nz
        rec["loss_rel_diff_vs_torch"] = abs(float(t_loss) - sub[H]) / abs(sub[H])
        rec["dalpha_max_rel_diff_vs_torch"] = float(np.abs(t_grad.cpu().numpy() - sub[:H]).max() / np.abs(sub[:H]).max())
        assert rec["loss_rel_diff_vs_torch"] < 1e-4 and rec["dalpha_max_rel_diff_vs_torch"] < 1e-3
        for name, fn in (("pair_loss", pair_loss), ("user_states_last", last_states), ("pair_loss_torch_users", lambda: pair_loss(m, nz, ip_m)),
                         ("torch_route_torch_users", torch_route)):
            ms, reps = timed_ms(torch, fn, a.window_ms)
            rec[name] = {"ms": round(ms, 4), "reps": reps, "peak_mem_bytes": peak_bytes(torch, fn)}
        rec["pair_loss"]["gathered_gbs"] = round(nnz * (1 + n_neg) * H * 4 / rec["pair_loss"]["ms"] * 1e-6, 1)
        rec["user_states_last"]["gathered_gbs"] = round(nnz * H * 4 / rec["user_states_last"]["ms"] * 1e-6, 1)
        rec["pair_loss_over_user_states"] = round(rec["pair_loss"]["ms"] / rec["user_states_last"]["ms"], 3)
        rec["pair_loss_over_torch_route"] = round(rec["pair_loss_torch_users"]["ms"] / rec["torch_route_torch_users"]["ms"], 4)
        rec["peak_mem_pair_loss_over_torch_route"] = round(rec["pair_loss_torch_users"]["peak_mem_bytes"]
                                                           / rec["torch_route_torch_users"]["peak_mem_bytes"], 6)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del E
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
