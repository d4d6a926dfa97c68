#!/usr/bin/env python3
"""The implicit-feedback ALS trainer at the log size of covisit_bench, against the same conjugate gradient written in torch ops.

  interactions  dae_als_interactions: the click log to both orientations of the count matrix.
  gram          dae_als_gram of the article and of the user factors.
  half-sweep    dae_als_solve_rows, users then articles, against the torch route on the same device: the entries' factor rows by
                a gather, their dot products row-wise, the scaled rows summed per row by index_add_, G by one matmul.  Both start
                from the same factors; the results are compared.
  loss          dae_als_loss.
  iteration     Gram, user half-sweep, Gram, article half-sweep -- what fit_als runs per iteration.

The log is that of covisit_bench (seeded: geometric history lengths, Zipf articles).  Buffers and workspaces are allocated
beforehand; a timing is a host clock around one call ending in a synchronise, the median and the minimum over --rounds after a
warm-up call.  No pass mark: the figures are what they are.

  python tools/als_bench.py                                      # 100000 articles, 1000000 users, mean length 12, F = 64
  python tools/als_bench.py --articles 20000 --users 100000 --factors 128
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.covisit_bench import timed, zipf_log  # noqa: E402
from tools.recommend_bench import device_record  # noqa: E402


def torch_half_sweep(torch, ptr, idx, cnt, Y, X, G, alpha, steps):
    """The half-sweep of dae_als_solve_rows by tensor ops, all rows at once; X is updated in place."""
    R = ptr.numel() - 1
    n = ptr[1:] - ptr[:-1]
    rows = torch.repeat_interleave(torch.arange(R, device=Y.device), n)
    a = alpha * cnt.float()
    idx = idx.long()

    def apply(V):
        Ye = Y[idx]
        d = (Ye * V[rows]).sum(dim=1)
        out = V @ G
        out.index_add_(0, rows, Ye * (a * d)[:, None])
        return out

    b = torch.zeros_like(X).index_add_(0, rows, Y[idx] * (1.0 + a)[:, None])
    r = b - apply(X)
    p = r.clone()
    rs = (r * r).sum(dim=1)
    live = rs > 1e-20
    for _ in range(steps):
        Ap = apply(p)
        pAp = (p * Ap).sum(dim=1)
        live = live & (rs > 1e-20) & (pAp > 0)
        step = torch.where(live, rs / pAp, torch.zeros_like(rs))
        X += step[:, None] * p
        r -= step[:, None] * Ap
        rsn = (r * r).sum(dim=1)
        p = r + torch.where(live, rsn / rs, torch.zeros_like(rs))[:, None] * p
        rs = rsn
    X[n == 0] = 0
    return X


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", type=int, default=100000)
    ap.add_argument("--users", type=int, default=1000000)
    ap.add_argument("--mean-len", type=float, default=12.0)
    ap.add_argument("--factors", type=int, default=64)
    ap.add_argument("--cg-steps", type=int, default=3)
    ap.add_argument("--alpha", type=float, default=40.0)
    ap.add_argument("--reg", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch route")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd.helpers._device import workspace
    assert torch.cuda.is_available(), "als_bench needs a GPU"
    lib, dev = L.load(), torch.device("cuda")
    print(json.dumps(device_record(torch)), flush=True)
    Na, M, F, steps = a.articles, a.users, a.factors, a.cg_steps
    lam, alpha = float(np.float32(a.reg)), float(np.float32(a.alpha))
    indptr, items = zipf_log(np, M, Na, a.mean_len, a.seed)
    nnz = int(items.size)
    d_ptr, d_items = torch.from_numpy(indptr).to(dev), torch.from_numpy(items).to(dev)
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    user = (torch.empty(M + 1, **i64), torch.empty(nnz, **i32), torch.empty(nnz, **i32))
    item = (torch.empty(Na + 1, **i64), torch.empty(nnz, **i32), torch.empty(nnz, **i32))
    totals = torch.empty(2, **i64)
    stream = L.current_stream()
    ws_bytes = int(lib.dae_als_interactions_workspace(nnz, M, Na))
    ws_p, ws = workspace(dev, ws_bytes)

    def interactions():
        L.call("dae_als_interactions", L.ptr(d_ptr), L.ptr(d_items), M, nnz, Na, L.ptr(user[0]), L.ptr(user[1]), L.ptr(user[2]), L.ptr(item[0]),
               L.ptr(item[1]), L.ptr(item[2]), nnz, L.ptr(totals), ws_p, ws_bytes, stream)

    t_inter = timed(torch, interactions, a.rounds)
    del ws
    events, pairs = (int(v) for v in totals.cpu().numpy())
    user = (user[0], user[1][:pairs], user[2][:pairs])
    item = (item[0], item[1][:pairs], item[2][:pairs])
    u_len, i_len = (user[0][1:] - user[0][:-1]).cpu().numpy(), (item[0][1:] - item[0][:-1]).cpu().numpy()
    rng = np.random.default_rng(a.seed)
    Y0 = torch.from_numpy((0.01 * rng.standard_normal((Na, F))).astype(np.float32)).to(dev)
    X, Y = torch.zeros((M, F), dtype=torch.float32, device=dev), Y0.clone()
    G = torch.empty((F, F), dtype=torch.float32, device=dev)
    g_bytes = int(lib.dae_als_gram_workspace(max(M, Na), F))
    g_p, g_ws = workspace(dev, g_bytes)
    s_bytes = int(lib.dae_als_solve_rows_workspace(max(M, Na)))
    s_p, s_ws = workspace(dev, s_bytes)
    l_bytes = int(lib.dae_als_loss_workspace(M, Na, F))
    l_p, l_ws = workspace(dev, l_bytes)
    loss = torch.empty(1, dtype=torch.float64, device=dev)

    def gram(Z):
        L.call("dae_als_gram", L.ptr(Z), Z.stride(0), Z.shape[0], F, lam, L.ptr(G), g_p, g_bytes, stream)

    def solve(csr, fixed, out):
        L.call("dae_als_solve_rows", L.ptr(csr[0]), L.ptr(csr[1]), L.ptr(csr[2]), out.shape[0], L.ptr(fixed), fixed.stride(0), fixed.shape[0], F,
               L.ptr(G), alpha, steps, L.ptr(out), out.stride(0), s_p, s_bytes, stream)

    def the_loss():
        L.call("dae_als_loss", L.ptr(user[0]), L.ptr(user[1]), L.ptr(user[2]), M, L.ptr(X), X.stride(0), L.ptr(Y), Y.stride(0), Na, F, alpha,
               lam, L.ptr(loss), l_p, l_bytes, stream)

    def iteration():
        gram(Y)
        solve(user, Y, X)
        gram(X)
        solve(item, X, Y)

    # the first iteration, step by step, each call timed from the same inputs (a half-sweep moves its factors: restore them)
    t_gram_y = timed(torch, lambda: gram(Y), a.rounds)
    X_start = X.clone()

    def user_sweep():
        X.copy_(X_start)
        solve(user, Y, X)

    t_user = timed(torch, user_sweep, a.rounds)
    t_copy_x = timed(torch, lambda: X.copy_(X_start), a.rounds)
    user_sweep()                                                          # (the restore alone left the start in X)
    G_y = G.clone()
    t_gram_x = timed(torch, lambda: gram(X), a.rounds)
    Y_start = Y.clone()

    def item_sweep():
        Y.copy_(Y_start)
        solve(item, X, Y)

    t_item = timed(torch, item_sweep, a.rounds)
    t_copy_y = timed(torch, lambda: Y.copy_(Y_start), a.rounds)
    item_sweep()
    G_x = G.clone()
    t_loss = timed(torch, the_loss, a.rounds)
    loss_1 = float(loss.cpu().numpy()[0])
    X_1, Y_1 = X.clone(), Y.clone()
    t_iter = timed(torch, iteration, a.rounds)                            # iterations 2 .. rounds + 2: warm starts
    the_loss()
    out = {"articles": Na, "users": M, "clicks": nnz, "events": events, "pairs": pairs, "factors": F, "cg_steps": steps, "alpha": alpha,
           "regularization": lam,
           "user_row": {"median": float(np.median(u_len)), "max": int(u_len.max()), "over_256": int((u_len > 256).sum())},
           "article_row": {"median": float(np.median(i_len)), "p99": float(np.percentile(i_len, 99)), "max": int(i_len.max()),
                           "over_256": int((i_len > 256).sum())},
           "interactions_ms": t_inter, "interactions_workspace_bytes": ws_bytes, "gram_articles_ms": t_gram_y, "gram_users_ms": t_gram_x,
           "user_half_sweep_ms_with_restore": t_user, "restore_users_ms": t_copy_x, "article_half_sweep_ms_with_restore": t_item,
           "restore_articles_ms": t_copy_y, "loss_ms": t_loss, "iteration_ms": t_iter, "loss_after_first_iteration": loss_1,
           "loss_after_%d_iterations" % (a.rounds + 2): float(loss.cpu().numpy()[0])}
    out["user_half_sweep_ms"] = round(t_user["median"] - t_copy_x["median"], 3)
    out["article_half_sweep_ms"] = round(t_item["median"] - t_copy_y["median"], 3)
    print(json.dumps(out), flush=True)
    if a.no_torch:
        return
    # the torch route from the same inputs
    Xt = X_start.clone()
    t_torch_user = timed(torch, lambda: torch_half_sweep(torch, *user, Y_start, Xt.copy_(X_start), G_y, alpha, steps), max(1, a.rounds // 2))
    diff_user = float((Xt - X_1).abs().max() / X_1.abs().max())
    Yt = Y_start.clone()
    t_torch_item = timed(torch, lambda: torch_half_sweep(torch, *item, X_1, Yt.copy_(Y_start), G_x, alpha, steps), max(1, a.rounds // 2))
    diff_item = float((Yt - Y_1).abs().max() / Y_1.abs().max())
    print(json.dumps({"torch_user_half_sweep_ms": t_torch_user, "torch_article_half_sweep_ms": t_torch_item,
                      "user_speedup_over_torch": round(t_torch_user["median"] / out["user_half_sweep_ms"], 2),
                      "article_speedup_over_torch": round(t_torch_item["median"] / out["article_half_sweep_ms"], 2),
                      "max_abs_diff_over_max_abs_users": diff_user, "max_abs_diff_over_max_abs_articles": diff_item,
                      "torch_peak_bytes": int(torch.cuda.max_memory_allocated())}), flush=True)


if __name__ == "__main__":
    main()
