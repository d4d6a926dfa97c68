#!/usr/bin/env python3
"""Candidate-window timing: recommend and recommend_ranks with and without per-user windows, all forms in one process.

Shape: --users user vectors in random order against Na articles of H columns, geometric histories (mean --mean-len) as exclusion
lists, k = --k, one held-out target per user.  Three forms of the top-k call and of the rank call, at the C ABI on operands
prepared beforehand (exclusion CSR normalised and uploaded once, rows ordered by their windows as the helpers order them):

  (a) the unwindowed call (dae_topk_similarity_ex / dae_rank_similarity): the yardstick;
  (b) the windowed call with the window [0, Na) for every row: the same tiles, two more compares;
  (c) the windowed call with windows of Na / --fraction columns at uniformly random offsets, rows ordered by (lo, hi).

The forms alternate a, b, c, a, b, c, ... for --rounds rounds (at least five); every timing is a HIP-event window of at least
--window-ms after a warm-up.  Recorded per call: every round's ms, the median, the spread of (a) ((max - min) / median), the
ratios of the medians b / a and c / a, and `tile_fraction`: the share of (query tile, corpus tile) pairs inside the unions of the
ordered windows -- what (c) / (a) would be if a call were nothing but its score tiles.  (b) and (a) are checked to agree bit for
bit, and (c) against the windows, before anything is timed.  `helper_s` is one wall-clock call of the helper, host preparation
(validation, ordering, copies) included.  One JSON line, preceded by one line describing the device.

  python tools/window_bench.py --out profiles/window_bench.json     # 100 000 users x 64 000 articles, H 500, k 10, windows of Na / 16
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


def tile_fraction(np, lo, hi, n_articles, tile=128):
    """The share of (query tile, corpus tile) pairs the windowed kernels walk for rows in this order: per 128 rows the tiles of
    the union of the non-empty windows."""
    walked, qtiles, ctiles = 0, 0, (int(n_articles) + tile - 1) // tile
    for a in range(0, lo.size, tile):
        l, h = lo[a:a + tile], hi[a:a + tile]
        ok = h > l
        qtiles += 1
        if ok.any():
            walked += (int(h[ok].max()) + tile - 1) // tile - int(l[ok].min()) // tile
    return walked / float(qtiles * ctiles)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", type=int, default=64000)
    ap.add_argument("--H", type=int, default=500)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--mean-len", type=float, default=50.0)
    ap.add_argument("--max-len", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fraction", type=int, default=16, help="windows of articles / FRACTION columns")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args(argv)
    assert a.rounds >= 5, "the spread of the yardstick wants at least five rounds"
    import numpy as np
    import torch
    from dae_rnn_news_recommendation_amd import _lib as L
    from dae_rnn_news_recommendation_amd import helpers
    assert torch.cuda.is_available(), "window_bench needs a GPU"
    lib = L.load()
    lines = [json.dumps(device_record(torch))]
    print(lines[0], flush=True)
    M, Na, H, k = a.users, a.articles, a.H, a.k
    rng = np.random.default_rng(a.seed)
    lens = np.minimum(rng.geometric(1.0 / a.mean_len, M), a.max_len).astype(np.int64)
    indptr = np.zeros(M + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    items = rng.integers(0, Na, int(indptr[-1])).astype(np.int32)
    width = max(Na // a.fraction, 1)
    lo = rng.integers(0, Na - width + 1, M).astype(np.int32)
    hi = (lo + width).astype(np.int32)
    tgt = (lo + rng.integers(0, width, M)).astype(np.int32)                 # the held-out click lies inside the window
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    E = torch.randn((Na, H), device="cuda", generator=g)
    U = torch.randn((M, H), device="cuda", generator=g)                     # users in random order
    xp, xi = helpers.normalize_exclusions((indptr, items), M, Na)
    perm = np.lexsort((hi, lo))                                             # the helpers' order: stable by (lo, hi)
    xp_s, xi_s = helpers.permute_histories(xp, xi, perm)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()        # noqa: E731
    xp_d, xi_d, xp_sd, xi_sd = dev(xp), dev(xi), dev(xp_s), dev(xi_s)
    perm_d = dev(perm)
    U_s = U[perm_d].contiguous()
    full_lo, full_hi = dev(np.zeros(M, np.int32)), dev(np.full(M, Na, np.int32))
    lo_sd, hi_sd, t_d, t_sd = dev(lo[perm]), dev(hi[perm]), dev(tgt), dev(tgt[perm])
    rec = {"users": M, "Na": Na, "H": H, "k": k, "nnz": int(indptr[-1]), "excluded_entries": int(xi.size), "window_columns": width,
           "tile_fraction_sorted": round(tile_fraction(np, lo[perm], hi[perm], Na), 4),
           "tile_fraction_given_order": round(tile_fraction(np, lo, hi, Na), 4), "rounds": a.rounds, "window_ms": a.window_ms}

    ws_bytes = max(int(lib.dae_topk_similarity_win_workspace(M, Na, H, k)), int(lib.dae_rank_similarity_win_workspace(M, Na, H)))
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    idx = [torch.empty((M, k), dtype=torch.int32, device="cuda") for _ in range(3)]
    sc = [torch.empty((M, k), dtype=torch.float32, device="cuda") for _ in range(3)]
    rk = [torch.empty(M, dtype=torch.int32, device="cuda") for _ in range(3)]
    rs = [torch.empty(M, dtype=torch.float32, device="cuda") for _ in range(3)]

    def topk(form):
        if form == 0:
            L.call("dae_topk_similarity_ex", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, k, 0, L.ptr(xp_d), L.ptr(xi_d),
                   L.ptr(idx[0]), L.ptr(sc[0]), k, wp, ws_bytes, L.current_stream())
        else:
            Q, p, i, wl, wh = (U, xp_d, xi_d, full_lo, full_hi) if form == 1 else (U_s, xp_sd, xi_sd, lo_sd, hi_sd)
            L.call("dae_topk_similarity_win", L.ptr(Q), Q.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, k, 0, L.ptr(p), L.ptr(i),
                   L.ptr(wl), L.ptr(wh), L.ptr(idx[form]), L.ptr(sc[form]), k, wp, ws_bytes, L.current_stream())

    def rank(form):
        if form == 0:
            L.call("dae_rank_similarity", L.ptr(U), U.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, 0, L.ptr(xp_d), L.ptr(xi_d),
                   L.ptr(t_d), L.ptr(rk[0]), L.ptr(rs[0]), wp, ws_bytes, L.current_stream())
        else:
            Q, p, i, wl, wh, t = (U, xp_d, xi_d, full_lo, full_hi, t_d) if form == 1 else (U_s, xp_sd, xi_sd, lo_sd, hi_sd, t_sd)
            L.call("dae_rank_similarity_win", L.ptr(Q), Q.stride(0), M, L.ptr(E), E.stride(0), Na, H, 0, 1, 0, L.ptr(p), L.ptr(i),
                   L.ptr(wl), L.ptr(wh), L.ptr(t), L.ptr(rk[form]), L.ptr(rs[form]), wp, ws_bytes, L.current_stream())

    # ---- warm-up and checks: (b) is (a) bit for bit; (c) stays inside its windows, and its ranks are at most (a)'s ----
    for form in range(3):
        topk(form); rank(form)
    torch.cuda.synchronize()
    assert torch.equal(idx[0], idx[1]) and torch.equal(sc[0].view(torch.int32), sc[1].view(torch.int32))
    assert torch.equal(rk[0], rk[1]) and torch.equal(rs[0].view(torch.int32), rs[1].view(torch.int32))
    assert ((idx[2] >= lo_sd[:, None]) & (idx[2] < hi_sd[:, None])).all()
    assert (rk[2] <= rk[0][perm_d]).all() and torch.equal(rs[2].view(torch.int32), rs[0][perm_d].view(torch.int32))
    names = ("a_unwindowed", "b_full_window", "c_windows")
    for call, fn, flop in (("recommend", topk, 2.0 * M * Na * H), ("recommend_ranks", rank, 2.0 * M * Na * H)):
        ms = {n: [] for n in names}
        for _ in range(a.rounds):
            for form, n in enumerate(names):
                ms[n].append(round(timed_ms(torch, lambda: fn(form), a.window_ms)[0], 4))
        med = {n: float(np.median(v)) for n, v in ms.items()}
        r = {n: {"ms": ms[n], "median_ms": round(med[n], 4)} for n in names}
        r["a_unwindowed"]["tflops"] = round(flop / med["a_unwindowed"] * 1e-9, 2)
        r["a_spread"] = round((max(ms["a_unwindowed"]) - min(ms["a_unwindowed"])) / med["a_unwindowed"], 4)
        r["b_over_a"] = round(med["b_full_window"] / med["a_unwindowed"], 4)
        r["c_over_a"] = round(med["c_windows"] / med["a_unwindowed"], 4)
        rec[call] = r
    del ws
    t0 = time.perf_counter()
    helpers.recommend(U, E, k=k, seen=(indptr, items), window=(lo, hi), return_tensor=True)
    torch.cuda.synchronize()
    rec["recommend"]["helper_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    helpers.recommend_ranks(U, E, tgt, seen=(indptr, items), window=(lo, hi), return_tensor=True)
    torch.cuda.synchronize()
    rec["recommend_ranks"]["helper_s"] = round(time.perf_counter() - t0, 3)
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
