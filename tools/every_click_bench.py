#!/usr/bin/env python3
"""Every-click timing: the shared stamped exclusion lists against materialised per-row prefix lists, on one set of rows in one process.

Shape: --users histories of geometric length (mean --mean-len, capped at --max-len, the trainer's max_events) over Na articles of H
columns; one query row per event (random vectors: the kernels' work does not depend on the values), k = --k, the target of a row is
the user's next click.  Two ways to tell row e which articles its user had clicked by then:

  (seq) one list per user with the position of every article's first click, shared by the user's rows (helpers.click_prefix_lists,
        dae_topk_similarity_seq / dae_rank_similarity_seq): the lists are no larger than the click log;
  (ex)  one sorted-unique prefix per event, built on the host (vectorised) and read by dae_topk_similarity_ex / dae_rank_similarity:
        sum of L (L + 1) / 2 items.

Both are checked to agree bit for bit before anything is timed.  The forms alternate seq, ex, seq, ex, ... for --rounds rounds (at
least five); every timing is a HIP-event window of at least --window-ms after a warm-up.  Recorded: per call every round's ms, the
medians, the spread of (ex) ((max - min) / median) and seq / ex; the host seconds to build either set of lists and the bytes either
uploads; and, for scale, the last-click-only calls (one row per user, the user's whole history as its list).  One JSON line,
preceded by one line describing the device.

  python tools/every_click_bench.py --out profiles/every_click_bench.json     # 4096 users x 64 000 articles, H 500, k 10
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


def materialise(np, helpers, lists, row_list, row_limit):
    """The per-row CSR {item : stamp <= limit} of the shared lists, in the form dae_topk_similarity_ex reads (vectorised, chunked)."""
    lp, li, ls = lists
    n_rows = row_list.size
    counts = np.zeros(n_rows, np.int64)
    parts = []
    lim = row_limit.astype(np.int64)
    for a, b in helpers.shared_row_chunks(np.diff(lp)[row_list]):
        rows, places = helpers.shared_pairs(lp, row_list, a, b)
        keep = ls[places] <= lim[rows]
        counts[a:b] = np.bincount(rows[keep] - a, minlength=b - a)
        parts.append(li[places[keep]])                                          # ascending within a row, as the shared list is
    indptr = np.zeros(n_rows + 1, np.int64)
    indptr[1:] = np.cumsum(counts)
    return indptr, (np.concatenate(parts) if parts else np.zeros(0, np.int32)).astype(np.int32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--articles", type=int, default=64000)
    ap.add_argument("--H", type=int, default=500)
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--mean-len", type=float, default=50.0)
    ap.add_argument("--max-len", type=int, default=50)
    ap.add_argument("--pool", type=int, default=2000, help="a user clicks within a pool of this many articles (repeats; 0: anywhere)")
    ap.add_argument("--k", type=int, default=10)
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
    assert torch.cuda.is_available(), "every_click_bench needs a GPU"
    lib = L.load()
    lines = [json.dumps(device_record(torch))]
    print(lines[0], flush=True)
    M, Na, H, k = a.users, a.articles, a.H, a.k
    rng = np.random.default_rng(a.seed)
    lens = np.minimum(rng.geometric(1.0 / a.mean_len, M), a.max_len).astype(np.int64)
    indptr = np.zeros(M + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    nnz = int(indptr[-1])
    if a.pool > 0:                                                              # articles near a per-user centre: repeated clicks
        centre = np.repeat(rng.integers(0, Na, M), lens)
        items = ((centre + rng.integers(0, a.pool, nnz)) % Na).astype(np.int64)
    else:
        items = rng.integers(0, Na, nnz).astype(np.int64)
    hist = (indptr, items)

    t0 = time.perf_counter()
    lists = helpers.click_prefix_lists(hist)
    rows = helpers.every_click_rows(hist)
    host_seq = time.perf_counter() - t0
    t0 = time.perf_counter()
    xp, xi = materialise(np, helpers, lists, rows["row_list"], rows["row_limit"])
    host_ex = time.perf_counter() - t0
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()            # noqa: E731
    seq_d = [dev(x) for x in lists] + [dev(rows["row_list"]), dev(rows["row_limit"])]
    xp_d, xi_d = dev(xp), dev(xi)
    t_d = dev(np.where(rows["targets"] >= 0, rows["targets"], -1).astype(np.int32))
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    E = torch.randn((Na, H), device="cuda", generator=g)
    S = torch.randn((nnz, H), device="cuda", generator=g)                       # one state per event
    # the last-click-only protocol, for scale: one row per user, the whole history as its list
    up, ui = helpers.normalize_exclusions(hist, M, Na)
    up_d, ui_d = dev(up), dev(ui)
    last = np.maximum(indptr[1:] - 1, 0)
    U = S[dev(last)].contiguous()
    ut_d = dev(items[last].astype(np.int32))
    rec = {"users": M, "rows": nnz, "Na": Na, "H": H, "k": k, "max_len": a.max_len, "pool": a.pool, "rounds": a.rounds, "window_ms": a.window_ms,
           "shared_items": int(lists[1].size), "per_row_items": int(xi.size), "per_row_over_shared": round(xi.size / max(lists[1].size, 1), 2),
           "host_build_s": {"seq": round(host_seq, 4), "ex": round(host_ex, 4)},
           "bytes_uploaded": {"seq": int(sum(x.numel() * x.element_size() for x in seq_d)),
                              "ex": int(xp_d.numel() * 8 + xi_d.numel() * 4)}}

    ws_bytes = max(int(lib.dae_topk_similarity_seq_workspace(nnz, Na, H, k)), int(lib.dae_rank_similarity_seq_workspace(nnz, Na, H)))
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    wp = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    idx = [torch.empty((nnz, k), dtype=torch.int32, device="cuda") for _ in range(2)]
    sc = [torch.empty((nnz, k), dtype=torch.float32, device="cuda") for _ in range(2)]
    rk = [torch.empty(nnz, dtype=torch.int32, device="cuda") for _ in range(2)]
    rs = [torch.empty(nnz, dtype=torch.float32, device="cuda") for _ in range(2)]
    uidx, usc = torch.empty((M, k), dtype=torch.int32, device="cuda"), torch.empty((M, k), dtype=torch.float32, device="cuda")
    urk, urs = torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(M, dtype=torch.float32, device="cuda")
    head = lambda Q, n: (L.ptr(Q), Q.stride(0), n, L.ptr(E), E.stride(0), Na, H, 0, 1)      # noqa: E731

    def topk(form):
        if form == 0:
            L.call("dae_topk_similarity_seq", *head(S, nnz), k, 0, *(L.ptr(x) for x in seq_d[:3]), M, L.ptr(seq_d[3]), L.ptr(seq_d[4]),
                   None, None, L.ptr(idx[0]), L.ptr(sc[0]), k, wp, ws_bytes, L.current_stream())
        elif form == 1:
            L.call("dae_topk_similarity_ex", *head(S, nnz), k, 0, L.ptr(xp_d), L.ptr(xi_d), L.ptr(idx[1]), L.ptr(sc[1]), k, wp, ws_bytes,
                   L.current_stream())
        else:
            L.call("dae_topk_similarity_ex", *head(U, M), k, 0, L.ptr(up_d), L.ptr(ui_d), L.ptr(uidx), L.ptr(usc), k, wp, ws_bytes,
                   L.current_stream())

    def rank(form):
        if form == 0:
            L.call("dae_rank_similarity_seq", *head(S, nnz), 0, *(L.ptr(x) for x in seq_d[:3]), M, L.ptr(seq_d[3]), L.ptr(seq_d[4]),
                   None, None, L.ptr(t_d), L.ptr(rk[0]), L.ptr(rs[0]), wp, ws_bytes, L.current_stream())
        elif form == 1:
            L.call("dae_rank_similarity", *head(S, nnz), 0, L.ptr(xp_d), L.ptr(xi_d), L.ptr(t_d), L.ptr(rk[1]), L.ptr(rs[1]), wp, ws_bytes,
                   L.current_stream())
        else:
            L.call("dae_rank_similarity", *head(U, M), 0, L.ptr(up_d), L.ptr(ui_d), L.ptr(ut_d), L.ptr(urk), L.ptr(urs), wp, ws_bytes,
                   L.current_stream())

    # ---- warm-up and checks: the two forms agree bit for bit ----
    for form in range(3):
        topk(form); rank(form)
    torch.cuda.synchronize()
    assert torch.equal(idx[0], idx[1]) and torch.equal(sc[0].view(torch.int32), sc[1].view(torch.int32))
    assert torch.equal(rk[0], rk[1]) and torch.equal(rs[0].view(torch.int32), rs[1].view(torch.int32))
    names = ("seq", "ex", "last_click_only")
    for call, fn in (("recommend", topk), ("recommend_ranks", rank)):
        ms = {n: [] for n in names}
        for _ in range(a.rounds):
            for form, n in enumerate(names):
                ms[n].append(round(timed_ms(torch, lambda: fn(form), a.window_ms)[0], 4))
        med = {n: float(np.median(v)) for n, v in ms.items()}
        r = {n: {"ms": ms[n], "median_ms": round(med[n], 4)} for n in names}
        r["ex"]["tflops"] = round(2.0 * nnz * Na * H / med["ex"] * 1e-9, 2)
        r["ex_spread"] = round((max(ms["ex"]) - min(ms["ex"])) / med["ex"], 4)
        r["seq_spread"] = round((max(ms["seq"]) - min(ms["seq"])) / med["seq"], 4)
        r["seq_over_ex"] = round(med["seq"] / med["ex"], 4)
        rec[call] = r
    del ws
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
