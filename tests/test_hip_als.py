"""dae_als_interactions / dae_als_gram / dae_als_solve_rows / dae_als_loss and helpers.als on the GPU against
tests/als_reference.py.  Integers are equal; the Gram is within 1 ulp of the float64 result rounded to float32; a half-sweep's
error against the float64 reference (max abs difference / max abs of the reference) is at most 8 x the same figure of the float32
NumPy restatement on the same input; the loss is within 1e-10 relative of the float64 host value.

Measured on an MI355X (every figure is in profiles/als_bench.txt), device / float32 restatement: the 32 half-sweep cases at most
4.17e-06 / 5.61e-06, the largest ratio 1.39; one CG step at most 2.97e-07 / 2.97e-07, three steps up to the figures above (the
one-entry rows of the log converge after two steps and the third works on rounding noise, on the host as on the device); the hub
log at most 4.83e-07 / 6.9e-07, ratio at most 0.94; fit_als after 8 iterations users 8.77e-07 / 1.96e-06, articles 1.49e-06 /
4.48e-06. Gram: no cell of any shape off by even 1 ulp. Loss: at most 2.7e-16 relative."""
import ctypes
import functools
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from als_reference import (fit_reference, gram_reference, half_sweep_reference, initial_item_factors, interactions_reference,
                           loss_reference)
from dae_rnn_news_recommendation_amd import _lib as L
from dae_rnn_news_recommendation_amd import helpers
from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LAM, ALPHA = float(F32(0.01)), 40.0
GATE = 8.0


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if indptr[-1] else np.zeros(0, dtype=np.int64)
    return indptr, items


def _up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).cuda()


def _ws(nbytes, extra=0):
    import torch
    t = torch.empty(nbytes + extra + 256, dtype=torch.uint8, device="cuda")
    return ctypes.c_void_p(t.data_ptr() + (-t.data_ptr()) % 256), t


def _rel(a, ref):
    return float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())


# ---- the logs ----
NA = 301                                                                 # article 300 is clicked by nobody


@functools.lru_cache(maxsize=None)
def the_log():
    """The log of the covisit tests plus users with repeated clicks, users without a click and an article nobody clicked.  The
    repeats sit in rows with other entries and stay small (counts of 4 against the log's own 3).  A row whose ONE entry has a large
    count is a system with two eigenvalue clusters: conjugate gradient ends after two steps and the third works on rounding noise.
    With a count of 40 (confidence 1601) the float32 restatement's own error on that row moves between 6e-7 and 5e-6 with nothing
    but the order of its sums, and the 8 x gate would compare two draws of that."""
    labels = np.random.default_rng(3).integers(0, 6, 300)
    indptr, items = synthetic_sessions(400, labels, mean_len=10, seed=5)
    rows = [items[indptr[u]:indptr[u + 1]] for u in range(400)]
    rows += [[7, 7, 7, 9, 7], [], [5, 5, 12, 40, 5, 77, 5], [], [299, 0, 299]]
    return _csr(rows)


@functools.lru_cache(maxsize=None)
def the_interactions():
    inter = interactions_reference(*the_log(), NA)
    assert np.diff(inter["user_ptr"]).max() <= 44 and np.diff(inter["item_ptr"]).max() <= 24
    assert (np.diff(inter["user_ptr"]) == 0).sum() == 2 and np.diff(inter["item_ptr"])[300] == 0 and inter["user_cnt"].max() == 4
    return inter


@functools.lru_cache(maxsize=None)
def hub_interactions():
    """Article 0 read by 5000 users with two clicks each (the second on one of 50 others); article 60 by exactly 256 users and
    article 61 by 257: the last row one wave solves and the first a workgroup solves."""
    rows = [[0, 1 + j % 50] for j in range(5000)] + [[60, 61]] * 256 + [[61]]
    inter = interactions_reference(*_csr(rows), 62)
    n = np.diff(inter["item_ptr"])
    assert n[0] == 5000 and n[60] == 256 and n[61] == 257 and n[1] == 100
    return inter


def orientation(inter, side):
    """``(ptr, idx, cnt, rows, n_fixed)`` of 'user' or 'item'."""
    ptr = inter[side + "_ptr"]
    other = "item" if side == "user" else "user"
    return ptr, inter[side + "_idx"], inter[side + "_cnt"], ptr.size - 1, inter[other + "_ptr"].size - 1


# ---- the raw calls ----
def raw_interactions(indptr, items, Na, pad=5, extra_ws=0):
    import torch
    lib = L.load()
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    M, nnz = indptr.size - 1, int(items.size)
    cap = nnz + pad
    i32, i64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.int64, device="cuda")
    out = {"user_ptr": torch.full((M + 1 + pad,), -7, **i64), "user_idx": torch.full((cap,), -7, **i32), "user_cnt": torch.full((cap,), -7, **i32),
           "item_ptr": torch.full((Na + 1 + pad,), -7, **i64), "item_idx": torch.full((cap,), -7, **i32), "item_cnt": torch.full((cap,), -7, **i32),
           "totals": torch.full((2,), -7, **i64)}
    ws_bytes = int(lib.dae_als_interactions_workspace(nnz, M, Na))
    assert (ws_bytes > 0) == (nnz > 0)
    ws_p, ws = _ws(ws_bytes, extra_ws)
    d_ptr, d_items = _up(indptr), _up(items.astype(np.int32))
    L.call("dae_als_interactions", L.ptr(d_ptr), L.ptr(d_items), M, nnz, Na, *(L.ptr(out[n]) for n in
           ("user_ptr", "user_idx", "user_cnt", "item_ptr", "item_idx", "item_cnt")), cap, L.ptr(out["totals"]),
           ws_p if nnz > 0 else None, ws_bytes + extra_ws if nnz > 0 else 0, L.current_stream())
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in out.items()}


def check_interactions(got, ref, M, Na):
    n = ref["pairs"]
    assert got["totals"].tolist() == [ref["events"], n]
    for side, rows in (("user", M), ("item", Na)):
        assert np.array_equal(got[side + "_ptr"][:rows + 1], ref[side + "_ptr"]) and (got[side + "_ptr"][rows + 1:] == -7).all()
        for part in ("_idx", "_cnt"):
            assert np.array_equal(got[side + part][:n], ref[side + part]) and (got[side + part][n:] == -7).all()
            assert got[side + part][n:].size >= 5


def raw_gram(Y, lam, ld=None):
    import torch
    lib = L.load()
    N, F = Y.shape
    ld = F if ld is None else ld
    buf = torch.full((N, ld), -7.0, dtype=torch.float32, device="cuda")
    buf[:, :F] = torch.from_numpy(Y)
    G = torch.full((F, F), -7.0, dtype=torch.float32, device="cuda")
    ws_bytes = int(lib.dae_als_gram_workspace(N, F))
    ws_p, ws = _ws(ws_bytes)
    L.call("dae_als_gram", L.ptr(buf), ld, N, F, lam, L.ptr(G), ws_p, ws_bytes, L.current_stream())
    torch.cuda.synchronize()
    return G.cpu().numpy()


def raw_solve(ptr, idx, cnt, Y, X0, G, alpha, steps, ldy=None, ldx=None, extra_ws=0):
    """The raw half-sweep; returns the whole X buffer [R x ldx] (pad columns pre-filled with -7)."""
    import torch
    lib = L.load()
    R, (N, F) = X0.shape[0], Y.shape
    ldy, ldx = F if ldy is None else ldy, F if ldx is None else ldx
    dY = torch.full((N, ldy), -7.0, dtype=torch.float32, device="cuda")
    dY[:, :F] = torch.from_numpy(np.array(Y, dtype=F32))
    dX = torch.full((R, ldx), -7.0, dtype=torch.float32, device="cuda")
    dX[:, :F] = torch.from_numpy(np.array(X0, dtype=F32))
    dG = _up(np.array(G, dtype=F32))
    ws_bytes = int(lib.dae_als_solve_rows_workspace(R))
    ws_p, ws = _ws(ws_bytes, extra_ws)
    d = [_up(ptr.astype(np.int64)), _up(idx.astype(np.int32)), _up(cnt.astype(np.int32))]
    L.call("dae_als_solve_rows", L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), R, L.ptr(dY), ldy, N, F, L.ptr(dG), alpha, steps, L.ptr(dX), ldx,
           ws_p, ws_bytes + extra_ws, L.current_stream())
    torch.cuda.synchronize()
    return dX.cpu().numpy()


@functools.lru_cache(maxsize=None)
def sweep_case(log, side, F, steps, warm):
    """Inputs and both host results of one half-sweep: ``(csr, Y, X0, G32, ref64, err32)``."""
    inter = the_interactions() if log == "log" else hub_interactions()
    ptr, idx, cnt, R, N = orientation(inter, side)
    rng = np.random.default_rng(100 + F)
    Y = (rng.standard_normal((N, F)) * 0.1).astype(F32)
    X0 = (rng.standard_normal((R, F)) * 0.1).astype(F32) if warm else np.zeros((R, F), dtype=F32)
    G32 = gram_reference(Y, LAM).astype(F32)
    ref = half_sweep_reference(ptr, idx, cnt, Y, X0, LAM, ALPHA, steps, np.float64)
    res = half_sweep_reference(ptr, idx, cnt, Y, X0, LAM, ALPHA, steps, np.float32, G32)
    for a in (Y, X0, G32, ref):
        a.setflags(write=False)
    return (ptr, idx, cnt), Y, X0, G32, ref, _rel(res, ref)


# ---- interactions ----
def test_interactions():
    indptr, items = the_log()
    check_interactions(raw_interactions(indptr, items, NA), the_interactions(), indptr.size - 1, NA)
    check_interactions(raw_interactions(indptr, items, NA, extra_ws=4096), the_interactions(), indptr.size - 1, NA)


def test_interactions_edge_logs():
    for rows, Na in (([[], [], []], 4), ([[2]], 3), ([[1, 1, 1, 1]], 2), ([[0, 5, -1, 2, 9]], 6)):
        indptr, items = _csr(rows)
        check_interactions(raw_interactions(indptr, items, Na), interactions_reference(indptr, items, Na), len(rows), Na)
    hub = _csr([[0, 1 + j % 50] for j in range(5000)])
    check_interactions(raw_interactions(*hub, 51), interactions_reference(*hub, 51), 5000, 51)


def test_interactions_helper():
    inter = helpers.als_interactions(the_log(), NA)
    ref = the_interactions()
    assert (inter.n_users, inter.n_articles, inter.n_events, inter.n_pairs) == (405, NA, ref["events"], ref["pairs"])
    for side, got in (("user", inter.user), ("item", inter.item)):
        assert all(np.array_equal(g, ref[side + part]) for g, part in zip(got, ("_ptr", "_idx", "_cnt")))
        assert got[0].dtype == np.int64 and got[1].dtype == got[2].dtype == np.int32
    cut = helpers.als_interactions(the_log(), NA, max_events=3, return_tensor=True)
    want = interactions_reference(*helpers.trim_histories(the_log(), 3), NA)
    assert cut.user[1].is_cuda and np.array_equal(cut.user[2].cpu().numpy(), want["user_cnt"]) and cut.n_events == want["events"]
    empty = helpers.als_interactions([[], []], 3)
    assert empty.n_pairs == 0 and empty.user[0].tolist() == [0, 0, 0] and empty.item[0].tolist() == [0, 0, 0, 0] and empty.user[1].size == 0


# ---- Gram ----
@pytest.mark.parametrize("F", [1, 7, 64, 128])
@pytest.mark.parametrize("N", [1, 63, 300, 5000])
def test_gram(N, F):
    Y = np.random.default_rng(N + F).standard_normal((N, F)).astype(F32)
    want = gram_reference(Y, LAM).astype(F32)
    for ld in (F, F + 3):
        got = raw_gram(Y, LAM, ld)
        off = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        off = np.where(np.signbit(got) == np.signbit(want), off, np.where((got == 0) & (want == 0), 0, 2))
        print("gram N %d F %d ld %d: %d of %d cells 1 ulp off" % (N, F, ld, int((off == 1).sum()), off.size))
        assert off.max() <= 1
    assert np.array_equal(helpers.als_gram(Y, LAM), raw_gram(Y, LAM))


# ---- half-sweep ----
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("F", [1, 7, 64, 128])
@pytest.mark.parametrize("side", ["user", "item"])
def test_half_sweep(side, F, steps, warm):
    csr, Y, X0, G32, ref, err32 = sweep_case("log", side, F, steps, warm)
    got = raw_solve(*csr, Y, X0, G32, ALPHA, steps)
    err = _rel(got, ref)
    print("half-sweep %s F %d steps %d warm %d: device %.3g, float32 restatement %.3g" % (side, F, steps, warm, err, err32))
    empty = np.diff(csr[0]) == 0
    assert empty.any() and not got[empty].any() and not np.signbit(got[empty]).any()      # exactly +0
    assert np.isfinite(got).all() and err <= GATE * err32


@pytest.mark.parametrize("F", [1, 7, 64, 128])
def test_half_sweep_hub(F):
    """Article rows of 5000 (a workgroup, many passes), 257 (a workgroup), 256 and 100 entries (a wave), warm start."""
    csr, Y, X0, G32, ref, err32 = sweep_case("hub", "item", F, 3, True)
    got = raw_solve(*csr, Y, X0, G32, ALPHA, 3)
    err = _rel(got, ref)
    per_row = np.abs(got - ref).max(axis=1) / np.abs(ref).max()
    print("hub F %d: device %.3g, float32 restatement %.3g; rows 0 / 60 / 61: %.3g %.3g %.3g" % (F, err, err32, *per_row[[0, 60, 61]]))
    assert np.isfinite(got).all() and err <= GATE * err32


@pytest.mark.parametrize("pads", [(3, 5), (4, 8)])
@pytest.mark.parametrize("F", [7, 64])
def test_half_sweep_leading_dimensions(F, pads):
    """ldy / ldx larger than F: the same bits as the contiguous call, and the pad columns stay."""
    csr, Y, X0, G32, _, _ = sweep_case("log", "user", F, 3, True)
    plain = raw_solve(*csr, Y, X0, G32, ALPHA, 3)
    wide = raw_solve(*csr, Y, X0, G32, ALPHA, 3, ldy=F + pads[0], ldx=F + pads[1])
    assert wide.shape[1] == F + pads[1] and (wide[:, F:] == -7).all()
    assert np.array_equal(wide[:, :F].view(np.uint32), plain.view(np.uint32))


@pytest.mark.parametrize("log, side, F", [("log", "user", 64), ("log", "item", 7), ("hub", "item", 64), ("hub", "item", 128)])
def test_half_sweep_is_deterministic(log, side, F):
    csr, Y, X0, G32, _, _ = sweep_case(log, side, F, 3, True)
    ptr, idx, cnt = csr
    first = raw_solve(ptr, idx, cnt, Y, X0, G32, ALPHA, 3)
    assert first.tobytes() == raw_solve(ptr, idx, cnt, Y, X0, G32, ALPHA, 3).tobytes()
    assert first.tobytes() == raw_solve(ptr, idx, cnt, Y, X0, G32, ALPHA, 3, extra_ws=1 << 20).tobytes()
    perm = np.random.default_rng(9).permutation(ptr.size - 1)
    n = np.diff(ptr)[perm]
    p_ptr = np.zeros(ptr.size, dtype=np.int64)
    p_ptr[1:] = np.cumsum(n)
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in perm]) if idx.size else np.zeros(0, dtype=np.int64)
    moved = raw_solve(p_ptr, idx[take], cnt[take], Y, X0[perm], G32, ALPHA, 3)
    back = np.empty_like(moved)
    back[perm] = moved
    assert first.tobytes() == back.tobytes()


def test_solve_rows_helper():
    csr, Y, X0, G32, ref, err32 = sweep_case("log", "user", 64, 3, True)
    got = helpers.als_solve_rows(*csr, Y, X0, regularization=LAM, alpha=ALPHA, cg_steps=3)
    assert got.dtype == F32 and _rel(got, ref) <= GATE * err32
    assert np.array_equal(got, helpers.als_solve_rows(*csr, Y, X0, regularization=LAM, alpha=ALPHA, cg_steps=3, gram=helpers.als_gram(Y, LAM)))
    import torch
    X = torch.from_numpy(np.array(X0)).cuda()
    out = helpers.als_solve_rows(*csr, torch.from_numpy(np.array(Y)).cuda(), X, regularization=LAM, alpha=ALPHA, return_tensor=True)
    assert out.data_ptr() == X.data_ptr() and np.array_equal(X.cpu().numpy(), got)            # a device tensor is updated in place


# ---- loss ----
@pytest.mark.parametrize("F", [1, 7, 64, 128])
def test_loss(F):
    for log, side in (("log", "user"), ("log", "item"), ("hub", "item")):
        (ptr, idx, cnt), Y, X0, _, _, _ = sweep_case(log, side, F, 3, True)
        want = loss_reference(ptr, idx, cnt, X0, Y, LAM, ALPHA)
        got = helpers.als_loss(ptr, idx, cnt, X0, Y, regularization=LAM, alpha=ALPHA)
        print("loss %s %s F %d: %.17g against %.17g, relative %.3g" % (log, side, F, got, want, abs(got - want) / abs(want)))
        assert abs(got - want) <= 1e-10 * abs(want)
        assert got == helpers.als_loss(ptr, idx, cnt, X0, Y, regularization=LAM, alpha=ALPHA)


# ---- fit_als ----
@functools.lru_cache(maxsize=None)
def fitted():
    return helpers.fit_als(the_log(), NA, factors=16, iterations=8, compute_loss=True)


def test_fit_als_loss_falls_and_factors_follow_the_reference():
    model = fitted()
    curve = model.loss_curve
    assert len(curve) == 16 and all(b < a for a, b in zip(curve, curve[1:])), curve
    inter = the_interactions()
    X64, Y64, curve64 = fit_reference(inter, 405, NA, 16, 0.01, 40.0, 8, 3, dtype=np.float64)
    X32, Y32, _ = fit_reference(inter, 405, NA, 16, 0.01, 40.0, 8, 3, dtype=np.float32)
    for name, got, r32, r64 in (("users", model.user_factors, X32, X64), ("articles", model.item_factors, Y32, Y64)):
        print("fit_als %s after 8 iterations: device %.3g, float32 restatement %.3g" % (name, _rel(got, r64), _rel(r32, r64)))
        assert _rel(got, r64) <= GATE * _rel(r32, r64)
    assert np.allclose(curve, curve64, rtol=1e-4)
    assert (model.factors, model.cg_steps, model.iterations, model.alpha) == (16, 3, 8, 40.0) and model.user_factors.shape == (405, 16)
    again = helpers.fit_als(the_log(), NA, factors=16, iterations=8)
    assert again.loss_curve == [] and again.user_factors.tobytes() == model.user_factors.tobytes()
    assert again.item_factors.tobytes() == model.item_factors.tobytes()
    start = helpers.fit_als(the_log(), NA, factors=16, iterations=0)
    assert np.array_equal(start.item_factors, initial_item_factors(NA, 16, 0)) and not start.user_factors.any()
    same = helpers.fit_als(the_log(), NA, factors=16, iterations=8, init=initial_item_factors(NA, 16, 0))
    assert same.item_factors.tobytes() == model.item_factors.tobytes()


def test_model_recommend_user_states_and_round_trip(tmp_path):
    model = fitted()
    hist = the_log()
    states = model.user_states(hist)
    inter = the_interactions()
    zero = helpers.als_solve_rows(inter["user_ptr"], inter["user_idx"], inter["user_cnt"], model.item_factors, None, regularization=model.regularization,
                                  alpha=model.alpha, cg_steps=model.cg_steps)
    assert states.tobytes() == zero.tobytes() and states.shape == (405, 16)
    idx, score = model.recommend(hist, 10)
    want = helpers.recommend(states, model.item_factors, 10, seen=hist)
    assert np.array_equal(idx, want[0]) and np.array_equal(score.view(np.uint32), want[1].view(np.uint32))
    indptr, items = hist
    assert not any(np.isin(idx[u], items[indptr[u]:indptr[u + 1]]).any() for u in range(405)) and (idx >= 0).all()
    new_users = [[3, 4, 3], [], [250]]
    assert model.user_states(new_users).shape == (3, 16) and not model.user_states(new_users)[1].any()
    near, sims = model.similar([5, 17], 4)
    assert near.shape == (2, 4) and 5 not in near[0] and 17 not in near[1] and (np.diff(sims, axis=1) <= 0).all()
    model.save(str(tmp_path / "als.npz"))
    back = helpers.ALSModel.load(str(tmp_path / "als.npz"))
    assert back.user_factors.tobytes() == model.user_factors.tobytes() and back.item_factors.tobytes() == model.item_factors.tobytes()
    assert back.loss_curve == model.loss_curve and (back.factors, back.cg_steps, back.iterations) == (16, 3, 8)
    assert np.array_equal(back.recommend(hist, 10)[0], idx)


# ---- the command line ----
def test_cli_als(tmp_path):
    """--als in a fresh child process: both files, the metric keys of the co-visitation file, the model equal to fit_als on the saved
    histories, the lists equal to the model's own."""
    args = ["--model_name", "rec", "--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4",
            "--sessions", "synthetic", "--recommend", "10", "--similarity", "False", "--als", "--als_factors", "16", "--als_iterations", "4"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "main_autoencoder.py")] + args, cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    found = glob.glob(str(tmp_path / "**" / "article_encoded_recommend10_als.npz"), recursive=True)
    models = glob.glob(str(tmp_path / "**" / "als_model.npz"), recursive=True)
    assert len(found) == 1 and len(models) == 1
    r = np.load(found[0])
    assert {"indices", "scores", "targets", "hist_indptr", "hist_items"} <= set(r.files)
    assert r["indices"].shape == r["scores"].shape == (200, 10) and r["indices"].dtype == np.int64 and r["scores"].dtype == F32
    model = helpers.ALSModel.load(models[0])
    assert model.item_factors.shape == (400, 16) and model.user_factors.shape == (200, 16) and model.iterations == 4
    hist = (r["hist_indptr"], r["hist_items"])
    mine = helpers.fit_als(hist, 400, factors=16, iterations=4)
    assert mine.item_factors.tobytes() == model.item_factors.tobytes() and mine.user_factors.tobytes() == model.user_factors.tobytes()
    assert np.array_equal(model.recommend(hist, 10)[0], r["indices"])
    assert run.stdout.count("hit@10") == 3 and re.search(r"hit@10 ALS factors +[0-9.]+  MRR [0-9.]+  nDCG [0-9.]+", run.stdout)
