"""CPU checks of the GRU user states (dae_gru_user_states, dae_gru_user_states_workspace) and of the host code around them:
both builds export the symbols under an unchanged ABI version, every argument error is reported before any HIP call (so on a
machine without a GPU), the workspace has no events x H term, and gru_schedule, trim_histories and GRUUserModel on hand-made
cases.  ``gru_reference`` below is the float64 (or, with ``dtype=np.float32``, float32) NumPy restatement of the recurrence
that tests/test_hip_gru.py takes as the truth; here it is pinned to an independent implementation, torch.nn.GRU in float64."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first


def gru_reference(E, w_ih, w_hh, b_ih, b_hh, indptr, items, initial=None, dtype=np.float64):
    """The recurrence of include/dae_hip.h, event by event, in ``dtype``: (states after every event [nnz x H], last states [M x H]).

        gi = W_ih x + b_ih   gh = W_hh h + b_hh   r = sigmoid(gi_r + gh_r)   z = sigmoid(gi_z + gh_z)
        n = tanh(gi_n + r * gh_n)   h' = (1 - z) * n + z * h
    """
    E, w_ih, w_hh, b_ih, b_hh = (np.asarray(a, dtype) for a in (E, w_ih, w_hh, b_ih, b_hh))
    H, M = w_hh.shape[1], len(indptr) - 1
    one = dtype(1)
    sig = lambda v: one / (one + np.exp(-v))
    gi_all = E @ w_ih.T + b_ih                                          # per article
    every, last = np.zeros((len(items), H), dtype), np.zeros((M, H), dtype)
    for u in range(M):
        h = np.zeros(H, dtype) if initial is None else np.asarray(initial[u], dtype)
        for e in range(indptr[u], indptr[u + 1]):
            gi, gh = gi_all[items[e]], w_hh @ h + b_hh
            r, z = sig(gi[:H] + gh[:H]), sig(gi[H:2 * H] + gh[H:2 * H])
            n = np.tanh(gi[2 * H:] + r * gh[2 * H:])
            h = (one - z) * n + z * h
            every[e] = h
        last[u] = h
    return every, last


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_gru_symbols_are_exported_and_the_abi_version_stays(fmt):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load(fmt)
    for name in ("dae_gru_user_states", "dae_gru_user_states_workspace"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.dae_abi_version() == _lib.ABI_VERSION == 9
    assert len(_lib.SIGNATURES["dae_gru_user_states"][1]) == 26


def _active(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _gru(lib, E=P, lde=64, Na=100, D=64, H=48, W_ih=P, ldwi=64, W_hh=P, ldwh=48, b_ih=P, b_hh=P, indptr=P, items=P, order=P, M=10,
         nnz=50, active=(10, 8, 3), T=None, h0=None, ldh0=0, all_states=0, U=P, ldu=48, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_gru_user_states_workspace(max(Na, 0), max(D, 0), max(H, 0), max(M, 0))
    act = None if active is None else _active(*active)
    T = (0 if active is None else len(active)) if T is None else T
    return lib.dae_gru_user_states(E, lde, Na, D, H, W_ih, ldwi, W_hh, ldwh, b_ih, b_hh, indptr, items, order, M, nnz, T, act, h0, ldh0,
                                   all_states, U, ldu, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(E=None), b"E / indptr are NULL"),
    (dict(indptr=None), b"E / indptr are NULL"),
    (dict(W_ih=None), b"W_ih / W_hh / b_ih / b_hh are NULL"),
    (dict(W_hh=None), b"W_ih / W_hh / b_ih / b_hh are NULL"),
    (dict(b_ih=None), b"W_ih / W_hh / b_ih / b_hh are NULL"),
    (dict(b_hh=None), b"W_ih / W_hh / b_ih / b_hh are NULL"),
    (dict(items=None), b"items is NULL"),
    (dict(order=None), b"order is NULL"),
    (dict(active=None, T=3), b"active_host is NULL"),
    (dict(U=None), b"U is NULL"),
    (dict(U=None, all_states=1), b"U is NULL"),
    (dict(ws=None), b"workspace too small"),
    (dict(Na=0), b"must be positive"),
    (dict(D=0), b"must be positive"),
    (dict(H=-2), b"must be positive"),
    (dict(M=-1), b"negative count"),
    (dict(nnz=-1), b"negative count"),
    (dict(T=-1), b"negative count"),
    (dict(lde=63), b"must be >= D"),
    (dict(ldwi=10), b"must be >= D"),
    (dict(ldwh=47), b"must be >= H"),
    (dict(ldu=47), b"must be >= H"),
    (dict(h0=P, ldh0=47), b"must be >= H"),
    (dict(active=(10, 3, 8)), b"non-increasing"),
    (dict(active=(11, 8, 3)), b"at most M"),
    (dict(active=(10, 8, -1)), b"non-increasing"),
    (dict(active=(10, 10, 10, 10, 10, 1)), b"more than nnz"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
    (dict(Na=3 * 10 ** 6, D=500, lde=500, ldwi=500), b"exceeds 4 GiB"),            # the E image
    (dict(M=3 * 10 ** 6, H=500, ldwh=500, ldu=500, active=(10,)), b"exceeds 4 GiB"),   # a state buffer
    (dict(H=20000, ldwh=20000, ldu=20000), b"exceeds 4 GiB"),                      # the W_hh image
])
def test_gru_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _gru(lib, **kw) != 0
    assert msg in lib.dae_last_error(), lib.dae_last_error()


def test_gru_states_of_no_users_is_a_no_op():
    lib = _lib()
    assert _gru(lib, M=0, nnz=0, items=None, order=None, U=None, active=None, ws=None, ws_bytes=0) == 0   # returns before any HIP call


def test_gru_workspace_has_no_events_term():
    lib = _lib()
    ws = lib.dae_gru_user_states_workspace
    assert len(ws.argtypes) == 4                                        # (Na, D, H, M): the number of events is not an argument
    pad = lambda n: (n + 127) // 128 * 128
    al = lambda b: (b + 255) // 256 * 256
    for Na, D, H, M in ((300, 70, 70, 306), (1000, 500, 500, 1), (400, 96, 160, 100000), (8000, 500, 500, 262144)):
        Nap, Dp, Hp, Mp = pad(Na), pad(D), pad(H), pad(M)
        want = (al(Nap * Dp * 4) + al(3 * Hp * Dp * 4) + al(3 * Hp * Hp * 4) + al(Nap * 3 * Hp * 4) + al(Hp * 4) + 2 * al(Mp * Hp * 4))
        assert ws(Na, D, H, M) == want
    # linear in the users: equal steps of M give equal growth
    a, b, c = (ws(8000, 500, 500, n * 128 * 1024) for n in (1, 2, 3))
    assert c - b == b - a == 2 * 128 * 1024 * 512 * 4
    assert ws(0, 10, 10, 10) == 0 and ws(10, 0, 10, 10) == 0 and ws(10, 10, 0, 10) == 0 and ws(10, 10, 10, -1) == 0
    assert ws(10, 10, 10, 0) > 0


def test_gru_schedule_on_hand_made_cases():
    from dae_rnn_news_recommendation_amd.helpers import gru_schedule
    order, active = gru_schedule([0, 2, 2, 5, 7, 7, 10])               # lengths 2 0 3 2 0 3
    assert order.dtype == np.int32 and active.dtype == np.int64
    assert order.tolist() == [2, 5, 0, 3, 1, 4]                         # longest first; ties (2 and 5, 0 and 3, 1 and 4) keep the input order
    assert active.tolist() == [4, 4, 2]
    order, active = gru_schedule([0, 4])                                # a single user
    assert order.tolist() == [0] and active.tolist() == [1, 1, 1, 1]
    order, active = gru_schedule([0, 0, 0])                             # only empty users
    assert order.tolist() == [0, 1] and active.shape == (0,)
    order, active = gru_schedule([0])                                   # no users
    assert order.shape == (0,) and active.shape == (0,)
    rng = np.random.default_rng(0)
    n = rng.integers(0, 40, 500)
    indptr = np.concatenate([[0], np.cumsum(n)])
    order, active = gru_schedule(indptr)
    assert sorted(order.tolist()) == list(range(500))
    assert (np.diff(n[order]) <= 0).all() and (np.diff(active) <= 0).all()
    assert active.size == n.max() and active.sum() == n.sum() and active[0] == (n > 0).sum()
    assert all(active[t] == (n > t).sum() for t in range(active.size))
    same = np.flatnonzero(np.diff(n[order]) == 0)
    assert (order[same] < order[same + 1]).all()                        # stable
    with pytest.raises(ValueError):
        gru_schedule([0, 3, 2])


def test_trim_histories_keeps_the_most_recent_events():
    from dae_rnn_news_recommendation_amd.helpers import trim_histories
    hist = [[1, 2, 3, 4, 5], [], [6], [7, 8, 9]]
    indptr, items = trim_histories(hist, 3)
    assert indptr.tolist() == [0, 3, 3, 4, 7] and items.tolist() == [3, 4, 5, 6, 7, 8, 9]
    indptr, items = trim_histories(hist, 1)
    assert indptr.tolist() == [0, 1, 1, 2, 3] and items.tolist() == [5, 6, 9]
    indptr, items = trim_histories(hist, 0)
    assert indptr.tolist() == [0, 0, 0, 0, 0] and items.size == 0
    indptr, items = trim_histories(hist, 100)
    assert indptr.tolist() == [0, 5, 5, 6, 9] and items.tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    indptr, items = trim_histories((np.array([0, 2, 5]), np.array([4, 5, 6, 7, 8])), 2)      # the (indptr, items) form
    assert indptr.tolist() == [0, 2, 4] and items.tolist() == [4, 5, 7, 8]
    with pytest.raises(ValueError):
        trim_histories(hist, -1)


def test_gru_user_states_refuses_max_events_with_all_states():
    from dae_rnn_news_recommendation_amd import helpers
    torch = pytest.importorskip("torch")
    model = helpers.GRUUserModel.from_torch(torch.nn.GRU(4, 4))
    with pytest.raises(ValueError, match="max_events"):
        helpers.gru_user_states([[1, 2]], np.ones((3, 4), np.float32), model, max_events=1, all_states=True)
    with pytest.raises(ValueError, match="columns"):
        helpers.gru_user_states([[1, 2]], np.ones((3, 5), np.float32), model)
    with pytest.raises(ValueError, match="history items"):
        helpers.gru_user_states([[1, 3]], np.ones((3, 4), np.float32), model)
    with pytest.raises(ValueError, match="initial"):
        helpers.gru_user_states([[1, 2]], np.ones((3, 4), np.float32), model, initial=np.zeros((2, 4), np.float32))
    with pytest.raises(TypeError):
        helpers.gru_user_states([[1, 2]], np.ones((3, 4), np.float32), {"weight_ih": 1})


def test_gru_user_model_round_trips(tmp_path):
    import torch
    from dae_rnn_news_recommendation_amd.helpers import GRUUserModel
    torch.manual_seed(0)
    gru = torch.nn.GRU(6, 5)
    m = GRUUserModel.from_torch(gru)
    assert (m.input_size, m.hidden_size) == (6, 5)
    sd = gru.state_dict()
    for n in GRUUserModel.NAMES:
        a = getattr(m, n)
        assert a.dtype == np.float32 and a.flags.c_contiguous and np.array_equal(a, sd[n + "_l0"].numpy())
    m2 = GRUUserModel.from_torch(sd)                                   # the state dict
    path = str(tmp_path / "gru.npz")
    m.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(GRUUserModel.NAMES)
    m3 = GRUUserModel.load(path)
    for n in GRUUserModel.NAMES:
        assert np.array_equal(getattr(m2, n), getattr(m, n)) and np.array_equal(getattr(m3, n), getattr(m, n))
    m4 = GRUUserModel.from_torch(torch.nn.GRU(6, 5).double())          # float64 weights are rounded once
    assert m4.weight_ih.dtype == np.float32
    for bad in (torch.nn.GRU(6, 5, num_layers=2), torch.nn.GRU(6, 5, bidirectional=True), torch.nn.GRU(6, 5, bias=False),
                torch.nn.LSTM(6, 5)):
        with pytest.raises(ValueError):
            GRUUserModel.from_torch(bad)
    with pytest.raises(ValueError):
        GRUUserModel(np.zeros((15, 6)), np.zeros((15, 4)), np.zeros(15), np.zeros(15))
    with pytest.raises(ValueError):
        GRUUserModel(np.zeros((12, 6)), np.zeros((15, 5)), np.zeros(15), np.zeros(15))
    with pytest.raises(ValueError):
        GRUUserModel(np.zeros((15, 6)), np.zeros((15, 5)), np.zeros(14), np.zeros(15))
    np.savez(str(tmp_path / "short.npz"), weight_ih=m.weight_ih, weight_hh=m.weight_hh, bias_ih=m.bias_ih)
    with pytest.raises(ValueError, match="bias_hh"):
        GRUUserModel.load(str(tmp_path / "short.npz"))


@pytest.mark.parametrize("D, H", [(7, 5), (24, 24)])
def test_the_restatement_equals_torch_gru_in_float64(D, H):
    import torch
    torch.manual_seed(D)
    rng = np.random.default_rng(H)
    gru = torch.nn.GRU(D, H, batch_first=True).double()
    w = [p.detach().numpy() for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    E = rng.standard_normal((40, D))
    lengths = [0, 1, 2, 17, 60]
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    items = rng.integers(0, 40, indptr[-1])
    h0 = rng.standard_normal((len(lengths), H))
    for initial in (None, h0):
        every, last = gru_reference(E, *w, indptr, items, initial=initial)
        for u, n in enumerate(lengths):
            start = torch.zeros(1, 1, H, dtype=torch.float64) if initial is None else torch.from_numpy(h0[u]).reshape(1, 1, H)
            if n == 0:
                assert np.array_equal(last[u], start.numpy().ravel())
                continue
            with torch.no_grad():
                out, hn = gru(torch.from_numpy(E[items[indptr[u]:indptr[u + 1]]])[None], start)
            assert np.abs(out[0].numpy() - every[indptr[u]:indptr[u + 1]]).max() <= 1e-12
            assert np.abs(hn[0, 0].numpy() - last[u]).max() <= 1e-12


def test_gru_fit_torch_writes_a_loadable_model(tmp_path):
    """Two epochs of tools/gru_fit_torch.py on about 50 users on the CPU: the file is what GRUUserModel.load accepts."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gru_fit_torch
    finally:
        sys.path.pop(0)
    from dae_rnn_news_recommendation_amd.helpers import GRUUserModel
    out = str(tmp_path / "gru.npz")
    assert gru_fit_torch.main(["--synthetic", "200x16", "--users", "50", "--epochs", "2", "--batch_users", "16", "--out", out,
                               "--device", "cpu"]) == 0
    m = GRUUserModel.load(out)
    assert (m.input_size, m.hidden_size) == (16, 16)
    assert all(np.isfinite(getattr(m, n)).all() for n in GRUUserModel.NAMES)
    assert np.abs(m.weight_hh).max() > 0
