"""CPU checks of the LSTM and plain-RNN user states (dae_lstm_user_states, dae_rnn_user_states and their _workspace functions) and
of the host code around them: both builds export the four symbols under an unchanged ABI version, every argument error is
reported before any HIP call (so on a machine without a GPU), the workspaces follow the header's formula, and LSTMUserModel /
RNNUserModel on hand-made cases.  ``lstm_reference`` and ``rnn_reference`` below are the float64 (or, with ``dtype=np.float32``,
float32) NumPy restatements of the recurrences that tests/test_hip_lstm_rnn.py takes as the truth; here they are pinned to
independent implementations, torch.nn.LSTM and torch.nn.RNN in float64."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first


def lstm_reference(E, w_ih, w_hh, b_ih, b_hh, indptr, items, initial=None, dtype=np.float64):
    """The LSTM recurrence of include/dae_hip.h, event by event, in ``dtype``: (h after every event [nnz x H], last h [M x H],
    last c [M x H]).  ``initial``: None or a pair (h, c) of [M x H], either of which may be None.

        i, f, o = sigmoid(W_i. x + b_i. + W_h. h + b_h.)   g = tanh(W_ig x + b_ig + W_hg h + b_hg)   c' = f * c + i * g   h' = o * tanh(c')
    """
    E, w_ih, w_hh, b_ih, b_hh = (np.asarray(a, dtype) for a in (E, w_ih, w_hh, b_ih, b_hh))
    H, M = w_hh.shape[1], len(indptr) - 1
    one = dtype(1)
    sig = lambda v: one / (one + np.exp(-v))
    h0, c0 = (None, None) if initial is None else initial
    gi_all = E @ w_ih.T + b_ih                                          # per article
    every, last, cell = np.zeros((len(items), H), dtype), np.zeros((M, H), dtype), np.zeros((M, H), dtype)
    for u in range(M):
        h = np.zeros(H, dtype) if h0 is None else np.asarray(h0[u], dtype)
        c = np.zeros(H, dtype) if c0 is None else np.asarray(c0[u], dtype)
        for e in range(indptr[u], indptr[u + 1]):
            a = gi_all[items[e]] + (w_hh @ h + b_hh)
            i, f, g, o = sig(a[:H]), sig(a[H:2 * H]), np.tanh(a[2 * H:3 * H]), sig(a[3 * H:])
            c = f * c + i * g
            h = o * np.tanh(c)
            every[e] = h
        last[u], cell[u] = h, c
    return every, last, cell


def rnn_reference(E, w_ih, w_hh, b_ih, b_hh, indptr, items, initial=None, dtype=np.float64):
    """The plain-RNN recurrence of include/dae_hip.h, event by event, in ``dtype``: (h after every event [nnz x H], last h [M x H]).

        h' = tanh(W_ih x + b_ih + W_hh h + b_hh)
    """
    E, w_ih, w_hh, b_ih, b_hh = (np.asarray(a, dtype) for a in (E, w_ih, w_hh, b_ih, b_hh))
    H, M = w_hh.shape[1], len(indptr) - 1
    gi_all = E @ w_ih.T + b_ih
    every, last = np.zeros((len(items), H), dtype), np.zeros((M, H), dtype)
    for u in range(M):
        h = np.zeros(H, dtype) if initial is None else np.asarray(initial[u], dtype)
        for e in range(indptr[u], indptr[u + 1]):
            h = np.tanh(gi_all[items[e]] + (w_hh @ h + b_hh))
            every[e] = h
        last[u] = h
    return every, last


CELLS = ("lstm", "rnn")
GATES = {"lstm": 4, "rnn": 1}
SYMBOLS = ("dae_lstm_user_states", "dae_lstm_user_states_workspace", "dae_rnn_user_states", "dae_rnn_user_states_workspace")


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


def _header_arity(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dae_hip.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_symbols_are_exported_and_the_abi_version_stays(fmt):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load(fmt)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == _header_arity(name) == len(getattr(lib, name).argtypes), name
    assert lib.dae_abi_version() == _lib.ABI_VERSION == 9
    assert len(_lib.SIGNATURES["dae_rnn_user_states"][1]) == len(_lib.SIGNATURES["dae_gru_user_states"][1]) == 26
    assert _lib.SIGNATURES["dae_rnn_user_states"] == _lib.SIGNATURES["dae_gru_user_states"]
    assert len(_lib.SIGNATURES["dae_lstm_user_states"][1]) == 30
    assert _lib.SIGNATURES["dae_lstm_user_states_workspace"] == _lib.SIGNATURES["dae_rnn_user_states_workspace"] \
        == _lib.SIGNATURES["dae_gru_user_states_workspace"]


def _active(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _call(lib, cell, E=P, lde=64, Na=100, D=64, H=48, W_ih=P, ldwi=64, W_hh=P, ldwh=48, b_ih=P, b_hh=P, indptr=P, items=P, order=P, M=10,
          nnz=50, active=(10, 8, 3), T=None, h0=None, ldh0=0, c0=None, ldc0=0, all_states=0, U=P, ldu=48, C=None, ldc=0, ws=P,
          ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = getattr(lib, "dae_%s_user_states_workspace" % cell)(max(Na, 0), max(D, 0), max(H, 0), max(M, 0))
    act = None if active is None else _active(*active)
    T = (0 if active is None else len(active)) if T is None else T
    head = (E, lde, Na, D, H, W_ih, ldwi, W_hh, ldwh, b_ih, b_hh, indptr, items, order, M, nnz, T, act, h0, ldh0)
    if cell == "lstm":
        return lib.dae_lstm_user_states(*head, c0, ldc0, all_states, U, ldu, C, ldc, ws, ws_bytes, None)
    return lib.dae_rnn_user_states(*head, all_states, U, ldu, ws, ws_bytes, None)


ERRORS = [
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
    (dict(H=40000, ldwh=40000, ldu=40000), b"exceeds 4 GiB"),                      # the W_hh image, one gate block or four
]
LSTM_ERRORS = [
    (dict(c0=P, ldc0=47), b"must be >= H"),
    (dict(C=P, ldc=47), b"must be >= H"),
    (dict(h0=P, ldh0=48, c0=P, ldc0=0), b"must be >= H"),
    # the four-gate images: each of these passes as one gate block (the RNN accepts the shape) and fails as four
    (dict(H=20000, ldwh=20000, ldu=20000), b"exceeds 4 GiB"),                      # 4 Hp x Hp
    (dict(H=2000, D=200000, lde=200000, ldwi=200000, ldwh=2000, ldu=2000, Na=100), b"exceeds 4 GiB"),     # 4 Hp x Dp
    (dict(Na=300000, H=1000, ldwh=1000, ldu=1000), b"exceeds 4 GiB"),             # Nap x 4 Hp
]


@pytest.mark.parametrize("cell, kw, msg", [(c, kw, msg) for c in CELLS for kw, msg in ERRORS] + [("lstm", kw, msg) for kw, msg in LSTM_ERRORS])
def test_argument_errors_without_a_gpu(cell, kw, msg):
    lib = _lib()
    assert _call(lib, cell, **kw) != 0
    err = lib.dae_last_error()
    assert msg in err and (cell + "_user_states: ").encode() in err, err


def test_the_four_gate_cases_are_one_gate_shapes_the_rnn_takes():
    """The three 4 GiB cases of the LSTM's four-gate images are below the limit with one gate block: there the RNN gets past the
    image check and stops at the next one (the workspace), still before any HIP call."""
    lib = _lib()
    for kw, _ in LSTM_ERRORS[3:]:
        assert _call(lib, "rnn", ws_bytes=1024, **kw) != 0
        assert b"workspace too small" in lib.dae_last_error(), lib.dae_last_error()


@pytest.mark.parametrize("cell", CELLS)
def test_states_of_no_users_is_a_no_op(cell):
    lib = _lib()
    assert _call(lib, cell, M=0, nnz=0, items=None, order=None, U=None, active=None, ws=None, ws_bytes=0) == 0   # returns before any HIP call


@pytest.mark.parametrize("cell", CELLS)
def test_workspace_follows_the_headers_formula(cell):
    lib = _lib()
    ws = getattr(lib, "dae_%s_user_states_workspace" % cell)
    assert len(ws.argtypes) == 4                                        # (Na, D, H, M): the number of events is not an argument
    pad = lambda n: (n + 127) // 128 * 128
    al = lambda b: (b + 255) // 256 * 256
    G, S = GATES[cell], 3 if cell == "lstm" else 2
    for Na, D, H, M in ((300, 70, 70, 306), (1000, 500, 500, 1), (400, 96, 160, 100000), (8000, 500, 500, 262144)):
        Nap, Dp, Hp, Mp = pad(Na), pad(D), pad(H), pad(M)
        want = al(4 * Nap * Dp) + al(4 * G * Hp * Dp) + al(4 * G * Hp * Hp) + al(4 * G * Nap * Hp) + S * al(4 * Mp * Hp)
        assert ws(Na, D, H, M) == want
    # linear in the users: equal steps of M give equal growth
    a, b, c = (ws(8000, 500, 500, n * 128 * 1024) for n in (1, 2, 3))
    assert c - b == b - a == S * 128 * 1024 * 512 * 4
    assert ws(0, 10, 10, 10) == 0 and ws(10, 0, 10, 10) == 0 and ws(10, 10, 0, 10) == 0 and ws(10, 10, 10, -1) == 0
    assert ws(10, 10, 10, 0) > 0


def _module(cell, D, H, **kw):
    import torch
    return (torch.nn.LSTM if cell == "lstm" else torch.nn.RNN)(D, H, **kw)


def _cls(cell):
    from dae_rnn_news_recommendation_amd import helpers
    return helpers.LSTMUserModel if cell == "lstm" else helpers.RNNUserModel


@pytest.mark.parametrize("cell", CELLS)
def test_user_model_round_trips(cell, tmp_path):
    import torch
    cls, G = _cls(cell), GATES[cell]
    torch.manual_seed(0)
    mod = _module(cell, 6, 5)
    m = cls.from_torch(mod)
    assert (m.input_size, m.hidden_size) == (6, 5)
    assert cls.NAMES == ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    assert m.weight_ih.shape == (G * 5, 6) and m.weight_hh.shape == (G * 5, 5) and m.bias_ih.shape == m.bias_hh.shape == (G * 5,)
    sd = mod.state_dict()
    for n in cls.NAMES:
        a = getattr(m, n)
        assert a.dtype == np.float32 and a.flags.c_contiguous and np.array_equal(a, sd[n + "_l0"].numpy())
    m2 = cls.from_torch(sd)                                             # the state dict
    path = str(tmp_path / "w.npz")
    m.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(cls.NAMES)
    m3 = cls.load(path)
    for n in cls.NAMES:
        assert np.array_equal(getattr(m2, n), getattr(m, n)) and np.array_equal(getattr(m3, n), getattr(m, n))
    assert cls.from_torch(_module(cell, 6, 5).double()).weight_ih.dtype == np.float32      # float64 weights are rounded once
    assert callable(m.states)
    # shapes and finiteness
    with pytest.raises(ValueError):
        cls(np.zeros((G * 5, 6)), np.zeros((G * 5, 4)), np.zeros(G * 5), np.zeros(G * 5))
    with pytest.raises(ValueError):
        cls(np.zeros((G * 5 + 1, 6)), np.zeros((G * 5, 5)), np.zeros(G * 5), np.zeros(G * 5))
    with pytest.raises(ValueError):
        cls(np.zeros((G * 5, 6)), np.zeros((G * 5, 5)), np.zeros(G * 5 - 1), np.zeros(G * 5))
    with pytest.raises(ValueError, match="finite"):
        cls(np.full((G * 5, 6), np.nan), np.zeros((G * 5, 5)), np.zeros(G * 5), np.zeros(G * 5))
    np.savez(str(tmp_path / "short.npz"), weight_ih=m.weight_ih, weight_hh=m.weight_hh, bias_ih=m.bias_ih)
    with pytest.raises(ValueError, match="bias_hh"):
        cls.load(str(tmp_path / "short.npz"))


@pytest.mark.parametrize("cell", CELLS)
def test_from_torch_and_load_refuse_what_is_not_the_cell(cell, tmp_path):
    import torch
    from dae_rnn_news_recommendation_amd import helpers
    cls = _cls(cell)
    others = {"lstm": (torch.nn.GRU(6, 5), torch.nn.RNN(6, 5)), "rnn": (torch.nn.GRU(6, 5), torch.nn.LSTM(6, 5))}[cell]
    bad = list(others) + [_module(cell, 6, 5, num_layers=2), _module(cell, 6, 5, bidirectional=True), _module(cell, 6, 5, bias=False)]
    bad.append(torch.nn.LSTM(6, 5, proj_size=3) if cell == "lstm" else torch.nn.RNN(6, 5, nonlinearity="relu"))
    for b in bad:
        with pytest.raises(ValueError):
            cls.from_torch(b)
    for b in bad[:4] + ([bad[5]] if cell == "lstm" else []):           # their state dicts too: other shapes or other entries
        with pytest.raises(ValueError):
            cls.from_torch(b.state_dict())
    with pytest.raises(ValueError):
        helpers.GRUUserModel.from_torch(_module(cell, 6, 5))
    # a weight file of another cell: weight_hh has the wrong row multiple
    for name, other in (("gru", helpers.GRUUserModel.from_torch(torch.nn.GRU(6, 5))),
                        ("lstm", helpers.LSTMUserModel.from_torch(torch.nn.LSTM(6, 5))),
                        ("rnn", helpers.RNNUserModel.from_torch(torch.nn.RNN(6, 5)))):
        path = str(tmp_path / (name + ".npz"))
        other.save(path)
        if name == cell:
            assert cls.load(path).hidden_size == 5
        else:
            with pytest.raises(ValueError, match="weight_hh"):
                cls.load(path)


def test_the_states_functions_refuse_bad_arguments_before_any_device_work():
    import torch
    from dae_rnn_news_recommendation_amd import helpers
    E = np.ones((3, 4), np.float32)
    for cell, fn in (("lstm", helpers.lstm_user_states), ("rnn", helpers.rnn_user_states)):
        model = _cls(cell).from_torch(_module(cell, 4, 4))
        with pytest.raises(ValueError, match="max_events"):
            fn([[1, 2]], E, model, max_events=1, all_states=True)
        with pytest.raises(ValueError, match="columns"):
            fn([[1, 2]], np.ones((3, 5), np.float32), model)
        with pytest.raises(ValueError, match="history items"):
            fn([[1, 3]], E, model)
        with pytest.raises(TypeError):
            fn([[1, 2]], E, helpers.GRUUserModel.from_torch(torch.nn.GRU(4, 4)))
        with pytest.raises(TypeError):
            fn([[1, 2]], E, {"weight_ih": 1})
    lstm, rnn = (_cls(c).from_torch(_module(c, 4, 4)) for c in CELLS)
    with pytest.raises(TypeError):
        helpers.gru_user_states([[1, 2]], E, lstm)
    with pytest.raises(ValueError, match="initial"):
        helpers.rnn_user_states([[1, 2]], E, rnn, initial=np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match="initial"):
        helpers.lstm_user_states([[1, 2]], E, lstm, initial=(np.zeros((2, 4), np.float32), None))
    with pytest.raises(ValueError, match="initial c"):
        helpers.lstm_user_states([[1, 2]], E, lstm, initial=(None, np.zeros((1, 3), np.float32)))
    with pytest.raises(ValueError, match="pair"):
        helpers.lstm_user_states([[1, 2]], E, lstm, initial=np.zeros((1, 4), np.float32))


def _torch_case(D, H):
    rng = np.random.default_rng(H)
    E = rng.standard_normal((40, D))
    lengths = [0, 1, 2, 17, 60]
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    items = rng.integers(0, 40, indptr[-1])
    return rng, E, lengths, indptr, items


@pytest.mark.parametrize("D, H", [(5, 7), (12, 12)])
def test_the_lstm_restatement_equals_torch_lstm_in_float64(D, H):
    import torch
    torch.manual_seed(D)
    rng, E, lengths, indptr, items = _torch_case(D, H)
    lstm = torch.nn.LSTM(D, H, batch_first=True).double()
    w = [p.detach().numpy() for p in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)]
    h0, c0 = rng.standard_normal((len(lengths), H)), rng.standard_normal((len(lengths), H))
    for initial in (None, (h0, c0), (h0, None), (None, c0)):
        every, last, cell = lstm_reference(E, *w, indptr, items, initial=initial)
        for u, n in enumerate(lengths):
            hs, cs = ((torch.zeros(1, 1, H, dtype=torch.float64) if initial is None or initial[k] is None
                       else torch.from_numpy(initial[k][u]).reshape(1, 1, H)) for k in (0, 1))
            if n == 0:
                assert np.array_equal(last[u], hs.numpy().ravel()) and np.array_equal(cell[u], cs.numpy().ravel())
                continue
            with torch.no_grad():
                out, (hn, cn) = lstm(torch.from_numpy(E[items[indptr[u]:indptr[u + 1]]])[None], (hs, cs))
            assert np.abs(out[0].numpy() - every[indptr[u]:indptr[u + 1]]).max() <= 1e-12
            assert np.abs(hn[0, 0].numpy() - last[u]).max() <= 1e-12
            assert np.abs(cn[0, 0].numpy() - cell[u]).max() <= 1e-12


@pytest.mark.parametrize("D, H", [(5, 7), (12, 12)])
def test_the_rnn_restatement_equals_torch_rnn_in_float64(D, H):
    import torch
    torch.manual_seed(D)
    rng, E, lengths, indptr, items = _torch_case(D, H)
    rnn = torch.nn.RNN(D, H, batch_first=True).double()
    w = [p.detach().numpy() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)]
    h0 = rng.standard_normal((len(lengths), H))
    for initial in (None, h0):
        every, last = rnn_reference(E, *w, indptr, items, initial=initial)
        for u, n in enumerate(lengths):
            start = torch.zeros(1, 1, H, dtype=torch.float64) if initial is None else torch.from_numpy(h0[u]).reshape(1, 1, H)
            if n == 0:
                assert np.array_equal(last[u], start.numpy().ravel())
                continue
            with torch.no_grad():
                out, hn = rnn(torch.from_numpy(E[items[indptr[u]:indptr[u + 1]]])[None], start)
            assert np.abs(out[0].numpy() - every[indptr[u]:indptr[u + 1]]).max() <= 1e-12
            assert np.abs(hn[0, 0].numpy() - last[u]).max() <= 1e-12


@pytest.mark.parametrize("cell", CELLS)
def test_gru_fit_torch_writes_a_loadable_model_of_the_cell(cell, tmp_path):
    """One epoch of tools/gru_fit_torch.py --cell on 50 users on the CPU: the file is what the matching class loads, and no other."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gru_fit_torch
    finally:
        sys.path.pop(0)
    from dae_rnn_news_recommendation_amd import helpers
    cls = _cls(cell)
    out = str(tmp_path / "w.npz")
    assert gru_fit_torch.main(["--cell", cell, "--synthetic", "200x16", "--users", "50", "--epochs", "1", "--out", out, "--device", "cpu"]) == 0
    m = cls.load(out)
    assert (m.input_size, m.hidden_size) == (16, 16) and m.weight_hh.shape == (GATES[cell] * 16, 16)
    assert all(np.isfinite(getattr(m, n)).all() for n in cls.NAMES)
    assert np.abs(m.weight_hh).max() > 0
    with pytest.raises(ValueError):
        helpers.GRUUserModel.load(out)
