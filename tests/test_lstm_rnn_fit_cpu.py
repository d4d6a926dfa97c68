"""CPU checks of the LSTM and plain-RNN trainers (dae_lstm_pair_loss, dae_rnn_pair_loss, their workspace functions,
helpers.lstm_pair_loss / rnn_pair_loss, helpers.fit_lstm_user_model / fit_rnn_user_model).

``lstm_bptt_reference`` and ``rnn_bptt_reference`` below restate the definition of include/dae_hip.h in NumPy -- forward over every
history without its last event, the pairwise ranking loss, back-propagation through time -- in float64 or, with
``dtype=np.float32``, in float32 (the yardstick of tests/test_hip_lstm_rnn_fit.py).  Here they are pinned two ways: against
torch.nn.LSTM / torch.nn.RNN with autograd in float64, and against central finite differences of their own loss; those tests touch
no code of the package.  The rest: both builds export the four symbols under the unchanged ABI version, every argument error is
reported before any HIP call with the entry point's prefix, a call without users needs no workspace, the workspace is the header's
formula, and the Python entry points refuse bad inputs before the library is loaded."""
import ctypes

import numpy as np
import pytest

P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case that uses it fails the argument checks first
CELLS = ("lstm", "rnn")
GATES = {"lstm": 4, "rnn": 1}


def _pairs(E, items, negatives, e, hn, dtype, margins):
    """The loss terms of event e, predicted by the state hn: (loss sum, pair count, G = d loss / d hn); writes the margins."""
    one = dtype(1)
    G, pos = np.zeros(hn.shape, dtype), E[items[e]]
    loss, n = 0.0, 0
    for j in range(negatives.shape[1]):
        ng = int(negatives[e, j])
        if ng >= 0 and ng != items[e]:
            d = pos - E[ng]
            x = dtype(hn @ d)
            margins[e, j] = x
            ee = np.exp(-np.abs(x))
            loss += float(np.maximum(-x, dtype(0)) + np.log1p(ee))
            n += 1
            G += -(ee / (one + ee) if x >= 0 else one / (one + ee)) * d      # -sigmoid(-x)
    return loss, n, G


def lstm_bptt_reference(E, w_ih, w_hh, b_ih, b_hh, indptr, items, negatives, dtype=np.float64):
    """``(loss, n_pairs, margins [nnz x n_neg], dW_ih, dW_hh, db_ih, db_hh)`` in ``dtype`` (gate row blocks i, f, g, o); the loss of
    a pair is computed in ``dtype`` and added up in float64, as the library does."""
    E, w_ih, w_hh, b_ih, b_hh = (np.asarray(a, dtype) for a in (E, w_ih, w_hh, b_ih, b_hh))
    negatives = np.asarray(negatives)
    H = w_hh.shape[1]
    one = dtype(1)
    sig = lambda v: one / (one + np.exp(-v))
    gi_all = E @ w_ih.T + b_ih
    loss, n_pairs = 0.0, 0
    margins = np.zeros(negatives.shape, dtype)
    dW_ih, dW_hh, db_ih, db_hh = np.zeros_like(w_ih), np.zeros_like(w_hh), np.zeros_like(b_ih), np.zeros_like(b_hh)
    for u in range(len(indptr) - 1):
        e0, e1 = int(indptr[u]), int(indptr[u + 1])
        h, c, stash = np.zeros(H, dtype), np.zeros(H, dtype), []
        for e in range(e0, e1 - 1):                                      # the state after the last event predicts nothing
            a = gi_all[items[e]] + (w_hh @ h + b_hh)
            i, f, g, o = sig(a[:H]), sig(a[H:2 * H]), np.tanh(a[2 * H:3 * H]), sig(a[3 * H:])
            cn = f * c + i * g
            hn = o * np.tanh(cn)
            stash.append((h, c, i, f, g, o, cn, hn))
            h, c = hn, cn
        carry_h, carry_c = np.zeros(H, dtype), np.zeros(H, dtype)
        for k in reversed(range(len(stash))):
            hp, cp, i, f, g, o, cn, hn = stash[k]
            e = e0 + k + 1                                               # the event this state predicts
            l, n, G = _pairs(E, items, negatives, e, hn, dtype, margins)
            loss += l
            n_pairs += n
            dh = G + carry_h
            tc = np.tanh(cn)
            dc = dh * o * (one - tc * tc) + carry_c
            da = np.concatenate([dc * g * i * (one - i), dc * cp * f * (one - f), dc * i * (one - g * g), dh * tc * o * (one - o)])
            carry_c = dc * f
            carry_h = da @ w_hh
            dW_ih += np.outer(da, E[items[e - 1]])
            dW_hh += np.outer(da, hp)
            db_ih += da
            db_hh += da
    return loss, n_pairs, margins, dW_ih, dW_hh, db_ih, db_hh


def rnn_bptt_reference(E, w_ih, w_hh, b_ih, b_hh, indptr, items, negatives, dtype=np.float64):
    """The same for the plain tanh RNN: ``(loss, n_pairs, margins, dW_ih, dW_hh, db_ih, db_hh)`` in ``dtype``."""
    E, w_ih, w_hh, b_ih, b_hh = (np.asarray(a, dtype) for a in (E, w_ih, w_hh, b_ih, b_hh))
    negatives = np.asarray(negatives)
    H = w_hh.shape[1]
    one = dtype(1)
    gi_all = E @ w_ih.T + b_ih
    loss, n_pairs = 0.0, 0
    margins = np.zeros(negatives.shape, dtype)
    dW_ih, dW_hh, db_ih, db_hh = np.zeros_like(w_ih), np.zeros_like(w_hh), np.zeros_like(b_ih), np.zeros_like(b_hh)
    for u in range(len(indptr) - 1):
        e0, e1 = int(indptr[u]), int(indptr[u + 1])
        h, stash = np.zeros(H, dtype), []
        for e in range(e0, e1 - 1):
            hn = np.tanh(gi_all[items[e]] + (w_hh @ h + b_hh))
            stash.append((h, hn))
            h = hn
        carry = np.zeros(H, dtype)
        for k in reversed(range(len(stash))):
            hp, hn = stash[k]
            e = e0 + k + 1
            l, n, G = _pairs(E, items, negatives, e, hn, dtype, margins)
            loss += l
            n_pairs += n
            da = (G + carry) * (one - hn * hn)
            carry = da @ w_hh
            dW_ih += np.outer(da, E[items[e - 1]])
            dW_hh += np.outer(da, hp)
            db_ih += da
            db_hh += da
    return loss, n_pairs, margins, dW_ih, dW_hh, db_ih, db_hh


REFERENCE = {"lstm": lstm_bptt_reference, "rnn": rnn_bptt_reference}


def _module(cell, H):
    import torch
    return {"lstm": torch.nn.LSTM, "rnn": torch.nn.RNN}[cell](H, H, batch_first=True)


def small_case(cell, H, seed=0, Na=30, n_neg=3):
    """About 12 users of lengths 0 to 9, with negatives that are -1 and the clicked article here and there."""
    import torch
    rng = np.random.default_rng(seed + H)
    torch.manual_seed(seed + H)
    net = _module(cell, H).double()
    w = [p.detach().numpy().copy() for p in (net.weight_ih_l0, net.weight_hh_l0, net.bias_ih_l0, net.bias_hh_l0)]
    E = rng.standard_normal((Na, H))
    n = np.array([0, 1, 2, 3, 9, 5, 0, 7, 2, 1, 4, 6])
    indptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    items = rng.integers(0, Na, indptr[-1])
    neg = rng.integers(0, Na, (indptr[-1], n_neg))
    neg[rng.random(neg.shape) < 0.15] = -1
    hit = np.flatnonzero(rng.random(indptr[-1]) < 0.2)
    neg[hit, 0] = items[hit]
    return net, w, E, indptr, items, neg


def _torch_loss(net, E, indptr, items, neg, dtype):
    """The same loss through the torch.nn module, user by user; returns (loss tensor, n_pairs, margins)."""
    import torch
    E_t = torch.as_tensor(E, dtype=dtype)
    loss, pairs = torch.zeros((), dtype=torch.float64), 0
    margins = np.zeros(neg.shape, E_t.numpy().dtype)
    for u in range(len(indptr) - 1):
        e0, e1 = int(indptr[u]), int(indptr[u + 1])
        if e1 - e0 < 2:
            continue
        states, _ = net(E_t[torch.as_tensor(items[e0:e1 - 1])][None])
        for k in range(e1 - e0 - 1):
            e = e0 + k + 1
            for j in range(neg.shape[1]):
                if neg[e, j] >= 0 and neg[e, j] != items[e]:
                    x = (states[0, k] * (E_t[items[e]] - E_t[neg[e, j]])).sum()
                    margins[e, j] = float(x.detach())
                    loss = loss + torch.nn.functional.softplus(-x).double()
                    pairs += 1
    return loss, pairs, margins


@pytest.mark.parametrize("H", [5, 16])
@pytest.mark.parametrize("cell", CELLS)
def test_the_restatement_equals_torch_autograd_in_float64(cell, H):
    import torch
    net, w, E, indptr, items, neg = small_case(cell, H)
    loss, n_pairs, margins, *grads = REFERENCE[cell](E, *w, indptr, items, neg)
    t_loss, t_pairs, t_margins = _torch_loss(net, E, indptr, items, neg, torch.float64)
    t_loss.backward()
    assert n_pairs == t_pairs > 20
    assert abs(loss - float(t_loss.detach())) <= 1e-10 * abs(float(t_loss.detach()))
    assert np.abs(margins - t_margins).max() <= 1e-10 * np.abs(t_margins).max()
    # no pair at a user's first event, at a negative of -1, at the clicked article
    firsts = indptr[:-1][np.diff(indptr) > 0]
    assert (margins[firsts] == 0).all() and (margins[neg < 0] == 0).all() and (margins[neg == items[:, None]] == 0).all()
    for g, p in zip(grads, (net.weight_ih_l0, net.weight_hh_l0, net.bias_ih_l0, net.bias_hh_l0)):
        want = p.grad.numpy()
        assert g.shape == want.shape == ((GATES[cell] * H, H) if want.ndim == 2 else (GATES[cell] * H,))
        assert np.abs(g - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("H", [5, 16])
@pytest.mark.parametrize("cell", CELLS)
def test_the_restatement_equals_central_differences(cell, H):
    _, w, E, indptr, items, neg = small_case(cell, H, seed=1)
    ref = REFERENCE[cell]
    _, _, _, *grads = ref(E, *w, indptr, items, neg)
    rng = np.random.default_rng(H)
    eps = 1e-6
    for k, g in enumerate(grads):
        for _ in range(5):
            at = tuple(int(rng.integers(0, s)) for s in g.shape)
            lo, hi = [a.copy() for a in w], [a.copy() for a in w]
            lo[k][at] -= eps
            hi[k][at] += eps
            fd = (ref(E, *hi, indptr, items, neg)[0] - ref(E, *lo, indptr, items, neg)[0]) / (2 * eps)
            assert abs(fd - g[at]) <= 1e-6 * max(np.abs(g).max(), 1.0), (k, at, fd, g[at])


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_fit_symbols_are_exported_and_the_abi_version_stays(fmt):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load(fmt)
    for cell in CELLS:
        for name in ("dae_%s_pair_loss" % cell, "dae_%s_pair_loss_workspace" % cell):
            assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES["dae_%s_pair_loss" % cell] == _lib.SIGNATURES["dae_gru_pair_loss"]        # argument for argument
        assert _lib.SIGNATURES["dae_%s_pair_loss_workspace" % cell] == _lib.SIGNATURES["dae_gru_pair_loss_workspace"]
    assert lib.dae_abi_version() == _lib.ABI_VERSION == 9


def _fit(lib, cell, E=P, lde=48, Na=100, H=48, W_ih=P, ldwi=48, W_hh=P, ldwh=48, b_ih=P, b_hh=P, indptr=P, items=P, order=P, M=10, nnz=50,
         active=(10, 8, 3), T=None, negatives=P, n_neg=4, loss=P, n_pairs=P, dW_ih=P, ld_dwi=48, dW_hh=P, ld_dwh=48, db_ih=P, db_hh=P,
         margin=None, ws=P, ws_bytes=None):
    T = (0 if active is None else len(active)) if T is None else T
    if ws_bytes is None:
        ws_bytes = getattr(lib, "dae_%s_pair_loss_workspace" % cell)(max(Na, 1), max(H, 1), max(M, 0), max(nnz, 0), max(T, 0),
                                                                      min(max(n_neg, 1), 16))
    act = None if active is None else (ctypes.c_int64 * len(active))(*active)
    return getattr(lib, "dae_%s_pair_loss" % cell)(E, lde, Na, H, W_ih, ldwi, W_hh, ldwh, b_ih, b_hh, indptr, items, order, M, nnz, T, act,
                                                   negatives, n_neg, loss, n_pairs, dW_ih, ld_dwi, dW_hh, ld_dwh, db_ih, db_hh, margin, ws,
                                                   ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(E=None), b"E / indptr are NULL"),
    (dict(indptr=None), b"E / indptr are NULL"),
    (dict(W_ih=None), b"W_ih / W_hh / b_ih / b_hh are NULL"),
    (dict(W_hh=None), b"W_ih / W_hh / b_ih / b_hh are NULL"),
    (dict(b_ih=None), b"W_ih / W_hh / b_ih / b_hh are NULL"),
    (dict(b_hh=None), b"W_ih / W_hh / b_ih / b_hh are NULL"),
    (dict(items=None), b"items / negatives are NULL"),
    (dict(negatives=None), b"items / negatives are NULL"),
    (dict(order=None), b"order is NULL"),
    (dict(active=None, T=3), b"active_host is NULL"),
    (dict(loss=None), b"loss / n_pairs are NULL"),
    (dict(n_pairs=None), b"loss / n_pairs are NULL"),
    (dict(dW_ih=None), b"dW_ih / dW_hh / db_ih / db_hh are NULL"),
    (dict(dW_hh=None), b"dW_ih / dW_hh / db_ih / db_hh are NULL"),
    (dict(db_ih=None), b"dW_ih / dW_hh / db_ih / db_hh are NULL"),
    (dict(db_hh=None), b"dW_ih / dW_hh / db_ih / db_hh are NULL"),
    (dict(n_neg=0), b"n_neg must be in 1..16 (got 0)"),
    (dict(n_neg=17), b"n_neg must be in 1..16 (got 17)"),
    (dict(Na=0), b"must be positive"),
    (dict(H=-2), b"must be positive"),
    (dict(M=-1), b"negative count"),
    (dict(nnz=-1), b"negative count"),
    (dict(T=-1), b"negative count"),
    (dict(lde=47), b"lde (47)"),
    (dict(ldwi=10), b"ldwi (10) must be >= H"),
    (dict(ldwh=47), b"ldwh (47)"),
    (dict(ld_dwi=47), b"ld_dwi (47)"),
    (dict(ld_dwh=0), b"ld_dwh (0) must be >= H"),
    (dict(active=(10, 3, 8)), b"non-increasing"),
    (dict(active=(11, 8, 3)), b"at most M"),
    (dict(active=(10, 8, -1)), b"non-increasing"),
    (dict(active=(10, 10, 10, 10, 10, 1)), b"more than nnz"),
    (dict(ws=None), b"workspace too small"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
    (dict(ws=None, margin=P), b"workspace too small"),                 # before the first HIP call, which would clear the margins
    (dict(Na=9 * 10 ** 6, H=500, lde=500, ldwi=500, ldwh=500, ld_dwi=500, ld_dwh=500), b"exceeds 4 GiB"),          # the E image (RNN), P (LSTM)
    (dict(M=3 * 10 ** 6, H=500, lde=500, ldwi=500, ldwh=500, ld_dwi=500, ld_dwh=500, active=(10,)), b"exceeds 4 GiB"),   # the carry buffer
    (dict(H=40000, lde=40000, ldwi=40000, ldwh=40000, ld_dwi=40000, ld_dwh=40000), b"exceeds 4 GiB"),               # the W_hh image
    (dict(nnz=3 * 10 ** 6, H=500, lde=500, ldwi=500, ldwh=500, ld_dwi=500, ld_dwh=500), b"exceeds 4 GiB"),          # the stash
])
@pytest.mark.parametrize("cell", CELLS)
def test_fit_argument_errors_without_a_gpu(cell, kw, msg):
    lib = _lib()
    assert _fit(lib, cell, **kw) == 1
    err = lib.dae_last_error()
    assert err.startswith(b"%s_pair_loss: " % cell.encode()), err
    assert msg in err, err


@pytest.mark.parametrize("cell", CELLS)
def test_pair_loss_of_no_users_needs_no_workspace(cell):
    """M == 0 (and T == 0) passes every argument check with a NULL workspace and goes straight to writing the zero outputs: on a
    device they are written and the call returns 0; without one the first launch is what fails, not an argument check."""
    import torch
    lib = _lib()
    none = dict(M=0, nnz=0, items=None, negatives=None, order=None, active=None, ws=None, ws_bytes=0)
    if torch.cuda.is_available():
        H, G = 48, GATES[cell]
        out = [torch.full(s, 7.0, device="cuda") for s in ((G * H, H), (G * H, H), (G * H,), (G * H,))]
        scal = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = _fit(lib, cell, loss=p(scal), n_pairs=ctypes.c_void_p(scal.data_ptr() + 8), dW_ih=p(out[0]), dW_hh=p(out[1]), db_ih=p(out[2]),
                  db_hh=p(out[3]), **none)
        torch.cuda.synchronize()
        assert rc == 0, lib.dae_last_error()
        assert all((o == 0).all() for o in out) and (scal.cpu().numpy().view(np.int64) == 0).all()
    else:
        rc = _fit(lib, cell, **none)
        assert rc in (0, 2), lib.dae_last_error()                      # 1 would be an argument error


@pytest.mark.parametrize("cell", CELLS)
def test_fit_workspace_is_the_formula_of_the_header(cell):
    lib = _lib()
    ws = getattr(lib, "dae_%s_pair_loss_workspace" % cell)
    pad = lambda n: (n + 127) // 128 * 128
    al = lambda b: (b + 255) // 256 * 256
    G, images = GATES[cell], {"lstm": 13, "rnn": 6}[cell]
    for Na, H, M, nnz, T in ((300, 70, 306, 0, 0), (300, 70, 306, 5000, 130), (600, 160, 306, 5000, 130), (8000, 500, 4096, 200000, 50),
                             (1, 1, 1, 1, 1), (129, 129, 129, 1000, 7)):
        Hp, Rb = pad(H), pad(nnz + 128 * T)
        want = (al(4 * pad(Na) * Hp) + 3 * al(4 * G * Hp * Hp) + al(4 * G * pad(Na) * Hp) + images * al(4 * Rb * Hp)
                + (al(4 * pad(M) * Hp) if cell == "lstm" else 0) + 2 * al(8 * Rb) + al(4 * Rb) + al(64 * G * Hp * Hp))
        assert ws(Na, H, M, nnz, T, 4) == want, (Na, H, M, nnz, T)
        assert ws(Na, H, M, nnz, T, 1) == ws(Na, H, M, nnz, T, 16) == want
    assert ws(0, 10, 10, 10, 1, 4) == 0 and ws(10, 0, 10, 10, 1, 4) == 0 and ws(10, 10, -1, 10, 1, 4) == 0
    assert ws(10, 10, 10, 10, 1, 0) == 0 and ws(10, 10, 10, 10, 1, 17) == 0


@pytest.mark.parametrize("cell", CELLS)
def test_python_entry_points_refuse_bad_inputs_before_the_library_is_loaded(cell, monkeypatch):
    import torch
    from dae_rnn_news_recommendation_amd import _lib, helpers

    def no_library(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    cls = {"lstm": helpers.LSTMUserModel, "rnn": helpers.RNNUserModel}[cell]
    other = {"lstm": helpers.RNNUserModel, "rnn": helpers.LSTMUserModel}[cell]
    mod, other_mod = {"lstm": (torch.nn.LSTM, torch.nn.RNN), "rnn": (torch.nn.RNN, torch.nn.LSTM)}[cell]
    pair_loss = getattr(helpers, "%s_pair_loss" % cell)
    fit = getattr(helpers, "fit_%s_user_model" % cell)
    torch.manual_seed(0)
    model = cls.from_torch(mod(4, 4))
    E = np.ones((3, 4), np.float32)
    hist, neg = [[1, 2, 0]], np.zeros((3, 2), np.int64)
    for wrong in (other.from_torch(other_mod(4, 4)), helpers.GRUUserModel.from_torch(torch.nn.GRU(4, 4)), {"weight_ih": 1}):
        with pytest.raises(TypeError, match=cls.__name__):
            pair_loss(hist, E, wrong, neg)
        with pytest.raises(TypeError, match=cls.__name__):
            fit(hist, E, init=wrong)
    with pytest.raises(ValueError, match="must equal the embedding size"):
        pair_loss(hist, np.ones((3, 5), np.float32), cls.from_torch(mod(5, 4)), neg)
    with pytest.raises(ValueError, match="columns"):
        pair_loss(hist, np.ones((3, 5), np.float32), model, neg)
    with pytest.raises(ValueError, match="history items"):
        pair_loss([[1, 3]], E, model, neg[:2])
    with pytest.raises(ValueError, match="negatives must be"):
        pair_loss(hist, E, model, neg[:2])                              # one row per event
    with pytest.raises(ValueError, match="negatives must be"):
        pair_loss(hist, E, model, np.zeros((3, 17), np.int64))
    with pytest.raises(ValueError, match="negatives must be below"):
        pair_loss(hist, E, model, neg + 3)
    with pytest.raises(ValueError, match="history items"):
        fit([[1, 3]], E)
    with pytest.raises(ValueError, match="must equal the embedding size"):
        fit(hist, np.ones((3, 5), np.float32), init=cls.from_torch(mod(5, 4)))
    for n_neg in (0, 17):
        with pytest.raises(ValueError, match="n_neg must be in 1..16"):
            fit(hist, E, n_neg=n_neg)
    with pytest.raises(ValueError, match="batch_users"):
        fit(hist, E, batch_users=0)
    with pytest.raises(ValueError, match="keep_best needs validation"):
        fit(hist, E, keep_best=True)
    m = cls(model.weight_ih, model.weight_hh, model.bias_ih, model.bias_hh, history=np.array([1.0, 0.5]), validation=[{"epoch": 1}])
    assert m.history.tolist() == [1.0, 0.5] and m.validation == [{"epoch": 1}] and model.history is None and model.validation is None
