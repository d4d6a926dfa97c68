"""GPU checks of the LSTM and plain-RNN trainers (dae_lstm_pair_loss / dae_rnn_pair_loss through helpers.lstm_pair_loss /
rnn_pair_loss, helpers.fit_lstm_user_model / fit_rnn_user_model and the CLI's --fit_cell).

Truth: ``lstm_bptt_reference`` / ``rnn_bptt_reference`` of tests/test_lstm_rnn_fit_cpu.py in float64 (there pinned to torch autograd
in float64 and to finite differences).  Yardstick: the same restatement in NumPy float32 on the same inputs.  For each of the four
gradients, for the margins and for the loss, the figure is the worst absolute error divided by the largest magnitude of the truth,
and the kernel's figure must stay within a fixed multiple of the yardstick's.  The multiple is derived as tests/test_hip_gru_fit.py
derives its own: torch.nn.LSTM / torch.nn.RNN with autograd in float32 on the CPU, on these inputs (``torch_float32_ratios`` below
recomputes the table); four times its worst ratio to the yardstick over both cells and both shapes, rounded up to a power of two --
for the margins and the four gradients together, and separately for the loss, which is ONE number (the float64 sum of some 4000
float32-rounded terms) whose yardstick figure is an accident of cancellation, as that file's docstring explains.  The table below
was computed on the CPU before any device run; the bounds were fixed from its torch rows alone.

    ratio to the yardstick                  loss    margins  weight_ih  weight_hh  bias_ih  bias_hh
    lstm (300, 70)    torch float32, CPU    0.013   1.393    0.607      0.471      0.481    0.481
                      dae_lstm_pair_loss    0.115   0.798    0.600      0.452      0.180    0.180      (one MI355X)
    lstm (600, 160)   torch float32, CPU    0.240   1.447    0.354      0.315      0.676    0.676
                      dae_lstm_pair_loss    0.140   0.863    0.490      0.263      0.250    0.250
    rnn  (300, 70)    torch float32, CPU    0.456   1.724    0.422      1.113      0.695    1.286
                      dae_rnn_pair_loss     0.383   1.069    0.380      0.494      0.283    0.283
    rnn  (600, 160)   torch float32, CPU    0.085   0.950    0.385      1.782      0.258    0.555
                      dae_rnn_pair_loss     0.716   0.949    0.689      0.490      0.204    0.204
    the users permuted, and the sum of two half batches: margins and gradients between 0.180 and 1.069, the loss as above

Over the margins and the four gradients torch sits at 1.782 x at worst: BOUND = 8.  Over the loss at 0.456 x: LOSS_BOUND = 2 (here the
yardstick's own figures, 1.2e-8 to 2.4e-8, are what a random walk of that length gives, so the loss needs no multiple in the
thousands as the GRU file's does).

``n_pairs`` is exact.  Bit for bit: run to run, margins on or off, a strided E, and -- the users permuted -- the pair count and
the margins; the margins of the two halves of the batch, concatenated, are the bits of the whole batch's (a user's states do not
depend on the other users); the gradients of a permuted batch and the sum of the gradients of its two halves meet the accuracy
bound."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from test_hip_gru import _lengths
from test_lstm_rnn_fit_cpu import GATES, REFERENCE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = ("lstm", "rnn")
SHAPES = [(300, 70), (600, 160)]                                        # (articles, H): Hp = 128 and 256
BOUND = 8.0                                                             # margins and gradients: 4 x 1.782, rounded up to a power of two
LOSS_BOUND = 2.0                                                        # the loss: 4 x 0.456
QUANTITIES = ("loss", "margins", "weight_ih", "weight_hh", "bias_ih", "bias_hh")
CASES = [(cell, shape) for cell in CELLS for shape in SHAPES]


def _helpers(cell):
    from dae_rnn_news_recommendation_amd import helpers
    return (helpers, {"lstm": helpers.LSTMUserModel, "rnn": helpers.RNNUserModel}[cell], getattr(helpers, "%s_pair_loss" % cell),
            getattr(helpers, "fit_%s_user_model" % cell))


def _module(cell, H):
    return {"lstm": torch.nn.LSTM, "rnn": torch.nn.RNN}[cell](H, H, batch_first=True)


@functools.lru_cache(maxsize=None)
def _case(cell, shape):
    """Inputs, the float64 truth and the float32 yardstick of a cell and a shape: computed once, shared by every test, never
    written to.  The histories, articles and negatives are those of tests/test_hip_gru_fit.py::_case."""
    helpers, cls, _, _ = _helpers(cell)
    Na, H = shape
    rng = np.random.default_rng(Na + H)
    E = rng.standard_normal((Na, H)).astype(np.float32)
    torch.manual_seed(Na + H)
    model = cls.from_torch(_module(cell, H))                           # torch's default initialisation, seeded
    n = np.minimum(_lengths(rng), 130)                                 # more than 256 users at step 0, 129 / 128 / 127 at steps 3 / 4 / 5
    rows = []
    for L in n:
        r = rng.integers(0, Na, L)
        if L >= 4:
            r[L // 2] = r[0]                                           # an article read twice,
            r[L - 1] = r[L - 2]                                        # and twice in a row
        rows.append(r)
    indptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    items = np.concatenate(rows).astype(np.int64)
    neg = helpers.sample_negatives(indptr, items, Na, 3, seed=Na)
    second = indptr[:-1][n >= 2] + 1                                   # events that are scored
    neg[second[:7], 0] = -1
    neg[second[7:14], 1] = items[second[7:14]]                         # the clicked article is no pair
    neg[second[14:16]] = -1                                            # an event without any pair
    w = [getattr(model, k) for k in cls.NAMES]
    truth = REFERENCE[cell](E, *w, indptr, items, neg)
    yard = REFERENCE[cell](E, *w, indptr, items, neg, dtype=np.float32)
    for a in (indptr, items, neg) + truth[2:] + yard[2:]:
        a.setflags(write=False)
    return dict(E=E, model=model, indptr=indptr, items=items, neg=neg, truth=_named(truth), yard=_named(yard), n=n)


def _named(t):
    return dict(loss=t[0], n_pairs=t[1], margins=t[2], weight_ih=t[3], weight_hh=t[4], bias_ih=t[5], bias_hh=t[6])


def _figure(got, truth):
    """worst absolute error / largest truth magnitude"""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    return float(np.abs(got - truth).max() / np.abs(truth).max())


def _ratios(got, c):
    return {q: _figure(got[q], c["truth"][q]) / _figure(c["yard"][q], c["truth"][q]) for q in QUANTITIES}


def torch_float32_ratios(cell, shape):
    """torch.nn.LSTM / torch.nn.RNN with autograd in float32 on the CPU, user by user: its ratio to the yardstick for every quantity."""
    c = _case(cell, shape)
    H = shape[1]
    net = _module(cell, H)
    with torch.no_grad():
        for p, k in zip((net.weight_ih_l0, net.weight_hh_l0, net.bias_ih_l0, net.bias_hh_l0), ("weight_ih", "weight_hh", "bias_ih", "bias_hh")):
            p.copy_(torch.from_numpy(getattr(c["model"], k)))
    E, indptr, items, neg = torch.from_numpy(c["E"]), c["indptr"], c["items"], c["neg"]
    margins = np.zeros(neg.shape, np.float32)
    total, loss64 = torch.zeros(()), 0.0
    for u in range(len(indptr) - 1):
        e0, e1 = int(indptr[u]), int(indptr[u + 1])
        if e1 - e0 < 2:
            continue
        states, _ = net(E[torch.from_numpy(items[e0:e1 - 1])][None])
        ng = torch.from_numpy(neg[e0 + 1:e1].astype(np.int64))
        it = torch.from_numpy(items[e0 + 1:e1])
        valid = (ng >= 0) & (ng != it[:, None])
        x = torch.einsum("th,tnh->tn", states[0], E[it][:, None, :] - E[ng.clamp(min=0)])
        margins[e0 + 1:e1] = (x * valid).detach().numpy()
        l = torch.nn.functional.softplus(-x) * valid
        total = total + l.sum()
        loss64 += float(l.detach().double().sum())
    total.backward()
    got = dict(loss=loss64, margins=margins, weight_ih=net.weight_ih_l0.grad.numpy(), weight_hh=net.weight_hh_l0.grad.numpy(),
               bias_ih=net.bias_ih_l0.grad.numpy(), bias_hh=net.bias_hh_l0.grad.numpy())
    return _ratios(got, c)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if not isinstance(a, np.ndarray):
        return type(a) is type(b) and a == b
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _within_bound(got, c, cell, what):
    r = _ratios(got, c)
    print("%s: " % what + "  ".join("%s %.3f" % (q, r[q]) for q in QUANTITIES))
    for q in QUANTITIES:
        assert r[q] <= (LOSS_BOUND if q == "loss" else BOUND), (what, q, r[q])


@functools.lru_cache(maxsize=None)
def _run(cell, shape):
    c = _case(cell, shape)
    return _helpers(cell)[2]((c["indptr"], c["items"]), c["E"], c["model"], c["neg"], return_margins=True)


@pytest.mark.parametrize("cell, shape", CASES)
def test_loss_and_gradients_against_float64(cell, shape):
    c, got = _case(cell, shape), _run(cell, shape)
    H, G = shape[1], GATES[cell]
    assert isinstance(got["loss"], float) and isinstance(got["n_pairs"], int)
    assert got["n_pairs"] == c["truth"]["n_pairs"] > 1000
    for q, s in (("weight_ih", (G * H, H)), ("weight_hh", (G * H, H)), ("bias_ih", (G * H,)), ("bias_hh", (G * H,)), ("margins", c["neg"].shape)):
        assert got[q].dtype == np.float32 and got[q].shape == s and np.isfinite(got[q]).all(), q
    for q in QUANTITIES:
        print("%s %s %s: yardstick figure %.3e" % (cell, shape, q, _figure(c["yard"][q], c["truth"][q])))
    _within_bound(got, c, cell, "%s %s kernel / yardstick" % (cell, shape))
    # where there is no pair the margin is an exact zero
    assert (_bits(got["margins"])[c["truth"]["margins"] == 0] == 0).all()
    # for these cells both bias gradients are the same sum
    assert _same(got["bias_ih"], got["bias_hh"])


@pytest.mark.parametrize("cell, shape", CASES)
def test_bit_for_bit(cell, shape):
    pair_loss = _helpers(cell)[2]
    c, got = _case(cell, shape), _run(cell, shape)
    E, model, indptr, items, neg = c["E"], c["model"], c["indptr"], c["items"], c["neg"]
    H = shape[1]
    # run to run
    assert _same(pair_loss((indptr, items), E, model, neg, return_margins=True), got)
    # margins off: the other outputs keep their bits
    off = pair_loss((indptr, items), E, model, neg)
    assert "margins" not in off and _same(off, {k: v for k, v in got.items() if k != "margins"})
    # a strided E is read in place
    wide = torch.full((E.shape[0], H + 13), float("nan"), device="cuda")
    wide[:, 5:5 + H] = torch.from_numpy(E).cuda()
    view = wide[:, 5:5 + H]
    assert view.stride(0) == H + 13 and not view.is_contiguous()
    assert _same(pair_loss((indptr, items), view, model, neg, return_margins=True), got)
    # the users permuted: the pair count and the margins are the same bits, the gradients meet the accuracy bound
    M = c["n"].size
    perm = np.random.default_rng(1).permutation(M)
    rows = [items[indptr[u]:indptr[u + 1]] for u in perm]
    pneg = np.concatenate([neg[indptr[u]:indptr[u + 1]] for u in perm])
    p = pair_loss(rows, E, model, pneg, return_margins=True)
    assert p["n_pairs"] == got["n_pairs"]
    assert _same(p["margins"], np.concatenate([got["margins"][indptr[u]:indptr[u + 1]] for u in perm]))
    back = dict(p, margins=got["margins"])
    _within_bound(back, c, cell, "%s %s permuted / yardstick" % (cell, shape))
    # a batch is the sum of its halves, and the margins of the halves are the whole batch's bits: the states of a user do not
    # depend on the other users of the call
    h = M // 2
    a = pair_loss((indptr[:h + 1], items[:indptr[h]]), E, model, neg[:indptr[h]], return_margins=True)
    b = pair_loss((indptr[h:] - indptr[h], items[indptr[h]:]), E, model, neg[indptr[h]:], return_margins=True)
    assert a["n_pairs"] + b["n_pairs"] == got["n_pairs"]
    both = {q: a[q] + b[q] for q in QUANTITIES if q != "margins"}
    both["margins"] = np.concatenate([a["margins"], b["margins"]])
    assert _same(both["margins"], got["margins"])
    _within_bound(both, c, cell, "%s %s two halves / yardstick" % (cell, shape))


@pytest.mark.parametrize("cell", CELLS)
def test_nothing_to_predict_gives_zeros(cell):
    pair_loss = _helpers(cell)[2]
    c = _case(cell, SHAPES[0])
    E, model = c["E"], c["model"]
    for hist in ([[1], [], [5], [7]], [[], []], []):
        nnz = sum(len(r) for r in hist)
        got = pair_loss(hist, E, model, np.zeros((nnz, 3), np.int64), return_margins=True)
        assert got["loss"] == 0.0 and got["n_pairs"] == 0 and got["margins"].shape == (nnz, 3) and (got["margins"] == 0).all()
        for q in QUANTITIES[2:]:
            assert got[q].shape == getattr(model, q).shape and (_bits(got[q]) == 0).all(), q
    # every pair masked out: still zeros, through the full forward and backward pass
    got = pair_loss([[1, 2, 3], [4, 5]], E, model, np.full((5, 2), -1))
    assert got["loss"] == 0.0 and got["n_pairs"] == 0
    for q in QUANTITIES[2:]:
        assert got[q].shape == getattr(model, q).shape and (_bits(got[q]) == 0).all(), q


def _synthetic_set():
    """The synthetic set of tools/gru_fit_torch.py --synthetic 400x32 --users 300 --seed 0."""
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
    Na, H = 400, 32
    rng = np.random.default_rng(0)
    labels = rng.integers(0, max(Na // 100, 2), Na)
    centres = rng.standard_normal((int(labels.max()) + 1, H))
    E = (centres[labels] + 0.5 * rng.standard_normal((Na, H))).astype(np.float32)
    indptr, items = synthetic_sessions(300, labels, mean_len=12, seed=0)
    return E, indptr, items


@pytest.mark.parametrize("cell", CELLS)
def test_the_trainer_learns_and_is_reproducible(cell):
    _, cls, _, fit = _helpers(cell)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gru_fit_torch
    finally:
        sys.path.pop(0)
    E, indptr, items = _synthetic_set()
    kw = dict(epochs=10, batch_users=64, n_neg=4, lr=1e-2, seed=0)
    _, stand_in = gru_fit_torch.fit(E, indptr, items, device="cpu", log=lambda s: None, cell=cell, **kw)
    m = fit((indptr, items), E, **kw)
    print("device fit %s\nstand-in   %s" % (np.round(m.history, 4).tolist(), np.round(stand_in, 4).tolist()))
    assert isinstance(m, cls) and m.validation is None
    assert m.history.dtype == np.float64 and m.history.shape == (10,) and np.isfinite(m.history).all()
    assert (m.input_size, m.hidden_size) == (32, 32) and m.weight_hh.shape == (GATES[cell] * 32, 32)
    assert m.history[-1] < m.history[0]
    assert m.history[-1] < (np.log(2.0) + stand_in[-1]) / 2
    again = fit((indptr, items), E, **kw)
    assert all(_same(getattr(m, k), getattr(again, k)) for k in cls.NAMES) and _same(m.history, again.history)
    more = fit((indptr, items), E, init=m, **dict(kw, epochs=1))
    assert more.history[0] < m.history[0]
    assert not _same(more.weight_hh, m.weight_hh)
    with pytest.raises(ValueError, match="keep_best needs validation"):
        fit((indptr, items), E, keep_best=True, **kw)


@pytest.mark.parametrize("cell", CELLS)
def test_cli_fit_cell(cell, tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    cls = _helpers(cell)[1]
    monkeypatch.chdir(tmp_path)
    common = ["--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4", "--sessions", "synthetic",
              "--recommend", "5", "--similarity", "False"]
    model = cli.main(["--model_name", "f"] + common + ["--user_model", cell, "--fit_cell", "--cell_epochs", "2"])
    out = capsys.readouterr().out
    d = model.data_dir
    m = cls.load(d + "%s_user_model.npz" % cell)
    emb = np.load(d + "article_encoded_train.npy")
    assert (m.input_size, m.hidden_size) == (emb.shape[1], emb.shape[1])
    assert out.count("loss per pair") == 2 and "%s user state" % cell in out
    g = np.load(d + "article_encoded_recommend5_%s.npz" % cell)
    assert sorted(g.files) == ["indices", "scores", "targets"] and g["indices"].shape == (200, 5)
    with pytest.raises(AssertionError, match="--user_weights PATH or --fit_cell"):
        cli.main(["--model_name", "q"] + common + ["--user_model", cell])


def test_cli_fit_cell_is_not_for_the_gru():
    import main_autoencoder as cli
    common = ["--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4", "--sessions", "synthetic",
              "--recommend", "5", "--similarity", "False"]
    with pytest.raises(AssertionError):
        cli.main(["--model_name", "q"] + common + ["--user_model", "gru", "--fit_cell"])
    with pytest.raises(AssertionError, match="--fit_cell needs --user_model lstm or rnn"):
        cli.main(["--model_name", "q"] + common + ["--fit_cell"])
