"""GPU checks of the GRU trainer (dae_gru_pair_loss through helpers.gru_pair_loss, helpers.fit_gru_user_model and the CLI).

Truth: ``gru_bptt_reference`` of tests/test_gru_fit_cpu.py in float64 (there pinned to torch autograd in float64 and to finite
differences).  Yardstick: the same restatement in NumPy float32 on the same inputs.  For each of the four gradients, for the
margins and for the loss, the figure is the worst absolute error divided by the largest magnitude of the truth, and the kernel's
figure must stay within a fixed multiple of the yardstick's.  The multiple is derived as tests/test_hip_gru.py derived its 8 x:
torch.nn.GRU with autograd in float32 on the CPU, on these inputs (``torch_float32_ratios`` below recomputes it); four times its
worst ratio to the yardstick, rounded up to a power of two.  Over the margins and the four gradients torch sits at 1.454 x at
worst: BOUND = 8.  The loss has a multiple of its own, LOSS_BOUND = 2048, from the same rule: it is ONE number, the float64 sum of
4199 float32-rounded terms, and at (300, 70) the yardstick's roundings happen to cancel to 3.4e-11 of the loss -- sixty times
below the 2e-9 a random walk of that length gives -- so that torch sits at 282 x there (and at 0.70 x at (600, 160), where the
yardstick's figure is 1.8e-8).  Folding that accident into one multiple for everything would have let the gradients off.

    ratio to the yardstick            loss    margins  weight_ih  weight_hh  bias_ih  bias_hh
    (300, 70)    torch float32, CPU   281.9   1.454    0.362      1.360      0.656    0.940
                 dae_gru_pair_loss    128.0   0.751    0.365      0.507      0.155    0.085      (one MI355X)
    (600, 160)   torch float32, CPU   0.700   0.955    0.365      1.216      0.508    0.844
                 dae_gru_pair_loss    0.661   0.953    0.549      0.550      0.218    0.176
    the users permuted, and the sum of two half batches: margins and gradients between 0.085 and 0.953, the loss as above

``n_pairs`` is exact.  Bit for bit: run to run, margins on or off, a strided E, and -- the users permuted -- the pair count and
the margins; the gradients of a permuted batch and the sum of the gradients of its two halves meet the accuracy bound."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from test_gru_fit_cpu import gru_bptt_reference
from test_hip_gru import _lengths

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 70), (600, 160)]                                        # (articles, H): Hp = 128 and 256
BOUND = 8.0                                                             # margins and gradients: 4 x 1.454, rounded up to a power of two
LOSS_BOUND = 2048.0                                                     # the loss: 4 x 282
QUANTITIES = ("loss", "margins", "weight_ih", "weight_hh", "bias_ih", "bias_hh")


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, the float64 truth and the float32 yardstick of a shape: computed once, shared by every test, never written to."""
    from dae_rnn_news_recommendation_amd import helpers
    Na, H = shape
    rng = np.random.default_rng(Na + H)
    E = rng.standard_normal((Na, H)).astype(np.float32)
    torch.manual_seed(Na + H)
    model = helpers.GRUUserModel.from_torch(torch.nn.GRU(H, H))        # torch's default initialisation, seeded
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
    w = [getattr(model, k) for k in helpers.GRUUserModel.NAMES]
    truth = gru_bptt_reference(E, *w, indptr, items, neg)
    yard = gru_bptt_reference(E, *w, indptr, items, neg, dtype=np.float32)
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


def torch_float32_ratios(shape):
    """torch.nn.GRU with autograd in float32 on the CPU, user by user: its ratio to the yardstick for every quantity."""
    c = _case(shape)
    H = shape[1]
    gru = torch.nn.GRU(H, H, batch_first=True)
    with torch.no_grad():
        for p, k in zip((gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0), ("weight_ih", "weight_hh", "bias_ih", "bias_hh")):
            p.copy_(torch.from_numpy(getattr(c["model"], k)))
    E, indptr, items, neg = torch.from_numpy(c["E"]), c["indptr"], c["items"], c["neg"]
    margins = np.zeros(neg.shape, np.float32)
    total, loss64 = torch.zeros(()), 0.0
    for u in range(len(indptr) - 1):
        e0, e1 = int(indptr[u]), int(indptr[u + 1])
        if e1 - e0 < 2:
            continue
        states, _ = gru(E[torch.from_numpy(items[e0:e1 - 1])][None])
        ng = torch.from_numpy(neg[e0 + 1:e1].astype(np.int64))
        it = torch.from_numpy(items[e0 + 1:e1])
        valid = (ng >= 0) & (ng != it[:, None])
        x = torch.einsum("th,tnh->tn", states[0], E[it][:, None, :] - E[ng.clamp(min=0)])
        margins[e0 + 1:e1] = (x * valid).detach().numpy()
        l = torch.nn.functional.softplus(-x) * valid
        total = total + l.sum()
        loss64 += float(l.detach().double().sum())
    total.backward()
    got = dict(loss=loss64, margins=margins, weight_ih=gru.weight_ih_l0.grad.numpy(), weight_hh=gru.weight_hh_l0.grad.numpy(),
               bias_ih=gru.bias_ih_l0.grad.numpy(), bias_hh=gru.bias_hh_l0.grad.numpy())
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


def _within_bound(got, c, what):
    r = _ratios(got, c)
    print("%s: " % what + "  ".join("%s %.3f" % (q, r[q]) for q in QUANTITIES))
    for q in QUANTITIES:
        assert r[q] <= (LOSS_BOUND if q == "loss" else BOUND), (what, q, r[q])


@functools.lru_cache(maxsize=None)
def _run(shape):
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(shape)
    return helpers.gru_pair_loss((c["indptr"], c["items"]), c["E"], c["model"], c["neg"], return_margins=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_loss_and_gradients_against_float64(shape):
    c, got = _case(shape), _run(shape)
    H = shape[1]
    assert isinstance(got["loss"], float) and isinstance(got["n_pairs"], int)
    assert got["n_pairs"] == c["truth"]["n_pairs"] > 1000
    for q, s in (("weight_ih", (3 * H, H)), ("weight_hh", (3 * H, H)), ("bias_ih", (3 * H,)), ("bias_hh", (3 * H,)), ("margins", c["neg"].shape)):
        assert got[q].dtype == np.float32 and got[q].shape == s and np.isfinite(got[q]).all(), q
    for q in QUANTITIES:
        print("%s %s: yardstick figure %.3e" % (shape, q, _figure(c["yard"][q], c["truth"][q])))
    _within_bound(got, c, "%s kernel / yardstick" % (shape,))
    # where there is no pair the margin is an exact zero
    assert (_bits(got["margins"])[c["truth"]["margins"] == 0] == 0).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_for_bit(shape):
    from dae_rnn_news_recommendation_amd import helpers
    c, got = _case(shape), _run(shape)
    E, model, indptr, items, neg = c["E"], c["model"], c["indptr"], c["items"], c["neg"]
    H = shape[1]
    # run to run
    assert _same(helpers.gru_pair_loss((indptr, items), E, model, neg, return_margins=True), got)
    # margins off: the other outputs keep their bits
    off = helpers.gru_pair_loss((indptr, items), E, model, neg)
    assert "margins" not in off and _same(off, {k: v for k, v in got.items() if k != "margins"})
    # a strided E is read in place
    wide = torch.full((E.shape[0], H + 13), float("nan"), device="cuda")
    wide[:, 5:5 + H] = torch.from_numpy(E).cuda()
    view = wide[:, 5:5 + H]
    assert view.stride(0) == H + 13 and not view.is_contiguous()
    assert _same(helpers.gru_pair_loss((indptr, items), view, model, neg, return_margins=True), got)
    # the users permuted: the pair count and the margins are the same bits, the gradients meet the accuracy bound
    M = c["n"].size
    perm = np.random.default_rng(1).permutation(M)
    rows = [items[indptr[u]:indptr[u + 1]] for u in perm]
    pneg = np.concatenate([neg[indptr[u]:indptr[u + 1]] for u in perm])
    p = helpers.gru_pair_loss(rows, E, model, pneg, return_margins=True)
    assert p["n_pairs"] == got["n_pairs"]
    assert _same(p["margins"], np.concatenate([got["margins"][indptr[u]:indptr[u + 1]] for u in perm]))
    back = dict(p, margins=got["margins"])
    _within_bound(back, c, "%s permuted / yardstick" % (shape,))
    # a batch is the sum of its halves
    h = M // 2
    a = helpers.gru_pair_loss((indptr[:h + 1], items[:indptr[h]]), E, model, neg[:indptr[h]], return_margins=True)
    b = helpers.gru_pair_loss((indptr[h:] - indptr[h], items[indptr[h]:]), E, model, neg[indptr[h]:], return_margins=True)
    assert a["n_pairs"] + b["n_pairs"] == got["n_pairs"]
    both = {q: a[q] + b[q] for q in QUANTITIES if q != "margins"}
    both["margins"] = np.concatenate([a["margins"], b["margins"]])
    assert _same(both["margins"], got["margins"])
    _within_bound(both, c, "%s two halves / yardstick" % (shape,))


def test_nothing_to_predict_gives_zeros():
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(SHAPES[0])
    E, model = c["E"], c["model"]
    for hist in ([[1], [], [5], [7]], [[], []], []):
        nnz = sum(len(r) for r in hist)
        got = helpers.gru_pair_loss(hist, E, model, np.zeros((nnz, 3), np.int64), return_margins=True)
        assert got["loss"] == 0.0 and got["n_pairs"] == 0 and got["margins"].shape == (nnz, 3) and (got["margins"] == 0).all()
        for q in QUANTITIES[2:]:
            assert got[q].shape == getattr(model, q).shape and (_bits(got[q]) == 0).all(), q
    # every pair masked out: still zeros, through the full forward and backward pass
    got = helpers.gru_pair_loss([[1, 2, 3], [4, 5]], E, model, np.full((5, 2), -1))
    assert got["loss"] == 0.0 and got["n_pairs"] == 0 and all((got[q] == 0).all() for q in QUANTITIES[2:])


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


def test_the_trainer_learns_and_is_reproducible():
    from dae_rnn_news_recommendation_amd import helpers
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gru_fit_torch
    finally:
        sys.path.pop(0)
    E, indptr, items = _synthetic_set()
    kw = dict(epochs=10, batch_users=64, n_neg=4, lr=1e-2, seed=0)
    _, stand_in = gru_fit_torch.fit(E, indptr, items, device="cpu", log=lambda s: None, **kw)
    m = helpers.fit_gru_user_model((indptr, items), E, **kw)
    print("device fit %s\nstand-in   %s" % (np.round(m.history, 4).tolist(), np.round(stand_in, 4).tolist()))
    assert m.history.dtype == np.float64 and m.history.shape == (10,) and np.isfinite(m.history).all()
    assert (m.input_size, m.hidden_size) == (32, 32)
    assert m.history[-1] < m.history[0]
    assert m.history[-1] < (np.log(2.0) + stand_in[-1]) / 2
    again = helpers.fit_gru_user_model((indptr, items), E, **kw)
    assert all(_same(getattr(m, k), getattr(again, k)) for k in helpers.GRUUserModel.NAMES) and _same(m.history, again.history)
    more = helpers.fit_gru_user_model((indptr, items), E, init=m, **dict(kw, epochs=1))
    assert more.history[0] < m.history[0]
    assert not _same(more.weight_hh, m.weight_hh)


def test_cli_fit_gru(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    monkeypatch.chdir(tmp_path)
    common = ["--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4", "--sessions", "synthetic",
              "--recommend", "5", "--similarity", "False"]
    model = cli.main(["--model_name", "f"] + common + ["--user_model", "gru", "--fit_gru", "--gru_epochs", "2"])
    out = capsys.readouterr().out
    d = model.data_dir
    m = helpers.GRUUserModel.load(d + "gru_user_model.npz")
    emb = np.load(d + "article_encoded_train.npy")
    assert (m.input_size, m.hidden_size) == (emb.shape[1], emb.shape[1])
    assert out.count("loss per pair") == 2 and "gru user state" in out
    g = np.load(d + "article_encoded_recommend5_gru.npz")
    assert sorted(g.files) == ["indices", "scores", "targets"] and g["indices"].shape == (200, 5)
    with pytest.raises(AssertionError, match="--gru_weights PATH or --fit_gru"):
        cli.main(["--model_name", "q"] + common + ["--user_model", "gru"])
