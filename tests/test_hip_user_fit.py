"""GPU checks of the training step of the decay user model (dae_user_pair_loss through helpers.user_pair_loss) and of
helpers.fit_user_model.  Truth: the float64 restatement of the definition in include/dae_hip.h, ``restate`` of
tests/test_user_fit_cpu.py, which is itself checked against finite differences there.

Gate of the float sums (test 2; reused by the permutation and partition tests): 16 * 2**-24 * S per output, S the float64 sum
over the valid pairs of the magnitudes that enter -- S_loss = sum(softplus(-x) + X), S_alpha[h] = sum((|c| + X / 4) |u_h D_h|),
S_beta = sum((|c| + X / 4) XB), X = sum_h |alpha_h u_h D_h|, XB = sum_h |alpha_h u'_h D_h|.  A float32 NumPy restatement (chain
and dot products in float32, pair sums in float64) deviates from float64 by at most 0.1 of 2**-24 * S at these shapes; a wave
tree with fmaf changes that by small factors, and 16 leaves two orders of magnitude."""
import numpy as np
import pytest
import torch

from test_user_fit_cpu import restate

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 63, 64, 65, 130, 0, 7, 33, 1, 256]
SHAPES = [(300, 70), (1000, 500)]              # scalar loads, 4 columns per lane; 16-byte loads, 8 columns per lane
EPS = 2.0 ** -24


def _histories(rng, Na, lengths=LENGTHS):
    rows = []
    for n in lengths:
        r = rng.integers(0, Na, n)
        if n >= 7:
            r[n // 2] = r[0]                                               # an article read twice,
            r[n - 1] = r[n - 2]                                            # and twice in a row
        rows.append(r)
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int64) if indptr[-1] else np.zeros(0, np.int64)


def _negatives(rng, items, Na, n_neg):
    neg = rng.integers(-1, Na, (items.size, n_neg))
    hit = rng.random(items.size) < 0.1
    neg[hit, rng.integers(0, n_neg)] = items[hit]                          # the click itself among its negatives: no pair
    return neg


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gates(ref):
    return 16 * EPS * ref["S_loss"], 16 * EPS * ref["S_alpha"], 16 * EPS * ref["S_beta"]


def _assert_sums(got, ref, what, gates=None):
    g_loss, g_alpha, g_beta = gates or _gates(ref)
    r_loss = abs(got["loss"] - ref["loss"]) / g_loss if g_loss else 0.0
    r_alpha = float((np.abs(got["dalpha"] - ref["dalpha"]) / np.where(g_alpha > 0, g_alpha, 1.0)).max())
    r_beta = abs(got["dbeta"] - ref["dbeta"]) / g_beta if g_beta else abs(got["dbeta"] - ref["dbeta"])
    print("%s: worst error / gate  loss %.4f  dalpha %.4f  dbeta %.4f   (S / |output|: loss %.3g, dbeta %.3g)"
          % (what, r_loss, r_alpha, r_beta, ref["S_loss"] / max(abs(ref["loss"]), 1e-300), ref["S_beta"] / max(abs(ref["dbeta"]), 1e-300)))
    assert got["n_pairs"] == ref["n_pairs"]
    assert r_loss <= 1.0 and r_alpha <= 1.0 and r_beta <= 1.0, (what, r_loss, r_alpha, r_beta)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("resets", [False, True])
def test_margins_bit_for_bit(shape, resets):
    """Small-integer embeddings, alpha in {0.5, 1, 2}, beta = 1 or factors in {0, 1} (session resets): every s, z and every partial
    sum of alpha s D is a multiple of 0.5 whose magnitude stays below 2**23 (asserted in float64 below), so any summation order
    is exact in float32 and margin == float32(sum) / float32(z), one correctly rounded division, as bits.  Pins the off-by-one of
    the state, the first-event rule, the skip rules and the single division."""
    from dae_rnn_news_recommendation_amd import helpers
    Na, H = shape
    rng = np.random.default_rng(H + resets)
    E = rng.integers(-4, 5, shape).astype(np.float32)
    alpha = rng.choice([0.5, 1.0, 2.0], H)
    indptr, items = _histories(rng, Na, LENGTHS + [1000])
    neg = _negatives(rng, items, Na, 3)
    if resets:
        t = np.cumsum(rng.choice([0.0, 1.0], items.size, p=[0.8, 0.2]))
        f = helpers.decay_factors(indptr, t, 0.0)
        assert set(np.unique(f)) == {0.0, 1.0}
        kw = dict(beta=0.0, timestamps=t)
    else:
        f, kw = np.ones(items.size), dict(beta=1.0)
    ref = restate(E, indptr, items, alpha, f, np.zeros(items.size), neg)
    assert ref["exact_bound"] < 2 ** 23 and np.array_equal(np.round(2 * ref["num"]), 2 * ref["num"])
    assert np.array_equal(np.round(ref["z"]), ref["z"]) and ref["z"].max() <= 1000
    want = np.where(ref["valid"], ref["num"].astype(np.float32) / np.maximum(ref["z"], 1).astype(np.float32)[:, None], np.float32(0))
    got = helpers.user_pair_loss((indptr, items), E, alpha, negatives=neg, return_margins=True, **kw)
    assert got["margins"].dtype == np.float32 and got["margins"].shape == neg.shape
    assert got["n_pairs"] == int(ref["valid"].sum()) and got["n_pairs"] > 0
    assert np.array_equal(_bits(got["margins"]), _bits(want))
    assert (got["margins"][~ref["valid"]] == 0).all()
    if resets:
        assert got["dbeta"] == 0.0                                         # no derivative factors: f' = 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("beta", [1.0, 0.9, 0.5, "timed"])
def test_sums_against_float64(shape, beta):
    """Loss, dalpha and dbeta against the float64 restatement, inside the gate of the module docstring.  'timed': factors and their
    derivatives from timestamps (decay_factors / decay_factor_derivatives at beta = 0.8, time_unit = 2), simultaneous events
    included."""
    from dae_rnn_news_recommendation_amd import helpers
    Na, H = shape
    rng = np.random.default_rng(H + (7 if beta == "timed" else int(10 * beta)))
    E = rng.standard_normal(shape).astype(np.float32)
    alpha = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)
    indptr, items = _histories(rng, Na)
    neg = _negatives(rng, items, Na, 3)
    if beta == "timed":
        t = np.cumsum(rng.choice([0.0, 0.5, 1.0, 3.0, 9.0], items.size))
        f = helpers.decay_factors(indptr, t, 0.8, 2.0)
        fp = helpers.decay_factor_derivatives(indptr, t, 0.8, 2.0)
        kw = dict(beta=0.8, timestamps=t, time_unit=2.0)
    else:
        f, fp, kw = np.full(items.size, np.float32(beta)), np.ones(items.size), dict(beta=beta)
    ref = restate(E, indptr, items, alpha, f, fp, neg)
    got = helpers.user_pair_loss((indptr, items), E, alpha, negatives=neg, return_margins=True, **kw)
    assert got["dalpha"].dtype == np.float64 and got["dalpha"].shape == (H,)
    _assert_sums(got, ref, "H %d beta %s" % (H, beta))
    # the margins: |x - x64| <= 16 eps X per pair (the loss gate without the softplus term)
    assert (got["margins"][~ref["valid"]] == 0).all()
    assert np.abs(got["margins"] - ref["margins"]).max() <= 16 * EPS * np.abs(E).max() ** 2 * 2 * np.abs(alpha).max() * H


def test_runs_agree_users_permute_strides_agree():
    from dae_rnn_news_recommendation_amd import helpers
    for shape in SHAPES:
        Na, H = shape
        rng = np.random.default_rng(8 + H)
        E = rng.standard_normal(shape).astype(np.float32)
        alpha = 1.0 + 0.3 * rng.standard_normal(H)
        lengths = LENGTHS + [1000]
        indptr, items = _histories(rng, Na, lengths)
        neg = _negatives(rng, items, Na, 3)
        a = helpers.user_pair_loss((indptr, items), E, alpha, 0.9, neg, return_margins=True)
        b = helpers.user_pair_loss((indptr, items), E, alpha, 0.9, neg, return_margins=True)
        assert a["loss"] == b["loss"] and a["dbeta"] == b["dbeta"] and a["n_pairs"] == b["n_pairs"]
        assert np.array_equal(a["dalpha"].view(np.uint64), b["dalpha"].view(np.uint64))
        assert np.array_equal(_bits(a["margins"]), _bits(b["margins"]))
        ref = restate(E, indptr, items, alpha.astype(np.float32), np.full(items.size, np.float32(0.9)), np.ones(items.size), neg)
        _assert_sums(a, ref, "H %d with a user of 1000 events" % H)
        perm = rng.permutation(len(lengths))
        rows = [items[indptr[u]:indptr[u + 1]] for u in perm]
        negp = np.concatenate([neg[indptr[u]:indptr[u + 1]] for u in perm])
        p = helpers.user_pair_loss(rows, E, alpha, 0.9, negp, return_margins=True)
        assert np.array_equal(_bits(p["margins"]), _bits(np.concatenate([a["margins"][indptr[u]:indptr[u + 1]] for u in perm])))
        _assert_sums(p, ref, "H %d permuted" % H)


def test_strided_embeddings_are_read_in_place():
    """A column slice of a wider tensor -- H = 70 at column 10 (scalar loads) and H = 64 at column 8 of a row of 100 (16-byte loads) --
    gives the margins and the pair count of its contiguous copy, and the same sums inside the gate."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(4)
    wide = torch.from_numpy(rng.standard_normal((300, 100)).astype(np.float32)).cuda()
    indptr, items = _histories(rng, 300)
    neg = _negatives(rng, items, 300, 3)
    for c0, c1 in ((10, 80), (8, 72)):
        view = wide[:, c0:c1]
        assert not view.is_contiguous()
        alpha = 1.0 + 0.3 * rng.standard_normal(c1 - c0)
        got = helpers.user_pair_loss((indptr, items), view, alpha, 0.9, neg, return_margins=True)
        Ec = view.contiguous().cpu().numpy()
        want = helpers.user_pair_loss((indptr, items), Ec, alpha, 0.9, neg, return_margins=True)
        assert got["n_pairs"] == want["n_pairs"] and np.array_equal(_bits(got["margins"]), _bits(want["margins"]))
        ref = restate(Ec, indptr, items, alpha.astype(np.float32), np.full(items.size, np.float32(0.9)), np.ones(items.size), neg)
        _assert_sums(got, ref, "columns %d:%d strided" % (c0, c1))
        _assert_sums(want, ref, "columns %d:%d contiguous" % (c0, c1))


def test_user_batches_as_sliced_csr():
    """A batch [u0, u1) of users passed as a sliced CSR gives the margins of the full call's rows; the pair counts of a partition
    add up exactly and the float sums inside the gate of the whole."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(12)
    E = rng.standard_normal((300, 70)).astype(np.float32)
    alpha = 1.0 + 0.3 * rng.standard_normal(70)
    indptr, items = _histories(rng, 300)
    neg = _negatives(rng, items, 300, 3)
    full = helpers.user_pair_loss((indptr, items), E, alpha, 0.9, neg, return_margins=True)
    ref = restate(E, indptr, items, alpha.astype(np.float32), np.full(items.size, np.float32(0.9)), np.ones(items.size), neg)
    parts = []
    for u0, u1 in ((0, 4), (4, 5), (5, 7), (7, 8), (8, 12)):
        a, b = int(indptr[u0]), int(indptr[u1])
        r = helpers.user_pair_loss((indptr[u0:u1 + 1] - a, items[a:b]), E, alpha, 0.9, neg[a:b], return_margins=True)
        assert np.array_equal(_bits(r["margins"]), _bits(full["margins"][a:b])), (u0, u1)
        parts.append(r)
    total = dict(loss=sum(r["loss"] for r in parts), dalpha=sum(r["dalpha"] for r in parts), dbeta=sum(r["dbeta"] for r in parts),
                 n_pairs=sum(r["n_pairs"] for r in parts))
    assert total["n_pairs"] == full["n_pairs"]
    _assert_sums(total, ref, "sum over a partition of the users")
    _assert_sums(full, ref, "all users")


def test_edge_cases():
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(3)
    E = rng.standard_normal((300, 70)).astype(np.float32)
    alpha = 1.0 + 0.3 * rng.standard_normal(70)
    zero = lambda r: r["loss"] == 0.0 and r["dbeta"] == 0.0 and r["n_pairs"] == 0 and (r["dalpha"] == 0).all()
    r = helpers.user_pair_loss([], E, alpha, 0.9, np.zeros((0, 3), np.int64), return_margins=True)            # M = 0
    assert zero(r) and r["margins"].shape == (0, 3)
    indptr, items = _histories(rng, 300, [0, 1, 1, 0, 1])                                                     # no user has a second click
    r = helpers.user_pair_loss((indptr, items), E, alpha, 0.9, rng.integers(0, 300, (3, 2)), return_margins=True)
    assert zero(r) and (r["margins"] == 0).all()
    indptr, items = _histories(rng, 300)
    r = helpers.user_pair_loss((indptr, items), E, alpha, 0.9, np.full((items.size, 4), -1), return_margins=True)      # no negatives at all
    assert zero(r) and (r["margins"] == 0).all()
    for n_neg in (1, 16):                                                                                     # one walk, and four walks of 4
        neg = _negatives(rng, items, 300, n_neg)
        got = helpers.user_pair_loss((indptr, items), E, alpha, 0.9, neg, return_margins=True)
        ref = restate(E, indptr, items, alpha.astype(np.float32), np.full(items.size, np.float32(0.9)), np.ones(items.size), neg)
        _assert_sums(got, ref, "n_neg %d" % n_neg)
        assert (got["margins"][~ref["valid"]] == 0).all() and (got["margins"][ref["valid"]] != 0).all()
    with pytest.raises(ValueError, match="negatives must be below 300"):
        helpers.user_pair_loss((indptr, items), E, alpha, 0.9, np.full((items.size, 2), 300))
    with pytest.raises(ValueError, match="n_neg"):
        helpers.user_pair_loss((indptr, items), E, alpha, 0.9, np.zeros((items.size, 17), np.int64))
    with pytest.raises(ValueError, match="alpha has"):
        helpers.user_pair_loss((indptr, items), E, alpha[:-1], 0.9, np.zeros((items.size, 2), np.int64))
    with pytest.raises(ValueError, match="1..1024"):
        helpers.user_pair_loss([[0, 1]], np.ones((4, 1025), np.float32), np.ones(1025), 0.9, np.zeros((2, 1), np.int64))


def test_widest_rows_sixteen_columns_per_lane():
    """H = 1024 (16 columns per lane, 16-byte loads) and H = 1022 (the same with scalar loads and a ragged last group)."""
    from dae_rnn_news_recommendation_amd import helpers
    for H in (1024, 1022):
        rng = np.random.default_rng(H)
        E = rng.standard_normal((120, H)).astype(np.float32)
        alpha = 1.0 + 0.3 * rng.standard_normal(H)
        indptr, items = _histories(rng, 120, [0, 1, 2, 9, 65, 3])
        neg = _negatives(rng, items, 120, 3)
        got = helpers.user_pair_loss((indptr, items), E, alpha, 0.9, neg)
        ref = restate(E, indptr, items, alpha.astype(np.float32), np.full(items.size, np.float32(0.9)), np.ones(items.size), neg)
        _assert_sums(got, ref, "H %d" % H)


def _fit_case():
    """2000 articles in 20 classes, H = 32 with the class signal in the first 8 dimensions; synthetic_sessions(1200, mean_len 12);
    users 0..899 to fit on, 900..1199 held out."""
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
    rng = np.random.default_rng(11)
    labels = np.repeat(np.arange(20), 100)
    E = rng.standard_normal((2000, 32))
    E[:, :8] = rng.standard_normal((20, 8))[labels] + 0.5 * rng.standard_normal((2000, 8))
    indptr, items = synthetic_sessions(1200, labels, mean_len=12, seed=3)
    a = int(indptr[900])
    return E.astype(np.float32), (indptr[:901], items[:a]), (indptr[900:] - a, items[a:])


def test_fit_user_model_end_to_end():
    """The float64 restatement of this recipe (60 full-batch Adam steps, lr 0.05) takes the held-out loss per pair from 1.016 to
    0.493 and the mean rank of the held-out last click from 543 to 412 of 2000, with alpha near 0.4 on the signal dimensions and
    near 0 elsewhere and beta 0.9 -> 0.963.  Asserted: improvement only."""
    from dae_rnn_news_recommendation_amd import helpers
    E, train, held = _fit_case()
    kw = dict(beta0=0.9, n_neg=4, epochs=60, lr=0.05, seed=0)
    model = helpers.fit_user_model(train, E, **kw)
    assert model.alpha.shape == (32,) and model.alpha.dtype == np.float64 and model.history.shape == (60,) and 0 < model.beta < 1
    again = helpers.fit_user_model(train, E, **kw)
    assert np.array_equal(model.alpha.view(np.uint64), again.alpha.view(np.uint64)) and model.beta == again.beta
    assert np.array_equal(model.history, again.history)
    neg0 = helpers.sample_negatives(train[0], train[1], 2000, 4, seed=0)
    start = helpers.user_pair_loss(train, E, np.ones(32), 0.9, neg0)
    assert model.history[0] == start["loss"] / start["n_pairs"]
    # held out: loss per pair on fixed negatives
    hneg = helpers.sample_negatives(held[0], held[1], 2000, 4, seed=999)
    before = helpers.user_pair_loss(held, E, np.ones(32), 0.9, hneg)
    after = helpers.user_pair_loss(held, E, model.alpha, model.beta, hneg)
    # ... and the rank of every held-out user's last click among the articles that user has not read
    ip, it = held
    L = np.diff(ip)
    hist = [it[ip[u]:ip[u + 1] - 1] for u in range(len(L))]
    targets = np.where(L >= 2, it[np.maximum(ip[1:] - 1, 0)], -1)
    auc = []
    for states in (helpers.user_states(hist, E, 0.9, return_tensor=True), model.states(hist, E, return_tensor=True)):
        rank, _, n_cand = helpers.recommend_ranks(states, E, targets, seen=hist)
        auc.append(helpers.rank_metrics(rank, n_cand, targets))
    print("held-out loss per pair %.4f -> %.4f   AUC %.4f -> %.4f   mean rank %.1f -> %.1f   beta %.4f   alpha[:8] %s  |alpha[8:]| max %.3f"
          % (before["loss"] / before["n_pairs"], after["loss"] / after["n_pairs"], auc[0]["auc"], auc[1]["auc"], auc[0]["mean_rank"],
             auc[1]["mean_rank"], model.beta, np.round(model.alpha[:8], 2), np.abs(model.alpha[8:]).max()))
    assert after["loss"] / after["n_pairs"] < before["loss"] / before["n_pairs"]
    assert auc[1]["auc"] > auc[0]["auc"]
    assert np.array_equal(model.states(hist, E), (helpers.user_states(hist, E, model.beta, return_tensor=True)
                                                  * torch.from_numpy(model.alpha.astype(np.float32)).cuda()).cpu().numpy())
    # mini-batches of consecutive users and a fixed beta: two steps per epoch, beta untouched, deterministic
    mb = helpers.fit_user_model(train, E, beta0=0.9, fit_beta=False, epochs=3, batch_users=450, seed=1)
    assert mb.history.shape == (6,) and mb.beta == float(np.float32(0.9)) and mb.history[-1] < mb.history[0]
    # with timestamps the decay is per unit of time: the fit runs and moves beta
    t = np.concatenate([np.cumsum(np.random.default_rng(u).choice([0.0, 1.0, 2.0], n)) for u, n in enumerate(np.diff(train[0]))])
    tm = helpers.fit_user_model(train, E, epochs=5, timestamps=t, time_unit=2.0, seed=2)
    assert tm.history.shape == (5,) and np.isfinite(tm.history).all() and tm.history[-1] < tm.history[0] and tm.beta != float(np.float32(0.9))
    assert tm.time_unit == 2.0


def test_cli_fit_user_model(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    monkeypatch.chdir(tmp_path)
    args = ["--model_name", "rec", "--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4",
            "--sessions", "synthetic", "--recommend", "10", "--similarity", "False"]
    cli.main(args)
    plain = capsys.readouterr().out
    model = cli.main(args + ["--fit_user_model"])
    out = capsys.readouterr().out
    assert plain.count("hit@10") == 2 and "fitted user model" not in plain and "fit user model" not in plain
    # the flag adds lines and changes none: what was printed without it is printed again, line for line
    keep = [ln for ln in out.splitlines() if ln in plain.splitlines()]
    assert [ln for ln in plain.splitlines() if "hit@10" in ln or "calculate recommend" in ln] == \
           [ln for ln in keep if "hit@10" in ln or "calculate recommend" in ln]
    assert out.count("hit@10") == 3 and "decayed user state" in out and "fitted user model" in out and "fit user model done" in out
    f = np.load(model.data_dir + "user_model.npz")
    emb = np.load(model.data_dir + "article_encoded_train.npy")
    assert f["alpha"].shape == (emb.shape[1],) and f["alpha"].dtype == np.float64 and 0 < float(f["beta"]) < 1
    assert f["history"].ndim == 1 and f["history"].size > 0 and f["history"][-1] < f["history"][0]
    with pytest.raises(AssertionError, match="--fit_user_model needs"):
        cli.main(["--model_name", "rec", "--fit_user_model"])
