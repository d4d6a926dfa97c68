"""GPU checks of the LSTM and plain-RNN user states (dae_lstm_user_states / dae_rnn_user_states through helpers.lstm_user_states /
helpers.rnn_user_states).

Truth: ``lstm_reference`` / ``rnn_reference`` of tests/test_lstm_rnn_cpu.py in float64 (there pinned to torch.nn.LSTM / torch.nn.RNN
in float64 to 1e-12).  Yardstick: the same restatement run in NumPy float32 on the same inputs -- what a straightforward fp32
implementation of the formula loses.  The kernel's worst absolute error -- over all states, over the last states and, for the LSTM,
over the last cell states -- must stay within ``BOUND[cell]`` x the yardstick's worst error on the case.

Where the bounds come from (measured on the CPU, not on the kernel): torch.nn.LSTM / torch.nn.RNN in float32 on the CPU, run on
exactly these inputs (every history through the module, as a batch of one), sit at most at
    LSTM: 1.131 x the yardstick   (the worst of the nine figures: three shapes x all states / last states / last cells)
    RNN:  1.015 x the yardstick   (the worst of the six figures: three shapes x all states / last states)
and the bound is ceil(4 x that ratio): BOUND = {lstm: 5, rnn: 5}.  The factor 4 is the margin of tests/test_hip_gru.py (8 against a
measured 2.1): it covers another summation order (the MFMA chain runs k ascending in one accumulator) and the device's expf / tanhf.

Everything else is bit for bit: run to run, the users permuted, a subset alone, the chunking, a history split in two and
continued through ``initial`` (for the LSTM with the cell states of ``return_cell``), a strided E, ``max_events`` against the
trimmed histories."""
import functools
import os

import numpy as np
import pytest
import torch

from test_hip_gru import _lengths
from test_lstm_rnn_cpu import lstm_reference, rnn_reference

pytestmark = pytest.mark.gpu

SHAPES = [(300, 70, 70), (400, 96, 160), (300, 130, 260)]               # (articles, D, H): one padded column tile; two, D != H; three, two input K tiles
CELLS = ["lstm", "rnn"]
BOUND = {"lstm": 5.0, "rnn": 5.0}


def _cls(cell):
    from dae_rnn_news_recommendation_amd import helpers
    return helpers.LSTMUserModel if cell == "lstm" else helpers.RNNUserModel


@functools.lru_cache(maxsize=None)
def _case(cell, shape):
    """Inputs, the float64 truth and the float32 yardstick of a cell and shape: computed once, shared by every test, never written to."""
    Na, D, H = shape
    rng = np.random.default_rng(Na + D + H)
    E = rng.standard_normal((Na, D)).astype(np.float32)
    torch.manual_seed(Na + H)
    cls = _cls(cell)
    model = cls.from_torch((torch.nn.LSTM if cell == "lstm" else torch.nn.RNN)(D, H))      # torch's default initialisation, seeded
    n = _lengths(rng)
    rows = []
    for L in n:
        r = rng.integers(0, Na, L)
        if L >= 4:
            r[L // 2] = r[0]                                           # an article read twice,
            r[L - 1] = r[L - 2]                                        # and twice in a row
        rows.append(r)
    indptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    items = np.concatenate(rows).astype(np.int64)
    w = [getattr(model, k) for k in cls.NAMES]
    ref = lstm_reference if cell == "lstm" else rnn_reference
    truth = ref(E, *w, indptr, items)
    yard = ref(E, *w, indptr, items, dtype=np.float32)
    for a in (indptr, items) + truth + yard:
        a.setflags(write=False)
    return dict(E=E, model=model, indptr=indptr, items=items, truth=truth, yard=yard, n=n)


def _run(cell, hist, E, model, **kw):
    """The states of a call as a tuple of arrays: (U,) for the RNN, (U, C) for the LSTM."""
    from dae_rnn_news_recommendation_amd import helpers
    if cell == "lstm":
        return tuple(helpers.lstm_user_states(hist, E, model, return_cell=True, **kw))
    return (helpers.rnn_user_states(hist, E, model, **kw),)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cell", CELLS)
def test_states_against_float64(cell, shape):
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(cell, shape)
    hist = (c["indptr"], c["items"])
    every = _run(cell, hist, c["E"], c["model"], all_states=True)
    last = _run(cell, hist, c["E"], c["model"])
    H, M = shape[2], c["n"].size
    assert every[0].dtype == np.float32 and every[0].shape == (c["items"].size, H)
    assert all(a.dtype == np.float32 and a.shape == (M, H) for a in last + every[1:])
    assert all(np.isfinite(a).all() for a in every + last)
    checks = [("all states", every[0], 0), ("last states", last[0], 1)] + ([("last cells", last[1], 2)] if cell == "lstm" else [])
    ratios = []
    for name, got, k in checks:
        want, yard = c["truth"][k], c["yard"][k]
        err = float(np.abs(got.astype(np.float64) - want).max())
        ref = float(np.abs(yard.astype(np.float64) - want).max())
        print("%s %s %s: kernel %.2f x 2^-24, float32 NumPy %.2f x 2^-24, ratio %.3f" % (cell, shape, name, err * 2 ** 24, ref * 2 ** 24, err / ref))
        ratios.append((name, err, ref))
    for name, err, ref in ratios:
        assert err <= BOUND[cell] * ref, (name, err / ref)
    # structure: a user's last all_states row is its last-state row, an empty history is the zero vector, C does not depend on all_states
    ends, has = c["indptr"][1:] - 1, c["n"] > 0
    assert np.array_equal(_bits(every[0][ends[has]]), _bits(last[0][has]))
    assert (c["n"] == 0).sum() == 3 and all((_bits(a[~has]) == 0).all() for a in last)
    assert _all_same(every[1:], last[1:])
    # return_cell is an addition: without it the LSTM returns the states alone, with the same bits
    fn = helpers.lstm_user_states if cell == "lstm" else helpers.rnn_user_states
    assert _same(fn(hist, c["E"], c["model"]), last[0]) and _same(c["model"].states(hist, c["E"], all_states=True), every[0])
    # tensors come back on request, with the same bits
    t = _run(cell, hist, c["E"], c["model"], return_tensor=True)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 for x in t)
    assert _all_same(tuple(x.cpu().numpy() for x in t), last)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cell", CELLS)
def test_a_users_states_do_not_depend_on_the_call(cell, shape):
    c = _case(cell, shape)
    E, model, indptr, items = c["E"], c["model"], c["indptr"], c["items"]
    M = c["n"].size
    rows = [items[indptr[u]:indptr[u + 1]] for u in range(M)]
    every = _run(cell, (indptr, items), E, model, all_states=True)
    last = _run(cell, (indptr, items), E, model)
    # run to run
    assert _all_same(_run(cell, (indptr, items), E, model, all_states=True), every)
    assert _all_same(_run(cell, (indptr, items), E, model), last)
    # the users in another order: other tiles, other rows of a tile
    perm = np.random.default_rng(1).permutation(M)
    assert _all_same(_run(cell, [rows[u] for u in perm], E, model), tuple(a[perm] for a in last))
    got = _run(cell, [rows[u] for u in perm], E, model, all_states=True)
    assert _same(got[0], np.concatenate([every[0][indptr[u]:indptr[u + 1]] for u in perm]))
    assert _all_same(got[1:], tuple(a[perm] for a in last[1:]))
    # a subset of the users alone: other launches (every step has fewer active users)
    sub = np.sort(np.random.default_rng(2).choice(M, 40, replace=False))
    assert _all_same(_run(cell, [rows[u] for u in sub], E, model), tuple(a[sub] for a in last))
    one = int(np.argmax(c["n"]))                                        # the longest history on its own
    got = _run(cell, [rows[one]], E, model, all_states=True)
    assert _same(got[0], every[0][indptr[one]:indptr[one + 1]]) and _all_same(got[1:], tuple(a[one:one + 1] for a in last[1:]))
    # chunks of 100 users against one chunk
    assert _all_same(_run(cell, (indptr, items), E, model, batch_users=100), last)
    assert _all_same(_run(cell, (indptr, items), E, model, batch_users=100, all_states=True), every)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cell", CELLS)
def test_continuing_from_stored_states(cell, shape):
    """Every history split in two: the states of the first half -- for the LSTM (h, c) from ``return_cell`` -- handed back as
    ``initial`` continue to the bits of the unsplit run."""
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(cell, shape)
    E, model, indptr, items = c["E"], c["model"], c["indptr"], c["items"]
    M, H = c["n"].size, shape[2]
    rows = [items[indptr[u]:indptr[u + 1]] for u in range(M)]
    every = _run(cell, (indptr, items), E, model, all_states=True)
    last = _run(cell, (indptr, items), E, model)
    first, second = [r[:r.size // 2] for r in rows], [r[r.size // 2:] for r in rows]
    mid = _run(cell, first, E, model, return_tensor=True)
    init = mid if cell == "lstm" else mid[0]
    assert _all_same(_run(cell, second, E, model, initial=init), last)                          # device tensors ...
    init = tuple(x.cpu().numpy() for x in mid) if cell == "lstm" else mid[0].cpu().numpy()
    tail = _run(cell, second, E, model, initial=init, all_states=True)                          # ... or arrays
    assert _same(tail[0], np.concatenate([every[0][indptr[u] + rows[u].size // 2:indptr[u + 1]] for u in range(M)]))
    assert _all_same(tail[1:], last[1:])
    grew = np.array([0 < r.size // 2 for r in rows])                    # users whose first half holds an event
    if cell == "lstm":                                                  # h alone is not the state: c matters
        got = helpers.lstm_user_states(second, E, model, initial=(mid[0], None))
        assert not np.array_equal(got[grew], last[0][grew])
    # an empty history keeps its initial rows; zeros as the initial rows are the default
    rng = np.random.default_rng(3)
    h0, c0 = rng.standard_normal((M, H)).astype(np.float32), rng.standard_normal((M, H)).astype(np.float32)
    got = _run(cell, (indptr, items), E, model, initial=(h0, c0) if cell == "lstm" else h0)
    empty = c["n"] == 0
    assert np.array_equal(_bits(got[0][empty]), _bits(h0[empty])) and not np.array_equal(got[0][~empty], last[0][~empty])
    zeros = np.zeros((M, H), np.float32)
    if cell == "lstm":
        assert np.array_equal(_bits(got[1][empty]), _bits(c0[empty])) and not np.array_equal(got[1][~empty], last[1][~empty])
        for init in ((zeros, zeros), (zeros, None), (None, zeros), (None, None)):
            assert _all_same(_run(cell, (indptr, items), E, model, initial=init), last)
        only_c = _run(cell, (indptr, items), E, model, initial=(None, c0))                      # c0 without h0: the first step skips its K loop
        assert _all_same(only_c, _run(cell, (indptr, items), E, model, initial=(zeros, c0)))
        assert np.array_equal(_bits(only_c[1][empty]), _bits(c0[empty])) and (_bits(only_c[0][empty]) == 0).all()
    else:
        assert _all_same(_run(cell, (indptr, items), E, model, initial=zeros), last)


@pytest.mark.parametrize("cell", CELLS)
def test_strided_embeddings_are_read_in_place(cell):
    c = _case(cell, SHAPES[0])
    D = SHAPES[0][1]
    wide = torch.full((c["E"].shape[0], D + 13), float("nan"), device="cuda")
    wide[:, 5:5 + D] = torch.from_numpy(c["E"]).cuda()
    view = wide[:, 5:5 + D]                                             # lde = D + 13, not 16-byte aligned
    assert view.stride(0) == D + 13 and not view.is_contiguous()
    hist = (c["indptr"], c["items"])
    assert _all_same(_run(cell, hist, view, c["model"], all_states=True), _run(cell, hist, c["E"], c["model"], all_states=True))
    assert _all_same(_run(cell, hist, view, c["model"]), _run(cell, hist, c["E"], c["model"]))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
@pytest.mark.parametrize("cell", CELLS)
def test_max_events_equals_the_trimmed_histories(cell, shape):
    c = _case(cell, shape)
    E, model, indptr, items = c["E"], c["model"], c["indptr"], c["items"]
    rows = [items[indptr[u]:indptr[u + 1]][-10:] for u in range(c["n"].size)]
    got = _run(cell, (indptr, items), E, model, max_events=10)
    assert _all_same(got, _run(cell, rows, E, model))
    assert not _same(got[0], _run(cell, (indptr, items), E, model)[0])
    with pytest.raises(ValueError, match="max_events"):
        _run(cell, (indptr, items), E, model, max_events=10, all_states=True)


@pytest.mark.parametrize("cell", CELLS)
def test_edge_cases_and_errors(cell):
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(cell, SHAPES[1])
    E, model, H = c["E"], c["model"], SHAPES[1][2]
    fn = helpers.lstm_user_states if cell == "lstm" else helpers.rnn_user_states
    assert fn([], E, model).shape == (0, H)
    assert fn([[], []], E, model, all_states=True).shape == (0, H)
    assert all(a.shape == (2, H) and (a == 0).all() for a in _run(cell, [[], []], E, model))
    if cell == "lstm":                                                  # no event at all: C is the initial c
        c0 = np.arange(2 * H, dtype=np.float32).reshape(2, H)
        U, C = helpers.lstm_user_states([[], []], E, model, all_states=True, return_cell=True, initial=(None, c0))
        assert U.shape == (0, H) and _same(C, c0)
        U, C = helpers.lstm_user_states([[], []], E, model, return_cell=True, initial=(c0, c0))
        assert _same(U, c0) and _same(C, c0)
    with pytest.raises(ValueError, match="history items"):
        fn([[1, 2, 400]], torch.from_numpy(E).cuda(), model)
    with pytest.raises(ValueError, match="history items"):
        fn([[1, -1]], E, model)
    with pytest.raises(ValueError, match="columns"):
        fn([[1, 2]], torch.from_numpy(E[:, :50].copy()).cuda(), model)
    # the wrong model class for the function
    other = _case("rnn" if cell == "lstm" else "lstm", SHAPES[1])["model"]
    with pytest.raises(TypeError):
        fn([[1, 2]], E, other)
    with pytest.raises(TypeError):
        helpers.gru_user_states([[1, 2]], E, model)
    # H != D: recommend refuses the states
    states = fn([[1, 2]], E, model)
    assert states.shape == (1, H) and H != E.shape[1]
    with pytest.raises(ValueError, match="candidates have %d columns, in_df has %d" % (E.shape[1], H)):
        helpers.recommend(states, E, k=3)


@pytest.mark.parametrize("cell", CELLS)
def test_evaluate_every_click_takes_the_model(cell):
    """evaluate_every_click(model=LSTMUserModel / RNNUserModel): the metrics of the model's all_states rows ranked by
    recommend_ranks_every_click, in user batches or at once."""
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(cell, SHAPES[0])                                          # D = H
    E, model = c["E"], c["model"]
    hist = (c["indptr"], c["items"])
    S = _run(cell, hist, E, model, all_states=True, return_tensor=True)[0]
    rank, score, n_cand, targets = helpers.recommend_ranks_every_click(S, E, hist)
    got = helpers.evaluate_every_click(hist, E, model, batch_users=100)
    assert np.array_equal(got["rank"], rank) and np.array_equal(_bits(got["score"]), _bits(score))
    assert np.array_equal(got["n_candidates"], n_cand) and np.array_equal(got["targets"], targets)
    assert got["metrics"] == helpers.rank_metrics(rank, n_cand, targets)
    assert got["metrics"]["n"] == int((c["n"][c["n"] > 0] - 1).sum())


def test_cli_lstm_user_model(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(5)
    W = str(tmp_path / "lstm.npz")
    helpers.LSTMUserModel.from_torch(torch.nn.LSTM(40, 40)).save(W)    # 800 features / compress factor 20
    common = ["--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4", "--sessions", "synthetic",
              "--recommend", "10", "--rank_metrics", "--similarity", "False"]
    users = 200

    def decay_files(d):
        return {f: dict(np.load(d + f)) for f in ("article_encoded_recommend10.npz", "article_encoded_ranks.npz")}

    model = cli.main(["--model_name", "l"] + common + ["--user_model", "lstm", "--user_weights", W])
    out = capsys.readouterr().out
    d = model.data_dir
    emb = np.load(d + "article_encoded_train.npy")
    labels = helpers.read_file(d + "article_label_category_publish_name.pkl", data_type="pandas_series").to_numpy()
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
    indptr, items = synthetic_sessions(users, np.unique(np.asarray(labels), return_inverse=True)[1], mean_len=12, seed=4)
    hist = [items[indptr[u]:indptr[u + 1] - 1] for u in range(users)]
    with_flag = decay_files(d)
    g, gk = np.load(d + "article_encoded_recommend10_lstm.npz"), np.load(d + "article_encoded_ranks_lstm.npz")
    assert sorted(g.files) == ["indices", "scores", "targets"] and sorted(gk.files) == ["n_candidates", "rank", "score", "targets"]
    assert g["indices"].shape == (users, 10) and g["indices"].dtype == np.int64 and g["scores"].shape == (users, 10)
    assert np.array_equal(g["targets"], with_flag["article_encoded_recommend10.npz"]["targets"]) and gk["rank"].shape == (users,)
    states = helpers.lstm_user_states(hist, emb, helpers.LSTMUserModel.load(W))
    idx, _ = helpers.recommend(states, emb, k=10, seen=hist)
    assert np.array_equal(g["indices"], idx)
    assert out.count("\n  hit@10 ") == 3 and "lstm user state" in out and "decayed user state" in out and out.count("  ranks ") == 3
    # the default stays what it was: no LSTM output, the same decay files
    model = cli.main(["--model_name", "p"] + common)
    out = capsys.readouterr().out
    plain = decay_files(model.data_dir)
    for f in plain:
        assert sorted(plain[f]) == sorted(with_flag[f])
        assert all(_same(plain[f][k], with_flag[f][k]) for k in plain[f]), f
    assert "lstm" not in out and out.count("\n  hit@10 ") == 2
    assert not [f for f in os.listdir(model.data_dir) if "lstm" in f]
    assert sorted(os.listdir(model.data_dir)) == sorted(f for f in os.listdir(d) if "lstm" not in f)
    with pytest.raises(AssertionError):
        cli.main(["--model_name", "q"] + common + ["--user_model", "lstm"])                    # no weights
    with pytest.raises(AssertionError):
        cli.main(["--model_name", "q"] + common + ["--user_model", "rnn", "--gru_weights", W])  # --gru_weights is the GRU's
