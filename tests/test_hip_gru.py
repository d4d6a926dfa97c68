"""GPU checks of the GRU user states (dae_gru_user_states through helpers.gru_user_states).

Truth: ``gru_reference`` of tests/test_gru_cpu.py in float64 (there pinned to torch.nn.GRU in float64 to 1e-12).  Yardstick: the
same restatement run in NumPy float32 on the same inputs -- what a straightforward fp32 implementation of the formula loses.
The kernel's worst absolute error, over all states and over the last states, must stay within 8 x the yardstick's worst error
on the case: torch.nn.GRU in float32 on the CPU sits at 2.1 x the yardstick on these inputs, so the bound leaves a factor of
about four for another summation order (the MFMA chain runs k ascending in one accumulator) and the device's expf / tanhf.

Everything else is bit for bit: run to run, the users permuted, a subset alone, the chunking, a history split in two and
continued through ``initial``, a strided E, ``max_events`` against the trimmed histories."""
import functools
import os

import numpy as np
import pytest
import torch

from test_gru_cpu import gru_reference

pytestmark = pytest.mark.gpu

SHAPES = [(300, 70, 70), (1000, 500, 500), (400, 96, 160)]             # (articles, D, H)


def _lengths(rng):
    """~300 users over more than two 128-user tiles.  127 users have at least 6 events, one has exactly 5 and one exactly 4, so
    step 3 runs 129 active users, step 4 runs 128 and step 5 runs 127; the rest have 1 to 3 events or none."""
    long = [63, 64, 65, 130, 300] + rng.integers(6, 10, 122).tolist()  # 127 users with >= 6 events
    n = np.array([0] + long + [5, 4] + rng.integers(1, 4, 170).tolist() + [0, 0])
    n = np.concatenate([n[:1], rng.permutation(n[1:])])                # an empty user first, the rest in any order
    active = [(n > t).sum() for t in range(7)]
    assert active[3] == 129 and active[4] == 128 and active[5] == 127 and active[0] > 256
    return n


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, the float64 truth and the float32 yardstick of a shape: computed once, shared by every test, never written to."""
    Na, D, H = shape
    rng = np.random.default_rng(Na + D + H)
    E = rng.standard_normal((Na, D)).astype(np.float32)
    torch.manual_seed(Na + H)
    from dae_rnn_news_recommendation_amd.helpers import GRUUserModel
    model = GRUUserModel.from_torch(torch.nn.GRU(D, H))                # torch's default initialisation, seeded
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
    w = [getattr(model, k) for k in GRUUserModel.NAMES]
    truth = gru_reference(E, *w, indptr, items)
    yard = gru_reference(E, *w, indptr, items, dtype=np.float32)
    for a in (indptr, items) + truth + yard:
        a.setflags(write=False)
    return dict(E=E, model=model, indptr=indptr, items=items, truth=truth, yard=yard, n=n)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("shape", SHAPES)
def test_states_against_float64(shape):
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(shape)
    hist = (c["indptr"], c["items"])
    every = helpers.gru_user_states(hist, c["E"], c["model"], all_states=True)
    last = helpers.gru_user_states(hist, c["E"], c["model"])
    H = shape[2]
    assert every.dtype == np.float32 and every.shape == (c["items"].size, H)
    assert last.dtype == np.float32 and last.shape == (c["n"].size, H)
    assert np.isfinite(every).all() and np.isfinite(last).all()
    for name, got, want, yard in (("all states", every, c["truth"][0], c["yard"][0]), ("last states", last, c["truth"][1], c["yard"][1])):
        err = float(np.abs(got.astype(np.float64) - want).max())
        ref = float(np.abs(yard.astype(np.float64) - want).max())
        print("%s %s: kernel %.2f x 2^-24, float32 NumPy %.2f x 2^-24, ratio %.3f" % (shape, name, err * 2 ** 24, ref * 2 ** 24, err / ref))
        assert err <= 8.0 * ref, (name, err / ref)
    # structure: a user's last all_states row is its last-state row, an empty history is the zero vector
    ends, has = c["indptr"][1:] - 1, c["n"] > 0
    assert np.array_equal(_bits(every[ends[has]]), _bits(last[has]))
    assert (c["n"] == 0).sum() == 3 and (_bits(last[~has]) == 0).all()
    # a tensor comes back on request, with the same bits
    t = helpers.gru_user_states(hist, c["E"], c["model"], return_tensor=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and _same(t.cpu().numpy(), last)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_users_states_do_not_depend_on_the_call(shape):
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(shape)
    E, model, indptr, items = c["E"], c["model"], c["indptr"], c["items"]
    M = c["n"].size
    rows = [items[indptr[u]:indptr[u + 1]] for u in range(M)]
    every = helpers.gru_user_states((indptr, items), E, model, all_states=True)
    last = helpers.gru_user_states((indptr, items), E, model)
    # run to run
    assert _same(helpers.gru_user_states((indptr, items), E, model, all_states=True), every)
    assert _same(helpers.gru_user_states((indptr, items), E, model), last)
    # the users in another order: other tiles, other rows of a tile
    perm = np.random.default_rng(1).permutation(M)
    assert _same(helpers.gru_user_states([rows[u] for u in perm], E, model), last[perm])
    got = helpers.gru_user_states([rows[u] for u in perm], E, model, all_states=True)
    assert _same(got, np.concatenate([every[indptr[u]:indptr[u + 1]] for u in perm]))
    # a subset of the users alone: other launches (every step has fewer active users)
    sub = np.sort(np.random.default_rng(2).choice(M, 40, replace=False))
    assert _same(helpers.gru_user_states([rows[u] for u in sub], E, model), last[sub])
    one = int(np.argmax(c["n"]))                                        # the longest history on its own
    assert _same(helpers.gru_user_states([rows[one]], E, model, all_states=True), every[indptr[one]:indptr[one + 1]])
    # chunks of 100 users against one chunk
    assert _same(helpers.gru_user_states((indptr, items), E, model, batch_users=100), last)
    assert _same(helpers.gru_user_states((indptr, items), E, model, batch_users=100, all_states=True), every)


@pytest.mark.parametrize("shape", SHAPES)
def test_continuing_from_stored_states(shape):
    """Every history split in two: the states of the first half, handed back as ``initial``, continue to the bits of the unsplit run."""
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(shape)
    E, model, indptr, items = c["E"], c["model"], c["indptr"], c["items"]
    M, H = c["n"].size, shape[2]
    rows = [items[indptr[u]:indptr[u + 1]] for u in range(M)]
    every = helpers.gru_user_states((indptr, items), E, model, all_states=True)
    last = helpers.gru_user_states((indptr, items), E, model)
    first, second = [r[:r.size // 2] for r in rows], [r[r.size // 2:] for r in rows]
    mid = helpers.gru_user_states(first, E, model, return_tensor=True)
    assert _same(helpers.gru_user_states(second, E, model, initial=mid), last)                 # a device tensor ...
    tail = helpers.gru_user_states(second, E, model, initial=mid.cpu().numpy(), all_states=True)   # ... or an array
    assert _same(tail, np.concatenate([every[indptr[u] + rows[u].size // 2:indptr[u + 1]] for u in range(M)]))
    # an empty history keeps its initial row; zeros as the initial rows are the default
    h0 = np.random.default_rng(3).standard_normal((M, H)).astype(np.float32)
    got = helpers.gru_user_states((indptr, items), E, model, initial=h0)
    assert np.array_equal(_bits(got[c["n"] == 0]), _bits(h0[c["n"] == 0]))
    assert not np.array_equal(got[c["n"] > 0], last[c["n"] > 0])
    assert _same(helpers.gru_user_states((indptr, items), E, model, initial=np.zeros((M, H), np.float32)), last)


def test_strided_embeddings_are_read_in_place():
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(SHAPES[0])
    D = SHAPES[0][1]
    wide = torch.full((c["E"].shape[0], D + 13), float("nan"), device="cuda")
    wide[:, 5:5 + D] = torch.from_numpy(c["E"]).cuda()
    view = wide[:, 5:5 + D]                                             # lde = D + 13, not 16-byte aligned
    assert view.stride(0) == D + 13 and not view.is_contiguous()
    hist = (c["indptr"], c["items"])
    assert _same(helpers.gru_user_states(hist, view, c["model"], all_states=True),
                 helpers.gru_user_states(hist, c["E"], c["model"], all_states=True))
    assert _same(helpers.gru_user_states(hist, view, c["model"]), helpers.gru_user_states(hist, c["E"], c["model"]))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_max_events_equals_the_trimmed_histories(shape):
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(shape)
    E, model, indptr, items = c["E"], c["model"], c["indptr"], c["items"]
    rows = [items[indptr[u]:indptr[u + 1]][-10:] for u in range(c["n"].size)]
    got = helpers.gru_user_states((indptr, items), E, model, max_events=10)
    assert _same(got, helpers.gru_user_states(rows, E, model))
    assert not _same(got, helpers.gru_user_states((indptr, items), E, model))
    with pytest.raises(ValueError, match="max_events"):
        helpers.gru_user_states((indptr, items), E, model, max_events=10, all_states=True)


def test_edge_cases_and_errors():
    from dae_rnn_news_recommendation_amd import helpers
    c = _case(SHAPES[2])
    E, model, H = c["E"], c["model"], SHAPES[2][2]
    assert helpers.gru_user_states([], E, model).shape == (0, H)
    assert helpers.gru_user_states([[], []], E, model, all_states=True).shape == (0, H)
    assert (helpers.gru_user_states([[], []], E, model) == 0).all()
    with pytest.raises(ValueError, match="history items"):
        helpers.gru_user_states([[1, 2, 400]], torch.from_numpy(E).cuda(), model)
    with pytest.raises(ValueError, match="history items"):
        helpers.gru_user_states([[1, -1]], E, model)
    with pytest.raises(ValueError, match="columns"):
        helpers.gru_user_states([[1, 2]], torch.from_numpy(E[:, :50].copy()).cuda(), model)
    # H != D: recommend refuses the states
    with pytest.raises(Exception):
        helpers.recommend(helpers.gru_user_states([[1, 2]], E, model), E, k=3)


def test_cli_gru_user_model(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(5)
    W = str(tmp_path / "gru.npz")
    helpers.GRUUserModel.from_torch(torch.nn.GRU(40, 40)).save(W)      # 800 features / compress factor 20
    common = ["--num_epochs", "1", "--train_row", "400", "--max_features", "800", "--seed", "4", "--sessions", "synthetic",
              "--recommend", "10", "--rank_metrics", "--similarity", "False"]
    users = 200

    def decay_files_are_the_decay_models(d):
        emb = np.load(d + "article_encoded_train.npy")
        r, k = np.load(d + "article_encoded_recommend10.npz"), np.load(d + "article_encoded_ranks.npz")
        assert sorted(r.files) == ["indices", "scores", "targets"] and sorted(k.files) == ["n_candidates", "rank", "score", "targets"]
        labels = helpers.read_file(d + "article_label_category_publish_name.pkl", data_type="pandas_series").to_numpy()
        from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
        indptr, items = synthetic_sessions(users, np.unique(np.asarray(labels), return_inverse=True)[1], mean_len=12, seed=4)
        hist = [items[indptr[u]:indptr[u + 1] - 1] for u in range(users)]
        states = helpers.user_states(hist, emb, 0.9)
        idx, score = helpers.recommend(states, emb, k=10, seen=hist)
        assert _same(r["indices"], idx) and _same(r["scores"], score)
        rank, rscore, _ = helpers.recommend_ranks(states, emb, r["targets"], seen=hist)
        assert _same(k["rank"], rank) and _same(k["score"], rscore)
        return emb, hist, r["targets"]

    model = cli.main(["--model_name", "g"] + common + ["--user_model", "gru", "--gru_weights", W])
    out = capsys.readouterr().out
    d = model.data_dir
    emb, hist, targets = decay_files_are_the_decay_models(d)
    g, gk = np.load(d + "article_encoded_recommend10_gru.npz"), np.load(d + "article_encoded_ranks_gru.npz")
    assert g["indices"].shape == (users, 10) and g["indices"].dtype == np.int64 and g["scores"].shape == (users, 10)
    assert np.array_equal(g["targets"], targets) and gk["rank"].shape == (users,)
    states = helpers.gru_user_states(hist, emb, helpers.GRUUserModel.load(W))
    idx, _ = helpers.recommend(states, emb, k=10, seen=hist)
    assert np.array_equal(g["indices"], idx)
    assert out.count("\n  hit@10 ") == 3 and "gru user state" in out and "decayed user state" in out and out.count("  ranks ") == 3
    # the default stays what it was: no GRU output, the same decay files
    model = cli.main(["--model_name", "p"] + common)
    out = capsys.readouterr().out
    decay_files_are_the_decay_models(model.data_dir)
    assert "gru" not in out and out.count("\n  hit@10 ") == 2
    assert not [f for f in os.listdir(model.data_dir) if "gru" in f]
    assert sorted(f for f in os.listdir(model.data_dir)) == sorted(f for f in os.listdir(d) if "gru" not in f)
    with pytest.raises(AssertionError):
        cli.main(["--model_name", "q"] + common + ["--user_model", "gru"])                     # no weights
