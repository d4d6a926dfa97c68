"""GPU checks of the decayed user states (dae_user_states through helpers.user_states).  Truth: the recurrence of the header,

    s = 0, z = 0;  for every event e of the user, oldest first:  s = d_e * s + E[items[e]];  z = d_e * z + 1;  state_e = s / z

restated in float64 below (``_truth``).  Tolerance, per element, for a user with L events: 4 * (L + 1) * 2**-24 * max|E| -- two
roundings per step on s, two on z, one division, to first order, times two (derived, not tuned; a float32 NumPy emulation of
the recurrence over L in 1..1000 and beta in {1, 0.9, 0.5} stays below 0.08 of it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 63, 64, 65, 1000, 0, 7, 130, 33, 1, 256]


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
    return indptr, np.concatenate(rows).astype(np.int64)


def _truth(E, indptr, items, d):
    """float64 states after every event [nnz x H], last states [M x H], and the history length of every event's user."""
    E = np.asarray(E, np.float64)
    M, H = len(indptr) - 1, E.shape[1]
    every = np.zeros((len(items), H))
    last = np.zeros((M, H))
    length = np.zeros(len(items), np.int64)
    for u in range(M):
        s, z = np.zeros(H), 0.0
        for e in range(indptr[u], indptr[u + 1]):
            de = 0.0 if e == indptr[u] else float(d[e])
            s = de * s + E[items[e]]
            z = de * z + 1.0
            every[e] = s / z
        if indptr[u + 1] > indptr[u]:
            last[u] = every[indptr[u + 1] - 1]
        length[indptr[u]:indptr[u + 1]] = indptr[u + 1] - indptr[u]
    return every, last, length


def _assert_close(got_all, got_last, E, indptr, items, d):
    every, last, length = _truth(E, indptr, items, d)
    amax = float(np.abs(E).max())
    L = np.diff(indptr)
    err_last = np.abs(got_last.astype(np.float64) - last).max(axis=1)
    bound_last = 4.0 * (L + 1) * 2.0 ** -24 * amax
    print("last states: worst error / bound = %.3f" % float((err_last / bound_last).max()))
    assert (err_last <= bound_last).all(), (err_last / bound_last).max()
    err_all = np.abs(got_all.astype(np.float64) - every).max(axis=1)
    bound_all = 4.0 * (length + 1) * 2.0 ** -24 * amax
    print("all states:  worst error / bound = %.3f" % float((err_all / bound_all).max()))
    assert (err_all <= bound_all).all(), (err_all / bound_all).max()
    assert (got_last[L == 0] == 0).all()                                   # an empty history is the zero vector


@pytest.mark.parametrize("shape", [(300, 70), (1000, 500)])
@pytest.mark.parametrize("beta", [1.0, 0.9, 0.5, 0.0])
def test_scalar_beta_against_float64(shape, beta):
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(shape[1] + int(beta * 10))
    E = rng.standard_normal(shape).astype(np.float32)
    indptr, items = _histories(rng, shape[0])
    last = helpers.user_states((indptr, items), E, beta)
    every = helpers.user_states((indptr, items), E, beta, all_states=True)
    assert last.shape == (len(LENGTHS), shape[1]) and every.shape == (len(items), shape[1])
    assert last.dtype == np.float32 and every.dtype == np.float32
    _assert_close(every, last, E, indptr, items, np.full(len(items), np.float32(beta), np.float32))


@pytest.mark.parametrize("shape", [(300, 70), (1000, 500)])
def test_per_event_factors_against_float64(shape):
    """Time-based decay: factors beta ** (dt / unit) from timestamps, with simultaneous events (factor 1) and, through beta = 0
    plus a gap, session resets (factor 0)."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(21)
    E = rng.standard_normal(shape).astype(np.float32)
    indptr, items = _histories(rng, shape[0])
    gaps = rng.choice([0.0, 0.5, 1.0, 3.0, 40.0], len(items))
    t = np.cumsum(gaps)                                                    # non-decreasing over the whole log, so within every user
    for beta, unit in ((0.8, 2.0), (0.0, None)):
        d = helpers.decay_factors(indptr, t, beta, unit)
        assert (d == 1).any() and ((d == 0).any() or beta > 0)
        last = helpers.user_states((indptr, items), E, beta, timestamps=t, time_unit=unit)
        every = helpers.user_states((indptr, items), E, beta, timestamps=t, time_unit=unit, all_states=True)
        _assert_close(every, last, E, indptr, items, d)
    # the list-of-sequences form of histories and timestamps gives the same bits
    hl = [items[indptr[u]:indptr[u + 1]] for u in range(len(LENGTHS))]
    tl = [t[indptr[u]:indptr[u + 1]] for u in range(len(LENGTHS))]
    again = helpers.user_states(hl, E, 0.0, timestamps=tl)
    assert np.array_equal(again.view(np.int32), last.view(np.int32))


def test_exact_cases_bit_for_bit():
    """Small-integer embeddings: with beta = 1 every s and z is an exact integer, with beta = 0.5 and at most 16 events an exact
    dyadic number, so the state is float32(s) / float32(z), one correctly rounded division -- bit for bit."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(2)
    E = rng.integers(-8, 9, (200, 70)).astype(np.float32)
    for beta, lengths in ((1.0, LENGTHS), (0.5, [0, 1, 2, 3, 7, 15, 16, 16, 9])):
        indptr, items = _histories(rng, 200, lengths)
        want_all = np.zeros((len(items), 70), np.float32)
        want_last = np.zeros((len(lengths), 70), np.float32)
        for u in range(len(lengths)):
            s, z = np.zeros(70), 0.0
            for e in range(indptr[u], indptr[u + 1]):
                de = 0.0 if e == indptr[u] else beta
                s = de * s + E[items[e]].astype(np.float64)                # exact in float64, and representable in float32
                z = de * z + 1.0
                assert np.array_equal(s.astype(np.float32).astype(np.float64), s) and float(np.float32(z)) == z
                want_all[e] = s.astype(np.float32) / np.float32(z)
            if indptr[u + 1] > indptr[u]:
                want_last[u] = want_all[indptr[u + 1] - 1]
        last = helpers.user_states((indptr, items), E, beta)
        every = helpers.user_states((indptr, items), E, beta, all_states=True)
        assert np.array_equal(last.view(np.int32), want_last.view(np.int32)), beta
        assert np.array_equal(every.view(np.int32), want_all.view(np.int32)), beta


def test_modes_agree_runs_agree_users_permute():
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(8)
    E = rng.standard_normal((1000, 500)).astype(np.float32)
    indptr, items = _histories(rng, 1000)
    for kw in (dict(beta=0.9), dict(beta=0.7, timestamps=np.cumsum(rng.choice([0.0, 1.0, 2.5], len(items))))):
        last = helpers.user_states((indptr, items), E, **kw)
        every = helpers.user_states((indptr, items), E, all_states=True, **kw)
        L = np.diff(indptr)
        has = L > 0
        assert np.array_equal(every[indptr[1:][has] - 1].view(np.int32), last[has].view(np.int32))      # one arithmetic for both modes
        assert np.array_equal(helpers.user_states((indptr, items), E, **kw).view(np.int32), last.view(np.int32))
        assert np.array_equal(helpers.user_states((indptr, items), E, all_states=True, **kw).view(np.int32), every.view(np.int32))
        perm = rng.permutation(len(L))
        rows = [items[indptr[u]:indptr[u + 1]] for u in perm]
        kw2 = dict(kw)
        if "timestamps" in kw:
            kw2["timestamps"] = [kw["timestamps"][indptr[u]:indptr[u + 1]] for u in perm]
        assert np.array_equal(helpers.user_states(rows, E, **kw2).view(np.int32), last[perm].view(np.int32))


def test_strided_embeddings_are_read_in_place():
    """A column slice of a wider tensor: an unaligned one (H = 70 at column 10: the scalar path) and an aligned one (H = 64 at
    column 8 of a row of 100: the vector path) give the bits of their contiguous copies; tensors in, tensor out."""
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(4)
    wide = torch.from_numpy(rng.standard_normal((300, 100)).astype(np.float32)).cuda()
    indptr, items = _histories(rng, 300)
    for c0, c1 in ((10, 80), (8, 72)):
        view = wide[:, c0:c1]
        assert not view.is_contiguous()
        got = helpers.user_states((indptr, items), view, 0.9, return_tensor=True)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(LENGTHS), c1 - c0)
        want = helpers.user_states((indptr, items), view.contiguous().cpu().numpy(), 0.9)
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
        _assert_close(helpers.user_states((indptr, items), view, 0.9, all_states=True), want, view.cpu().numpy(), indptr, items,
                      np.full(len(items), np.float32(0.9)))


def test_caller_errors_raise_value_error():
    from dae_rnn_news_recommendation_amd import helpers
    E = np.ones((10, 8), np.float32)
    with pytest.raises(ValueError, match="history items must be in 0..9"):
        helpers.user_states([[1, 2, 10]], E)
    with pytest.raises(ValueError, match="history items must be in 0..9"):
        helpers.user_states([[1, -1]], E)
    with pytest.raises(ValueError, match="decrease within a user"):
        helpers.user_states([[1, 2, 3]], E, timestamps=[[0.0, 2.0, 1.0]])
    with pytest.raises(ValueError, match="beta"):
        helpers.user_states([[1, 2, 3]], E, beta=1.2)
    assert helpers.user_states([], E).shape == (0, 8)
    assert np.array_equal(helpers.user_states([[], [3]], E), np.array([[0.0] * 8, [1.0] * 8], np.float32))
