"""helpers._competitors, the host bookkeeping of target_ranks (how many candidates compete in a row, which targets can never be
returned), against a brute-force count over an explicit boolean admissibility matrix.  No GPU, no library."""
import numpy as np
import pytest

from dae_rnn_news_recommendation_amd.helpers import _competitors, normalize_exclusions, normalize_window


def _case(seed, Nq, Nc, self_mode, with_excl, with_window):
    """Seeded inputs that hit every special case: rows without a target, targets equal to the row index, lists that hold the
    target and / or the row itself (and lists that hold neither, and empty ones), empty windows, windows that miss the target."""
    rng = np.random.default_rng(seed)
    tgt = rng.integers(0, Nc, Nq)
    tgt[rng.random(Nq) < 0.15] = -1
    if self_mode:
        own = rng.random(Nq) < 0.2
        tgt[own] = np.arange(Nq)[own]                              # the target is the row itself
    lists = None
    if with_excl:
        lists = []
        for i in range(Nq):
            items = list(rng.integers(0, Nc, rng.integers(0, 9)))
            if tgt[i] >= 0 and rng.random() < 0.3:
                items.append(int(tgt[i]))                          # the target is in its own row's list
            if self_mode and rng.random() < 0.3:
                items.append(i)                                    # and so is the row
            lists.append(items)
        lists[0] = []
    window = None
    if with_window:
        lo = rng.integers(0, Nc + 1, Nq)
        hi = np.minimum(lo + rng.integers(0, Nc // 2, Nq), Nc)
        hi[::7] = lo[::7]                                          # empty windows
        hit = (tgt >= 0) & (rng.random(Nq) < 0.5)                  # half of the others are made to hold the target
        lo[hit] = np.minimum(lo[hit], tgt[hit])
        hi[hit] = np.maximum(hi[hit], tgt[hit] + 1)
        window = (lo, hi)
    return tgt.astype(np.int64), lists, window


def _brute(tgt, Nq, Nc, exclude_self, lists, window):
    j = np.arange(Nc)[None, :]
    i = np.arange(Nq)[:, None]
    admissible = np.ones((Nq, Nc), dtype=bool)                     # what most_similar could return in the row
    if window is not None:
        admissible &= (j >= np.asarray(window[0])[:, None]) & (j < np.asarray(window[1])[:, None])
    in_window = admissible.copy()
    if lists is not None:
        for r, items in enumerate(lists):
            admissible[r, [x for x in items if 0 <= x < Nc]] = False
    if exclude_self:
        admissible &= j != i
    is_target = j == tgt[:, None]
    n_cand = (admissible | (in_window & is_target)).sum(axis=1)    # the target counts wherever the window holds it
    barred = np.array([t >= 0 and not admissible[r, t] for r, t in enumerate(tgt)])
    return n_cand.astype(np.int64), barred


@pytest.mark.parametrize("with_window", [False, True])
@pytest.mark.parametrize("with_excl", [False, True])
@pytest.mark.parametrize("self_mode, exclude_self", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_competitors_match_a_brute_force_count(seed, self_mode, exclude_self, with_excl, with_window):
    Nq, Nc = (48, 48) if self_mode else (40, 60)
    tgt, lists, window = _case(seed, Nq, Nc, self_mode, with_excl, with_window)
    xp, xi = normalize_exclusions(lists, Nq, Nc) if lists is not None else (None, None)
    win = normalize_window(window, Nq, Nc) if window is not None else None
    n_cand, barred = _competitors(tgt, Nq, Nc, exclude_self, xp, xi, win)
    want_n, want_b = _brute(tgt, Nq, Nc, exclude_self, lists, window)
    assert n_cand.dtype == np.int64 and barred.dtype == bool
    assert np.array_equal(n_cand, want_n), np.flatnonzero(n_cand != want_n)
    assert np.array_equal(barred, want_b), np.flatnonzero(barred != want_b)
    if with_window:                                                # the cases are what they claim to be
        assert (win[0] == win[1]).any() and (barred & (tgt >= 0) & ~((tgt >= win[0]) & (tgt < win[1]))).any()
    if with_excl:
        in_list = np.array([t in l for t, l in zip(tgt, lists)])
        assert in_list.any() and (~in_list & (tgt >= 0)).any()
        if self_mode:
            own = np.array([r in l for r, l in enumerate(lists)])
            assert own.any() and (~own).any()
    if self_mode:
        assert (tgt == np.arange(Nq)).any()


@pytest.mark.parametrize("with_excl", [False, True])
@pytest.mark.parametrize("self_mode, exclude_self", [(False, False), (True, False), (True, True)])
def test_no_window_is_the_full_window(self_mode, exclude_self, with_excl):
    Nq, Nc = (48, 48) if self_mode else (40, 60)
    tgt, lists, _ = _case(3, Nq, Nc, self_mode, with_excl, False)
    xp, xi = normalize_exclusions(lists, Nq, Nc) if lists is not None else (None, None)
    full = normalize_window((np.zeros(Nq, int), np.full(Nq, Nc)), Nq, Nc)
    a, b = _competitors(tgt, Nq, Nc, exclude_self, xp, xi, None), _competitors(tgt, Nq, Nc, exclude_self, xp, xi, full)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype
