"""CPU checks of the list de-duplication (dae_dedup_lists, helpers.dedup_lists): both builds export the two symbols with the
header's arity, the workspace grows with the corpus and saturates in the number of lists, every argument error is reported
before any HIP call (so on a machine without a GPU), the float64 greedy reference of tests/dedup_reference.py on hand-made
cases, and the ValueErrors of recommend / most_similar, raised before the device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from dedup_reference import dedup_reference, near_tie_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_builds_export_the_symbols(fmt):
    lib = _lib(fmt)
    assert hasattr(lib, "dae_dedup_lists_workspace") and hasattr(lib, "dae_dedup_lists")


def test_arity_matches_the_header():
    from dae_rnn_news_recommendation_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dae_hip.h")).read(), flags=re.S)
    for name, want in (("dae_dedup_lists_workspace", 4), ("dae_dedup_lists", 19)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == want == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["dae_dedup_lists"][0] is ctypes.c_int32 and _lib.SIGNATURES["dae_dedup_lists_workspace"][0] is ctypes.c_uint64
    assert _lib.ABI_VERSION == 9


def test_workspace_grows_with_the_corpus_and_saturates_in_the_lists():
    ws = _lib().dae_dedup_lists_workspace
    D, Dp = 100, 128
    per_list = 128 * Dp * 4
    image = lambda Na: (Na + 127) // 128 * 128 * Dp * 4
    assert ws(1, 600, D, 32) == image(600) + per_list + 256               # the image, one list's rows, its validity mask
    assert ws(1, 6000, D, 32) - ws(1, 600, D, 32) == image(6000) - image(600)
    assert ws(10, 600, D, 32) - ws(1, 600, D, 32) == 9 * per_list
    assert ws(10, 600, D, 7) == ws(10, 600, D, 128)                       # a list is one 128-row tile whatever L
    cap = (256 << 20) // per_list                                         # lists whose rows fill 256 MiB
    at_cap = ws(cap, 600, D, 32)
    assert ws(cap - 1, 600, D, 32) < at_cap == ws(cap + 1, 600, D, 32) == ws(10 ** 8, 600, D, 32)
    assert at_cap - image(600) - (cap * 16 + 255) // 256 * 256 == 256 << 20
    assert ws(10 ** 8, 600, 500, 32) - image(600) * 4 <= (256 << 20) + (1 << 20)      # D = 500: wider rows, fewer lists
    assert ws(0, 600, D, 32) == 0 and ws(10, 0, D, 32) == 0 and ws(10, 600, 0, 32) == 0 and ws(10, 600, D, 0) == 0


def _call(lib, E=P, lde=None, Na=600, D=48, norm=0, metric=0, lists=P, ldl=None, Nr=10, L=32, k=10, threshold=0.5, out=P, ldo=None,
          counts=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_dedup_lists_workspace(Nr, Na, D, L)
    return lib.dae_dedup_lists(E, D if lde is None else lde, Na, D, norm, metric, lists, L if ldl is None else ldl, Nr, L, k, threshold,
                               out, out, k if ldo is None else ldo, counts, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(k=0), b"k must be in 1..L"),
    (dict(k=33), b"k must be in 1..L"),
    (dict(L=129, k=10, ws_bytes=1 << 30), b"L must be in 1..128"),
    (dict(L=0, k=1, ws_bytes=1 << 30), b"L must be in 1..128"),
    (dict(norm=4), b"norm must be"),
    (dict(norm=-1), b"norm must be"),
    (dict(metric=2), b"metric must be 0 (cosine) or 1 (linear kernel)"),
    (dict(threshold=float("nan")), b"threshold is NaN"),
    (dict(ldl=31), b"ldl"),
    (dict(ldo=9), b"ldo"),
    (dict(lde=47), b"bad input"),
    (dict(E=None), b"bad input"),
    (dict(lists=None), b"bad input"),
    (dict(out=None), b"bad input"),
    (dict(counts=None), b"bad input"),
    (dict(Nr=0, ws_bytes=1 << 30), b"bad input"),
    (dict(Na=2 ** 21, D=512, ws_bytes=1 << 40), b"corpus image exceeds 4 GiB"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
])
def test_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _call(lib, **kw) != 0
    assert msg in lib.dae_last_error(), lib.dae_last_error()


def test_the_smallest_accepted_workspace_is_the_image_and_one_list():
    """One byte less than dae_dedup_lists_workspace(1, ...) is refused, whatever Nr (the entry chunks the rows)."""
    lib = _lib()
    one = lib.dae_dedup_lists_workspace(1, 600, 48, 32)
    assert _call(lib, Nr=1000, ws_bytes=one - 1) != 0 and b"workspace too small" in lib.dae_last_error()


def _scores(n, pairs, value=1.0):
    S = np.eye(n)
    for a, b in pairs:
        S[a, b] = S[b, a] = value
    return S


def test_reference_hand_made_cases():
    # articles 0, 1, 2 are one story, 3 and 4 another, 5 and 6 stand alone
    S = _scores(7, [(0, 1), (0, 2), (1, 2), (3, 4)])
    idx, pos, cnt = dedup_reference([[0, 1, 3, 2, 4, 5, 6]], S, 4, 0.5)
    assert idx.tolist() == [[0, 3, 5, 6]] and pos.tolist() == [[0, 2, 5, 6]]
    assert cnt[0, 0] == 4
    assert idx.dtype == pos.dtype == cnt.dtype == np.int64


def test_reference_counts_pairs_among_the_first_k_only():
    S = _scores(7, [(0, 1), (0, 2), (1, 2), (3, 4)])
    # first k = 4 entries 0, 1, 3, 2: the pairs (1, 0), (2, 0), (2, 1) -> 3; (4, 3) lies at position 4, outside
    _, _, cnt = dedup_reference([[0, 1, 3, 2, 4, 5, 6]], S, 4, 0.5)
    assert cnt[0, 1] == 3
    _, _, cnt = dedup_reference([[0, 1, 3, 2, 4, 5, 6]], S, 7, 0.5)
    assert cnt.tolist() == [[4, 4]]
    _, _, cnt = dedup_reference([[0, 1, 3, 2, 4, 5, 6]], S, 1, 0.5)
    assert cnt.tolist() == [[1, 0]]


def test_reference_invalid_entries_repeats_and_short_rows():
    S = _scores(7, [(0, 1), (0, 2), (1, 2), (3, 4)])
    # -1 and 7 (= Na) are skipped, never kept and never counted; the second 5 is a duplicate of the first (S[5, 5] = 1)
    idx, pos, cnt = dedup_reference([[-1, 5, 7, 5, 0, -1, 1, 6]], S, 8, 0.5)
    assert idx.tolist() == [[5, 0, 6, -1, -1, -1, -1, -1]] and pos.tolist() == [[1, 4, 7, -1, -1, -1, -1, -1]]
    assert cnt.tolist() == [[3, 2]]                                        # (5, 5) and (1, 0)
    # k reached early: the walk stops, the rest of the row is never looked at
    idx, pos, cnt = dedup_reference([[5, 6, 0, 1]], S, 2, 0.5)
    assert idx.tolist() == [[5, 6]] and pos.tolist() == [[0, 1]] and cnt.tolist() == [[2, 0]]
    # fewer than k survivors: the tail is -1
    idx, pos, cnt = dedup_reference([[0, 1, 2, -1]], S, 3, 0.5)
    assert idx.tolist() == [[0, -1, -1]] and pos.tolist() == [[0, -1, -1]] and cnt.tolist() == [[1, 3]]
    # a row without a valid entry
    idx, pos, cnt = dedup_reference([[-1, -1, 9]], S, 2, 0.5)
    assert idx.tolist() == [[-1, -1]] and cnt.tolist() == [[0, 0]]
    # under the linear kernel a repeated index is a duplicate only if its own score reaches the threshold
    idx, _, _ = dedup_reference([[5, 5]], 0.25 * S, 2, 0.5)
    assert idx.tolist() == [[5, 5]]


def test_reference_threshold_is_inclusive_and_greedy_is_not_transitive():
    # a chain 0 ~ 1 ~ 2 with 0 and 2 unrelated: 1 goes (duplicate of the kept 0), 2 stays (1 was not kept)
    S = _scores(3, [(0, 1), (1, 2)], value=0.5)
    assert dedup_reference([[0, 1, 2]], S, 3, 0.5)[0].tolist() == [[0, 2, -1]]
    assert dedup_reference([[0, 1, 2]], S, 3, np.nextafter(0.5, 1.0))[0].tolist() == [[0, 1, 2]]
    assert near_tie_rows([[0, 1, 2], [0, 2, -1]], S, 0.5, 1e-9).tolist() == [True, False]


def test_value_errors_before_the_device():
    from dae_rnn_news_recommendation_amd import helpers
    rng = np.random.default_rng(0)
    U, E = rng.standard_normal((5, 8)).astype(np.float32), rng.standard_normal((50, 8)).astype(np.float32)
    for call in (lambda **kw: helpers.recommend(U, E, k=10, **kw), lambda **kw: helpers.most_similar(U, 10, candidates=E, **kw),
                 lambda **kw: helpers.most_similar(E, 10, **kw)):
        with pytest.raises(ValueError, match="dedup_pool"):
            call(dedup_threshold=0.9, dedup_pool=9)
        with pytest.raises(ValueError, match="dedup_pool"):
            call(dedup_threshold=0.9, dedup_pool=129)
    with pytest.raises(ValueError, match="dedup_pool"):
        helpers.recommend(U, E, k=40, dedup_threshold=0.9, dedup_pool=39)
    with pytest.raises(ValueError, match="chunk_rows"):
        helpers.most_similar(E, 10, chunk_rows=128, dedup_threshold=0.9)
    with pytest.raises(ValueError, match="NaN"):
        helpers.dedup_lists(np.zeros((2, 4), np.int64), E, 2, float("nan"))
    with pytest.raises(ValueError, match="at most 128"):
        helpers.dedup_lists(np.zeros((2, 129), np.int64), E, 2, 0.5)
    with pytest.raises(ValueError, match="k must be"):
        helpers.dedup_lists(np.zeros((2, 4), np.int64), E, 5, 0.5)
    with pytest.raises(ValueError, match="not a supported norm"):
        helpers.dedup_lists(np.zeros((2, 4), np.int64), E, 2, 0.5, norm="l3")
