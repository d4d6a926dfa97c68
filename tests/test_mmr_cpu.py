"""CPU checks of the list diversification (dae_mmr_lists; helpers.diversify_lists, recommend_diverse, list_diversity): both builds
export the two symbols with the header's arity, every argument error of the entry is reported before any HIP call, the NumPy
reference of tests/mmr_reference.py on hand-made cases, list_diversity, and the ValueErrors of the helpers, raised before the
device or the library is touched."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mmr_reference import mmr_reference, near_tie_rows_mmr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(1 << 20)          # never dereferenced: every case below fails the argument checks first
INF = float("inf")


def _lib(fmt="bf16"):
    from dae_rnn_news_recommendation_amd import _lib
    return _lib.load(fmt)


# ---- the C entry ----

@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_builds_export_the_symbols(fmt):
    lib = _lib(fmt)
    assert hasattr(lib, "dae_mmr_lists_workspace") and hasattr(lib, "dae_mmr_lists")


def test_arity_matches_the_header_and_the_abi_version_stays():
    from dae_rnn_news_recommendation_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dae_hip.h")).read(), flags=re.S)
    for name, want in (("dae_mmr_lists_workspace", 4), ("dae_mmr_lists", 26)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == want == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["dae_mmr_lists"][0] is ctypes.c_int32 and _lib.SIGNATURES["dae_mmr_lists_workspace"][0] is ctypes.c_uint64
    assert _lib.ABI_VERSION == 9


def test_workspace_is_that_of_dedup_lists():
    lib = _lib()
    for args in ((1, 600, 100, 32), (10, 600, 100, 7), (10 ** 8, 600, 500, 128), (3, 6000, 48, 1)):
        assert lib.dae_mmr_lists_workspace(*args) == lib.dae_dedup_lists_workspace(*args) > 0
    assert lib.dae_mmr_lists_workspace(0, 600, 100, 32) == 0 and lib.dae_mmr_lists_workspace(10, 600, 100, 0) == 0


def _call(lib, E=P, lde=None, Na=600, D=48, norm=0, metric=0, lists=P, ldl=None, rel=P, ldr=None, labels=None, cap=0, Nr=10, L=32, k=10,
          lam=0.7, threshold=INF, out=P, outf=P, ldo=None, counts=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dae_mmr_lists_workspace(Nr, Na, D, L)
    return lib.dae_mmr_lists(E, D if lde is None else lde, Na, D, norm, metric, lists, L if ldl is None else ldl, rel,
                             L if ldr is None else ldr, labels, cap, Nr, L, k, lam, threshold, out, out, outf, outf,
                             k if ldo is None else ldo, counts, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(k=0), b"k must be in 1..L"),
    (dict(k=33), b"k must be in 1..L"),
    (dict(L=129, k=10, ws_bytes=1 << 30), b"L must be in 1..128"),
    (dict(L=0, k=1, ws_bytes=1 << 30), b"L must be in 1..128"),
    (dict(norm=4), b"norm must be"),
    (dict(metric=2), b"metric must be 0 (cosine) or 1 (linear kernel)"),
    (dict(lam=-0.01), b"lambda must be in [0, 1]"),
    (dict(lam=1.01), b"lambda must be in [0, 1]"),
    (dict(lam=float("nan")), b"lambda must be in [0, 1]"),
    (dict(threshold=float("nan")), b"threshold is NaN"),
    (dict(cap=-1, labels=P), b"max_per_label must not be negative"),
    (dict(cap=2), b"needs labels"),
    (dict(ldl=31), b"ldl"),
    (dict(ldr=31), b"ldr"),
    (dict(ldo=9), b"ldo"),
    (dict(lde=47), b"bad input"),
    (dict(E=None), b"bad input"),
    (dict(lists=None), b"bad input"),
    (dict(rel=None), b"bad input"),
    (dict(out=None), b"bad input"),
    (dict(outf=None), b"bad input"),
    (dict(counts=None), b"bad input"),
    (dict(Nr=0, ws_bytes=1 << 30), b"bad input"),
    (dict(Na=2 ** 21, D=512, ws_bytes=1 << 40), b"corpus image exceeds 4 GiB"),
    (dict(ws_bytes=1024), b"workspace too small"),
    (dict(ws=ctypes.c_void_p((1 << 20) + 64)), b"256-byte aligned"),
])
def test_argument_errors_without_a_gpu(kw, msg):
    lib = _lib()
    assert _call(lib, **kw) != 0
    assert msg in lib.dae_last_error() and b"mmr_lists" in lib.dae_last_error(), lib.dae_last_error()


def test_the_smallest_accepted_workspace_is_the_image_and_one_list():
    lib = _lib()
    one = lib.dae_mmr_lists_workspace(1, 600, 48, 32)
    assert _call(lib, Nr=1000, ws_bytes=one - 1) != 0 and b"workspace too small" in lib.dae_last_error()


# ---- the reference ----

def _scores(n, pairs, value=1.0):
    S = np.eye(n)
    for a, b in pairs:
        S[a, b] = S[b, a] = value
    return S


def test_reference_first_pick_is_the_most_relevant_whatever_the_order():
    S = _scores(5, [(0, 1)], 0.9)
    for lam in (0.01, 0.3, 1.0):
        idx, pos, val, near, cnt = mmr_reference([[3, 1, 4, 0]], [[0.2, 0.9, 0.1, 0.5]], S, 1, lam)
        assert idx.tolist() == [[1]] and pos.tolist() == [[1]] and near.tolist() == [[0.0]] and val[0, 0] == lam * 0.9
        assert cnt.tolist() == [[1, 1]]                                    # position 1 is not the first valid position
    # lam = 0: every v of the first step is 0, so it is the list's first valid entry -- the most relevant of a best-first list
    assert mmr_reference([[-1, 3, 1, 4, 0]], [[0.95, 0.2, 0.9, 0.1, 0.5]], S, 1, 0.0)[1].tolist() == [[1]]
    assert idx.dtype == pos.dtype == cnt.dtype == np.int64 and val.dtype == near.dtype == np.float64


def test_reference_lambda_one_is_the_stable_sort():
    rng = np.random.default_rng(0)
    S = rng.random((20, 20))
    rel = np.round(rng.random((6, 12)), 1)                                # many equal relevances
    lists = np.stack([rng.permutation(20)[:12] for _ in range(6)])
    idx, pos, val, near, cnt = mmr_reference(lists, rel, S, 12, 1.0)
    want = np.argsort(-rel, axis=1, kind="stable")
    assert np.array_equal(pos, want) and np.array_equal(idx, np.take_along_axis(lists, want, 1))
    assert np.array_equal(val, np.take_along_axis(rel, want, 1))
    # a best-first list: its first k valid entries
    lists = np.array([[7, -1, 3, 25, 9, 1]])
    idx, pos, _, _, cnt = mmr_reference(lists, [[.9, .8, .7, .6, .5, .4]], S, 3, 1.0)
    assert idx.tolist() == [[7, 3, 9]] and pos.tolist() == [[0, 2, 4]] and cnt.tolist() == [[3, 0]]


def test_reference_lambda_zero_prefers_the_farthest_after_the_first_pick():
    S = np.eye(4)
    S[0, 1] = S[1, 0] = 0.8
    S[0, 2] = S[2, 0] = 0.3
    S[0, 3] = S[3, 0] = 0.5
    S[2, 3] = S[3, 2] = 0.1
    S[1, 2] = S[2, 1] = 0.9
    idx, pos, val, near, _ = mmr_reference([[0, 1, 2, 3]], [[1.0, 0.9, 0.1, 0.2]], S, 4, 0.0)
    # the first step: every v is 0 -> the lowest position; then the smallest penalty: 2 (0.3), then 3 (max(0.5, 0.1)), then 1 (0.9)
    assert idx.tolist() == [[0, 2, 3, 1]]
    assert near.tolist() == [[0.0, 0.3, 0.5, 0.9]] and val.tolist() == [[0.0, -0.3, -0.5, -0.9]]


def test_reference_penalty_is_never_negative_and_ignores_nan_scores():
    S = np.eye(3)
    S[0, 1] = S[1, 0] = -0.5                                               # a negative similarity earns no bonus
    S[0, 2] = S[2, 0] = np.nan                                             # a NaN score leaves m unchanged
    idx, _, val, near, _ = mmr_reference([[0, 1, 2]], [[1.0, 0.5, 0.4]], S, 3, 0.5)
    assert idx.tolist() == [[0, 1, 2]] and near.tolist() == [[0.0, 0.0, 0.0]] and val.tolist() == [[0.5, 0.25, 0.2]]


def test_reference_ties_go_to_the_lowest_position():
    S = np.eye(6)
    idx, pos, _, _, _ = mmr_reference([[4, 2, 5, 1]], [[0.5, 0.7, 0.7, 0.5]], S, 4, 0.6)
    assert pos.tolist() == [[1, 2, 0, 3]] and idx.tolist() == [[2, 5, 4, 1]]
    idx, pos, _, _, _ = mmr_reference([[4, 2]], [[-0.0, 0.0]], S, 2, 1.0)      # -0 == +0
    assert pos.tolist() == [[0, 1]]


def test_reference_invalid_and_non_finite_entries_and_a_duplicate_index():
    S = np.eye(6)
    lists = [[-1, 3, 6, 2, 3, 1, 0]]
    rel = [[9.0, 0.5, 9.0, np.nan, 0.4, INF, -INF]]
    idx, pos, val, near, cnt = mmr_reference(lists, rel, S, 7, 0.5)
    # only positions 1 and 4 are valid; the second 3 is at similarity 1 to the first
    assert idx.tolist() == [[3, 3, -1, -1, -1, -1, -1]] and pos.tolist() == [[1, 4, -1, -1, -1, -1, -1]]
    assert near[0, :2].tolist() == [0.0, 1.0] and val[0, :2].tolist() == [0.25, 0.2 - 0.5]
    assert np.isneginf(val[0, 2:]).all() and np.isneginf(near[0, 2:]).all() and cnt.tolist() == [[2, 0]]
    idx, _, _, _, cnt = mmr_reference([[-1, 9]], [[1.0, 1.0]], S, 2, 0.5)
    assert idx.tolist() == [[-1, -1]] and cnt.tolist() == [[0, 0]]
    # with the threshold the duplicate goes
    idx, _, _, _, cnt = mmr_reference(lists, rel, S, 7, 0.5, threshold=1.0)
    assert idx[0, :2].tolist() == [3, -1] and cnt.tolist() == [[1, 0]]


def test_reference_cap_and_negative_labels_and_threshold():
    S = _scores(8, [(0, 1), (0, 2), (1, 2), (3, 4)], 0.9)
    labels = np.array([0, 0, 0, 1, 1, -1, -1, -1])
    lists, rel = [[0, 1, 2, 3, 4, 5, 6, 7]], [[.9, .8, .7, .6, .5, .4, .3, .2]]
    idx, _, _, _, cnt = mmr_reference(lists, rel, S, 8, 1.0, labels=labels, max_per_label=1)
    assert idx.tolist() == [[0, 3, 5, 6, 7, -1, -1, -1]] and cnt.tolist() == [[5, 0]]          # labels < 0 are never capped
    idx, _, _, _, cnt = mmr_reference(lists, rel, S, 8, 1.0, labels=labels, max_per_label=2)
    assert idx.tolist() == [[0, 1, 3, 4, 5, 6, 7, -1]]
    idx, _, _, _, cnt = mmr_reference(lists, rel, S, 4, 1.0, labels=labels, max_per_label=1)
    assert idx.tolist() == [[0, 3, 5, 6]] and cnt.tolist() == [[4, 2]]     # 5 and 6 lie past the first 4 valid positions
    # max_per_label = 0 and labels alone: off
    assert mmr_reference(lists, rel, S, 8, 1.0, labels=labels)[0].tolist() == [lists[0]]
    # the threshold is inclusive and is the greedy de-dup rule
    idx, _, _, _, _ = mmr_reference(lists, rel, S, 8, 1.0, threshold=0.9)
    assert idx.tolist() == [[0, 3, 5, 6, 7, -1, -1, -1]]
    idx, _, _, _, _ = mmr_reference(lists, rel, S, 8, 1.0, threshold=np.nextafter(0.9, 1.0))
    assert idx.tolist() == [lists[0]]


def test_reference_counts_beyond_the_top_k():
    S = _scores(6, [(0, 1), (0, 2)], 0.95)
    lists, rel = [[0, -1, 1, 2, 3, 4]], [[1.0, .99, .98, .97, .5, .4]]
    # k = 3: the first 3 valid positions are 0, 2, 3; lam = 0.5 picks 0, then 3 and 4 at (0.25, 0.2) over 1 and 2 at (0.015, 0.01)
    idx, pos, _, _, cnt = mmr_reference(lists, rel, S, 3, 0.5)
    assert idx.tolist() == [[0, 3, 4]] and pos.tolist() == [[0, 4, 5]] and cnt.tolist() == [[3, 2]]
    assert mmr_reference(lists, rel, S, 3, 1.0)[4].tolist() == [[3, 0]]


def test_reference_float32_rounds_every_operation():
    rng = np.random.default_rng(1)
    S = rng.random((30, 30)).astype(np.float32)
    lists = np.stack([rng.permutation(30)[:16] for _ in range(8)])
    rel = rng.random((8, 16)).astype(np.float32)
    lam = np.float32(0.3)
    idx, pos, val, near, _ = mmr_reference(lists, rel, S, 16, lam)
    assert val.dtype == near.dtype == np.float32
    m = np.zeros(16, np.float32)
    for t in range(16):                                                    # row 0, step by step, in float32
        p = pos[0, t]
        assert near[0, t] == m[p] and val[0, t] == np.float32(lam * rel[0, p]) - np.float32(np.float32(np.float32(1) - lam) * m[p])
        m = np.fmax(m, S[lists[0, p], lists[0]])


def test_near_tie_rows():
    S = np.eye(4)
    S[0, 1] = S[1, 0] = 0.5
    lists, rel = [[0, 1, 2], [0, 1, 2]], [[1.0, 0.6, 0.3 + 1e-9], [1.0, 0.6, 0.2]]
    # step 2, lam = 0.5: v[1] = 0.3 - 0.25 = 0.05 against v[2] = 0.15 / 0.1: no tie; a band of 0.06 reaches the second row's 0.05
    assert near_tie_rows_mmr(lists, rel, S, 3, 0.5, 1e-6).tolist() == [False, False]
    assert near_tie_rows_mmr(lists, rel, S, 3, 0.5, 0.06).tolist() == [False, True]
    assert near_tie_rows_mmr([[0, 2, 3]], [[0.5, 0.5, 0.2]], S, 3, 0.5, 1e-6).tolist() == [False]      # an exact tie is no near-tie
    assert near_tie_rows_mmr([[0, 2, 3]], [[0.5, 0.5 - 1e-8, 0.2]], S, 3, 0.5, 1e-6).tolist() == [True]
    assert near_tie_rows_mmr([[0, 1, 2]], [[1.0, 0.6, 0.2]], S, 3, 0.5, 1e-6, threshold=0.5 + 1e-7, tol=1e-6).tolist() == [True]
    assert near_tie_rows_mmr([[0, 1, 2]], [[1.0, 0.6, 0.2]], S, 3, 0.5, 1e-6, threshold=0.7, tol=1e-6).tolist() == [False]


# ---- list_diversity ----

def test_list_diversity():
    from dae_rnn_news_recommendation_amd import helpers
    idx = np.array([[0, 1, 2, 3], [4, 5, -1, -1], [6, -1, -1, -1], [-1, -1, -1, -1]])
    near = np.array([[0.0, 0.5, 0.25, 0.75], [0.0, 0.2, -INF, -INF], [0.0, -INF, -INF, -INF], [-INF] * 4])
    labels = np.array([0, 0, 1, 0, 2, 3, 4])
    d = helpers.list_diversity(idx, nearest=near, labels=labels)
    assert np.allclose(d["nearest"][:2], [0.5, 0.2]) and np.isnan(d["nearest"][2:]).all() and abs(d["mean_nearest"] - 0.35) < 1e-12
    assert d["n_labels"].tolist() == [2, 2, 1, 0] and d["mean_n_labels"] == 1.25
    assert np.allclose(d["max_label_share"][:3], [0.75, 0.5, 1.0]) and np.isnan(d["max_label_share"][3])
    assert abs(d["mean_max_label_share"] - 0.75) < 1e-12
    assert set(helpers.list_diversity(idx)) == set() and set(helpers.list_diversity(idx, labels=labels)) == \
        {"n_labels", "mean_n_labels", "max_label_share", "mean_max_label_share"}
    with pytest.raises(ValueError, match="shape of indices"):
        helpers.list_diversity(idx, nearest=near[:, :3])
    with pytest.raises(ValueError, match="labels holds"):
        helpers.list_diversity(idx, labels=labels[:5])
    with pytest.raises(ValueError, match="n_lists x k"):
        helpers.list_diversity(idx[0])


# ---- the helpers' argument checks ----

def test_value_errors_before_the_device_or_the_library(monkeypatch):
    from dae_rnn_news_recommendation_amd import _lib, helpers

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    rng = np.random.default_rng(0)
    E = rng.standard_normal((50, 8)).astype(np.float32)
    U = rng.standard_normal((5, 8)).astype(np.float32)
    idx, rel = np.zeros((2, 4), np.int64), np.zeros((2, 4), np.float32)
    labels = np.zeros(50, np.int64)
    div = helpers.diversify_lists
    for bad, msg in ((lambda: div(idx[0], rel[0], E, 2), "n_rows x L"),
                     (lambda: div(idx, rel[:, :3], E, 2), "shape of indices"),
                     (lambda: div(np.zeros((2, 129), np.int64), np.zeros((2, 129), np.float32), E, 2), "at most 128"),
                     (lambda: div(idx, rel, E, 0), "k must be"),
                     (lambda: div(idx, rel, E, 5), "k must be"),
                     (lambda: div(idx, rel, E, 2, -0.1), "lam must be"),
                     (lambda: div(idx, rel, E, 2, 1.5), "lam must be"),
                     (lambda: div(idx, rel, E, 2, float("nan")), "lam must be"),
                     (lambda: div(idx, rel, E, 2, labels=labels, max_per_label=0), "max_per_label must be at least 1"),
                     (lambda: div(idx, rel, E, 2, max_per_label=2), "needs labels"),
                     (lambda: div(idx, rel, E, 2, labels=labels[:49], max_per_label=2), "one entry per row"),
                     (lambda: div(idx, rel, E, 2, labels=labels[:49]), "one entry per row"),
                     (lambda: div(idx, rel, E, 2, scale_relevance="zscore"), "scale_relevance"),
                     (lambda: div(idx, rel, E, 2, dedup_threshold=float("nan")), "NaN"),
                     (lambda: div(idx, rel, E, 2, norm="l3"), "not a supported norm"),
                     (lambda: div(idx, rel, E[0], 2), "2D"),
                     (lambda: helpers.recommend_diverse(U, E, k=10, pool=9), "pool must be"),
                     (lambda: helpers.recommend_diverse(U, E, k=10, pool=129), "pool must be"),
                     (lambda: helpers.recommend_diverse(U, E, k=40, pool=39), "pool must be"),
                     (lambda: helpers.recommend_diverse(U, E, k=10, lam=2.0), "lam must be"),
                     (lambda: helpers.recommend_diverse(U, E, k=10, max_per_label=2), "max_per_label"),
                     (lambda: helpers.recommend_diverse(U, E, k=10, scale_relevance="zscore"), "scale_relevance")):
        with pytest.raises(ValueError, match=msg):
            bad()


def test_new_names_are_importable_and_the_import_still_needs_numpy_alone():
    code = ("import sys; from dae_rnn_news_recommendation_amd.helpers import diversify_lists, recommend_diverse, list_diversity; "
            "import inspect; print(sorted(m for m in ('torch', 'scipy', 'pandas') if m in sys.modules)); "
            "print(list(inspect.signature(diversify_lists).parameters)[:5])")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True)
    assert out.stdout.splitlines() == ["[]", "['indices', 'relevance', 'embeddings', 'k', 'lam']"], out.stdout
