"""The word-based user model without a GPU: the NumPy reference (tests/words_reference.py) against scipy's product and a brute-force
sort, the new symbols of both library builds, the argument errors of the entry points (reported before any HIP call) and of
helpers.words (raised before the device is touched), and the import of the package with numpy alone."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from dae_rnn_news_recommendation_amd import _lib, helpers
from words_reference import entry_weights_reference, profiles_reference, ranks_reference, scores_reference, topk_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SYMBOLS = ("dae_word_profiles_bytes", "dae_word_profiles", "dae_word_entry_weights_bytes", "dae_word_entry_weights",
           "dae_word_topk_workspace", "dae_word_topk", "dae_word_rank_workspace", "dae_word_rank")


def _case(seed, M=23, Na=37, V=29, density=0.2, integer=True):
    rng = np.random.default_rng(seed)
    A = sp.random(Na, V, density=density, random_state=np.random.RandomState(seed), format="csr", dtype=np.float32)
    A.data = rng.integers(1, 4, A.nnz).astype(F32) if integer else rng.normal(size=A.nnz).astype(F32)
    A.sort_indices()
    rows = [rng.integers(0, Na, rng.integers(0, 6)) for _ in range(M)]
    indptr = np.zeros(M + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate(rows).astype(np.int64)
    return A, indptr, items


@pytest.mark.parametrize("weights", [False, True])
def test_reference_scores_equal_the_sparse_product_on_integers(weights):
    A, indptr, items = _case(1)
    V = A.shape[1]
    P = profiles_reference(indptr, items, A, V)
    H = sp.csr_matrix((np.ones(items.size), items, indptr), shape=(indptr.size - 1, A.shape[0]))
    assert np.array_equal(P, ((H @ (A != 0).astype(np.int64)).toarray() > 0))
    tw = np.random.default_rng(2).integers(-2, 4, V).astype(F32) if weights else None
    R = scores_reference(P, A, tw)
    B = A if tw is None else A @ sp.diags(tw.astype(np.float64))
    want = (sp.csr_matrix(P.astype(np.float64)) @ B.T).toarray()
    assert np.array_equal(R.astype(np.float64), want)                   # small integers: every partial sum is exact in fp32
    Rb = scores_reference(P, (A.indptr, A.indices, None))
    assert np.array_equal(Rb.astype(np.int64), (sp.csr_matrix(P.astype(np.int64)) @ (A != 0).astype(np.int64).T).toarray())


def test_reference_profiles_last_events_and_dropped_entries():
    A, indptr, items = _case(3)
    V = A.shape[1]
    for me in (1, 3):
        P = profiles_reference(indptr, items, A, V, me)
        for u in range(indptr.size - 1):
            h = items[indptr[u]:indptr[u + 1]][-me:]
            want = np.zeros(V, dtype=bool)
            for a in h:
                want[A.indices[A.indptr[a]:A.indptr[a + 1]]] = True
            assert np.array_equal(P[u], want)
    bad_items = items.copy()
    bad_items[::3] = A.shape[0] + 5
    assert np.array_equal(profiles_reference(indptr, bad_items, A, V), profiles_reference(indptr, np.where(bad_items < A.shape[0], bad_items, -1), A, V))
    e = entry_weights_reference((A.indptr, np.where(np.arange(A.nnz) % 4 == 0, V + 1, A.indices), A.data), V)
    assert (e[::4] == 0).all() and np.array_equal(e[1::4], A.data[1::4])


def test_reference_topk_and_ranks_against_brute_force():
    A, indptr, items = _case(5, integer=False)
    M, Na = indptr.size - 1, A.shape[0]
    rng = np.random.default_rng(6)
    P = profiles_reference(indptr, items, A, A.shape[1])
    R = scores_reference(P, A)
    seen = [rng.integers(0, Na, rng.integers(0, 8)) for _ in range(M)]
    lo = rng.integers(0, Na, M)
    hi = np.minimum(lo + rng.integers(0, Na, M), Na)
    targets = rng.integers(-1, Na, M)
    for sn, win in ((None, None), (seen, None), (None, (lo, hi)), (seen, (lo, hi))):
        idx, sc = topk_reference(R, 7, sn, win)
        rank, ts = ranks_reference(R, targets, sn, win)
        for u in range(M):
            cand = [a for a in range(Na) if (sn is None or a not in set(sn[u].tolist())) and (win is None or lo[u] <= a < hi[u])]
            best = sorted(cand, key=lambda a: (-float(R[u, a]), a))
            n = min(7, len(best))
            assert idx[u, :n].tolist() == best[:n] and (idx[u, n:] == -1).all() and np.isneginf(sc[u, n:]).all()
            assert np.array_equal(sc[u, :n], R[u, best[:n]] + F32(0))
            t = int(targets[u])
            if t < 0:
                assert rank[u] == 0 and np.isneginf(ts[u])
            else:
                others = sorted(set(cand) | {t}, key=lambda a: (-float(R[u, a]), a))
                assert rank[u] == others.index(t) + 1 and ts[u] == R[u, t]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_libraries_export_the_symbols(fmt):
    lib = _lib.load(fmt)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dae_abi_version() == _lib.ABI_VERSION == 9
    assert lib.dae_word_profiles_bytes(129, 33) == 2 * 33 * 16 and lib.dae_word_profiles_bytes(0, 33) == 0
    assert lib.dae_word_entry_weights_bytes(100) == 512 and lib.dae_word_rank_workspace(130) == 256 * 8
    assert lib.dae_word_topk_workspace(1, 1, 1) > 0 and lib.dae_word_topk_workspace(1, 1, 0) == 0


def test_entry_points_report_argument_errors_before_any_hip_call():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    p = ctypes.c_void_p((p.value + 255) // 256 * 256)

    def message(rc):
        assert rc == 1
        return lib.dae_last_error().decode()
    topk = lambda **kw: lib.dae_word_topk(*[kw.get(n, d) for n, d in (  # noqa: E731
        ("bitmaps", p), ("M", 4), ("V", 8), ("ip", p), ("ix", p), ("w", p), ("nnz", 5), ("Na", 3), ("k", 2), ("xp", None), ("xi", None),
        ("lo", None), ("hi", None), ("idx", p), ("score", p), ("ldk", 2), ("ws", p), ("ws_bytes", 1 << 20), ("stream", None))])
    assert message(topk(k=0)).startswith("word_topk: k must be in 1..128")
    assert message(topk(k=129, ldk=129)).startswith("word_topk: k must be in 1..128")
    assert message(topk(ldk=1)).startswith("word_topk: ldk")
    assert message(topk(V=0)).startswith("word_topk: M")
    assert message(topk(bitmaps=None)).startswith("word_topk: bitmaps")
    assert message(topk(xp=p)).startswith("word_topk: excl_indptr and excl_items go together")
    assert message(topk(lo=p)).startswith("word_topk: win_lo and win_hi go together")
    assert message(topk(ws_bytes=8)).startswith("word_topk: workspace too small")
    assert message(topk(ws=ctypes.c_void_p(p.value + 8))).startswith("word_topk: workspace must be 256-byte aligned")
    rank = lambda **kw: lib.dae_word_rank(*[kw.get(n, d) for n, d in (  # noqa: E731
        ("bitmaps", p), ("M", 4), ("V", 8), ("ip", p), ("ix", p), ("w", p), ("nnz", 5), ("Na", 3), ("xp", None), ("xi", None), ("lo", None),
        ("hi", None), ("t", p), ("rank", p), ("ts", p), ("ws", p), ("ws_bytes", 1 << 20), ("stream", None))])
    assert message(rank(t=None)).startswith("word_rank: targets")
    assert message(rank(nnz=-1)).startswith("word_rank: nnz")
    assert message(rank(ws_bytes=0)).startswith("word_rank: workspace too small")
    prof = lambda **kw: lib.dae_word_profiles(*[kw.get(n, d) for n, d in (  # noqa: E731
        ("hp", p), ("hi", p), ("hnnz", 3), ("M", 4), ("me", 0), ("ip", p), ("ix", p), ("nnz", 5), ("Na", 3), ("V", 8), ("bitmaps", p),
        ("bytes", 128), ("sizes", p), ("stream", None))])
    assert message(prof(me=-1)).startswith("word_profiles: max_events")
    assert message(prof(bytes=64)).startswith("word_profiles: bitmaps too small")
    assert message(prof(sizes=None)).startswith("word_profiles: bitmaps / sizes")
    assert message(lib.dae_word_entry_weights(p, None, 4, 0, None, p, None)).startswith("word_entry_weights: nnz")
    assert message(lib.dae_word_entry_weights(None, None, 4, 3, None, p, None)).startswith("word_entry_weights: art_indices")


def test_helpers_raise_value_errors_before_the_device_is_touched():
    A, indptr, items = _case(9)
    Na, V = A.shape
    hist = (indptr, items)
    for k in (0, 129):
        with pytest.raises(ValueError, match="k must be in 1..128"):
            helpers.word_recommend(hist, A, k)
    with pytest.raises(ValueError, match="term_weights for"):
        helpers.word_recommend(hist, A, 3, term_weights=np.ones(V + 1))
    for bad in (np.nan, np.inf):
        w = np.ones(V)
        w[3] = bad
        with pytest.raises(ValueError, match="term_weights must be finite"):
            helpers.word_recommend(hist, A, 3, term_weights=w)
        with pytest.raises(ValueError, match="term_weights must be finite"):
            helpers.word_ranks(hist, A, np.zeros(indptr.size - 1, dtype=np.int64), term_weights=w)
    for bad_items in (np.where(np.arange(items.size) == 2, Na, items), np.where(np.arange(items.size) == 2, -1, items)):
        with pytest.raises(ValueError, match="history items must be in"):
            helpers.word_recommend((indptr, bad_items), A, 3)
        with pytest.raises(ValueError, match="history items must be in"):
            helpers.word_profiles((indptr, bad_items), A)
    with pytest.raises(ValueError, match="max_events must be at least 1"):
        helpers.word_profiles(hist, A, max_events=0)
    with pytest.raises(ValueError, match="batch_users must be positive"):
        helpers.word_recommend(hist, A, 3, batch_users=0)
    other = helpers.WordProfiles(None, indptr.size - 1, V + 2, None)
    with pytest.raises(ValueError, match="the profiles are over"):
        helpers.word_recommend(other, A, 3)
    with pytest.raises(ValueError, match="max_events belongs to word_profiles"):
        helpers.word_recommend(helpers.WordProfiles(None, indptr.size - 1, V, None), A, 3, max_events=2)
    with pytest.raises(ValueError, match="window hi must not exceed"):
        helpers.word_recommend(hist, A, 3, window=(np.zeros(indptr.size - 1, dtype=np.int64), np.full(indptr.size - 1, Na + 1)))
    with pytest.raises(ValueError, match="exclude has"):
        helpers.word_recommend(hist, A, 3, seen=[[0]])
    with pytest.raises(ValueError, match="targets must be below"):
        helpers.word_ranks(hist, A, np.full(indptr.size - 1, Na))
    with pytest.raises(ValueError, match="targets for"):
        helpers.word_ranks(hist, A, np.zeros(2, dtype=np.int64))


def test_helpers_import_needs_numpy_alone():
    code = ("import sys; from dae_rnn_news_recommendation_amd.helpers import word_profiles, word_recommend, word_ranks, idf_weights, "
            "WordProfiles; print(sorted(m for m in ('torch', 'scipy', 'pandas') if m in sys.modules))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "[]", out.stdout
