"""GPU checks of helpers.vectorize (csrc/dae_vectorize.hip): column_stats, select_columns and TfidfTransformer on a 300 x 700 count
matrix with empty rows, rows of 1, 64, 65, 256 and 257 entries (the pass boundaries of a wave walking its row 64 entries at a
time), one row of 680 entries, a non-empty last row and 20 columns that never occur; a second, binary case with values=None.

The tf-idf values are compared with sklearn's TfidfTransformer on the float64 copy, every entry, within a relative 2**-21: the chain
has at most four fp32 roundings (idf, sublinear tf, product, final quotient), each at most 2**-24 relative, and the norm is summed in
fp64 -- 4 * 2**-24, doubled for margin."""
import ctypes
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

from dae_rnn_news_recommendation_amd import _lib as L
from dae_rnn_news_recommendation_amd import helpers

gpu = pytest.mark.gpu

N, F, N_TRAIN, USED = 300, 700, 200, 680
TOL = 2.0 ** -21
LENGTHS = {0: 0, 1: 1, 2: 64, 3: 65, 4: 256, 5: 257, 6: USED, 7: 0, 150: 0, 210: 0, 220: 65, 230: 257, 299: 5}
TOPK, TOPK_GAP, TOPK_CAP = 10, 2.0 ** -20, 0.05


def _counts():
    """Row 6 (a train row) holds every used column, so no column of the validation rows is new to a transformer fitted on train."""
    rng = np.random.default_rng(11)
    indptr, cols, vals = [0], [], []
    for i in range(N):
        n = LENGTHS.get(i, int(rng.integers(2, 120)))
        c = np.sort(rng.choice(USED, n, replace=False))
        cols.append(c.astype(np.int32))
        vals.append(rng.integers(1, 9, n).astype(np.float32))
        indptr.append(indptr[-1] + n)
    m = sp.csr_matrix((np.concatenate(vals), np.concatenate(cols), np.asarray(indptr, dtype=np.int64)), shape=(N, F))
    assert m.has_canonical_format and m.indptr[-1] > m.indptr[-2] and m.indices.max() == USED - 1
    return m


X = _counts()
XB = sp.csr_matrix((np.ones(X.nnz, np.float32), X.indices, X.indptr), shape=X.shape)


def _dev(m, binary=False):
    """The device CSR dict of a scipy matrix, stored as given (explicit zeros stay); binary: values=None."""
    import torch
    return dict(indptr=torch.from_numpy(m.indptr.astype(np.int64)).cuda(), indices=torch.from_numpy(m.indices.astype(np.int32)).cuda(),
                values=None if binary else torch.from_numpy(m.data.astype(np.float32)).cuda(), n_rows=m.shape[0], nnz=int(m.nnz),
                n_cols=m.shape[1])


def _same_csr(got, want):
    want = want.tocsr()
    want.sort_indices()
    assert got.shape == want.shape and got.dtype == np.float32
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(got.data, want.data.astype(np.float32))


# ---- column_stats -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("binary", [False, True])
def test_column_stats_are_exact(binary):
    m = XB if binary else X
    df, tf = helpers.column_stats(_dev(m, binary))
    assert df.dtype == np.int64 and tf.dtype == np.int64 and df.shape == (F,)
    np.testing.assert_array_equal(df, np.bincount(m.indices, minlength=F))
    np.testing.assert_array_equal(tf, np.asarray(m.astype(np.float64).sum(axis=0)).ravel().astype(np.int64))
    assert (df[USED:] == 0).all()
    for chunk in (N_TRAIN, 7):                                           # row chunks add up to the one call
        df2, tf2 = helpers.column_stats(m, chunk_rows=chunk)
        np.testing.assert_array_equal(df2, df)
        np.testing.assert_array_equal(tf2, tf)


@gpu
def test_column_stats_counts_bad_entries_and_explicit_zeros():
    import torch
    lib = L.load()
    m = sp.csr_matrix((np.array([1, 2.5, 3, 0, 4], np.float32), np.array([0, 3, 9, 1, 2], np.int32), np.array([0, 3, 5], np.int64)), shape=(2, 8))
    d = _dev(m)                                                          # column 9 lies outside F = 8; 2.5 is no count; one explicit zero
    df = torch.zeros(8, dtype=torch.int64, device="cuda")
    tf = torch.zeros(8, dtype=torch.int64, device="cuda")
    ws = torch.zeros(int(lib.dae_csr_column_stats_workspace()) + 256, dtype=torch.uint8, device="cuda")
    ws_p = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    rec = (ctypes.c_uint64 * 2)()
    L.call("dae_csr_column_stats", L.ptr(d["indptr"]), L.ptr(d["indices"]), L.ptr(d["values"]), 2, 8, L.ptr(df), L.ptr(tf), rec, ws_p,
           int(lib.dae_csr_column_stats_workspace()), L.current_stream())
    assert list(rec) == [1, 1]
    assert df.cpu().tolist() == [1, 1, 1, 1, 0, 0, 0, 0]                 # the explicit zero (column 1) and the 2.5 (column 3) are stored entries
    assert tf.cpu().tolist() == [1, 0, 4, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="outside"):
        helpers.column_stats(d)


# ---- select_columns -----------------------------------------------------------------------------------------------------------------
def _kept_maps():
    every_third = np.arange(1, F, 3)
    high = np.arange(400, F)                                             # empties the short rows whose columns are all low
    return {"every third": every_third, "high": high, "everything": np.arange(F), "nothing": np.zeros(0, np.int64),
            "one": np.array([int(X.indices[X.indptr[1]])])}


@gpu
@pytest.mark.parametrize("name", list(_kept_maps()))
@pytest.mark.parametrize("binary", [False, True])
def test_select_columns_equals_scipy(name, binary):
    kept = _kept_maps()[name]
    m = XB if binary else X
    want = m[:, kept]
    if name == "high":
        assert (np.diff(want.indptr) == 0).sum() > (np.diff(m.indptr) == 0).sum()
    _same_csr(helpers.select_columns(m, kept), want)                         # a scipy matrix in, a scipy matrix out
    d = helpers.select_columns(_dev(m, binary), kept, return_device=True)
    assert d["n_cols"] == kept.size and d["nnz"] == want.nnz and d["indices"].is_cuda and (d["values"] is None) == binary
    _same_csr(helpers.device_csr_to_scipy(d), want)


@gpu
def test_select_columns_capacity_error_writes_nothing():
    import torch
    lib = L.load()
    d = _dev(X)
    kept = np.arange(1, F, 3)
    remap = np.full(F, -1, np.int32)
    remap[kept] = np.arange(kept.size, dtype=np.int32)
    remap_d = torch.from_numpy(remap).cuda()
    need = int(X[:, kept].nnz)
    guard = 4096
    ws_bytes = int(lib.dae_csr_select_columns_workspace(N))
    ws = torch.zeros(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    ws_p = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    rec = (ctypes.c_int64 * 2)()
    for cap, ok in ((need - 1, False), (need // 2, False), (0, False), (need, True)):
        oi = torch.full((need + guard,), -7, dtype=torch.int32, device="cuda")
        ov = torch.full((need + guard,), -7.0, dtype=torch.float32, device="cuda")
        op = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
        rc = lib.dae_csr_select_columns(L.ptr(d["indptr"]), L.ptr(d["indices"]), L.ptr(d["values"]), N, F, L.ptr(remap_d), L.ptr(op), L.ptr(oi),
                                        L.ptr(ov), cap, rec, ws_p, ws_bytes, L.current_stream())
        torch.cuda.synchronize()
        assert rec[0] == need and rec[1] == 0                            # the needed size comes back either way
        if ok:
            assert rc == 0
            assert (oi[need:] == -7).all() and (ov[need:] == -7.0).all() and (oi[:need] >= 0).all()
        else:
            assert rc == 1 and b"capacity" in lib.dae_last_error()
            assert (oi == -7).all() and (ov == -7.0).all()                   # the buffers and the guard region past them: untouched


@gpu
def test_select_columns_entry_with_nothing_kept():
    """The C entry itself with a remap of all -1 (helpers.select_columns returns before the call): count, scan, no fill."""
    import torch
    lib = L.load()
    d = _dev(X)
    remap_d = torch.full((F,), -1, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.dae_csr_select_columns_workspace(N))
    ws = torch.zeros(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    ws_p = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    rec = (ctypes.c_int64 * 2)(-1, -1)
    oi = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    ov = torch.full((64,), -7.0, dtype=torch.float32, device="cuda")
    op = torch.full((N + 1,), -7, dtype=torch.int64, device="cuda")
    L.call("dae_csr_select_columns", L.ptr(d["indptr"]), L.ptr(d["indices"]), L.ptr(d["values"]), N, F, L.ptr(remap_d), L.ptr(op), L.ptr(oi),
           L.ptr(ov), 64, rec, ws_p, ws_bytes, L.current_stream())
    torch.cuda.synchronize()
    assert list(rec) == [0, 0] and (op == 0).all() and (oi == -7).all() and (ov == -7.0).all()


# ---- tf-idf ------------------------------------------------------------------------------------------------------------------------
COMBOS = list(itertools.product(["l2", "l1", None], [True, False], [False, True], [True, False]))


def _sklearn_tfidf(norm, smooth_idf, sublinear_tf, use_idf, dtype=np.float64):
    from sklearn.feature_extraction.text import TfidfTransformer
    t = TfidfTransformer(norm=norm, use_idf=use_idf, smooth_idf=smooth_idf, sublinear_tf=sublinear_tf)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # df == 0 of the unused columns with smooth_idf=False
        t.fit(X[:N_TRAIN].astype(dtype))
        return t, t.transform(X.astype(dtype)).tocsr()


@gpu
@pytest.mark.parametrize("norm,smooth_idf,sublinear_tf,use_idf", COMBOS)
def test_tfidf_equals_sklearn(norm, smooth_idf, sublinear_tf, use_idf):
    ref_t, want = _sklearn_tfidf(norm, smooth_idf, sublinear_tf, use_idf)
    t = helpers.TfidfTransformer(norm=norm, use_idf=use_idf, smooth_idf=smooth_idf, sublinear_tf=sublinear_tf).fit(X[:N_TRAIN])
    assert t.n_features_in_ == F
    if use_idf:
        np.testing.assert_array_equal(t.idf_, ref_t.idf_)
    got = t.transform(X)
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(want.data).all()
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    err = np.abs(got.data.astype(np.float64) - want.data) / np.abs(want.data)
    print("norm=%s smooth=%s sublinear=%s use_idf=%s: max relative error %.3f * 2**-24 over %d entries"
          % (norm, smooth_idf, sublinear_tf, use_idf, err.max() * 2.0 ** 24, err.size))
    assert err.size == X.nnz and err.max() <= TOL
    # two runs, and the device-dict route, are bit-identical
    again = t.transform(_dev(X), return_device=True)
    assert again["values"].is_cuda and np.array_equal(again["values"].cpu().numpy().view(np.uint32), got.data.view(np.uint32))


@gpu
def test_tfidf_binary_matrix_and_in_place():
    import torch
    from sklearn.feature_extraction.text import TfidfTransformer
    want = TfidfTransformer().fit(XB[:N_TRAIN].astype(np.float64)).transform(XB.astype(np.float64)).tocsr()
    t = helpers.TfidfTransformer().fit(_dev(XB[:N_TRAIN], binary=True))
    got = t.transform(_dev(XB, binary=True))
    np.testing.assert_array_equal(got.indices, want.indices)
    assert (np.abs(got.data - want.data) <= TOL * np.abs(want.data)).all()
    # in place (out == values) equals out of place bit for bit, for every norm
    lib = L.load()
    d = _dev(X)
    idf = torch.from_numpy(t.idf_.astype(np.float32)).cuda()
    ws = torch.zeros(512, dtype=torch.uint8, device="cuda")
    ws_p = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    rec = (ctypes.c_uint64 * 1)()
    for norm, sub in itertools.product((0, 1, 2), (0, 1)):
        out = torch.full((X.nnz,), float("nan"), dtype=torch.float32, device="cuda")
        inp = d["values"].clone()
        for src, dst in ((d["values"], out), (inp, inp)):
            L.call("dae_tfidf_transform", L.ptr(d["indptr"]), L.ptr(d["indices"]), L.ptr(src), N, F, L.ptr(idf), sub, norm, L.ptr(dst), rec,
                   ws_p, 256, L.current_stream())
            assert rec[0] == 0
        assert torch.equal(out.view(torch.int32), inp.view(torch.int32))
        assert torch.equal(d["values"], torch.from_numpy(X.data).cuda())     # the out-of-place call left its input alone


@gpu
def test_tfidf_zero_norm_row_keeps_its_values():
    m = sp.csr_matrix((np.array([0, 0, 0, 2, 1], np.float32), np.array([1, 4, 6, 0, 4], np.int32), np.array([0, 3, 3, 5], np.int64)), shape=(3, 8))
    for norm in ("l2", "l1"):
        got = helpers.TfidfTransformer(norm=norm).fit(m).transform(m)
        assert got.nnz == 5 and (got.data[:3] == 0).all() and np.isfinite(got.data).all()
        assert abs((np.abs(got.data[3:]) ** (2 if norm == "l2" else 1)).sum() - 1) < 1e-6


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_device_csr_trains_like_its_scipy_copy():
    import torch
    from dae_rnn_news_recommendation_amd.engine import Engine
    counts, kept = helpers.limit_features(X[:N_TRAIN], 2, 0.9, 400, return_device=True)
    assert kept.size == 400 and counts["n_cols"] == 400
    tfidf = helpers.TfidfTransformer().fit_transform(counts, return_device=True)
    host = helpers.device_csr_to_scipy(tfidf)
    H, B = 32, 128
    rng = np.random.default_rng(3)
    W0 = rng.uniform(-0.2, 0.2, (kept.size, H)).astype(np.float32)
    idx = torch.from_numpy(rng.permutation(N_TRAIN)[:B].astype(np.int32)).cuda()
    bits = []
    for data in (tfidf, host):
        eng = Engine(kept.size, H, B, dtype="fp32", triplet="none", loss_func="mean_squared", learning_rate=0.1)
        csr = eng.upload_csr(data)
        assert csr["values"] is not None and csr["nnz"] == host.nnz
        if data is tfidf:
            assert csr["indices"].data_ptr() == tfidf["indices"].data_ptr() and csr["values"].data_ptr() == tfidf["values"].data_ptr()
        eng.set_params(W0)
        stats = torch.zeros(8, device="cuda")
        eng.train_step(idx, None, stats)
        torch.cuda.synchronize()
        bits.append(stats.cpu().numpy().view(np.uint32).copy())
    assert np.isfinite(bits[0][:1].view(np.float32)).all() and bits[0][:1].view(np.float32)[0] > 0
    assert bits[0][0] == bits[1][0], (bits[0][:1].view(np.float32), bits[1][:1].view(np.float32))


def _topk_reference():
    """sklearn's float32 tf-idf of X and, from its float64 score matrix (self pair excluded), the rows whose first TOPK + 1 scores
    are pairwise further apart than TOPK_GAP: every adjacent gap inside the top k and the one between the k-th and the (k+1)-th.
    Only in those rows is the ORDER of the k neighbours decided by more than the rounding of the two inputs."""
    _, T = _sklearn_tfidf("l2", True, False, True, dtype=np.float32)
    assert T.dtype == np.float32
    S = (T.astype(np.float64) @ T.astype(np.float64).T).toarray()
    np.fill_diagonal(S, -np.inf)
    s = -np.sort(-S, axis=1)[:, :TOPK + 1]
    return T, ((s[:, :-1] - s[:, 1:]) > TOPK_GAP).all(axis=1)


def test_topk_comparison_leaves_out_few_rows():
    """sklearn alone, no GPU: the share of rows the ordered top-k comparison below leaves out -- the four empty rows and the rows with
    two of their first k + 1 scores within 2**-20 -- stays under its cap (5 of 300 rows, 1.7 %, on this input)."""
    _, clear = _topk_reference()
    left_out = 1.0 - clear.mean()
    print("top-%d comparison leaves out %d of %d rows (%.2f %%)" % (TOPK, int((~clear).sum()), N, 100 * left_out))
    assert left_out <= TOPK_CAP, left_out


@gpu
def test_most_similar_on_device_tfidf_equals_sklearns():
    """The ordered index arrays are compared; rows in which two of sklearn's first k + 1 scores are within 2**-20 are left out, at
    most 5 % of them."""
    T, clear = _topk_reference()
    left_out = 1.0 - clear.mean()
    print("top-%d comparison leaves out %d of %d rows (%.2f %%)" % (TOPK, int((~clear).sum()), N, 100 * left_out))
    assert left_out <= TOPK_CAP
    ours = helpers.TfidfTransformer().fit(X[:N_TRAIN]).transform(X)
    got, _ = helpers.most_similar(ours, k=TOPK, metric="linear kernel")
    want, _ = helpers.most_similar(T, k=TOPK, metric="linear kernel")
    np.testing.assert_array_equal(got[clear], want[clear])
