"""GPU checks of ``main_autoencoder.py --vectorize``: a raw count matrix becomes the pruned count, binary and tf-idf matrices under
the reference's artefact names, fitted on the train rows and applied to the validation rows; without the flag ``--data`` is trained
on as before."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -21            # tests/test_hip_vectorize.py: four fp32 roundings of at most 2**-24, doubled
N_TRAIN, N_VAL, F = 200, 60, 400


def _counts_file(tmp_path):
    rng = np.random.default_rng(5)
    p = 0.4 * np.exp(-np.arange(F) / 90.0) + 0.003
    M = (rng.random((N_TRAIN + N_VAL + 15, F)) < p) * rng.integers(1, 9, (N_TRAIN + N_VAL + 15, F))
    M[:, F - 10:] = 0
    M[:N_TRAIN, 300:320] = 0                                             # columns that occur in validation rows only
    X = sp.csr_matrix(M.astype(np.float32))
    path = str(tmp_path / "counts.npz")
    sp.save_npz(path, X)
    return path, X


def _same(got, want):
    got, want = got.tocsr(), want.tocsr()
    got.sort_indices(); want.sort_indices()
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(got.data, want.data)


def test_vectorize_flag_writes_the_reference_artefacts(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    from sklearn.feature_extraction.text import TfidfTransformer
    from dae_rnn_news_recommendation_amd import helpers
    path, X = _counts_file(tmp_path)
    monkeypatch.chdir(tmp_path)
    model = cli.main(["--model_name", "bow", "--data", path, "--vectorize", "--validation", "--train_row", str(N_TRAIN), "--validate_row",
                      str(N_VAL), "--min_df", "0.01", "--max_df", "0.9", "--max_features", "150", "--input_format", "tfidf", "--loss_func",
                      "mean_squared", "--triplet_strategy", "none", "--num_epochs", "1", "--similarity", "false", "--seed", "1"])
    d = model.data_dir
    names = ["article_%s_vectorized%s.npz" % (s, v) for s in ("count", "binary_count", "tfidf") for v in ("", "_validate")]
    for name in names + ["vocabulary_kept.npy", "tfidf_transformer.npz"]:
        assert os.path.exists(d + name), name
    train, val = X[:N_TRAIN], X[N_TRAIN:N_TRAIN + N_VAL]
    df = np.bincount(train.indices, minlength=F)
    tf = np.asarray(train.sum(axis=0)).ravel().astype(np.int64)
    kept = helpers.limit_features_columns(df, tf, N_TRAIN, 0.01, 0.9, 150)
    assert kept.size == 150 and not ((kept >= 300) & (kept < 320)).any()
    np.testing.assert_array_equal(np.load(d + "vocabulary_kept.npy"), kept)
    ref = TfidfTransformer().fit(train[:, kept].astype(np.float64))
    for suffix, part in (("", train), ("_validate", val)):
        _same(helpers.read_file(d + "article_count_vectorized%s.npz" % suffix), part[:, kept])
        want_b = part[:, kept].copy()
        want_b.data[:] = 1
        _same(helpers.read_file(d + "article_binary_count_vectorized%s.npz" % suffix), want_b)
        got = helpers.read_file(d + "article_tfidf_vectorized%s.npz" % suffix).tocsr()
        want = ref.transform(part[:, kept].astype(np.float64)).tocsr()      # the TRAIN idf and vocabulary on both parts
        got.sort_indices(); want.sort_indices()
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.indices, want.indices)
        assert (np.abs(got.data - want.data) <= TOL * np.abs(want.data)).all()
    t = helpers.TfidfTransformer.load(d + "tfidf_transformer.npz")
    np.testing.assert_array_equal(t.idf_, ref.idf_)
    assert t.n_features_in_ == 150
    emb, emb_v = np.load(d + "article_encoded_train.npy"), np.load(d + "article_encoded_validate.npy")      # it trained on the tf-idf matrix
    assert emb.shape == (N_TRAIN, 150 // 20) and emb_v.shape == (N_VAL, 150 // 20) and np.isfinite(emb).all() and np.isfinite(emb_v).all()


def test_without_the_flag_data_is_trained_on_as_before(tmp_path, monkeypatch, capsys):
    import main_autoencoder as cli
    from dae_rnn_news_recommendation_amd import helpers
    path, X = _counts_file(tmp_path)
    monkeypatch.chdir(tmp_path)
    argv = ["--model_name", "plain", "--data", path, "--validation", "--train_row", str(N_TRAIN), "--validate_row", str(N_VAL), "--min_df",
            "0.01", "--max_df", "0.9", "--max_features", "150", "--input_format", "tfidf", "--loss_func", "mean_squared",
            "--triplet_strategy", "none", "--num_epochs", "1", "--similarity", "false", "--seed", "1"]
    a = cli.validate(cli.build_parser().parse_args(argv))
    assert a.vectorize is False
    want, _ = cli.load_data(a)                                           # load_data as it is: whatever values the file holds
    model = cli.main(argv)
    d = model.data_dir
    _same(helpers.read_file(d + "article_tfidf_vectorized.npz"), want[:N_TRAIN])
    _same(helpers.read_file(d + "article_tfidf_vectorized_validate.npz"), want[N_TRAIN:N_TRAIN + N_VAL])
    _same(want, X[:N_TRAIN + N_VAL])
    assert not os.path.exists(d + "vocabulary_kept.npy") and not os.path.exists(d + "article_count_vectorized.npz")
