"""CPU checks of the sparse / chunked operands of top-k and label statistics: the new entry points are exported by both builds of
the library, their argument errors are reported before any device call, and the chunk plan of helpers.most_similar /
label_similarity_stats(chunk_rows=...) is what the sweeps assume."""
import ctypes

import numpy as np
import pytest

NEW = ("dae_sweep_image_bytes", "dae_sweep_image_dense", "dae_sweep_image_csr", "dae_sweep_image_norm2_max_workspace",
       "dae_sweep_image_norm2_max", "dae_topk_carry_bytes", "dae_topk_images_workspace", "dae_topk_images",
       "dae_pair_hist_images_workspace", "dae_pair_hist_images")
P = ctypes.c_void_p


def _fails(lib, rc, *words):
    msg = lib.dae_last_error().decode()
    assert rc != 0, "the call was accepted"
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_symbols_are_exported_and_the_abi_version_stays(fmt):
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load(fmt)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.dae_abi_version() == 9 == _lib.ABI_VERSION


def test_sizes():
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load()
    assert lib.dae_sweep_image_bytes(200, 1000) == 256 * 1024 * 4
    assert lib.dae_sweep_image_bytes(128, 128) == 128 * 128 * 4 and lib.dae_sweep_image_bytes(129, 129) == 256 * 256 * 4
    assert lib.dae_sweep_image_bytes(0, 10) == 0
    assert lib.dae_topk_carry_bytes(200, 10) == 256 * 10 * 8 + 256 * 4          # each row's keys, then its count
    assert lib.dae_topk_carry_bytes(100, 3) == 128 * 3 * 8 + 128 * 4
    assert lib.dae_topk_images_workspace(256, 256, 10) > 0 and lib.dae_topk_images_workspace(256, 0, 10) == 0
    assert lib.dae_pair_hist_images_workspace(256, 256, 2048) >= 2 * 2048 * 8 + 2 * 256 * 4
    assert lib.dae_sweep_image_norm2_max_workspace() >= 256 * 8
    # the images are no part of the *_images workspaces: they do not grow with D (there is no D to pass)
    assert lib.dae_topk_images_workspace(256, 256, 10) < lib.dae_topk_similarity_workspace(256, 256, 128, 10)


def test_image_argument_errors_without_a_gpu():
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load()
    a = P(256 * 1000)                                                           # aligned, never dereferenced: every call below is refused
    big = 1 << 40
    _fails(lib, lib.dae_sweep_image_dense(None, 1000, 200, 1000, 0, 0, a, big, None), "sweep_image_dense", "NULL")
    _fails(lib, lib.dae_sweep_image_dense(a, 1000, 200, 1000, 0, 0, None, big, None), "sweep_image_dense", "NULL")
    _fails(lib, lib.dae_sweep_image_csr(None, a, a, 200, 1000, 0, 0, a, big, None), "sweep_image_csr", "NULL")
    _fails(lib, lib.dae_sweep_image_csr(a, None, None, 200, 1000, 0, 0, a, big, None), "sweep_image_csr", "NULL")
    _fails(lib, lib.dae_sweep_image_csr(a, a, None, 200, 1000, 0, 0, None, big, None), "sweep_image_csr", "NULL")
    need = lib.dae_sweep_image_bytes(200, 1000)
    for call in (lambda nb: lib.dae_sweep_image_dense(a, 1000, 200, 1000, 0, 0, a, nb, None),
                 lambda nb: lib.dae_sweep_image_csr(a, a, None, 200, 1000, 0, 0, a, nb, None)):
        _fails(lib, call(need - 1), "image too small")
    # 21 504 rows of a 50 000-word vocabulary: 21 504 x 50 048 x 4 bytes is just over 4 GiB
    assert 21504 * 50048 * 4 >= 1 << 32 > 21376 * 50048 * 4
    _fails(lib, lib.dae_sweep_image_dense(a, 50000, 21504, 50000, 0, 0, a, big, None), "exceeds 4 GiB")
    _fails(lib, lib.dae_sweep_image_csr(a, a, a, 21504, 50000, 0, 0, a, big, None), "exceeds 4 GiB")
    _fails(lib, lib.dae_sweep_image_csr(a, a, a, 200, 1000, 4, 0, a, big, None), "norm must be")
    _fails(lib, lib.dae_sweep_image_csr(a, a, a, 200, 1000, 0, 2, a, big, None), "metric must be")
    _fails(lib, lib.dae_sweep_image_csr(a, a, a, 200, 1000, 0, 0, P(256 * 1000 + 4), big, None), "aligned")
    _fails(lib, lib.dae_sweep_image_dense(a, 999, 200, 1000, 0, 0, a, big, None), "ldx")
    out = ctypes.c_double()
    _fails(lib, lib.dae_sweep_image_norm2_max(None, 200, 1000, ctypes.byref(out), a, big, None), "sweep_image_norm2_max", "NULL")
    _fails(lib, lib.dae_sweep_image_norm2_max(a, 200, 1000, None, a, big, None), "NULL")
    _fails(lib, lib.dae_sweep_image_norm2_max(a, 200, 1000, ctypes.byref(out), a, 8, None), "workspace")
    _fails(lib, lib.dae_sweep_image_norm2_max(a, 21504, 50000, ctypes.byref(out), a, big, None), "exceeds 4 GiB")


def test_topk_images_argument_errors_without_a_gpu():
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load()
    a = P(256 * 1000)
    big = 1 << 40

    def call(Qi=a, Nq=200, row0=0, Ci=a, Nc=300, col0=0, D=1000, k=10, xs=0, xp=None, xi=None, carry=a, idx=a, score=a, ldk=10, ws=a,
             wsb=big):
        return lib.dae_topk_images(Qi, Nq, row0, Ci, Nc, col0, D, k, xs, xp, xi, carry, idx, score, ldk, ws, wsb, None)
    _fails(lib, call(Qi=None), "topk_images")
    _fails(lib, call(idx=None), "topk_images", "NULL")
    _fails(lib, call(score=None), "NULL")
    _fails(lib, call(carry=None), "NULL")
    _fails(lib, call(ws=None), "topk_images")
    for k in (0, 129, -1):
        _fails(lib, call(k=k, ldk=200), "k must be in 1..128")
    _fails(lib, call(xp=a), "excl_indptr and excl_items go together")
    _fails(lib, call(xi=a), "excl_indptr and excl_items go together")
    _fails(lib, call(ldk=9), "ldk")
    _fails(lib, call(row0=-1), "row0")
    _fails(lib, call(col0=2 ** 31 - 100), "31 bits")
    _fails(lib, call(Ci=None), "bad corpus")                                    # Ci == NULL means the corpus is Qi: Nc == Nq
    _fails(lib, call(Nq=21504, D=50000), "exceeds 4 GiB")
    _fails(lib, call(Nc=21504, D=50000), "exceeds 4 GiB")
    _fails(lib, call(wsb=lib.dae_topk_images_workspace(200, 300, 10) - 1), "workspace too small")
    _fails(lib, call(carry=P(256 * 1000 + 8)), "aligned")


def test_pair_hist_images_argument_errors_without_a_gpu():
    from dae_rnn_news_recommendation_amd import _lib
    lib = _lib.load()
    a = P(256 * 1000)
    big = 1 << 40

    def call(Qi=a, Nq=200, lq=a, Ci=a, Nc=300, lc=a, D=1000, lo=-1.0, hi=1.0, bins=64, hist=a, out=a, ws=a, wsb=big):
        return lib.dae_pair_hist_images(Qi, Nq, lq, Ci, Nc, lc, D, lo, hi, bins, hist, out, ws, wsb, None)
    _fails(lib, call(Qi=None), "pair_hist_images")
    _fails(lib, call(lq=None), "NULL")
    _fails(lib, call(hist=None), "NULL")
    _fails(lib, call(out=None), "NULL")
    _fails(lib, call(lc=None), "labels_c")
    _fails(lib, call(ws=None), "pair_hist_images")
    for lo, hi in ((1.0, 1.0), (0.5, -0.5), (0.0, 0.0), (float("nan"), 1.0), (0.0, float("inf")), (-3e38, 3e38)):
        _fails(lib, call(lo=lo, hi=hi), "lo < hi")                              # no automatic range here
    _fails(lib, call(bins=1), "bins must be in 2..2048")
    _fails(lib, call(bins=4096), "bins must be in 2..2048")
    _fails(lib, call(Ci=None), "bad corpus")
    _fails(lib, call(Nq=21504, D=50000), "exceeds 4 GiB")
    _fails(lib, call(wsb=lib.dae_pair_hist_images_workspace(200, 300, 64) - 1), "workspace too small")


def test_chunk_rows_rounding_and_auto():
    from dae_rnn_news_recommendation_amd import helpers
    f = helpers.sweep_chunk_rows
    assert f(None, 1000) is None
    assert [f(c, 1000) for c in (1, 127, 128, 129, 256, 1000)] == [128, 128, 128, 256, 256, 1024]
    assert f(np.int64(300), 10) == 384
    for bad in (0, -5, "all", "AUTO"):
        with pytest.raises(ValueError, match="chunk_rows"):
            f(bad, 1000)
    # "auto": the largest multiple of 128 whose image of pad128(D) fp32 columns is at most 1 GiB
    assert helpers.SWEEP_AUTO_IMAGE_BYTES == 1 << 30
    for D, Dp in ((50000, 50048), (10000, 10112), (500, 512), (1, 128)):
        c = f("auto", D)
        assert c % 128 == 0 and c * Dp * 4 <= 1 << 30 < (c + 128) * Dp * 4, (D, c)
    assert f("auto", 50000) == 5248 and f("auto", 10000) == 26496
    assert f("auto", 10 ** 7) == 128                                            # never less than one tile of rows


def test_chunk_plan():
    from dae_rnn_news_recommendation_amd import helpers
    plan = helpers.sweep_chunk_plan
    assert plan(500, 128) == [(0, 128), (128, 256), (256, 384), (384, 500)]     # ragged last chunk
    assert plan(512, 256) == [(0, 256), (256, 512)]
    assert plan(500, 512) == [(0, 500)] and plan(500, 1024) == [(0, 500)]       # chunk_rows >= N: one chunk
    assert plan(1, 128) == [(0, 1)] and plan(0, 128) == []
    for n, c in ((4096, 256), (4097, 256), (700, 384)):
        p = plan(n, c)
        assert p[0][0] == 0 and p[-1][1] == n and all(a[1] == b[0] for a, b in zip(p, p[1:]))
        assert all(a % 128 == 0 and 0 < b - a <= c for a, b in p) and all(b - a == c for a, b in p[:-1])
    for bad in (0, 100, -128):
        with pytest.raises(ValueError, match="multiple of 128"):
            plan(500, bad)


def test_lower_triangle_block_list():
    from dae_rnn_news_recommendation_amd import helpers
    assert helpers.label_stats_blocks(1) == [(0, 0, True)]
    assert helpers.label_stats_blocks(3) == [(0, 0, True), (1, 0, False), (1, 1, True), (2, 0, False), (2, 1, False), (2, 2, True)]
    assert helpers.label_stats_blocks(2, 3) == [(0, 0, False), (0, 1, False), (0, 2, False), (1, 0, False), (1, 1, False), (1, 2, False)]
    # the blocks cover the pairs j < i of the operand exactly once: diagonal blocks in self mode (j < i inside), the blocks below in full
    n, c = 700, 256
    plan = helpers.sweep_chunk_plan(n, c)
    seen = np.zeros((n, n), dtype=np.int32)
    for a, b, self_mode in helpers.label_stats_blocks(len(plan)):
        (q0, q1), (c0, c1) = plan[a], plan[b]
        blk = np.ones((q1 - q0, c1 - c0), dtype=np.int32)
        seen[q0:q1, c0:c1] += np.tril(blk, -1) if self_mode else blk
    assert np.array_equal(seen, np.tril(np.ones((n, n), dtype=np.int32), -1))


def test_window_and_shared_lists_do_not_go_with_chunk_rows():
    from dae_rnn_news_recommendation_amd import helpers
    X = np.zeros((10, 4), dtype=np.float32)
    win = (np.zeros(10, dtype=np.int32), np.full(10, 10, dtype=np.int32))
    with pytest.raises(ValueError, match="chunk_rows does not go with window"):
        helpers.most_similar(X, k=2, window=win, chunk_rows=128)
    shared = ([[1, 2]], [[0, 1]], np.zeros(10, dtype=np.int32), np.zeros(10, dtype=np.int32))
    with pytest.raises(ValueError, match="chunk_rows does not go with window"):
        helpers.most_similar(X, k=2, exclude_shared=shared, chunk_rows="auto")


def test_cli_flag():
    import main_autoencoder as cli
    p = cli.build_parser()
    base = ["--model_name", "m"]
    assert cli.sweep_chunk_rows_arg(p.parse_args(base)) is None
    assert cli.sweep_chunk_rows_arg(p.parse_args(base + ["--sweep_chunk_rows", "-1"])) == "auto"
    assert cli.sweep_chunk_rows_arg(p.parse_args(base + ["--sweep_chunk_rows", "300"])) == 300
