"""GPU tests of the kernels that turn gradients into parameters, each called on its own through the C ABI:
optimizer row bands, bias update, shadow transpose, the data-parallel unpack, the split-K finish epilogues above their
slab-group size, the bias gradients with the fused update, sym_scale in bf16, the step statistics and the row losses.

Every output buffer sits between two 4 KiB guard regions of a fixed byte that are checked after each call; padding inside a
buffer is checked for the exact value the kernel promises (zero, or its bits from before the call); inputs that must not be
read (chunk rows beyond Fp, the gap behind a chunk's payload, padding of partial sums) hold NaN bit patterns.

Tolerances are the suite's own: bit for bit for integer / transposed / rounded images, rtol 2e-5 + atol 2e-6 for fp32
optimizer results against oracle.opt_apply (test_opt_step), 2e-5 relative for fp32 sums against float64 (header of
test_hip_kernels.py), 1e-5 for dh_finish's delta1 (test_dh_finish_and_bias_grads), bf16 images == bf16_round(fp32 result).

The defect each entry's cases would catch (C: confirmed by building the library with that edit; A: argued from the code):
  dae_dp_unpack          dropping `r * chunk_stride` from the source (every tile from chunk 0): all cases with world >= 2     (C)
                         dropping `r * chunk_rows` from the source row: world >= 2 copies later, partly NaN, rows             (A)
                         summing the bias gradients over `world - 1` ranks or from chunk 0 only: grad_b differs bit for bit   (A)
  dae_opt_step_rows      offsetting grad_rows by f0 as W is: band (64, 192) reads other (or NaN) gradient rows               (C)
  dae_transpose_shadow   a non-square mix-up of Fp and Hp in the store index: the (192, 128) and (128, 320) images differ    (A)
  dae_opt_bias           swapping the [bh | bv] slot halves: Hp != Fp and every slot element differs                         (C)
  dae_bias_grads apply   slot index k instead of Hp + k for b_v: b_v is updated with b_h's accumulators                       (A)
  dae_dh_finish          dropping the slabs after the 8th (or adding the clamped last slab twice): splits = 9 and 17          (C)
  dae_encode_finish      stepping the slab groups by 8 instead of 4, or masking the tail with `<`/`<=` confused: splits = 5, 9      (A)
  dae_sym_scale bf16     truncating instead of rounding to nearest even: half of the elements differ in the last bit          (A)
  dae_step_stats         folding with B instead of N_valid, or not writing tri_scalars[1..3] back in the batch_all fold      (A)
  dae_weighted_loss_rows striding rows by F instead of ldx / ldy: rows >= 1 read the NaN gap                                  (A)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
import update_reference as R

pytestmark = pytest.mark.gpu

GUARD = 4096
GUARD_BYTE = 0xA5
ACTS = ("sigmoid", "tanh", "none")


@pytest.fixture(scope="module")
def ops():
    from dae_rnn_news_recommendation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from dae_rnn_news_recommendation_amd import _lib
    _lib.load()
    return _lib


class Buf:
    """A device buffer initialised from a NumPy array, with GUARD bytes of GUARD_BYTE in front of it and behind it."""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        self.init = arr.copy()
        raw = np.full(arr.nbytes + 2 * GUARD, GUARD_BYTE, np.uint8)
        raw[GUARD:GUARD + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        self.raw = torch.as_tensor(raw).cuda()

    @property
    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + GUARD)

    def get(self):
        """The buffer's content now (same dtype and shape); asserts that both guards still hold their byte."""
        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        n = self.init.nbytes
        assert (raw[:GUARD] == GUARD_BYTE).all() and (raw[GUARD + n:] == GUARD_BYTE).all(), "guard region overwritten"
        return raw[GUARD:GUARD + n].view(self.init.dtype).reshape(self.init.shape).copy()

    def unchanged(self):
        return bits_equal(self.get(), self.init)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def opt_close(a, b):
    return np.allclose(a, b, rtol=2e-5, atol=2e-6)


def nan_padded(a, rows, cols):
    """float32 [rows x cols] holding `a` in its top-left corner and NaN everywhere else."""
    out = np.full((rows, cols), np.nan, np.float32)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def nan_tail(a, n):
    out = np.full(n, np.nan, np.float32)
    out[:len(a)] = a
    return out


def call_rc(L, name, *args):
    return getattr(L.load(), name)(*args)


def lr_dev(opt, lr, t):
    """The step size the device entries take: Adam's carries the bias correction of step t."""
    return R.adam_lr(lr, t) if opt == "adam" else lr


def make_state(opt, parts_s1, parts_s2):
    """oracle.OptState whose slots start from the given float32 arrays (one per parameter)."""
    st = O.OptState(opt, [p.shape for p in parts_s1], np.float32)
    if opt in ("ada_grad", "momentum"):
        st.acc = [p.copy() for p in parts_s1]
    if opt == "adam":
        st.m = [p.copy() for p in parts_s1]
        st.v = [p.copy() for p in parts_s2]
    return st


def state_slots(st):
    """(s1 parts, s2 parts) of an OptState; None where the optimizer has no such slot."""
    if st.opt in ("ada_grad", "momentum"):
        return st.acc, None
    if st.opt == "adam":
        return st.m, st.v
    return None, None


def lo_dtype(dtype):
    return np.uint16 if dtype == "bf16" else np.float32


def lo_image(W, dtype):
    """What the low-precision shadow of the fp32 matrix W holds: bf16 bits, or the floats themselves."""
    return R.bf16_bits(W) if dtype == "bf16" else np.asarray(W, np.float32)


def lo_sentinel(shape, dtype):
    return np.full(shape, 0x4B4B, np.uint16) if dtype == "bf16" else np.full(shape, 7.25, np.float32)


# ----------------------------------------------------------------------------------------------- #
# 1. dae_dp_unpack
# ----------------------------------------------------------------------------------------------- #
def _unpack_buffers(rng, Fp, Hp, dtype, extra_slots=32):
    n = Hp + Fp
    return dict(W_lo=Buf(lo_sentinel((Fp, Hp), dtype)), Wt_lo=Buf(lo_sentinel((Hp, Fp), dtype)),
                bh=Buf(rng.standard_normal(Hp).astype(np.float32)), bv=Buf(rng.standard_normal(Fp).astype(np.float32)),
                s1=Buf((rng.random(n + extra_slots) + 0.1).astype(np.float32)), s2=Buf(rng.random(n + extra_slots).astype(np.float32)),
                grad_b=Buf(np.full(n, 123.0, np.float32)))


def _unpack_call(L, b, recv, world, chunk_rows, stride, bias_off, Fp, Hp, dtype, opt, lr, mom, gscale):
    return call_rc(L, "dae_dp_unpack", L.ptr(recv), world, chunk_rows, stride, bias_off, Fp, Hp, L.BF16 if dtype == "bf16" else L.F32,
                   b["W_lo"].ptr, b["Wt_lo"].ptr, L.OPT[opt], lr, mom, gscale, b["bh"].ptr, b["bv"].ptr, b["s1"].ptr, b["s2"].ptr,
                   b["grad_b"].ptr, L.current_stream())


@pytest.mark.parametrize("opt", R.OPTS)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("case", R.UNPACK_CASES, ids=lambda c: "Fp%d-Hp%d-w%d-c%d" % c)
def test_dp_unpack(L, case, dtype, opt):
    """Three successive unpacks of a synthetic receive buffer (chunk_stride = payload rounded to 16 bytes + 64; NaN bytes in
    chunk rows beyond Fp and in the gap): W_lo / Wt_lo bit for bit, grad_b == the fp32 rank-order sum bit for bit, biases and
    their slots against oracle.opt_apply on that sum."""
    Fp, Hp, world, chunk_rows = case
    es = 2 if dtype == "bf16" else 4
    n = Hp + Fp
    rng = np.random.default_rng(Fp + Hp + world)
    b = _unpack_buffers(rng, Fp, Hp, dtype)
    s1_0, s2_0 = b["s1"].init, b["s2"].init
    st = make_state(opt, [s1_0[:Hp], s1_0[Hp:n]], [s2_0[:Hp], s2_0[Hp:n]])
    want_bh, want_bv = b["bh"].init.copy(), b["bv"].init.copy()
    base = R.distinct_bits(Fp, Hp, es)
    for t in range(1, 4):
        rows = np.roll(base, 7 * t, axis=0)
        gb = rng.standard_normal((world, n)).astype(np.float32)
        buf, stride, bias_off = R.build_recv(rows, gb, world, chunk_rows)
        assert stride > bias_off + 4 * n and stride % 16 == 0
        recv = dev(buf)
        rc = _unpack_call(L, b, recv, world, chunk_rows, stride, bias_off, Fp, Hp, dtype, opt, lr_dev(opt, 0.1, t), 0.5, 0.5)
        L.check(rc, "dae_dp_unpack")
        acc = np.zeros(n, np.float32)
        for r in range(world):
            acc = acc + gb[r]
        assert np.array_equal(bits(b["W_lo"].get()), rows), t
        assert np.array_equal(bits(b["Wt_lo"].get()), rows.T), t
        assert bits_equal(b["grad_b"].get(), acc), t
        gs = acc * np.float32(0.5)
        O.opt_apply(st, [want_bh, want_bv], [gs[:Hp], gs[Hp:]], 0.1, 0.5, np.float32)
    assert opt_close(b["bh"].get(), want_bh) and opt_close(b["bv"].get(), want_bv)
    assert not opt_close(b["bv"].init, want_bv)
    for got, init, parts in zip((b["s1"].get(), b["s2"].get()), (s1_0, s2_0), state_slots(st)):
        if parts is None:
            assert bits_equal(got, init)                      # a slot the optimizer does not have is not written
        else:
            assert opt_close(got[:n], np.concatenate(parts))
            assert bits_equal(got[n:], init[n:])              # elements behind [bh | bv] stay


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("world,chunk_rows", [(1, 192), (4, 96)], ids=["chunks-do-not-cover-W", "chunk-rows-not-64n"])
def test_dp_unpack_argument_checks(L, dtype, world, chunk_rows):
    """world * chunk_rows < Fp and chunk_rows % 64 != 0 are refused and nothing is written.  (The buffer is large enough for
    whatever rows a launch would read, so a missing check shows as changed outputs, not as a fault.)"""
    Fp, Hp = 384, 128
    rng = np.random.default_rng(5)
    b = _unpack_buffers(rng, Fp, Hp, dtype)
    bias_off, stride = R.chunk_layout(Fp, Hp, 192, 2 if dtype == "bf16" else 4)
    recv = torch.zeros(4 * stride, dtype=torch.uint8, device="cuda")
    rc = _unpack_call(L, b, recv, world, chunk_rows, stride, bias_off, Fp, Hp, dtype, "adam", 0.1, 0.5, 1.0)
    assert rc != 0
    assert b"dp_unpack" in L.load().dae_last_error()
    for k, buf in b.items():
        assert buf.unchanged(), k


# ----------------------------------------------------------------------------------------------- #
# 2. dae_opt_step_rows
# ----------------------------------------------------------------------------------------------- #
ROWS_FP, ROWS_HP = 384, 192


def _rows_buffers(rng, dtype):
    Fp, Hp = ROWS_FP, ROWS_HP
    return dict(W=Buf(rng.standard_normal((Fp, Hp)).astype(np.float32)), s1=Buf((rng.random((Fp, Hp)) + 0.1).astype(np.float32)),
                s2=Buf(rng.random((Fp, Hp)).astype(np.float32)), W_lo=Buf(lo_sentinel((Fp, Hp), dtype)))


def _rows_call(L, b, opt, lr, grad_rows, f0, f1, dtype):
    """grad_rows: float32 [f1 - f0 x Hp], handed over at the start of an Fp-row buffer whose other rows are NaN."""
    g = dev(nan_padded(grad_rows, ROWS_FP, ROWS_HP))
    return call_rc(L, "dae_opt_step_rows", L.OPT[opt], lr, 0.5, 0.5, b["W"].ptr, L.ptr(g), b["s1"].ptr, b["s2"].ptr, ROWS_HP, f0, f1,
                   L.BF16 if dtype == "bf16" else L.F32, b["W_lo"].ptr, L.current_stream())


@pytest.mark.parametrize("opt", R.OPTS)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("band", [(0, 384), (64, 192), (320, 384), (128, 128)], ids=lambda b: "rows%d-%d" % b)
def test_opt_step_rows_band(L, band, dtype, opt):
    """Three steps on one row band from band-local gradients with distinct rows: rows inside match oracle.opt_apply on the band
    and W_lo == round(W); rows outside keep their bits in W, both slots and W_lo.  The empty band returns 0 and writes nothing."""
    f0, f1 = band
    rng = np.random.default_rng(30 + f0 + f1)
    b = _rows_buffers(rng, dtype)
    W0, s10, s20 = b["W"].init, b["s1"].init, b["s2"].init
    st = make_state(opt, [s10[f0:f1]], [s20[f0:f1]])
    want = W0[f0:f1].copy()
    for t in range(1, 4):
        g = rng.standard_normal((max(f1 - f0, 1), ROWS_HP)).astype(np.float32)
        assert _rows_call(L, b, opt, lr_dev(opt, 0.1, t), g[:f1 - f0], f0, f1, dtype) == 0
        if f1 > f0:
            O.opt_apply(st, [want], [g * np.float32(0.5)], 0.1, 0.5, np.float32)
    W, s1, s2, W_lo = (b[k].get() for k in ("W", "s1", "s2", "W_lo"))
    out = np.ones(ROWS_FP, bool); out[f0:f1] = False
    for got, buf in ((W, b["W"]), (s1, b["s1"]), (s2, b["s2"]), (W_lo, b["W_lo"])):
        assert bits_equal(got[out], buf.init[out])
    if f1 == f0:
        return
    assert opt_close(W[f0:f1], want) and not opt_close(W0[f0:f1], want)
    assert bits_equal(W_lo[f0:f1], lo_image(W[f0:f1], dtype))
    for got, init, parts in zip((s1, s2), (s10, s20), state_slots(st)):
        if parts is None:
            assert bits_equal(got, init)
        else:
            assert opt_close(got[f0:f1], parts[0])


@pytest.mark.parametrize("opt", R.OPTS)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_opt_step_rows_tiling_equals_whole(L, dtype, opt):
    """[0, Fp) tiled by three bands in shuffled order gives the bits of one (0, Fp) call, in W, both slots and W_lo."""
    rng = np.random.default_rng(31)
    whole = _rows_buffers(rng, dtype)
    tiled = {k: Buf(v.init) for k, v in whole.items()}
    for t in range(1, 4):
        g = rng.standard_normal((ROWS_FP, ROWS_HP)).astype(np.float32)
        assert _rows_call(L, whole, opt, lr_dev(opt, 0.1, t), g, 0, ROWS_FP, dtype) == 0
        for f0, f1 in ((128, 320), (320, 384), (0, 128)):
            assert _rows_call(L, tiled, opt, lr_dev(opt, 0.1, t), g[f0:f1], f0, f1, dtype) == 0
    for k in whole:
        assert bits_equal(whole[k].get(), tiled[k].get()), k
    assert not bits_equal(whole["W"].get(), whole["W"].init)


# ----------------------------------------------------------------------------------------------- #
# 3. dae_transpose_shadow
# ----------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("Fp,Hp", [(64, 64), (192, 128), (128, 320)])
def test_transpose_shadow(L, Fp, Hp, dtype):
    W = R.distinct_bits(Fp, Hp, 2 if dtype == "bf16" else 4)
    out = Buf(np.zeros((Hp, Fp), W.dtype))
    d_W = dev(W.view(np.int16 if dtype == "bf16" else np.int32))
    L.call("dae_transpose_shadow", L.ptr(d_W), Fp, Hp, L.BF16 if dtype == "bf16" else L.F32,
           out.ptr, L.current_stream())
    assert np.array_equal(out.get(), W.T)


# ----------------------------------------------------------------------------------------------- #
# 4. dae_opt_bias
# ----------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("opt", R.OPTS)
@pytest.mark.parametrize("Hp,Fp", [(64, 256), (128, 384)])
def test_opt_bias(L, Hp, Fp, opt):
    """Three steps; slot layout [bh | bv]; the elements of a longer slot buffer behind Hp + Fp stay untouched."""
    rng = np.random.default_rng(40 + Hp)
    n, tail = Hp + Fp, 64
    bh, bv = Buf(rng.standard_normal(Hp).astype(np.float32)), Buf(rng.standard_normal(Fp).astype(np.float32))
    s1, s2 = Buf((rng.random(n + tail) + 0.1).astype(np.float32)), Buf(rng.random(n + tail).astype(np.float32))
    st = make_state(opt, [s1.init[:Hp], s1.init[Hp:n]], [s2.init[:Hp], s2.init[Hp:n]])
    want_bh, want_bv = bh.init.copy(), bv.init.copy()
    for t in range(1, 4):
        g = rng.standard_normal(n).astype(np.float32)
        d_g = dev(g)
        L.call("dae_opt_bias", L.OPT[opt], lr_dev(opt, 0.1, t), 0.5, 0.5, bh.ptr, bv.ptr, L.ptr(d_g), s1.ptr, s2.ptr, Hp, Fp,
               L.current_stream())
        gs = g * np.float32(0.5)
        O.opt_apply(st, [want_bh, want_bv], [gs[:Hp], gs[Hp:]], 0.1, 0.5, np.float32)
    assert opt_close(bh.get(), want_bh) and opt_close(bv.get(), want_bv)
    assert not opt_close(bh.init, want_bh)
    for got, buf, parts in zip((s1.get(), s2.get()), (s1, s2), state_slots(st)):
        if parts is None:
            assert bits_equal(got, buf.init)
        else:
            assert opt_close(got[:n], np.concatenate(parts))
            assert bits_equal(got[n:], buf.init[n:])


# ----------------------------------------------------------------------------------------------- #
# 5. dae_bias_grads with apply = 1
# ----------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("opt", R.OPTS)
def test_bias_grads_apply(L, opt):
    """The fused bias update: gradients bit-equal to the apply = 0 call on the same inputs, biases and slots (b_h at j, b_v at
    Hp + k) against oracle.opt_apply on those gradients; the padded entries get a zero gradient whatever the partial sums'
    padding columns hold (NaN here)."""
    rng = np.random.default_rng(50)
    B, H, F = 150, 100, 300
    Bp, Hp, Fp = L.pad(B), L.pad(H), L.pad(F)
    n, nrw, nrb = Hp + Fp, 2 * Bp // 128, Bp // 32
    act = ACTS[R.OPTS.index(opt) % 3]
    bh0 = np.zeros(Hp, np.float32); bh0[:H] = rng.standard_normal(H) * 0.3
    bv0 = np.zeros(Fp, np.float32); bv0[:F] = rng.standard_normal(F) * 0.3
    bh, bv = Buf(bh0), Buf(bv0)
    s1, s2 = Buf((rng.random(n) + 0.1).astype(np.float32)), Buf(rng.random(n).astype(np.float32))
    st = make_state(opt, [s1.init[:Hp], s1.init[Hp:]], [s2.init[:Hp], s2.init[Hp:]])
    want_bh, want_bv = bh0.copy(), bv0.copy()
    for t in range(1, 4):
        dbv_part = np.full((nrw, Fp), np.nan, np.float32); dbv_part[:, :F] = rng.standard_normal((nrw, F))
        colsum = np.full((2, nrb, Hp), np.nan, np.float32); colsum[:, :, :H] = rng.standard_normal((2, nrb, H))
        d_dbv, d_cs = dev(dbv_part), dev(colsum)
        outs = []
        for apply in (0, 1):
            dbh, dbv = Buf(np.full(Hp, 9.0, np.float32)), Buf(np.full(Fp, 9.0, np.float32))
            L.call("dae_bias_grads", L.ptr(d_dbv), nrw, L.ptr(d_cs), nrb, bh.ptr, H, Hp, F, Fp, L.ACT[act], dbh.ptr, dbv.ptr, apply,
                   L.OPT[opt], lr_dev(opt, 0.1, t), 0.5, 0.5, bv.ptr, s1.ptr, s2.ptr, L.current_stream())
            outs.append((dbh.get(), dbv.get()))
            if apply == 0:                                  # apply = 0 leaves the parameters alone
                assert opt_close(bh.get(), want_bh) and opt_close(bv.get(), want_bv)
        (dbh0, dbv0), (dbh1, dbv1) = outs
        assert bits_equal(dbh0, dbh1) and bits_equal(dbv0, dbv1)
        assert (dbh1[H:] == 0).all() and (dbv1[F:] == 0).all()
        ab = R.act(act, want_bh[:H].astype(np.float64))
        cs = colsum.astype(np.float64)[:, :, :H].sum(1)
        assert rel_err(dbh1[:H], cs[0] - R.act_grad_from_output(act, ab) * cs[1]) < 2e-5
        assert rel_err(dbv1[:F], dbv_part.astype(np.float64)[:, :F].sum(0)) < 2e-5
        O.opt_apply(st, [want_bh, want_bv], [dbh1 * np.float32(0.5), dbv1 * np.float32(0.5)], 0.1, 0.5, np.float32)
        assert opt_close(bh.get(), want_bh) and opt_close(bv.get(), want_bv), t
    assert not opt_close(bv0, want_bv)
    for got, buf, parts in zip((s1.get(), s2.get()), (s1, s2), state_slots(st)):
        if parts is None:
            assert bits_equal(got, buf.init)
        else:
            assert opt_close(got, np.concatenate(parts))


# ----------------------------------------------------------------------------------------------- #
# 6. dae_dh_finish
# ----------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("extra", [False, True], ids=["plain", "dh_extra"])
@pytest.mark.parametrize("splits", [1, 8, 9, 17])
def test_dh_finish_slab_groups(L, splits, extra, dtype):
    """Slab counts at, just above and two groups above the kernel's group of 8, against float64; the activation rotates with
    the case.  The padding of every input is NaN: delta1, its transpose and the column sums must be zero there all the same."""
    act = ACTS[(splits + int(extra)) % 3]
    for B, H in ((150, 100), (33, 65)):
        rng = np.random.default_rng(60 + splits + B)
        Bp, Hp = L.pad(B), L.pad(H)
        slabs = np.full((splits, Bp, Hp), np.nan, np.float32); slabs[:, :B, :H] = rng.standard_normal((splits, B, H))
        bh = nan_tail(rng.standard_normal(H) * 0.3, Hp)
        a1 = R.act(act, rng.standard_normal((B, H))).astype(np.float32)
        h = nan_padded(a1 - R.act(act, bh[:H]), Bp, Hp)
        ex = nan_padded(rng.standard_normal((B, H)), Bp, Hp) if extra else None
        d1 = Buf(np.full((Bp, Hp), 5.0, np.float32))
        d1t = Buf(lo_sentinel((Hp, Bp), dtype))
        colsum = Buf(np.full((2, Bp // 32, Hp), 5.0, np.float32))
        d_slabs, d_ex, d_h, d_bh = dev(slabs), None if ex is None else dev(ex), dev(h), dev(bh)
        L.call("dae_dh_finish", L.ptr(d_slabs), splits, Bp * Hp, Hp, L.ptr(d_ex), L.ptr(d_h), Hp,
               L.ptr(d_bh), B, H, L.ACT[act], L.BF16 if dtype == "bf16" else L.F32, d1t.ptr, Bp, colsum.ptr, d1.ptr, L.current_stream())
        want_d1, want_cs = R.dh_finish(slabs, ex, h, bh, B, H, act)
        got = d1.get()
        assert rel_err(got[:B, :H], want_d1[:B, :H]) < 1e-5, (B, H)
        assert (got[B:] == 0).all() and (got[:, H:] == 0).all()
        assert bits_equal(d1t.get(), lo_image(got, dtype).T.copy())
        cs = colsum.get()
        nb = -(-B // 32)
        for which in (0, 1):
            assert rel_err(cs[which, :nb, :H], want_cs[which, :nb, :H]) < 2e-5, (B, H, which)
        assert (cs[:, nb:] == 0).all() and (cs[:, :, H:] == 0).all()


# ----------------------------------------------------------------------------------------------- #
# 7. dae_encode_finish
# ----------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("splits", [1, 4, 5, 9])
def test_encode_finish_slab_groups(ops, L, splits, dtype, act):
    """test_encode_finish's assertions at slab counts at and above the kernel's group of 4, in both dtypes; NaN in the inputs'
    padding."""
    for B, H in ((70, 200), (33, 65)):
        rng = np.random.default_rng(70 + splits + B)
        Bp, Hp = L.pad(B), L.pad(H)
        slabs = np.full((splits, Bp, Hp), np.nan, np.float32); slabs[:, :B, :H] = rng.standard_normal((splits, B, H))
        bh = nan_tail(rng.standard_normal(H) * 0.3, Hp)
        lo = lo_dtype(dtype)
        h32, hlo, ht = Buf(np.full((Bp, Hp), 5.0, np.float32)), Buf(lo_sentinel((Bp, Hp), dtype)), Buf(lo_sentinel((Hp, Bp), dtype))
        ha, hb = Buf(np.full((Bp, 3 * Hp), 0x4B4B, np.uint16)), Buf(np.full((Bp, 3 * Hp), 0x4B4B, np.uint16))
        d_slabs, d_bh = dev(slabs), dev(bh)
        L.call("dae_encode_finish", L.ptr(d_slabs), splits, Bp * Hp, Hp, L.ptr(d_bh), B, H, L.ACT[act], L.BF16 if dtype == "bf16" else L.F32,
               h32.ptr, hlo.ptr, Hp, ht.ptr, Bp, ha.ptr, hb.ptr, L.current_stream())
        z = slabs[:, :B, :H].sum(0) + bh[:H]
        want = np.zeros((Bp, Hp), np.float32); want[:B, :H] = O.act(act, z) - O.act(act, bh[:H])
        got = h32.get()
        assert np.allclose(got, want, rtol=1e-5, atol=2e-6), (B, H)
        assert (got[B:] == 0).all() and (got[:, H:] == 0).all()
        got_lo = hlo.get()
        assert got_lo.dtype == lo and bits_equal(got_lo, lo_image(got, dtype))
        assert bits_equal(ht.get(), got_lo.T.copy())
        a, b = ha.get(), hb.get()
        assert np.array_equal(a[:, :Hp], R.bf16_bits(got))
        D = ops.gemm_nt(dev(a.view(np.int16)).view(torch.bfloat16), dev(b.view(np.int16)).view(torch.bfloat16))[0].cpu().numpy()
        hd = got.astype(np.float64)
        ref = hd @ hd.T
        assert np.abs(D - ref).max() <= 3e-5 * np.abs(ref).max()


# ----------------------------------------------------------------------------------------------- #
# 8. dae_sym_scale in bf16
# ----------------------------------------------------------------------------------------------- #
def test_sym_scale_bf16(L):
    """The bf16 image is bf16_round of the fp32 image bit for bit; both are zero outside [0, B)^2 though G's padding is NaN."""
    rng = np.random.default_rng(80)
    B = 200
    Bp = L.pad(B)
    G = nan_padded(rng.standard_normal((B, B)), Bp, Bp)
    tri = np.array([0.37, 1.0, 2.0, 3.0], np.float32)
    g32, g16 = Buf(np.full((Bp, Bp), 5.0, np.float32)), Buf(np.full((Bp, Bp), 0x4B4B, np.uint16))
    dG, dtri = dev(G), dev(tri)
    L.call("dae_sym_scale", L.ptr(dG), B, Bp, L.ptr(dtri), L.F32, g32.ptr, L.current_stream())
    L.call("dae_sym_scale", L.ptr(dG), B, Bp, L.ptr(dtri), L.BF16, g16.ptr, L.current_stream())
    got = g32.get()
    Gd = G[:B, :B].astype(np.float64)
    assert rel_err(got[:B, :B], float(tri[0]) * (Gd + Gd.T)) < 2e-5
    assert (got[B:] == 0).all() and (got[:, B:] == 0).all()
    assert np.array_equal(g16.get(), R.bf16_bits(got))
    assert len(np.unique(g16.get())) > 1000


# ----------------------------------------------------------------------------------------------- #
# 9. dae_step_stats
# ----------------------------------------------------------------------------------------------- #
def _stats_case(L, rng, strategy, B, Bp, alpha, ae, **inputs):
    """Run dae_step_stats on `inputs` (rowloss_part + cw, or tile_part) for one strategy and check all eight slots."""
    tri0 = np.array([0.31, 0.6, 0.25, 17.0], np.float32)
    tri = nvalid = loss_part = cnt_part = None
    nv = None
    if strategy == "batch_hard":
        tri = Buf(tri0)
    elif strategy == "batch_all":
        tri = Buf(np.array([0.31, -1.0, -1.0, -1.0], np.float32))
        nv = B * 200000 + 7                                 # above the largest possible sum of cnt_part
        nvalid = dev(np.array([nv], np.int64))
        lp = nan_tail(rng.random(B) * 50.0, Bp)
        cp = np.full(Bp, 0xFFFFFFFF, np.uint32); cp[:B] = rng.integers(0, 100000, B)
        loss_part, cnt_part = dev(lp), dev(cp.view(np.int32))
    stats = Buf(np.full(L.STATS_STRIDE, 5.0, np.float32))
    rp, tp, cw = inputs.get("rowloss_part"), inputs.get("tile_part"), inputs.get("cw")
    d_rp, d_tp, d_cw = (None if a is None else dev(a) for a in (rp, tp, cw))
    L.call("dae_step_stats", L.ptr(d_rp), 0 if rp is None else rp.shape[0], L.ptr(d_tp),
           0 if tp is None else len(tp), L.ptr(d_cw), B, Bp, L.TRIPLET[strategy], alpha,
           None if tri is None else tri.ptr, L.ptr(nvalid), L.ptr(loss_part), L.ptr(cnt_part), stats.ptr, L.current_stream())
    if strategy == "batch_all":
        want = R.step_stats(ae, strategy, alpha, nvalid=nv, loss_part=lp[:B], cnt_part=cp[:B])
        t = tri.get()
        assert t[0] == np.float32(0.31)                                   # the miner's scale is not this kernel's to write
        assert np.allclose(t[1:], want[2:5], rtol=2e-5, atol=0)           # folded loss / fraction / count are written back
    else:
        want = R.step_stats(ae, strategy, alpha, tri_scalars=tri0)
        assert tri is None or tri.unchanged()
    got = stats.get()
    assert np.allclose(got[:6], want, rtol=2e-5, atol=0), (got, want)
    assert np.allclose(got[0], got[1] + np.float32(alpha) * got[2], rtol=2e-6) and got[6] == 0 and got[7] == 0
    if strategy == "none":
        assert (got[2:6] == 0).all()


@pytest.mark.parametrize("strategy", ["none", "batch_hard", "batch_all"])
@pytest.mark.parametrize("B", [70, 1500])
@pytest.mark.parametrize("n_col_waves", [1, 3])
def test_step_stats_rowloss_path(L, n_col_waves, B, strategy):
    rng = np.random.default_rng(90 + B + n_col_waves)
    Bp = L.pad(B)
    rp = np.full((n_col_waves, Bp), np.nan, np.float32); rp[:, :B] = rng.random((n_col_waves, B)) * 40.0
    w = rng.integers(1, 50, B).astype(np.float64)
    cw = nan_tail(w / w.sum(), Bp)
    ae = float((rp[:, :B].astype(np.float64).sum(0) * cw[:B].astype(np.float64)).sum())
    _stats_case(L, rng, strategy, B, Bp, 0.75, ae, rowloss_part=rp, cw=cw)


@pytest.mark.parametrize("strategy", ["none", "batch_hard", "batch_all"])
@pytest.mark.parametrize("n_tiles", [1, 37, 2000])
def test_step_stats_tile_path(L, n_tiles, strategy):
    rng = np.random.default_rng(95 + n_tiles)
    B = 300
    tp = (rng.random(n_tiles) * 3.0).astype(np.float32)
    _stats_case(L, rng, strategy, B, L.pad(B), 0.75, float(tp.astype(np.float64).sum()), tile_part=tp)


# ----------------------------------------------------------------------------------------------- #
# 10. dae_weighted_loss_rows
# ----------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("F", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("loss_func", ["cross_entropy", "mean_squared", "cosine_proximity"])
def test_weighted_loss_rows(L, loss_func, F):
    """Row losses around the 256-thread pass length, with leading dimensions larger than F and NaN in the gap."""
    rng = np.random.default_rng(100 + F)
    B, ldx, ldy = 5, F + 13, F + 7
    x = (rng.random((B, F)) < 0.3).astype(np.float32) if loss_func == "cross_entropy" else (rng.random((B, F)) + 0.05).astype(np.float32)
    y = (rng.random((B, F)) * 0.98 + 0.01).astype(np.float32)
    out = Buf(np.full(B, 5.0, np.float32))
    d_x, d_y = dev(nan_padded(x, B, ldx)), dev(nan_padded(y, B, ldy))
    L.call("dae_weighted_loss_rows", L.ptr(d_x), ldx, L.ptr(d_y), ldy, B, F, L.LOSS[loss_func],
           out.ptr, L.current_stream())
    want = O.weighted_loss_rows(x.astype(np.float64), y.astype(np.float64), loss_func, np.float64)
    assert rel_err(out.get(), want) < 2e-5


def test_weighted_loss_rows_ce_saturation(L):
    """The row of test_decode_ce_saturation: y exactly 0 and 1 against x = 0 / 1 alternating -- log(1e-16) terms stay finite."""
    B, F = 3, 128
    y = np.zeros((B, F), np.float32); y[:, :64] = 1.0
    x = np.zeros((B, F), np.float32); x[:, ::2] = 1.0
    out = Buf(np.full(B, 5.0, np.float32))
    d_x, d_y = dev(x), dev(y)
    L.call("dae_weighted_loss_rows", L.ptr(d_x), F, L.ptr(d_y), F, B, F, L.LOSS["cross_entropy"], out.ptr, L.current_stream())
    got = out.get()
    assert np.isfinite(got).all()
    assert np.allclose(got, O.weighted_loss_rows(x, y, "cross_entropy", np.float32), rtol=1e-4)
