"""Plain NumPy restatement of the update half of the step: optimizer element update, row-band update, the packed
data-parallel receive buffer and its unpack, the split-K finish epilogues and the per-step statistics.

Everything floating point is computed in the dtype the caller names (float64 for the reference proper, float32 for
a same-formula restatement that measures what fp32 itself costs); the 16-bit images are handled as exact uint16 bit
patterns.  The module imports nothing from the package under test."""
import numpy as np

OPTS = ("gradient_descent", "ada_grad", "momentum", "adam")
NAN_BYTE = 0xFF                    # 0xFFFF is a bf16 NaN, 0xFFFFFFFF an fp32 NaN: a buffer of these bytes poisons whatever reads it


# ----------------------------------------------------------------------------------------------- #
# exact bit helpers
# ----------------------------------------------------------------------------------------------- #
def bf16_bits(a):
    """float32 -> bf16 bit patterns (uint16), round to nearest even; NaN stays NaN (quiet bit set)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(a, np.float32))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_from_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(a):
    return bf16_from_bits(bf16_bits(a))


def distinct_bits(rows, cols, es):
    """[rows x cols] of bit patterns of finite numbers, uint16 for es = 2 and uint32 for es = 4.  The 32-bit ones are all
    different; the 16-bit ones are different up to 32639 elements and then repeat with that odd period, so that no two rows,
    columns or 64 x 64 tiles of a matrix with even dimensions hold the same values."""
    k = np.arange(rows * cols, dtype=np.uint64)
    if es == 2:
        return (k % 32639).astype(np.uint16).reshape(rows, cols)                        # 32639 = 0x7F7F: below +inf (0x7F80)
    return (0x3F000000 + k * 7919).astype(np.uint32).reshape(rows, cols)                # floats from 0.5 upwards, 7919 ulp apart


# ----------------------------------------------------------------------------------------------- #
# optimizers (tf.train.{GradientDescent,Adagrad,Momentum,Adam}Optimizer element formulas)
# ----------------------------------------------------------------------------------------------- #
def adam_lr(lr, t):
    return float(lr) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)


def opt_update(opt, p, g, s1, s2, lr, momentum, t, dt=np.float64):
    """One update of the elements p with gradient g at step t (1-based); s1 / s2 are the slots (accumulator or m / v).
    Returns new (p, s1, s2) arrays in dt; nothing is modified in place.  Unused slots are returned unchanged."""
    p = np.asarray(p, dt); g = np.asarray(g, dt)
    s1 = None if s1 is None else np.asarray(s1, dt)
    s2 = None if s2 is None else np.asarray(s2, dt)
    lr = dt(lr)
    if opt == "gradient_descent":
        return p - lr * g, s1, s2
    if opt == "ada_grad":
        a = s1 + g * g
        return p - lr * g / np.sqrt(a), a, s2
    if opt == "momentum":
        a = dt(momentum) * s1 + g
        return p - lr * a, a, s2
    if opt == "adam":
        lr_t = dt(adam_lr(lr, t))
        m = dt(0.9) * s1 + dt(1 - 0.9) * g
        v = dt(0.999) * s2 + dt(1 - 0.999) * g * g
        return p - lr_t * m / (np.sqrt(v) + dt(1e-8)), m, v
    raise ValueError(opt)


def init_slots(opt, shape, dt=np.float64):
    """Slot values of a fresh optimizer: Adagrad's accumulator starts at 0.1, everything else at zero."""
    return np.full(shape, 0.1 if opt == "ada_grad" else 0.0, dt), np.zeros(shape, dt)


def band_update(opt, W, s1, s2, grad_rows, f0, f1, lr, momentum, t, dt=np.float64):
    """Update rows [f0, f1) of W / s1 / s2 IN PLACE from the band-local grad_rows (row 0 of grad_rows is row f0 of W)."""
    if f1 == f0:
        return
    g = np.asarray(grad_rows, dt)[:f1 - f0]
    p, a, b = opt_update(opt, W[f0:f1], g, s1[f0:f1], s2[f0:f1], lr, momentum, t, dt)
    W[f0:f1] = p
    if a is not None:
        s1[f0:f1] = a
    if b is not None:
        s2[f0:f1] = b


# ----------------------------------------------------------------------------------------------- #
# packed data-parallel receive buffer: one chunk per rank,
#   [chunk_rows x Hp low-precision rows owned by that rank | that rank's Hp + Fp fp32 bias gradients at bias_off | gap]
# ----------------------------------------------------------------------------------------------- #
UNPACK_CASES = ((256, 128, 1, 256), (384, 128, 2, 192), (384, 192, 3, 128), (640, 128, 4, 192), (256, 64, 8, 64))


def chunk_layout(Fp, Hp, chunk_rows, es, extra=64):
    """(bias_off, chunk_stride) in bytes: the payload rounded up to 16 bytes plus `extra` bytes nobody may read."""
    bias_off = chunk_rows * Hp * es
    payload = bias_off + (Hp + Fp) * 4
    return bias_off, -(-payload // 16) * 16 + extra


def build_recv(rows_bits, bias_grads, world, chunk_rows, extra=64):
    """rows_bits: [Fp x Hp] uint16 / uint32 bit patterns of W_lo; bias_grads: float32 [world x (Hp + Fp)].
    Returns (uint8 buffer, chunk_stride, bias_off).  Every byte that is no real row and no bias gradient -- chunk rows
    beyond Fp, the gap up to chunk_stride -- is NAN_BYTE."""
    rows_bits = np.ascontiguousarray(rows_bits)
    Fp, Hp = rows_bits.shape
    es = rows_bits.dtype.itemsize
    bias_off, stride = chunk_layout(Fp, Hp, chunk_rows, es, extra)
    buf = np.full(world * stride, NAN_BYTE, np.uint8)
    bias_grads = np.ascontiguousarray(bias_grads, np.float32)
    assert bias_grads.shape == (world, Hp + Fp)
    for r in range(world):
        lo, hi = min(r * chunk_rows, Fp), min((r + 1) * chunk_rows, Fp)
        raw = rows_bits[lo:hi].view(np.uint8).reshape(-1)
        buf[r * stride:r * stride + raw.size] = raw
        buf[r * stride + bias_off:r * stride + bias_off + 4 * (Hp + Fp)] = bias_grads[r].view(np.uint8)
    return buf, stride, bias_off


def unpack_recv(buf, world, chunk_rows, stride, bias_off, Fp, Hp, es):
    """The inverse: (W_lo bits [Fp x Hp], per-rank bias gradients [world x (Hp + Fp)], their fp32 sum in rank order)."""
    bt = np.uint16 if es == 2 else np.uint32
    W = np.zeros((Fp, Hp), bt)
    gb = np.zeros((world, Hp + Fp), np.float32)
    for f0 in range(0, Fp, 64):                       # tile by tile, as a rank-local row index
        r = f0 // chunk_rows
        o = r * stride + (f0 - r * chunk_rows) * Hp * es
        W[f0:f0 + 64] = buf[o:o + 64 * Hp * es].view(bt).reshape(64, Hp)
    acc = np.zeros(Hp + Fp, np.float32)
    for r in range(world):
        o = r * stride + bias_off
        gb[r] = buf[o:o + 4 * (Hp + Fp)].view(np.float32)
        acc = (acc + gb[r]).astype(np.float32)
    return W, gb, acc


# ----------------------------------------------------------------------------------------------- #
# epilogues and statistics
# ----------------------------------------------------------------------------------------------- #
def act(name, z):
    z = np.asarray(z)
    if name == "sigmoid":
        return 0.5 * (1.0 + np.tanh(0.5 * z))         # == 1 / (1 + exp(-z)), no overflow
    if name == "tanh":
        return np.tanh(z)
    return z.copy()


def act_grad_from_output(name, a):
    if name == "sigmoid":
        return a * (1.0 - a)
    if name == "tanh":
        return 1.0 - a * a
    return np.ones_like(a)


def dh_finish(slabs, dh_extra, h, bh, B, H, enc_act, dt=np.float64):
    """dh = sum_s slab_s (+ dh_extra); delta1 = dh * act'(h + act(bh)); both zero outside [0,B) x [0,H).
    Returns (delta1 [Bp x Hp], colsum [2 x Bp/32 x Hp]: per-32-row-block column sums of delta1 and of dh)."""
    S, Bp, Hp = slabs.shape
    dh = np.zeros((Bp, Hp), dt)
    for s in range(S):                                # slab order, as the kernel
        dh[:B, :H] += np.asarray(slabs[s, :B, :H], dt)
    if dh_extra is not None:
        dh[:B, :H] += np.asarray(dh_extra[:B, :H], dt)
    a1 = np.asarray(h[:B, :H], dt) + act(enc_act, np.asarray(bh[:H], dt))
    d1 = np.zeros((Bp, Hp), dt)
    d1[:B, :H] = dh[:B, :H] * act_grad_from_output(enc_act, a1)
    colsum = np.stack([d1.reshape(Bp // 32, 32, Hp).sum(1), dh.reshape(Bp // 32, 32, Hp).sum(1)])
    return d1, colsum


def step_stats(ae, triplet, alpha, tri_scalars=None, nvalid=None, loss_part=None, cnt_part=None):
    """The six statistics [COST, AE, TRIPLET, FRACTION, NUM, NVALID] in float64.  `ae` is the weighted reconstruction loss.
    With loss_part / cnt_part (batch_all) the triplet scalars are folded from the miner's partials; otherwise they come
    from tri_scalars[1..3]."""
    ae = float(ae)
    if triplet == "none":
        return np.array([ae, ae, 0.0, 0.0, 0.0, 0.0])
    if loss_part is not None:
        nv = float(nvalid)
        nm = float(np.sum(np.asarray(cnt_part, np.float64)))
        tl = float(np.sum(np.asarray(loss_part, np.float64))) / (nv + 1e-16)
        fr = nm / (nv + 1e-16)
    else:
        tl, fr, nm = (float(v) for v in tri_scalars[1:4])
        nv = float(nvalid) if (triplet == "batch_all" and nvalid is not None) else nm
    return np.array([ae + float(alpha) * tl, ae, tl, fr, nm, nv])
