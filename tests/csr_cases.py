"""Long-row CSR cases and a per-row float64 reference of the fused corrupt + gather + encode kernel (csrc/dae_gather.hip:
encode_csr_kernel) and of the side images it writes.

The kernel's row walk changes with the number of STORED entries of a row: a lane owns four entries of a 256-entry pass (64 lanes
each), rows beyond 256 entries take further passes that reuse the per-wave kept-entry list, the list is walked in trips of 72 (bf16
shadow, 64-column fp32 slice) or 36 (128-column fp32 slice) kept entries with a masked last trip, and the step tail un-scatters the
same rows 256 entries per round.  `long_row_csr` builds one small matrix that holds every such boundary, with keep masks that hit
the extremes, and `encode_csr_reference` restates the operation row by row in float64.

The inputs sit on dyadic grids, so that EVERY fp32 evaluation order gives the same bits as float64 (`exact_sum_bits`): the kernels are
compared bit for bit, not within a tolerance.  tests/test_csr_cases_cpu.py pins the builder and the reference on the CPU;
tests/test_hip_encode_csr.py and tests/test_hip_step.py use them on the device.
"""
import numpy as np
from scipy import sparse

PASS = 256                      # stored entries per pass of the kernel's entry loop (and per round of the step tail's clear)
LENGTHS = (0, 1, 63, 64, 65, 72, 73, 144, 145, 255, 256, 257, 288, 512, 513, 700)
PAD = 128

# (stored length, mask).  Masks: "all", "none", "last" (only the last stored entry), "pass1" (only indices < 256), "pass2" (only
# indices >= 256), "rand70" (each entry kept with probability 0.7), or a tuple of kept counts per pass (random positions).
# The first eight rows are one 8-row workgroup at i0 = 0: an empty row, a 700-entry row and a 1-entry row share it.
ROWS = (
    (0, "all"), (700, "rand70"), (1, "all"), (257, "last"), (513, "pass2"), (513, "pass1"), (256, "all"), (700, "none"),
    (63, "all"), (64, "all"), (65, "all"), (72, "all"), (73, "all"), (144, "all"), (145, "all"), (255, "all"),
    (257, "all"), (288, "all"), (512, "all"), (513, "all"), (700, "all"), (144, (36,)), (145, (37,)), (255, (72,)),
    (256, (73,)), (700, (256, 73, 37)), (513, (36, 256, 1)), (288, "pass2"), (700, "pass2"), (700, "pass1"), (700, "last"), (257, "none"),
    (700, "rand70"), (0, "rand70"), (513, "rand70"), (1, "rand70"), (512, "rand70"), (63, "rand70"), (288, "rand70"), (64, "rand70"),
    (257, "rand70"), (65, "rand70"), (256, "rand70"), (72, "rand70"), (255, "rand70"), (73, "rand70"), (145, "rand70"), (144, "rand70"),
    (0, "all"), (1, "none"), (64, "last"), (65, "last"), (513, "last"), (257, "pass1"), (72, (36,)), (73, (37,)),
    (512, (72, 73)), (1, "last"), (288, (256, 0)), (513, "none"),
)
# rows that get three stored columns in [F, Fp) when pad_cols is asked for (their masks do not depend on the last entries)
PAD_COL_ROWS = (1, 4, 20, 32)


def pad(n):
    return (int(n) + PAD - 1) // PAD * PAD


def _mask(rng, n, kind):
    k = np.zeros(n, bool)
    idx = np.arange(n)
    if kind == "all":
        k[:] = True
    elif kind == "none":
        pass
    elif kind == "last":
        k[n - 1:] = True
    elif kind == "pass1":
        k[idx < PASS] = True
    elif kind == "pass2":
        k[idx >= PASS] = True
    elif kind == "rand70":
        k = rng.random(n) < 0.7
    else:
        for p, cnt in enumerate(kind):
            lo, hi = p * PASS, min(n, (p + 1) * PASS)
            k[rng.choice(np.arange(lo, hi), size=cnt, replace=False)] = True
    return k


def long_row_csr(rng, F, valued, pad_cols=False):
    """(m, keep): a sorted CSR matrix [len(ROWS) x F] (float32; values multiples of 2^-4 in (0, 1], or all ones) whose rows have the stored
    lengths and keep masks of ROWS, and the per-entry keep mask (bool[nnz], CSR entry order).  pad_cols: the rows PAD_COL_ROWS end in
    three stored columns in [F, Fp) and the matrix is [.. x Fp] -- entries every kernel has to ignore."""
    Fp = pad(F)
    assert F >= max(LENGTHS) and (not pad_cols or Fp - F >= 3)
    indptr, indices, keep = [0], [], []
    for r, (n, kind) in enumerate(ROWS):
        cols = np.sort(rng.choice(F, size=n, replace=False))
        if pad_cols and r in PAD_COL_ROWS:
            cols[-3:] = (F, (F + Fp) // 2, Fp - 1)
        indices.append(cols)
        keep.append(_mask(rng, n, kind))
        indptr.append(indptr[-1] + n)
    indices = np.concatenate(indices).astype(np.int32)
    keep = np.concatenate(keep)
    nnz = len(indices)
    data = (rng.integers(1, 17, nnz) / 16.0).astype(np.float32) if valued else np.ones(nnz, np.float32)
    m = sparse.csr_matrix((data, indices, np.asarray(indptr, np.int64)), shape=(len(ROWS), Fp if pad_cols else F))
    assert m.has_sorted_indices
    return m, keep


def kept_per_pass(m, keep):
    """Per row: (stored length, tuple of kept counts per 256-entry pass)."""
    out = []
    for r in range(m.shape[0]):
        s, e = int(m.indptr[r]), int(m.indptr[r + 1])
        k = keep[s:e]
        out.append((e - s, tuple(int(k[p:p + PASS].sum()) for p in range(0, e - s, PASS))))
    return out


def keep_words(keep):
    """The keep mask as the library's bit stream: bit e of the little-endian uint32 words (viewed as int32 for torch)."""
    bits = np.packbits(np.asarray(keep, bool), bitorder="little")
    return np.concatenate([bits, np.zeros((-len(bits)) % 4, np.uint8)]).view(np.int32)


def grid_params(rng, F, H, w_bits=8, w_max=0.25):
    """(W [F x H], b_h [H]) float32 on dyadic grids: W multiples of 2^-w_bits in [-w_max, w_max] (w_bits = 8, w_max = 0.25: exact in
    bf16 and fp16; w_bits = 12, w_max = 0.125: NOT exact in bf16 -- the fp32-master legs), b_h multiples of 2^-13 in [-0.5, 0.5]."""
    q = int(round(w_max * 2 ** w_bits))
    W = (rng.integers(-q, q + 1, (F, H)) / 2.0 ** w_bits).astype(np.float32)
    bh = (rng.integers(-2 ** 12, 2 ** 12 + 1, H) / 2.0 ** 13).astype(np.float32)
    return W, bh


def exact_sum_bits(n, w_bits, w_max, v_bits=4, scale_bits=1, b_bits=13, b_max=0.5):
    """Significand bits that hold every partial sum of up to n products (scale * v) * W plus the bias: v a multiple of 2^-v_bits in
    (0, 1], scale a multiple of 2^-scale_bits in (0, 1], W a multiple of 2^-w_bits with |W| <= w_max, b a multiple of 2^-b_bits with
    |b| <= b_max.  Every such number is a multiple of 2^-frac with frac = max(v_bits + scale_bits + w_bits, b_bits) and smaller in
    magnitude than n * w_max + b_max: (bits of that range) + frac.  <= 24 means fp32 holds them all, so every summation order and
    every fused multiply-add returns the exact value."""
    frac = max(v_bits + scale_bits + w_bits, b_bits)
    top = n * w_max + b_max
    return int(np.ceil(np.log2(top))) + frac


def encode_csr_reference(m, keep, row_idx, F, W, bh, scale, act, oracle_act):
    """Per-row float64 restatement of dae_encode_csr for the batch rows row_idx of the CSR matrix m (stored columns >= F are ignored,
    as the kernel ignores them).  W [F x H], bh [H].  Returns float64 / integer arrays over the UNPADDED extents:
         z      [B x H]      sum over the kept entries of (scale * v) * W[col, :]   (no bias)
         h      [B x H]      act(z + b_h) - act(b_h)
         x_bits [B x Fp/32]  uint32 bit image of the CLEAN rows (bit b of word w <=> column 32 w + b stored)
         xc     [B x F]      x~ = scale * v at the kept entries, 0 elsewhere
         rowsq  [B]          sum of v^2 over the clean row (dropped entries included)
    oracle_act(name, z) is the activation (oracle.act)."""
    W = np.asarray(W, np.float64); bh = np.asarray(bh, np.float64)
    B, H, Fp = len(row_idx), W.shape[1], pad(F)
    z = np.zeros((B, H)); xc = np.zeros((B, F)); rowsq = np.zeros(B)
    x_bits = np.zeros((B, Fp // 32), np.uint32)
    for i, r in enumerate(np.asarray(row_idx)):
        s, e = int(m.indptr[r]), int(m.indptr[r + 1])
        for k in range(s, e):
            c = int(m.indices[k])
            if c >= F:
                continue
            v = float(m.data[k])
            rowsq[i] += v * v
            x_bits[i, c >> 5] |= np.uint32(1 << (c & 31))
            if keep[k]:
                w = float(scale) * v
                xc[i, c] = w
                z[i] += w * W[c]
    h = oracle_act(act, z + bh) - oracle_act(act, bh)
    return dict(z=z, h=h, x_bits=x_bits, xc=xc, rowsq=rowsq)
