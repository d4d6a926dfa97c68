"""Per-anchor float64 references of the two triplet miners, for an anchor RANGE of a batch.

The library's `_rows` entry points (include/dae_hip.h: dae_triplet_batch_all_rows / dae_triplet_batch_hard_rows) mine the anchors
[a0, a0 + n) of a batch of B against all B columns: D is [n x ldd], row r belongs to batch element a0 + r.  These helpers compute
the same per-anchor outputs, un-normalised, exactly as the header defines them, from the anchors' D rows and the labels of the
whole batch -- nP * nN work per anchor, nothing B^3.  tests/test_miner_reference_cpu.py pins both to the whole-batch oracle
(oracle/dae_oracle.py) on the CPU; tests/test_hip_miner_rows.py compares the kernels with them.

Every DECISION (the positive-triplet mask and count, batch_hard's selections and ties) is taken in float32 on the given float32 D,
the way the kernels and the oracle take it, so counts, role counts and data weights are integers that compare exactly.  Loss and
gradient VALUES are float64.
"""
import numpy as np

EPS32 = np.float32(1e-16)


def _softplus_sigmoid64(t):
    """softplus(t) = log(1 + e^t) and its derivative sigmoid(t), float64, stable for any t (one exponential for both)."""
    t = np.asarray(t, np.float64)
    e = np.exp(-np.abs(t))                                                  # in (0, 1]
    return np.maximum(t, 0.0) + np.log1p(e), np.where(t >= 0, 1.0, e) / (1.0 + e)


def anchor_sets(labels, a):
    """(positives, negatives) of anchor a in index order: same label and != a; different label."""
    labels = np.asarray(labels)
    same = labels == labels[a]
    neg = np.flatnonzero(~same)
    same[a] = False
    return np.flatnonzero(same), neg


def batch_all_rows_reference(D_rows, labels, a0=0, pos_only=False, want_grad=True):
    """D_rows: float32 [n x >= B] (columns beyond B = len(labels) are ignored).  Returns a dict of per-anchor arrays:
         loss_part f64[n]   sum of softplus(D[a,n] - D[a,p]) over the valid (p, n) -- only the positive triplets if pos_only
         npos_part i64[n]   #{valid (p, n): float32(D[a,n]) - float32(D[a,p]) > float32(1e-16)}
         G         f64[n,B] d loss_part[a] / d D[a,:]  (minus the sigmoid sums at the positives, plus at the negatives; 0 at a)
         role_cnt  i64[n,B] (pos_only, else None) positive triplets of anchor a that column j takes part in
         nvalid_part i64[n] nP * nN
         row_range f32[n]   max - min of D[a, j] over the anchor's positives and negatives (what selects the kernel's sweep)
         nzero_part i64[n]  valid (p, n) with D[a,n] == D[a,p] exactly (column ties: never positive triplets)
       want_grad=False leaves G zero (loss and counts only)."""
    D_rows = np.asarray(D_rows)
    assert D_rows.dtype == np.float32
    labels = np.asarray(labels)
    B, n = labels.shape[0], D_rows.shape[0]
    assert 0 <= a0 and a0 + n <= B and D_rows.shape[1] >= B
    out = dict(loss_part=np.zeros(n), npos_part=np.zeros(n, np.int64), G=np.zeros((n, B)),
               role_cnt=np.zeros((n, B), np.int64) if pos_only else None, nvalid_part=np.zeros(n, np.int64),
               row_range=np.zeros(n, np.float32), nzero_part=np.zeros(n, np.int64))
    for r in range(n):
        a = a0 + r
        P, N = anchor_sets(labels, a)
        d = D_rows[r, :B]
        out["nvalid_part"][r] = len(P) * len(N)
        both = np.concatenate([d[P], d[N]])
        out["row_range"][r] = (both.max() - both.min()) if both.size else np.float32(0)
        if len(P) == 0 or len(N) == 0:
            continue
        pos = (d[N][None, :] - d[P][:, None]) > EPS32                       # float32 arithmetic: the decision
        T = d[N].astype(np.float64)[None, :] - d[P].astype(np.float64)[:, None]
        mask = pos if pos_only else np.ones_like(pos)
        out["npos_part"][r] = int(pos.sum())
        out["nzero_part"][r] = int((T == 0).sum())
        sp, sg = _softplus_sigmoid64(T)
        out["loss_part"][r] = float(np.sum(np.where(mask, sp, 0.0)))
        if want_grad:
            sg = np.where(mask, sg, 0.0)
            out["G"][r, P] = -sg.sum(axis=1)
            out["G"][r, N] = sg.sum(axis=0)
        if pos_only:
            out["role_cnt"][r, P] = pos.sum(axis=1)
            out["role_cnt"][r, N] = pos.sum(axis=0)
    return out


def batch_hard_rows_reference(D_rows, labels, a0=0):
    """D_rows: float32 [n x >= B].  triplet_loss_utils.py:202-259 restated for the anchors [a0, a0 + n), un-normalised:
         loss_part f64[n]   softplus(dist_a) * cnt_a,  dist_a = max(hn_a - hp_a, 0)
         cnt_part  i64[n]   dist_a > 0
         G         f64[n,B] d loss_part[a] / d D[a,:]: ties of the hardest negative / positive / row maximum split equally, and the
                            shift of the invalid positives by the row maximum carries its gradient to the row maximum
         dw        i64[B]   THESE anchors' contribution: cnt_a * ([D[a,j] == hp_a] + [D[a,j] == hn_a] + [j == a])
       The quirks are the reference's: invalid negatives enter the maximum as 0, invalid positives as D + rowmax."""
    D_rows = np.asarray(D_rows)
    assert D_rows.dtype == np.float32
    labels = np.asarray(labels)
    B, n = labels.shape[0], D_rows.shape[0]
    assert 0 <= a0 and a0 + n <= B and D_rows.shape[1] >= B
    one = np.float32(1.0)
    out = dict(loss_part=np.zeros(n), cnt_part=np.zeros(n, np.int64), G=np.zeros((n, B)), dw=np.zeros(B, np.int64))
    for r in range(n):
        a = a0 + r
        d = D_rows[r, :B]
        ap = (labels == labels[a]); ap[a] = False
        an = labels != labels[a]
        apf, anf = ap.astype(np.float32), an.astype(np.float32)
        rowmax = d.max()
        apd = d + rowmax * (one - apf)                                      # float32
        hp = apd.min()
        and_ = anf * d
        hn = and_.max()
        if not (hn - hp > np.float32(0)):                                   # dist = max(hn - hp, 0); cnt = dist > 0
            continue
        dist = float(hn) - float(hp)
        out["cnt_part"][r] = 1
        out["loss_part"][r], gd = (float(v) for v in _softplus_sigmoid64(dist))
        out["dw"] += (d == hp).astype(np.int64) + (d == hn).astype(np.int64)
        out["dw"][a] += 1
        ind_n = (and_ == hn).astype(np.float64)
        g = an * gd * ind_n / ind_n.sum()
        ind_p = (apd == hp).astype(np.float64)
        d_apd = -gd * ind_p / ind_p.sum()
        g += d_apd
        ind_m = (d == rowmax).astype(np.float64)
        g += np.sum(d_apd * (1.0 - apf)) * ind_m / ind_m.sum()
        out["G"][r] = g
    return out
