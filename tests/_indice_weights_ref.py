"""The per-sample-weight gradient of the pooled TBE lookup (include/tbe_hip.h `tbe_backward_indice_weights_*`) in
float64, plus inputs for which every FP32 summation order gives exactly that value.  numpy only.

Designed values: table entries k/8 with k in [-8, 8] (exact in FP16 too), integer output gradients in [-4, 4],
per-sample weights in {0.5, 1, 2}, D <= 256.  Every product is a multiple of 1/8 of magnitude <= 4 and a dot has at most
256 of them, so each partial sum is a multiple of 1/8 below 2^10: 13 significant bits, exact in FP32 in any order, with
or without fma (up to the largest dim the kernels take, 2048, it is 2^13 and 16 bits: still exact).  A GPU result on these inputs is therefore compared with the float64 value BIT FOR BIT.  MEAN divides
the exact dot by the bag length once; an FP32 division of two FP32 values rounded correctly equals the float64
quotient rounded to FP32 (53 >= 2 * 24 + 2 bits: the double rounding is innocuous), so that comparison is exact as well.
tests/test_indice_weights_grad.py guards the premise on the CPU.
"""
import numpy as np

SUM, MEAN, NONE = 0, 1, 2  # TBE_POOL_*
ID_SKIP = np.iinfo(np.int64).min  # TBE_ID_SKIP


class Case:
    """One batch: per-TABLE weights (any float dtype), feature -> table map, ids, complete offsets [F*B+1], the pooled
    output gradient [B, stride] and where each feature's block starts in a gradient row."""

    def __init__(self, tables, ftm, B, indices, offsets, grad, out_offset=None):
        self.tables, self.ftm, self.B = tables, list(ftm), int(B)
        self.F = len(self.ftm)
        self.feat_D = [int(tables[t].shape[1]) for t in self.ftm]
        self.feat_rows = [int(tables[t].shape[0]) for t in self.ftm]
        self.indices = np.asarray(indices, dtype=np.int64)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.grad = np.asarray(grad, dtype=np.float32)
        self.N = int(self.indices.size)
        if out_offset is None:
            out_offset = np.concatenate([[0], np.cumsum(self.feat_D)[:-1]])
        self.out_offset = np.asarray(out_offset, dtype=np.int64)
        for a in (self.indices, self.offsets, self.grad, self.out_offset):
            a.setflags(write=False)


def reference(case, pooling=SUM, feat_pooling=None, feat_requires_grad=None, feat_window=None, tables=None):
    """giw[N] in float64, by the contract of include/tbe_hip.h: position by position, no vectorised shortcuts.
    feat_window: [(first global row, global rows)] per feature or None.  tables: override of case.tables."""
    tables = case.tables if tables is None else tables
    out = np.zeros(case.N, dtype=np.float64)
    g64 = case.grad.astype(np.float64)
    for f in range(case.F):
        if feat_requires_grad is not None and not feat_requires_grad[f]:
            continue
        W = tables[case.ftm[f]].astype(np.float64)
        D, rows = case.feat_D[f], case.feat_rows[f]
        lo = 0 if feat_window is None else int(feat_window[f][0])
        mean = pooling == MEAN and (feat_pooling is None or feat_pooling[f] == MEAN)
        c0 = int(case.out_offset[f])
        for b in range(case.B):
            s, e = int(case.offsets[f * case.B + b]), int(case.offsets[f * case.B + b + 1])
            if s < 0 or e > case.N or s > e:
                continue  # malformed: its positions keep 0
            for i in range(s, e):
                local = int(case.indices[i]) - lo
                if int(case.indices[i]) == ID_SKIP or not 0 <= local < rows:
                    continue
                dot = float(np.dot(g64[b, c0:c0 + D], W[local]))
                out[i] = dot / (e - s) if mean else dot
    return out


def abs_dot(case, tables=None):
    """sum_d |g_d * w_d| per position in float64 (0 where the reference is 0 by contract): the scale of the dot-product
    error bound.  SUM pooling, no window."""
    absolute = Case([np.abs(t.astype(np.float64)) for t in (case.tables if tables is None else tables)], case.ftm, case.B,
                    case.indices, case.offsets, np.abs(case.grad), case.out_offset)
    return reference(absolute)


def designed_table(rng, rows, D, dtype=np.float32):
    return (rng.integers(-8, 9, size=(rows, D)) / 8.0).astype(dtype)


def designed_grad(rng, B, stride):
    return rng.integers(-4, 5, size=(B, stride)).astype(np.float32)


def designed_weights(rng, N):
    return rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), size=N)


def short_lengths(rng, F, B):
    """Bag lengths from {0, 1, 2, 4}: average 1.75, the short-bag kernel."""
    return rng.choice(np.array([0, 1, 2, 4], dtype=np.int64), size=F * B)


def long_lengths(rng, F, B, total=3000):
    """Per feature one bag of 1000 and one of 100 ids next to empty ones, the rest from {0, 1, 2, 4}, topped up so that the
    batch averages >= 4 ids per bag (the wave-per-bag kernel) at about `total` ids."""
    lengths = np.zeros((F, B), dtype=np.int64)
    for f in range(F):
        if f % 2 == 0 or F == 1:
            big = rng.choice(B, size=min(2, B), replace=False)
            lengths[f, big[0]] = 1000 if f == 0 else 100
            if B > 1:
                lengths[f, big[1]] = 100
        free = np.nonzero(lengths[f] == 0)[0]
        free = free[rng.random(free.size) < 0.5]  # half of the others stay empty
        lengths[f, free] = rng.choice(np.array([1, 2, 4], dtype=np.int64), size=free.size)
    short = max(0, max(total, 4 * F * B) - int(lengths.sum()))
    lengths[F - 1, B - 1] += short
    return lengths.reshape(-1)


def make_case(dims, rows, ftm=None, B=67, bags="short", seed=0, dtype=np.float32, designed=True, bad_ids=False):
    """Tables of `dims` x `rows`, features `ftm`; designed (exact) or standard-normal values.  bad_ids: sprinkles -1,
    `rows` and TBE_ID_SKIP over the ids."""
    ftm = list(range(len(dims))) if ftm is None else list(ftm)
    rng = np.random.default_rng([seed, len(ftm), B, sum(dims)])
    if designed:
        tables = [designed_table(rng, r, d, dtype) for r, d in zip(rows, dims)]
    else:
        tables = [rng.standard_normal((r, d)).astype(dtype) for r, d in zip(rows, dims)]
    F = len(ftm)
    lengths = short_lengths(rng, F, B) if bags == "short" else long_lengths(rng, F, B)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    per_feature = offsets[::B]
    ids = [rng.integers(0, rows[ftm[f]], size=int(per_feature[f + 1] - per_feature[f])) for f in range(F)]
    if bad_ids:
        for f in range(F):
            n = ids[f].size
            if n == 0:
                continue
            pick = rng.choice(n, size=min(n, 9), replace=False)
            ids[f][pick] = np.resize(np.array([-1, rows[ftm[f]], ID_SKIP], dtype=np.int64), pick.size)
    stride = sum(dims[t] for t in ftm)
    grad = designed_grad(rng, B, stride) if designed else rng.standard_normal((B, stride)).astype(np.float32)
    return Case(tables, ftm, B, np.concatenate(ids).astype(np.int64), offsets, grad)
