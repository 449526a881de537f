"""The TBE forward driven straight through the C ABI (include/tbe_hip.h), plus inputs designed around its dispatch.

Two halves, as in tests/_bwd_abi.py:

* numpy only: table values that are multiples of 1/8 in [-4, 4] (exact in FP16 too), per-sample weights in {0.5, 1, 2} and
  bags of at most 300 ids, so every term is a multiple of 1/16 and |sum| * 16 <= 38 400, far below 2^24: the FP32 oracle
  (sequential fmaf, MEAN as `* (1.f / len)`) and a kernel that sums in any association give the same bits, and a dropped,
  doubled or misattributed row moves a sum by >= 1/16.  `dispatch` restates the host's choices of
  csrc/tbe_forward_impl.hpp (bags per wave, long or short kernel, (G, NV), `vec` per feature); it is used ONLY to name the
  path in a failure message and to assert that a case list reaches a path.  No expected value depends on it.  `expected`
  builds the oracle's answer, `verify` is the one comparison the GPU tests use, `standin_forward` is a numpy forward that
  can carry an injected fault: tests/test_forward_inputs.py (CPU) shows that `verify` rejects each of them.
* `ForwardCase` lays the tables in one flat device buffer between guard bytes (each table can be pushed off its grid), puts
  `out` [B, out_row_stride] inside guards of its own, prefilled with a NaN canary, and calls `tbe_forward_pooled_*` or
  `tbe_forward_nobag_*` with an explicit max_D.
"""
import functools

import numpy as np

import _paths  # noqa: F401
from oracle import oracle

SUM, MEAN = oracle.POOL_SUM, oracle.POOL_MEAN
ID_SKIP = -(1 << 63)  # TBE_ID_SKIP
# (largest max_D, lanes per row group G, 16-B column slots per lane NV) of launch_fwd / TBE_N
CLASSES = [(64, 16, 1), (128, 32, 1), (256, 64, 1), (512, 64, 2), (1024, 64, 4), (2048, 64, 8)]
CLASS_LOWER = [0, 64, 128, 256, 512, 1024]  # the class of max_D is (lower, upper]
U = 4  # bags (short kernel) / rows (long kernel) in flight per group
BPW64_BAGS = 1 << 19  # F * B from which a wave owns 64 bags
LONG_AVG = 3.5  # average bag length from which the wave-per-bag kernel runs
NOBAG_GRID_CAP = 4096
LONG_LENGTHS = [0, 1, 5, 17, 63, 64, 65, 127, 128, 129, 200]
_LONG_FIRST = [64, 65, 200, 0, 128, 63, 129, 1, 127, 17, 5]  # the order they are handed out in when B < 11
MAX_BAG = 300
CANARY_BITS = 0x7FC0BEEF  # a quiet NaN no arithmetic produces
GUARD_BYTE = 0xC3
GUARD_BYTES = 256


# ---- dispatch, restated --------------------------------------------------------------------------------------------
def class_of(max_D):
    for top, G, NV in CLASSES:
        if max_D <= top:
            return G, NV
    raise ValueError(max_D)


class Dispatch:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def key(self, f):
        return (self.kernel, self.G, self.NV, self.bags_per_wave, self.vec[f])

    def path(self, f=None):
        s = f"{self.kernel} kernel, G={self.G} NV={self.NV}, {self.bags_per_wave} bags per wave"
        if f is not None:
            s += f", feature {f} ({'vec' if self.vec[f] else 'scalar'})"
        return s


def _table_grid(dtype):
    return 16 if np.dtype(dtype) == np.float32 else 8


def dispatch(F, B, N, max_D, feat_D, out_row_stride, dtype="float32", table_off=None, out_off=0):
    """What forward_pooled launches.  table_off: bytes each feature's table base lies past a 16-B boundary."""
    G, NV = class_of(max_D)
    table_off = table_off if table_off is not None else [0] * F
    doff = np.concatenate([[0], np.cumsum(feat_D)[:-1]]).astype(np.int64)
    vec = tuple(bool(feat_D[f] % 4 == 0 and doff[f] % 4 == 0 and out_row_stride % 4 == 0 and
                     table_off[f] % _table_grid(dtype) == 0 and out_off % 16 == 0) for f in range(F))
    return Dispatch(kernel="long" if N / (F * B) >= LONG_AVG else "short", G=G, NV=NV,
                    bags_per_wave=64 if F * B >= BPW64_BAGS else 16, vec=vec)


def dispatch_nobag(F, N, D, dtype="float32", table_off=None, out_off=0):
    G, NV = class_of(D)
    table_off = table_off if table_off is not None else [0] * F
    per_block = 16 * (64 // G)
    grid = min((N + per_block - 1) // per_block, NOBAG_GRID_CAP)
    vec = tuple(bool(D % 4 == 0 and out_off % 16 == 0 and table_off[f] % _table_grid(dtype) == 0) for f in range(F))
    return Dispatch(kernel="nobag", G=G, NV=NV, bags_per_wave=0, vec=vec, per_block=per_block, grid=grid,
                    trips=(N + grid * per_block - 1) // (grid * per_block))


def quad_mates(B, bags_per_wave, G):
    """[4, B]: the bags the short kernel holds in flight together with bag b (-1: a slot past B or past the wave's bags)."""
    NG = 64 // G
    b = np.arange(B)
    local = b % bags_per_wave
    p = local // (NG * U) * (NG * U)
    slot = p[None, :] + np.arange(U)[:, None] * NG + (local % NG)[None, :]
    mates = (b - local)[None, :] + slot
    return np.where((slot < bags_per_wave) & (mates < B), mates, -1)


# ---- designed inputs -----------------------------------------------------------------------------------------------
class Batch:
    """indices / offsets / psw of one call.  Arrays are read-only: tests share them."""

    def __init__(self, F, B, indices, offsets, psw):
        self.F, self.B, self.N = int(F), int(B), int(indices.size)
        self.indices, self.offsets, self.psw = indices, offsets, psw
        for a in (indices, offsets, psw):
            if a is not None:
                a.setflags(write=False)
        self._dev = None


def make_tables(rows, dims, seed=0):
    """One FP32 table per feature, multiples of 1/8 in [-4, 4]."""
    rng = np.random.default_rng([seed, len(rows), int(sum(dims))])
    out = [(rng.integers(-32, 33, size=(r, d)) / 8).astype(np.float32) for r, d in zip(rows, dims)]
    for t in out:
        t.setflags(write=False)
    return out


def long_lengths(rng, F, B):
    """[F, B] from LONG_LENGTHS, each at least once per feature (B >= 11; a smaller B hands them out in turn over the
    features, the chunk edges first); the average is >= 3.5, so the wave-per-bag kernel runs."""
    out = np.empty((F, B), dtype=np.int64)
    for f in range(F):
        if B >= len(LONG_LENGTHS):
            v = np.concatenate([LONG_LENGTHS, rng.choice(LONG_LENGTHS, size=B - len(LONG_LENGTHS))])
            out[f] = rng.permutation(v)
        else:
            out[f] = [_LONG_FIRST[(f * B + i) % len(_LONG_FIRST)] for i in range(B)]
    assert out.mean() >= LONG_AVG
    return out


def short_lengths(rng, F, B):
    """[F, B] from {0, 1, 2, 3} in equal shares: average 1.5, the short kernel."""
    out = rng.permutation(np.arange(F * B, dtype=np.int64) % 4).reshape(F, B)
    assert F * B < 4 or out.mean() < LONG_AVG
    return out


def skewed_lengths(F, B):
    """[F, B]: at least 90 % empty bags; in every 8th block of 16 bags, bag 5 holds 200, 64 or 65 ids, and in every 16th
    block bags 7 and 9 hold one of the other two lengths.  Whatever G is, the 4 bags in flight with bag 5 (stride 1, 2 or 4
    inside the block: 4..7, 1 3 5 7 or 1 5 9 13) are empty or — bag 7 at G = 64 and 32, bag 9 at G = 16 — of another
    length: the `i < maxlen` loop walks very unequal `len[u]`.  The average stays below 3.5."""
    b = np.arange(B)
    block, pos = b // 16, b % 16
    row = np.zeros(B, dtype=np.int64)
    at5 = (pos == 5) & (block % 8 == 0)
    row[at5] = np.array([200, 64, 65])[(block[at5] // 8) % 3]
    for where, lens in ((7, [64, 65, 200]), (9, [65, 200, 64])):
        at = (pos == where) & (block % 16 == 0)
        row[at] = np.array(lens)[(block[at] // 16) % 3]
    out = np.tile(row, (F, 1))
    assert (out == 0).mean() >= 0.9 and out.mean() < LONG_AVG
    return out


def make_batch(rng, lengths, rows, weighted, ids="plain", windows=None):
    """Ids for bags of `lengths` [F, B].  ids: "plain" (all in range), "bad" (a tenth out of range) or "window" (global
    ids for `windows` [(first, global rows)]: local, foreign, TBE_ID_SKIP and bad ones)."""
    F, B = lengths.shape
    assert lengths.max() <= MAX_BAG
    vals = []
    for f in range(F):
        n = int(lengths[f].sum())
        v = rng.integers(0, rows[f], size=n).astype(np.int64)
        kind = rng.random(n)
        if ids == "bad":
            v = np.where(kind < 0.1, rng.choice(np.array([-1, rows[f], rows[f] + 3, -(1 << 40)]), size=n), v)
        elif ids == "window":
            first, glob = windows[f]
            assert first >= 1 and first + rows[f] < glob
            foreign = np.where(rng.random(n) < 0.5, rng.integers(0, first, size=n), rng.integers(first + rows[f], glob, size=n))
            bad = rng.choice(np.array([-1, glob, glob + 5, -7, 1 << 40]), size=n)
            v = np.where(kind < 0.6, v + first, np.where(kind < 0.85, foreign, np.where(kind < 0.9, ID_SKIP, bad)))
        else:
            assert ids == "plain"
        vals.append(v.astype(np.int64))
    indices = np.concatenate(vals) if vals else np.zeros(0, np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
    psw = rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), size=indices.size) if weighted else None
    return Batch(F, B, indices, offsets, psw)


def with_malformed_offsets(batch, where):
    """The batch with offsets[k] replaced, for k in `where`: even positions of the list get N + 5, odd ones -3.  Either makes
    BOTH bags that meet at k malformed (bag k-1 ends past N resp. goes backwards, bag k goes backwards resp. starts
    negative) and leaves every other bag as it was, so no two good bags overlap.  k = 0 (start negative) and k = F * B
    (end past N) touch one bag each."""
    off = batch.offsets.copy()
    for n, k in enumerate(where):
        off[k] = -3 if (n % 2 or k == 0) and k != batch.F * batch.B else batch.N + 5
    return Batch(batch.F, batch.B, batch.indices, off, batch.psw)


# ---- expectation ---------------------------------------------------------------------------------------------------
class Sanitized:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def sanitize(tables, batch, feat_window=None):
    """What the kernels are documented to see: malformed bags emptied (counted once each); with a window, ids made local
    (id - first), foreign ids and TBE_ID_SKIP turned into an id that contributes nothing (-1: the bag keeps its length,
    which MEAN divides by), bad ids counted."""
    F, B, N = batch.F, batch.B, batch.N
    s, e = batch.offsets[:-1], batch.offsets[1:]
    malformed = (s < 0) | (e > N) | (s > e)
    lens = np.where(malformed, 0, e - s).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos = np.repeat(np.where(malformed, 0, s), lens) + (np.arange(offs[-1]) - np.repeat(offs[:-1], lens))
    idx = batch.indices[pos]
    psw = None if batch.psw is None else np.ascontiguousarray(batch.psw[pos])
    feat = np.repeat(np.arange(F * B) // B, lens)
    rows = np.array([t.shape[0] for t in tables], dtype=np.int64)[feat]
    if feat_window is None:
        local = idx
        is_local = (idx >= 0) & (idx < rows)
        foreign = np.zeros(idx.size, dtype=bool)
    else:
        win = np.asarray(feat_window, dtype=np.int64).reshape(F, 2)
        local = idx - win[feat, 0]
        is_local = (idx >= win[feat, 0]) & (local < rows)
        foreign = ~is_local & ((idx == ID_SKIP) | ((idx >= 0) & (idx < win[feat, 1])))
    return Sanitized(idx=np.where(is_local, local, -1).astype(np.int64), offs=offs, psw=psw, lens=lens,
                     n_bad=int((~is_local & ~foreign).sum()), n_foreign=int(foreign.sum()), n_malformed=int(malformed.sum()))


class Expected:
    def __init__(self, out, errors):
        self.out, self.errors = out, int(errors)
        out.setflags(write=False)


def _oracle_tables(tables):
    tabs = oracle.Tables([t.shape[0] for t in tables], [t.shape[1] for t in tables])
    tabs.weights = [np.ascontiguousarray(t, dtype=np.float32) for t in tables]
    return tabs


def oracle_pooled(tables, idx, offs, psw, pooling, feat_pooling=None):
    """oracle.tbe_forward; with feat_pooling the features run per pooling type and are spliced by column block (as
    tests/_util.oracle_forward_mixed does)."""
    tabs = _oracle_tables(tables)
    if pooling == MEAN and feat_pooling is not None:
        out_s, _ = oracle.tbe_forward(tabs, idx, offs, psw, SUM)
        out_m, _ = oracle.tbe_forward(tabs, idx, offs, psw, MEAN)
        cols = np.repeat(np.asarray(feat_pooling) == MEAN, tabs.feat_D)
        return np.where(cols[None, :], out_m, out_s)
    return oracle.tbe_forward(tabs, idx, offs, psw, pooling)[0]


def expected(tables, batch, pooling, feat_pooling=None, feat_window=None):
    """The oracle on the FP32 tables (for FP16 tables: the up-cast ones, which hold the same values) + the exact error
    count: bad ids plus malformed bags."""
    san = sanitize(tables, batch, feat_window)
    return Expected(oracle_pooled(tables, san.idx, san.offs, san.psw, pooling, feat_pooling), san.n_bad + san.n_malformed)


def expected_nobag(tables, batch):
    out, bad = oracle.tbe_forward(_oracle_tables(tables), batch.indices, batch.offsets, None, oracle.POOL_NONE)
    return Expected(out, bad)


def pooled_f64(tables, idx, offs, psw, F, B, mean, mean_len=None):
    """Every bag summed in float64 (prefix sums: all of them are multiples of 1/16 far below 2^53) and rounded ONCE to
    FP32; MEAN features then multiply by the FP32 reciprocal of `mean_len` (the bag's own length unless given)."""
    lens = np.diff(offs)
    mean_len = lens if mean_len is None else mean_len
    scale = np.where(mean_len > 0, np.float32(1) / np.maximum(mean_len, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    blocks = []
    for f in range(F):
        W = tables[f].astype(np.float64)
        lo, hi = int(offs[f * B]), int(offs[(f + 1) * B])
        ids = idx[lo:hi]
        ok = (ids >= 0) & (ids < W.shape[0])
        w = (np.ones(ids.size) if psw is None else psw[lo:hi].astype(np.float64)) * ok
        start, end = offs[f * B:(f + 1) * B] - lo, offs[f * B + 1:(f + 1) * B + 1] - lo
        blk = np.empty((B, W.shape[1]), dtype=np.float32)
        for c in range(0, W.shape[1], 256):
            cs = np.zeros((ids.size + 1, min(256, W.shape[1] - c)))
            np.cumsum(W[np.where(ok, ids, 0), c:c + 256] * w[:, None], axis=0, out=cs[1:])
            blk[:, c:c + 256] = (cs[end] - cs[start] + 0.0).astype(np.float32)  # + 0.0: a sum that starts at +0.0 is never -0.0
        if mean[f]:
            blk *= scale[f * B:(f + 1) * B, None]
        blocks.append(blk)
    return np.concatenate(blocks, axis=1)


def mean_flags(F, pooling, feat_pooling):
    return [pooling == MEAN and (feat_pooling is None or feat_pooling[f] == MEAN) for f in range(F)]


def reversed_bags(san):
    """The sanitized ids (and weights) with every bag's order reversed."""
    n = san.idx.size
    start = np.repeat(san.offs[:-1], san.lens)
    perm = start + (np.repeat(san.lens, san.lens) - 1 - (np.arange(n) - start))
    return san.idx[perm], None if san.psw is None else np.ascontiguousarray(san.psw[perm])


# ---- the comparison ------------------------------------------------------------------------------------------------
class Result:
    """out: the raw [B, out_row_stride] block (gap columns included); pooled: its first sum D columns."""

    def __init__(self, out, errors, outer_ok=True, tables_ok=True, sum_D=None):
        self.out, self.errors = out, int(errors)
        self.sum_D = out.shape[1] if sum_D is None else int(sum_D)
        self.outer_ok, self.tables_ok = bool(outer_ok), bool(tables_ok)
        self.gap_ok = bool((bits(out[:, self.sum_D:]) == CANARY_BITS).all())
        self.guards_ok = self.outer_ok and self.tables_ok and self.gap_ok

    @property
    def written(self):
        return self.out[:, :self.sum_D]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def canary_block(B, stride):
    return np.full((B, stride), CANARY_BITS, dtype=np.uint32).view(np.float32)


def verify(res, exp, disp, feat_D, what=""):
    """THE comparison: bits of every written element (so an empty bag must read +0.0, never the canary), the gap columns,
    the guards, the tables, the exact error count.  A failure names the dispatch path of the first wrong element."""
    doff = np.concatenate([[0], np.cumsum(feat_D)]).astype(np.int64)
    where = f"{what + ': ' if what else ''}{disp.path()}"
    got = res.written
    assert got.shape == exp.out.shape and got.dtype == np.float32, f"{where}: shape {got.shape} vs {exp.out.shape}"
    diff = bits(got) != bits(exp.out)
    if diff.any():
        r, c = (int(x) for x in np.argwhere(diff)[0])
        f = 0 if disp.kernel == "nobag" else int(np.searchsorted(doff, c, side="right") - 1)
        d = c - (0 if disp.kernel == "nobag" else int(doff[f]))
        unit = "position" if disp.kernel == "nobag" else "bag"
        raise AssertionError(
            f"{what + ': ' if what else ''}{disp.path(None if disp.kernel == 'nobag' else f)}: {int(diff.sum())} elements "
            f"differ in {np.unique(np.nonzero(diff)[0]).size} rows; first at {unit} {r} column {d} (slot v = {d // (4 * disp.G)}): "
            f"got {float(got[r, c])!r}, want {float(exp.out[r, c])!r}")
    if not res.gap_ok:
        r, c = (int(x) for x in np.argwhere(bits(res.out[:, res.sum_D:]) != CANARY_BITS)[0])
        raise AssertionError(f"{where}: gap column {res.sum_D + c} of row {r} was written ({float(res.out[r, res.sum_D + c])!r})")
    assert res.outer_ok, f"{where}: guard bytes around out or the tables changed"
    assert res.tables_ok, f"{where}: a table changed"
    assert res.errors == exp.errors, f"{where}: bounds_errors {res.errors}, want exactly {exp.errors}"
    assert res.guards_ok


# ---- a numpy forward that can be wrong on purpose ---------------------------------------------------------------------
FAULTS = ("drop_pos64", "drop_group1", "zero_bags_16_63", "skip_last_slot", "drop_4th_scalar", "mean_maxlen", "foreign_bad",
          "gap_overwrite")


def standin_forward(tables, batch, max_D, pooling, feat_pooling=None, feat_window=None, stride=None, fault=None):
    """The forward in numpy (float64 sums rounded once), laid out as the kernels lay it out; `fault` injects one of FAULTS.
    Returns (Result, Dispatch)."""
    assert fault is None or fault in FAULTS
    F, B = batch.F, batch.B
    feat_D = [t.shape[1] for t in tables]
    sum_D = int(sum(feat_D))
    stride = sum_D if stride is None else stride
    disp = dispatch(F, B, batch.N, max_D, feat_D, stride)
    NG = 64 // disp.G
    san = sanitize(tables, batch, feat_window)
    idx = san.idx.copy()
    at = np.arange(idx.size) - np.repeat(san.offs[:-1], san.lens)  # position inside the bag
    if fault == "drop_pos64":
        idx[at == 64] = -1
    if fault == "drop_group1":
        assert disp.kernel == "long" and NG > 1
        idx[(at % 64) % NG == 1] = -1
    mean_len = None
    if fault == "mean_maxlen":
        assert disp.kernel == "short"
        mates = quad_mates(B, disp.bags_per_wave, disp.G)
        lens2 = np.concatenate([san.lens.reshape(F, B), np.zeros((F, 1), dtype=np.int64)], axis=1)  # mate -1 reads 0
        mean_len = lens2[:, mates].max(axis=1).reshape(-1)
    out = pooled_f64(tables, idx, san.offs, san.psw, F, B, mean_flags(F, pooling, feat_pooling), mean_len)
    written = np.ones(sum_D, dtype=bool)
    doff = np.concatenate([[0], np.cumsum(feat_D)]).astype(np.int64)
    for f in range(F):
        d = np.arange(feat_D[f])
        if fault == "skip_last_slot":
            written[doff[f] + d[d // (4 * disp.G) == disp.NV - 1]] = False
        if fault == "drop_4th_scalar" and not disp.vec[f] and feat_D[f] % 4 == 3:
            written[doff[f] + d[d % 4 == 3]] = False
    full = canary_block(B, stride)
    full[:, :sum_D][:, written] = out[:, written]
    if fault == "zero_bags_16_63":
        assert disp.kernel == "short" and disp.bags_per_wave == 64
        full[np.arange(B) % 64 >= 16, :sum_D] = 0.0
    if fault == "gap_overwrite":
        assert stride > sum_D
        full[B // 2, sum_D] = 0.0
    errors = san.n_bad + san.n_malformed + (san.n_foreign if fault == "foreign_bad" else 0)
    return Result(full, errors, sum_D=sum_D), disp


# ---- the case lists ------------------------------------------------------------------------------------------------
class Spec:
    """One designed call.  dims: D per feature (one table each); lengths: "long" / "short" / "skewed"; ids: "plain" / "bad" /
    "window" / "malformed"; misalign: {feature: bytes its table is pushed off the grid}; dtypes: the table types it runs with."""

    def __init__(self, name, dims, B, lengths, max_D, weighted=False, pooling=SUM, mixed=False, rows=None, pad=0, ids="plain",
                 misalign=None, out_off=0, stride=None, dtypes=("float32", "float16"), seed=0):
        self.name, self.dims, self.B, self.lengths, self.max_D = name, list(dims), int(B), lengths, int(max_D)
        self.weighted, self.pooling, self.ids = weighted, pooling, ids
        self.F = len(self.dims)
        self.feat_pooling = [MEAN if f % 2 == 0 else SUM for f in range(self.F)] if mixed else None
        self.rows = list(rows) if rows is not None else [40 + 3 * f for f in range(self.F)]
        self.sum_D = int(sum(self.dims))
        self.stride = int(stride) if stride is not None else (self.sum_D + 3) // 4 * 4 + pad
        self.misalign, self.out_off, self.dtypes, self.seed = dict(misalign or {}), int(out_off), tuple(dtypes), seed
        self.windows = [(r + 2, 3 * r + 7) for r in self.rows] if ids == "window" else None

    @property
    def feat_window(self):
        return None if self.windows is None else [x for w in self.windows for x in w]

    def batch_key(self):
        return (tuple(self.dims), tuple(self.rows), self.B, self.lengths, self.weighted, self.ids, self.seed)

    def dispatch(self, dtype="float32"):
        b = build_batch(self)
        off = [self.misalign.get(f, 0) for f in range(self.F)]
        return dispatch(self.F, self.B, b.N, self.max_D, self.dims, self.stride, dtype, off, self.out_off)


@functools.lru_cache(maxsize=4)
def _build_batch(key):
    dims, rows, B, lengths, weighted, ids, seed = key
    F = len(dims)
    rng = np.random.default_rng([seed, F, B, len(lengths)])
    lens = {"long": lambda: long_lengths(rng, F, B), "short": lambda: short_lengths(rng, F, B),
            "skewed": lambda: skewed_lengths(F, B)}[lengths]()
    windows = [(r + 2, 3 * r + 7) for r in rows] if ids == "window" else None
    batch = make_batch(rng, lens, rows, weighted, "plain" if ids == "malformed" else ids, windows)
    if ids == "malformed":
        n = F * B
        where = sorted({0, n} | {int(k) for k in np.linspace(2, n - 2, 9).astype(np.int64) if 0 < k < n})
        batch = with_malformed_offsets(batch, where)
    return batch


def build_batch(spec):
    return _build_batch(spec.batch_key())


@functools.lru_cache(maxsize=4)
def _build_tables(dims, rows, seed):
    return make_tables(rows, dims, seed)


def build_tables(spec):
    return _build_tables(tuple(spec.dims), tuple(spec.rows), spec.seed)


@functools.lru_cache(maxsize=4)
def _expected(key, pooling, feat_pooling, feat_window, dims, rows, seed):
    return expected(_build_tables(dims, rows, seed), _build_batch(key), pooling, feat_pooling, feat_window)


def spec_expected(spec):
    """Shared among the cases that differ only in max_D, the table type or an alignment: none of them enters the values."""
    fp, fw = spec.feat_pooling, spec.feat_window
    return _expected(spec.batch_key(), spec.pooling, None if fp is None else tuple(fp), None if fw is None else tuple(fw),
                     tuple(spec.dims), tuple(spec.rows), spec.seed)


MODES = {  # name -> weighted, pooling_mode, per-feature mix
    "sum": (False, SUM, False), "wsum": (True, SUM, False), "wmean": (True, MEAN, False), "mixmean": (False, MEAN, True)}
BATCHES = [1, 15, 16, 17, 63, 64, 65, 130]
ODD_D = [63, 65, 129, 257, 513, 2047]


def class_cases():
    """Every (G, NV) class at 16 bags per wave, both kernels, four modes.  Features: D = max_D, the class's lower edge + 4,
    the narrow 8, an odd D last (so it alone is scalar); the long kernel's cases of every second class carry a fifth feature
    (D = 12), which makes F * B no multiple of 4 at B = 130, 1, 15.  The out stride leaves 1 .. 9 gap columns."""
    out = []
    for ci, (top, G, NV) in enumerate(CLASSES):
        for ki, kernel in enumerate(("short", "long")):
            for mi, (mode, (weighted, pooling, mixed)) in enumerate(MODES.items()):
                B = BATCHES[(mi + 4 * ki + 3 * ci) % 8]
                dims = [top, CLASS_LOWER[ci] + 4, 8] + ([12] if kernel == "long" and ci % 2 else []) + [ODD_D[ci]]
                out.append(Spec(f"D{top}-{kernel}-{mode}-B{B}", dims, B, kernel, top, weighted, pooling, mixed, pad=4 * (mi % 3),
                                seed=ci))
    return out


SHAPES_64 = [(2, 262144 + 65), (1, 524288 + 200), (26, 20165)]


def bpw64_cases():
    """F * B >= 2^19: 64 bags per wave.  Tiny tables (50 rows), D = 8, so `out` stays near 20 MB."""
    out = []
    for F, B in SHAPES_64:
        for lengths in ("short", "skewed"):
            for mode in ("wmean", "sum"):
                weighted, pooling, mixed = MODES[mode]
                for max_D in (64, 128, 256, 2048):
                    out.append(Spec(f"F{F}xB{B}-{lengths}-{mode}-maxD{max_D}", [8] * F, B, lengths, max_D, weighted, pooling,
                                    mixed, rows=[50] * F, pad=4, seed=7))
    return out


def vec_cases():
    """D = 128 and D = 64 features at max_D = 128 (G = 32), with exactly one reason for the scalar path at a time."""
    out = []
    for lengths, B in (("short", 33), ("long", 18)):
        def spec(name, dims=(128, 64), **kw):
            return Spec(f"{name}-{lengths}", list(dims), B, lengths, 128, True, MEAN, pad=4, seed=11, **kw)

        out += [spec("aligned"),
                spec("odd_front", (7, 128, 64)),  # Doff = 7, 135
                spec("odd_middle", (128, 7, 64)),  # the first feature stays on the 16-B path
                spec("stride", stride=128 + 64 + 5),
                spec("table_off_4B", misalign={0: 4}, dtypes=("float32",)),
                spec("table_off_2B", misalign={1: 2}, dtypes=("float16",)),
                spec("table_off_4B_f16", misalign={0: 4}, dtypes=("float16",)),
                spec("table_off_6B", misalign={0: 6, 1: 6}, dtypes=("float16",)),
                spec("out_off", out_off=4)]
    return out


def vec_expectation(spec, dtype):
    """Which features must take the scalar path, said without dispatch()."""
    name = spec.name.rsplit("-", 1)[0]
    if name in ("stride", "out_off"):
        return [False] * spec.F
    if name == "odd_front":
        return [False, False, False]
    if name == "odd_middle":
        return [True, False, False]
    if name.startswith("table_off"):
        return [f not in spec.misalign for f in range(spec.F)]
    return [True] * spec.F


def id_cases():
    """Windows, bad ids and malformed offsets: both kernels at 16 bags per wave, the short kernel also at 64."""
    out = []
    for tag, dims, B, lengths, rows in (("short16", [8, 132, 63], 65, "short", None), ("skewed16", [8, 132, 63], 300, "skewed", None),
                                        ("long16", [8, 132, 63], 18, "long", None),
                                        ("short64", [8, 8], 262144 + 65, "short", [50, 50]),
                                        ("skewed64", [8, 8], 262144 + 65, "skewed", [50, 50])):
        for ids in ("window", "bad", "malformed"):
            out.append(Spec(f"{ids}-{tag}", dims, B, lengths, max(dims), True, MEAN, rows=rows, pad=4, ids=ids, seed=13))
    return out


class NobagSpec:
    """PoolingMode.NONE: F features of one D; `counts` ids per feature (0 = an empty feature)."""

    def __init__(self, name, D, counts, B=2, bad=False, misalign=None, out_off=0, dtypes=("float32", "float16"), seed=0):
        self.name, self.D, self.counts, self.B, self.bad = name, int(D), [int(c) for c in counts], int(B), bad
        self.F, self.N = len(self.counts), int(sum(self.counts))
        self.rows = [30 + (5 * f) % 23 for f in range(self.F)]
        self.misalign, self.out_off, self.dtypes, self.seed = dict(misalign or {}), int(out_off), tuple(dtypes), seed

    def dispatch(self, dtype="float32"):
        return dispatch_nobag(self.F, self.N, self.D, dtype, [self.misalign.get(f, 0) for f in range(self.F)], self.out_off)


@functools.lru_cache(maxsize=4)
def _nobag_batch(counts, rows, B, bad, seed):
    rng = np.random.default_rng([seed, len(counts), B])
    lens = []
    for c in counts:  # c ids over B bags: only offsets[f * B] matters to the kernel
        cut = np.sort(rng.integers(0, c + 1, size=B - 1))
        lens.append(np.diff(np.concatenate([[0], cut, [c]])))
    lengths = np.array(lens, dtype=np.int64).reshape(len(counts), B)
    vals = []
    for f, c in enumerate(counts):
        v = rng.integers(0, rows[f], size=c).astype(np.int64)
        if bad:
            v = np.where(rng.random(c) < 0.15, rng.choice(np.array([-1, rows[f], rows[f] + 9, -(1 << 40)]), size=c), v)
        vals.append(v)
    offsets = np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
    return Batch(len(counts), B, np.concatenate(vals).astype(np.int64), offsets, None)


def nobag_batch(spec):
    return _nobag_batch(tuple(spec.counts), tuple(spec.rows), spec.B, spec.bad, spec.seed)


def nobag_tables(spec):
    return _build_tables(tuple([spec.D] * spec.F), tuple(spec.rows), spec.seed)


def _split3(n):
    return [n // 3, n - n // 3 - n // 4, n // 4] if n >= 3 else [n, 0, 0]


NOBAG_ODD_D = [63, 127, 255, 511, 1023, 2047]
NOBAG_PAST_CAP = {16: (4, 262144 + 77), 32: (68, 131072 + 77), 64: (132, 65536 + 77)}  # G -> (D, N)


def nobag_edge_cases():
    """Both edges of every class (the lower one is odd: 1, 65, ...), an odd D just below the upper edge (D % 4 == 3), each at
    N = 1, per_block - 1, per_block, per_block + 1 over three features."""
    out = []
    for ci, (top, G, NV) in enumerate(CLASSES):
        per_block = 16 * (64 // G)
        for D in (CLASS_LOWER[ci] + 1, top, NOBAG_ODD_D[ci]):
            for N in (1, per_block - 1, per_block, per_block + 1):
                out.append(NobagSpec(f"D{D}-N{N}", D, _split3(N), seed=ci))
    return out


def nobag_other_cases():
    out = []
    for G, (D, N) in NOBAG_PAST_CAP.items():
        out.append(NobagSpec(f"past_cap-G{G}-D{D}-N{N}", D, _split3(N), seed=G))
    out.append(NobagSpec("empty_first_middle_last", 68, [0, 0, 37, 0, 0, 90, 1, 0], seed=3))
    out.append(NobagSpec("F1", 132, [300], seed=4))
    counts70 = [0 if f % 7 in (0, 3) or f >= 68 else 1 + (11 * f) % 9 for f in range(70)]
    out.append(NobagSpec("F70", 8, counts70, seed=5))
    out.append(NobagSpec("F70-bad", 260, counts70, bad=True, seed=5))
    out.append(NobagSpec("bad-D64", 64, [50, 0, 77], bad=True, seed=6))
    out.append(NobagSpec("bad-D2047", 2047, [20, 9, 0], bad=True, seed=6))
    out.append(NobagSpec("table_off_4B", 128, [40, 41, 42], misalign={1: 4}, dtypes=("float32",), seed=8))
    for off in (2, 4, 6):
        out.append(NobagSpec(f"table_off_{off}B_f16", 128, [40, 41, 42], misalign={1: off}, dtypes=("float16",), seed=8))
    out.append(NobagSpec("out_off", 128, [40, 41, 42], out_off=4, seed=8))
    return out


# ---- the GPU half ----------------------------------------------------------------------------------------------------
class ForwardCase:
    """Tables in ONE flat device buffer: every table starts 16-B aligned — `misalign[f]` bytes further — and is followed by
    GUARD_BYTES of GUARD_BYTE; the gaps before it hold the same byte.  `out` lies in a buffer of its own, `out_off` bytes
    past a 16-B boundary, between guards."""

    def __init__(self, tables, dtype="float32", misalign=None, out_off=0):
        self.dtype = np.dtype(dtype)
        self.tables = [np.ascontiguousarray(t.astype(self.dtype)) for t in tables]
        for t16, t in zip(self.tables, tables):
            assert np.array_equal(t16.astype(np.float32), t)  # exact in FP16: the up-cast table IS the FP32 one
        self.F = len(tables)
        self.feat_D = [t.shape[1] for t in tables]
        self.rows = [t.shape[0] for t in tables]
        self.misalign, self.out_off = dict(misalign or {}), int(out_off)
        assert all(m % self.dtype.itemsize == 0 for m in self.misalign.values()) and self.out_off % 4 == 0
        self._slots = []
        off = GUARD_BYTES
        for f, t in enumerate(self.tables):
            off = (off + 15) // 16 * 16 + self.misalign.get(f, 0)
            self._slots.append(off)
            off += t.nbytes + GUARD_BYTES
        self.nbytes = off
        self._host = np.full(self.nbytes, GUARD_BYTE, dtype=np.uint8)
        for o, t in zip(self._slots, self.tables):
            self._host[o:o + t.nbytes] = t.view(np.uint8).reshape(-1)
        self._dev = None

    def _device(self):
        import torch

        if self._dev is None:
            buf = torch.tensor(self._host).cuda()
            assert buf.data_ptr() % 16 == 0
            self._dev = dict(
                buf=buf, weights=torch.tensor([buf.data_ptr() + o for o in self._slots], dtype=torch.int64).cuda(),
                feat_D=torch.tensor(self.feat_D, dtype=torch.int32).cuda(), feat_rows=torch.tensor(self.rows, dtype=torch.int64).cuda(),
                out_offset=torch.tensor(np.concatenate([[0], np.cumsum(self.feat_D)[:-1]]).astype(np.int64)).cuda())
        return self._dev

    def run(self, batch, max_D, pooling=SUM, feat_pooling=None, feat_window=None, stride=None, nobag=False):
        """tbe_forward_pooled_* (nobag: tbe_forward_nobag_*, D = max_D) with a zeroed bounds_errors -> Result."""
        import torch
        from fbgemm_gpu import _lib

        lib, d = _lib.load(), self._device()
        if batch._dev is None:
            batch._dev = tuple(None if a is None else torch.tensor(a).cuda() for a in (batch.indices, batch.offsets, batch.psw))
        indices, offsets, psw = batch._dev
        sum_D = max_D if nobag else int(sum(self.feat_D))
        n_rows = batch.N if nobag else batch.B
        stride = sum_D if stride is None else int(stride)
        assert stride >= sum_D and (not nobag or stride == sum_D)
        lo = GUARD_BYTES + self.out_off
        host = np.full(lo + n_rows * stride * 4 + GUARD_BYTES, GUARD_BYTE, dtype=np.uint8)
        host[lo:lo + n_rows * stride * 4] = canary_block(n_rows, stride).view(np.uint8).reshape(-1)
        obuf = torch.tensor(host).cuda()
        assert obuf.data_ptr() % 16 == 0
        out_ptr = obuf.data_ptr() + lo
        bounds = torch.zeros(1, dtype=torch.int32, device="cuda")
        st = _lib.stream_ptr(torch.device("cuda", 0))
        p = _lib.ptr
        wt = "f16w" if self.dtype == np.float16 else "f32"
        if nobag:
            assert all(D == max_D for D in self.feat_D)
            _lib.check(getattr(lib, f"tbe_forward_nobag_{wt}")(
                p(d["weights"]), p(d["feat_rows"]), self.F, batch.B, max_D, p(indices), batch.N, p(offsets), out_ptr, p(bounds),
                st), f"tbe_forward_nobag_{wt}")
        else:
            fpool = None if feat_pooling is None else torch.tensor(list(feat_pooling), dtype=torch.int32).cuda()
            fwin = None if feat_window is None else torch.tensor(list(feat_window), dtype=torch.int64).cuda()
            _lib.check(getattr(lib, f"tbe_forward_pooled_{wt}")(
                p(d["weights"]), p(d["feat_D"]), p(d["out_offset"]), p(d["feat_rows"]), self.F, batch.B, max_D, p(indices), batch.N,
                p(offsets), p(psw), int(pooling), p(fpool), out_ptr, stride, p(bounds), p(fwin), st), f"tbe_forward_pooled_{wt}")
        torch.cuda.synchronize()
        after = obuf.cpu().numpy()
        out = after[lo:lo + n_rows * stride * 4].copy().view(np.float32).reshape(n_rows, stride)
        outer = (after[:lo] == GUARD_BYTE).all() and (after[lo + n_rows * stride * 4:] == GUARD_BYTE).all()
        tables_ok = bool((d["buf"].cpu().numpy() == self._host).all())  # the tables AND the guard bytes around them
        return Result(out, int(bounds.item()), outer, tables_ok, sum_D)


def run_spec(spec, dtype):
    """(Result, Dispatch) of one pooled Spec with tables of `dtype`."""
    case = ForwardCase(build_tables(spec), dtype, spec.misalign, spec.out_off)
    res = case.run(build_batch(spec), spec.max_D, spec.pooling, spec.feat_pooling, spec.feat_window, spec.stride)
    return res, spec.dispatch(dtype)


def run_nobag(spec, dtype):
    case = ForwardCase(nobag_tables(spec), dtype, spec.misalign, spec.out_off)
    return case.run(nobag_batch(spec), spec.D, nobag=True), spec.dispatch(dtype)
