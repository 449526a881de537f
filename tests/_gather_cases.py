"""Inputs, expected results and guarded device buffers for the tests that call the three gather entry points of the dot
interaction (tbe_dlrm_interaction_gather_forward_f32 / _gather_backward_f32 / _gather_backward_sgd_f32, include/tbe_hip.h)
through the C ABI.  Importing this needs no device.

The kernels (csrc/dlrm_interaction.hip, "pooling factor 1") are the dense pair's with one change: row r >= 1 of sample b is
the table row that id (r - 1, b) selects.  What that row is, is restated here in plain numpy from classify_id
(csrc/common.hpp); everything after it is the oracle's: oracle.interaction_forward / interaction_backward on the gathered
rows, and oracle.tbe_backward (exact SGD, one fmaf per element) for the tables the SGD variant leaves behind.  Layouts, trip
counts and the images of `out` / `grad_out`: tests/_interaction_cases.py.  Both directions run 256 * 2 blocks of 4 waves at
D = 64 and 128, so a wave moves 2048 samples per trip in all three kernels."""
import functools

import numpy as np

import _paths  # noqa: F401
import _interaction_cases as ic
from _guarded import Buf, TypedBuf
from oracle import oracle

ID_SKIP = -(1 << 63)  # TBE_ID_SKIP
DIMS = (64, 128)
MAX_F = ic.BWD_MAX_F

# ---- shape lists -----------------------------------------------------------------------------------------------------
EVERY_F_B = 9
EVERY_F_LAYOUTS = ("dense", "padded", "odd")
LOOP_B = ic.loop_batch("fwd", 128)  # 4101: two full trips of every wave and a third of five waves, in both directions
LOOP_F = (1, 10, 11, 15, 16, 20, 23, 27)  # T = 1, 1, 2, 2, 3, 4, 5, 6; R = 16 | 17 at F = 15 | 16
TRIP_EDGES = ((2053, 16, 128, "odd"), (6149, 16, 128, "odd"))  # waves that end after 2 | 1 and after 4 | 3 trips
FEW_B = ic.FEW_B
FEW_SHAPES = ((16, 128), (15, 64))
ID_EDGE_SHAPES = ((LOOP_B, 7, 128), (LOOP_B, 27, 128))
ISOLATION = ((LOOP_B, 16, 128), (LOOP_B, 15, 64))
SGD_F = (1, 16, 27)
SGD_LAYOUTS = ("dense", "padded", "shifted")
LR = 0.05
BIG_LO = (1 << 33) + 5  # first global row of a window whose local ids have a high word


def row_cycle(B, F):
    """Rows per table cycling through 1, 3, 40 and B + 5: rows that repeat in every sample next to rows that rarely do."""
    return tuple((1, 3, 40, B + 5)[f % 4] for f in range(F))


def distinct_rows(B, F):
    return (B + 5,) * F


def duplicate_rows(F):
    return tuple((1, 3, 1000, 5000)[f % 4] for f in range(F))


# ---- a case ----------------------------------------------------------------------------------------------------------
class GatherCase:
    """rows [F] per feature, starts [F] (element offset of each feature's table in `flat`; two features may share one),
    flat float32 table buffer, ids [F, B] int64, dense [B, D], grad [B, D + P], window [F, 2] (first global row, global
    rows) or None.  Shared between tests: every array is read-only; `replace` makes a case with some of them changed."""

    FIELDS = ("rows", "starts", "flat", "ids", "dense", "grad", "window")

    def __init__(self, B, F, D, rows, starts, flat, ids, dense, grad, window=None):
        self.B, self.F, self.D = B, F, D
        self.rows = np.asarray(rows, dtype=np.int64)
        self.starts = np.asarray(starts, dtype=np.int64)
        self.flat, self.dense, self.grad = flat, dense, grad
        self.ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(F, B)
        self.window = None if window is None else np.ascontiguousarray(window, dtype=np.int64).reshape(F, 2)
        assert self.rows.shape == self.starts.shape == (F,) and dense.shape == (B, D) and grad.shape == (B, D + ic.pairs(F))
        assert flat.dtype == dense.dtype == grad.dtype == np.float32
        assert (self.starts % D == 0).all() and (self.starts + self.rows * D <= flat.size).all()
        for a in (self.rows, self.starts, self.flat, self.ids, self.dense, self.grad, self.window):
            if a is not None:
                a.setflags(write=False)

    def replace(self, **changed):
        assert set(changed) <= set(self.FIELDS)
        return GatherCase(self.B, self.F, self.D, *(changed.get(k, getattr(self, k)) for k in self.FIELDS))

    def table(self, f, flat=None):
        flat = self.flat if flat is None else flat
        return flat[self.starts[f]:self.starts[f] + self.rows[f] * self.D].reshape(self.rows[f], self.D)

    @functools.cached_property
    def classes(self):
        """classify_id for every (f, b): (local row [F, B], is a row of this shard, is counted in bounds_errors).
        local = id - lo in 64-bit wrap-around arithmetic; a local row when 0 <= local < rows; else silently a zero row
        when the id is TBE_ID_SKIP or another shard's row (0 <= id < global_rows); else a counted zero row."""
        lo = np.zeros(self.F, dtype=np.int64) if self.window is None else self.window[:, 0]
        global_rows = self.rows if self.window is None else self.window[:, 1]
        u = self.ids.view(np.uint64)
        local = u - lo.view(np.uint64)[:, None]
        is_local = local < self.rows.view(np.uint64)[:, None]
        silent = (self.ids == ID_SKIP) | (u < global_rows.view(np.uint64)[:, None])
        return local.view(np.int64), is_local, ~is_local & ~silent

    @property
    def bad(self):
        """Expected bounds_errors of one classification of every id."""
        return int(self.classes[2].sum())

    @functools.cached_property
    def sparse(self):
        """[B, F, D]: what the lookup would have written."""
        local, is_local, _ = self.classes
        s = np.zeros((self.B, self.F, self.D), dtype=np.float32)
        for f in range(self.F):
            s[is_local[f], f] = self.table(f)[local[f][is_local[f]]]
        s.setflags(write=False)
        return s

    @functools.cached_property
    def dot(self):
        """The dense-interaction case of the gathered rows: .out, .grads and what RowBuf / expected_out / grad_image of
        tests/_interaction_cases.py take."""
        return ic._Case(self.B, self.F, self.D, self.dense, self.sparse, self.grad)

    def updated(self, single):
        """[F, B] bool: the contributions whose table row the SGD variant must rewrite: flagged and a row of the shard."""
        return (np.asarray(single).reshape(self.F, self.B) != 0) & self.classes[1]

    def sgd_flat(self, single, lr=LR):
        """The table buffer after the SGD variant with flags `single` [F * B]: fmaf(-lr, g, w) with g the oracle's
        grad_sparse row on the rows `updated` names (no two of them the same row), every other element as it was.  The
        rounding is the oracle's: oracle.tbe_backward with an empty bag for every other contribution."""
        assert len(set(self.starts.tolist())) == self.F, "tables shared between features have no single-row update"
        local, upd = self.classes[0], self.updated(single)
        flat = self.flat.copy()
        tabs = oracle.Tables(self.rows.tolist(), [self.D] * self.F)
        tabs.weights = [self.table(f, flat) for f in range(self.F)]  # views: the oracle writes into `flat`
        offsets = np.concatenate([[0], np.cumsum(upd.reshape(-1))]).astype(np.int64)
        grads = self.dot.grads[1].reshape(self.B, self.F * self.D)
        assert oracle.tbe_backward(tabs, local[upd], offsets, grads, oracle.OPT_EXACT_SGD, lr) == 0
        return flat

    def sgd_grad_sparse(self, single, canary):
        """grad_sparse [B, F, D] after the SGD variant on a buffer of `canary`: rows of updated contributions unwritten."""
        gs = self.dot.grads[1].copy()
        gs[self.updated(single).T] = canary
        return gs


def make(B, F, D, rows, distinct=False, seed=0):
    """A windowless case with one table per feature, packed in feature order.  distinct: no row is touched twice."""
    rng = np.random.default_rng([2026, B, F, D, int(distinct), seed])
    draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    rows = np.asarray(rows, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(rows * D)])
    if distinct:
        ids = np.stack([rng.permutation(rows[f])[:B] for f in range(F)])
    else:
        ids = np.stack([rng.integers(0, rows[f], size=B) for f in range(F)])
    return GatherCase(B, F, D, rows, starts[:-1], draw(int(starts[-1])), ids, draw(B, D), draw(B, D + ic.pairs(F)))


@functools.lru_cache(maxsize=3)  # a test asks for one shape and loops over layouts and entries; big shapes are not kept
def case(B, F, D, rows=None, distinct=False, seed=0):
    return make(B, F, D, (distinct_rows if distinct else row_cycle)(B, F) if rows is None else rows, distinct, seed)


def poison(c, samples):
    """ic.poison for a case with distinct ids: in every sample b of `samples`, NaN in column POISON_COL of the table row
    that only (b % F, b) reaches, +Inf in dense[b, POISON_COL] and -Inf in the gradient of the pair b % P."""
    flat, dense, grad = c.flat.copy(), c.dense.copy(), c.grad.copy()
    local, is_local, _ = c.classes
    for b in samples:
        f = b % c.F
        assert is_local[f, b] and (local[f] == local[f, b]).sum() == 1
        c.table(f, flat)[local[f, b], ic.POISON_COL] = np.nan
        dense[b, ic.POISON_COL] = np.inf
        grad[b, c.D + b % ic.pairs(c.F)] = -np.inf
    return c.replace(flat=flat, dense=dense, grad=grad)


def assert_same(got, want, err_msg=""):
    """np.testing.assert_array_equal; arrays with the same bits (nearly always) are not walked a second time for the
    report, which at 14 million elements costs more than the kernel call."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and got.dtype == want.dtype and got.flags.c_contiguous and want.flags.c_contiguous:
        bits = np.dtype(f"u{got.dtype.itemsize}")
        if np.array_equal(got.reshape(-1).view(bits), want.reshape(-1).view(bits)):
            return
    np.testing.assert_array_equal(got, want, err_msg=err_msg)


# ---- guarded device buffers ------------------------------------------------------------------------------------------
class Device:
    """Every input of a case on the device between guard elements, uploaded once for all layouts and entries.  The
    tables: one guarded float32 buffer; the SGD variant runs on `fresh_tables()`."""

    def __init__(self, c):
        self.c = c
        self.dense = Buf(c.dense.size, c.dense)
        self.ids = TypedBuf(c.ids.size, np.int64, c.ids)
        self.feat_rows = TypedBuf(c.F, np.int64, c.rows)
        self.feat_window = TypedBuf(2 * c.F, np.int64, c.window) if c.window is not None else None
        self.window_ptr = self.feat_window.ptr if c.window is not None else None
        self.tables, self.feat_weights, self.addresses = self.fresh_tables()

    def fresh_tables(self):
        tables = Buf(self.c.flat.size, self.c.flat)
        addresses = tables.ptr + 4 * self.c.starts
        return tables, TypedBuf(self.c.F, np.int64, addresses), addresses

    def assert_inputs_untouched(self):
        """Everything the forward and the plain backward only read, the whole table buffer included."""
        c = self.c
        assert_same(self.tables.get(), c.flat)
        self.assert_arguments_untouched(self.feat_weights, self.addresses)

    def assert_arguments_untouched(self, feat_weights, addresses):
        c = self.c
        assert_same(self.dense.get(c.dense.shape), c.dense)
        assert_same(self.ids.get(c.ids.shape), c.ids)
        np.testing.assert_array_equal(self.feat_rows.get(), c.rows)
        np.testing.assert_array_equal(feat_weights.get(), addresses)
        if self.feat_window is not None:
            np.testing.assert_array_equal(self.feat_window.get(c.window.shape), c.window)
