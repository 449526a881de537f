"""GPU: the three gather entry points of the dot interaction (tbe_dlrm_interaction_gather_forward_f32 /
_gather_backward_f32 / _gather_backward_sgd_f32, include/tbe_hip.h) through the C ABI, bit for bit against the CPU oracle
at every edge that is the gather kernels' own (csrc/dlrm_interaction.hip, "pooling factor 1"): rows that arrive from raw
table addresses, from `dense` or as a zero row; ids that travel two samples ahead of the rows; feature lanes clamped to
F - 1; the SGD variant's row addresses in the pad columns of the LDS image and its stores into the tables.

Every buffer sits between guard elements (tests/_guarded.py): ids, flags, feat_* arrays and the counter too.  `out`,
`grad_dense` and `grad_sparse` start as canaries, so every element a call must not write is compared; every input is
read back, after the forward and the plain backward the whole table buffer.  No expected value comes from a GPU kernel.
Cases and expected results: tests/_gather_cases.py; layouts and trip counts: tests/_interaction_cases.py."""
import functools
import types

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _gather_cases as gc
import _interaction_cases as ic
from _guarded import CANARY, Buf, TypedBuf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

OK = 0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _done(lib, rc):
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()


def _counter(wanted):
    return TypedBuf(1, np.int32, [0]) if wanted else None


def _count(err):
    return None if err is None else int(err.get()[0])


def _forward(lib, dev, name, counter=True):
    """One forward in layout `name` -> (the whole [B, stride] image of `out`, stride, shift, bounds_errors or None)."""
    c = dev.c
    _, stride, shift = ic.layout(c.F, c.D, name)
    out, err = ic.RowBuf(c.B, stride, shift), _counter(counter)
    _done(lib, lib.tbe_dlrm_interaction_gather_forward_f32(
        dev.dense.ptr, dev.feat_weights.ptr, dev.feat_rows.ptr, dev.window_ptr, dev.ids.ptr, c.B, c.F, c.D, out.ptr, stride,
        err.ptr if err else None, _stream()))
    return out.get(), stride, shift, _count(err)


def _backward(lib, dev, name, counter=False, single=None, lr=gc.LR):
    """One backward with grad_out in layout `name` on canary-filled outputs -> (grad_dense [B, D], grad_sparse [B, F, D],
    bounds_errors or None, table buffer).  single [F * B] uint8: the SGD variant, on a fresh clone of the tables."""
    c = dev.c
    _, stride, shift = ic.layout(c.F, c.D, name)
    image = ic.grad_image(c.dot, stride)
    g = ic.RowBuf(c.B, stride, shift, image)
    gd, gs, err = Buf(c.B * c.D), Buf(c.B * c.F * c.D), _counter(counter)
    tables, feat_weights, addresses = (dev.tables, dev.feat_weights, dev.addresses) if single is None else dev.fresh_tables()
    args = (dev.dense.ptr, feat_weights.ptr, dev.feat_rows.ptr, dev.window_ptr, dev.ids.ptr, g.ptr, stride, c.B, c.F, c.D,
            gd.ptr, gs.ptr, err.ptr if err else None)
    if single is None:
        _done(lib, lib.tbe_dlrm_interaction_gather_backward_f32(*args, _stream()))
    else:
        flags = TypedBuf(c.F * c.B, np.uint8, single)
        _done(lib, lib.tbe_dlrm_interaction_gather_backward_sgd_f32(*args, flags.ptr, lr, _stream()))
        gc.assert_same(flags.get(), np.asarray(single, dtype=np.uint8).reshape(-1))
        dev.assert_arguments_untouched(feat_weights, addresses)
    gc.assert_same(g.get(), image)  # grad_out is an input
    return gd.get((c.B, c.D)), gs.get((c.B, c.F, c.D)), _count(err), tables.get()


def _tag(c, name):
    return f"B={c.B} F={c.F} D={c.D} {name}"


def _check_forward(lib, c, names, dev=None):
    dev = dev or gc.Device(c)
    for name in names:
        image, stride, shift, bad = _forward(lib, dev, name)
        gc.assert_same(image, ic.expected_out(c.dot, stride, shift), err_msg=_tag(c, name))
        assert bad == c.bad, _tag(c, name)
    dev.assert_inputs_untouched()


def _check_backward(lib, c, names, dev=None):
    dev = dev or gc.Device(c)
    for name in names:
        gd, gs, _, _ = _backward(lib, dev, name)
        gc.assert_same(gd, c.dot.grads[0], err_msg=_tag(c, name))
        gc.assert_same(gs, c.dot.grads[1], err_msg=_tag(c, name))
    dev.assert_inputs_untouched()


def _check_sgd(lib, c, names, single, dev=None, twice=False):
    """The SGD variant with flags `single`: the whole guarded table buffer, grad_dense, and grad_sparse with the rows of
    updated contributions still canaries.  Returns the table buffer of the last layout."""
    dev = dev or gc.Device(c)
    single = np.asarray(single, dtype=np.uint8).reshape(-1)
    want_flat, want_gs = c.sgd_flat(single), c.sgd_grad_sparse(single, CANARY)
    flat = None
    for name in names:
        for _ in range(2 if twice else 1):  # the second run, on a fresh clone, gives the same bits
            gd, gs, _, flat = _backward(lib, dev, name, single=single)
            gc.assert_same(flat, want_flat, err_msg=_tag(c, name))
            gc.assert_same(gd, c.dot.grads[0], err_msg=_tag(c, name))
            gc.assert_same(gs, want_gs, err_msg=_tag(c, name))
    dev.assert_inputs_untouched()  # the SGD runs had clones: the case's own tables are as uploaded
    return flat


def _all_flags(c, value=1):
    return np.full(c.F * c.B, value, dtype=np.uint8)


# ---- a. every row count ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", gc.DIMS)
def test_forward_every_row_count(D):
    """F = 1 .. 27: the feature-lane clamps min(lane, F - 1) and min(lane >> 1, F - 1), the id slot and the copy
    instructions of every R, in a 16-B layout, one with P mod 4 pad columns and a scalar one."""
    lib = _lib.load()
    for F in range(1, gc.MAX_F + 1):
        _check_forward(lib, gc.case(gc.EVERY_F_B, F, D), gc.EVERY_F_LAYOUTS)


@pytest.mark.parametrize("D", gc.DIMS)
def test_backward_every_row_count(D):
    lib = _lib.load()
    for F in range(1, gc.MAX_F + 1):
        _check_backward(lib, gc.case(gc.EVERY_F_B, F, D), gc.EVERY_F_LAYOUTS)


@pytest.mark.parametrize("D", gc.DIMS)
def test_sgd_every_row_count(D):
    """All ids distinct and every contribution flagged: every row of every R is stored through its pad-column address."""
    lib = _lib.load()
    for F in range(1, gc.MAX_F + 1):
        c = gc.case(gc.EVERY_F_B, F, D, distinct=True)
        assert c.updated(_all_flags(c)).all()
        _check_sgd(lib, c, gc.EVERY_F_LAYOUTS, _all_flags(c))


# ---- b. loop edges in every layout -------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", gc.LOOP_F)
@pytest.mark.parametrize("D", gc.DIMS)
def test_forward_three_trips_in_every_layout(D, F):
    """Two full trips of every wave and a third of five waves: the id pipeline two samples deep, the row copy one sample
    deep and, in the scalar layouts ("dense" unless P mod 4 == 0, "odd", "shifted"), the counted wait behind DS + T
    stores, at R = 16 | 17 too."""
    assert ic.trips("fwd", gc.LOOP_B, D) == 3
    _check_forward(_lib.load(), gc.case(gc.LOOP_B, F, D), ic.LAYOUTS)


@pytest.mark.parametrize("F", gc.LOOP_F)
@pytest.mark.parametrize("D", gc.DIMS)
def test_backward_three_trips_in_every_layout(D, F):
    assert ic.trips("bwd", gc.LOOP_B, D) == 3
    _check_backward(_lib.load(), gc.case(gc.LOOP_B, F, D), ic.LAYOUTS)


@pytest.mark.parametrize("B,F,D,name", gc.TRIP_EDGES)
def test_waves_that_end_after_other_trip_counts(B, F, D, name):
    """2053: five waves make two trips and the rest one (`b + stride_b < B` false at once).  6149: four and three."""
    lib = _lib.load()
    c = gc.case(B, F, D)
    dev = gc.Device(c)
    _check_forward(lib, c, (name,), dev)
    _check_backward(lib, c, (name,), dev)


# ---- c. fewer samples than waves -------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,D", gc.FEW_SHAPES)
@pytest.mark.parametrize("B", gc.FEW_B)
def test_fewer_samples_than_waves(B, F, D):
    """Waves with b >= B issue nothing, not even an id copy; at B = 5 the second block runs with one active wave."""
    lib = _lib.load()
    c = gc.case(B, F, D)
    dev = gc.Device(c)
    _check_forward(lib, c, ic.LAYOUTS, dev)
    _check_backward(lib, c, ic.LAYOUTS, dev)
    d = gc.case(B, F, D, distinct=True)
    _check_sgd(lib, d, ic.LAYOUTS, _all_flags(d))


@pytest.mark.parametrize("F,D", gc.FEW_SHAPES)
def test_empty_batch_returns_ok_and_writes_nothing(F, D):
    lib = _lib.load()
    stride = D + ic.pairs4(F)
    x, out, g, gd, gs = Buf(4 * F * D), Buf(4 * stride), Buf(4 * stride), Buf(4 * D), Buf(4 * F * D)
    ids, rows, flags, err = TypedBuf(4 * F, np.int64), TypedBuf(F, np.int64), TypedBuf(4 * F, np.uint8), TypedBuf(1, np.int32)
    fw = TypedBuf(F, np.int64, [x.ptr] * F)
    _done(lib, lib.tbe_dlrm_interaction_gather_forward_f32(x.ptr, fw.ptr, rows.ptr, None, ids.ptr, 0, F, D, out.ptr, stride,
                                                           err.ptr, _stream()))
    args = (x.ptr, fw.ptr, rows.ptr, None, ids.ptr, g.ptr, stride, 0, F, D, gd.ptr, gs.ptr, err.ptr)
    _done(lib, lib.tbe_dlrm_interaction_gather_backward_f32(*args, _stream()))
    _done(lib, lib.tbe_dlrm_interaction_gather_backward_sgd_f32(*args, flags.ptr, gc.LR, _stream()))
    for b in (x, out, g, gd, gs):
        assert (b.all() == CANARY).all()
    for b in (ids, rows, flags, err):
        assert (b.all() == b.canary).all()


# ---- d. ids at the loop edges ----------------------------------------------------------------------------------------
def _edge_places(B, F):
    """One wave's three trips and the last sample, at the first and the last feature lane."""
    stride = ic.sample_stride("fwd", B, 128)
    assert 2 + 2 * stride < B
    return [(f, b) for b in (2, 2 + stride, 2 + 2 * stride, B - 1) for f in sorted({0, F - 1})]


def _check_ids(lib, c, name="odd", backward=True):
    """Forward with a counter and with none; backward with none (the ids are classified again: nothing to count into)
    and with one of its own."""
    dev = gc.Device(c)
    _check_forward(lib, c, (name,), dev)
    image, stride, shift, none = _forward(lib, dev, name, counter=False)
    assert none is None
    gc.assert_same(image, ic.expected_out(c.dot, stride, shift))
    if backward:
        _check_backward(lib, c, (name,), dev)
        gd, gs, bad, _ = _backward(lib, dev, name, counter=True)
        assert bad == c.bad
        gc.assert_same(gd, c.dot.grads[0])
        gc.assert_same(gs, c.dot.grads[1])
    dev.assert_inputs_untouched()


@pytest.mark.parametrize("B,F,D", gc.ID_EDGE_SHAPES)
def test_bad_and_skipped_ids_at_the_loop_edges(B, F, D):
    """Zero rows for -1, the row count, 1 << 40, the largest int64 and TBE_ID_SKIP where a wave starts, loops and ends;
    each bad one counted once although every lane >= F classifies the id of feature F - 1 too."""
    base = gc.case(B, F, D)
    ids = base.ids.copy()
    places = _edge_places(B, F)
    for i, (f, b) in enumerate(places):
        ids[f, b] = (-1, int(base.rows[f]), 1 << 40, (1 << 63) - 1, gc.ID_SKIP)[(i + i // 5) % 5]
    c = base.replace(ids=ids)
    skipped = sum(int(ids[f, b]) == gc.ID_SKIP for f, b in places)
    assert skipped >= 1 and c.bad == len(places) - skipped
    assert c.classes[2][F - 1].sum() >= 2 and c.classes[2][0].sum() >= 2
    _check_ids(_lib.load(), c)


@pytest.mark.parametrize("B,F,D", gc.ID_EDGE_SHAPES)
def test_row_windows_above_two_to_the_32(B, F, D):
    """Every other feature's shard starts at global row 2^33 + 5: a local id has a high word, and the id with the same low
    word and none is another shard's row.  Dropping or doubling a half of an id turns one into the other or into a bad one."""
    base = gc.case(B, F, D)
    rng = np.random.default_rng([7, B, F, D])
    lo = np.where(np.arange(F) % 2 == 0, gc.BIG_LO, 3).astype(np.int64)
    window = np.stack([lo, lo + base.rows + 11], axis=1)
    foreign = rng.random((F, B)) < 0.25
    ids = np.where(foreign, base.ids, base.ids + lo[:, None])  # k alone: the same low word, below global_rows
    places = _edge_places(B, F)
    for i, (f, b) in enumerate(places):
        ids[f, b] = (-1, int(window[f, 1]), 1 << 40, (1 << 63) - 1, gc.ID_SKIP, int(lo[f] + base.rows[f]),
                     int(lo[f]) - 1, int(lo[f]))[i % 8]
    c = base.replace(ids=ids, window=window)
    _, is_local, bad = c.classes
    drawn = np.ones((F, B), dtype=bool)  # not one of the places above
    drawn[tuple(zip(*places))] = False
    high = lo == gc.BIG_LO
    assert (is_local[high] == ~foreign[high])[drawn[high]].all() and not bad[drawn].any() and c.bad == 4
    assert 0.6 < is_local[0].mean() < 0.9 and 0.6 < is_local[F - 1].mean() < 0.9
    assert (c.ids[0][is_local[0]] >> 32 == 2).all() and (c.ids[0][~is_local[0] & drawn[0]] >> 32 == 0).all()
    _check_ids(_lib.load(), c)


def test_two_features_of_one_table():
    """Equal feat_weights entries: both features' rows come from the same addresses (forward and plain backward)."""
    B, F, D = gc.ID_EDGE_SHAPES[0]
    base = gc.case(B, F, D)
    assert base.rows[2] == base.rows[6] == 40
    starts = base.starts.copy()
    starts[6] = starts[2]
    c = base.replace(starts=starts)
    assert not np.array_equal(c.sparse[:, 6], base.sparse[:, 6])
    _check_ids(_lib.load(), c)


# ---- e. isolation ----------------------------------------------------------------------------------------------------
def _assert_isolated(got, poisoned_ref, clean_ref, clean_rows):
    gc.assert_same(got, poisoned_ref)
    assert np.isfinite(got[clean_rows]).all()
    gc.assert_same(got[clean_rows], clean_ref[clean_rows])


@functools.lru_cache(maxsize=2)
def _isolation_cases(B, F, D):
    """(clean, poisoned, poisoned samples, clean samples).  Sample 2's wave visits 2 + 2048 next: that one misses (a bad
    id) at the feature whose row held the NaN, so its LDS row must be the zero row, not what the poisoned row left."""
    samples = ic.poisoned_samples("fwd", B, D)
    assert samples == ic.poisoned_samples("bwd", B, D)
    follower = samples[0] + ic.sample_stride("fwd", B, D)
    assert follower not in samples and follower + ic.sample_stride("fwd", B, D) < B
    base = gc.case(B, F, D, distinct=True)
    ids = base.ids.copy()
    ids[samples[0] % F, follower] = -1
    clean = base.replace(ids=ids)
    assert clean.bad == 1 and not clean.sparse[follower, samples[0] % F].any()
    return clean, gc.poison(clean, samples), samples, np.setdiff1d(np.arange(B), samples)


@pytest.mark.parametrize("B,F,D", gc.ISOLATION)
def test_forward_keeps_nonfinite_values_in_their_sample(B, F, D):
    lib = _lib.load()
    clean, p, _, rows = _isolation_cases(B, F, D)
    dev = gc.Device(p)
    for name in ("dense", "padded"):
        image, stride, shift, bad = _forward(lib, dev, name)
        gc.assert_same(image, ic.expected_out(p.dot, stride, shift))
        _assert_isolated(image[:, :D + ic.pairs(F)], p.dot.out, clean.dot.out, rows)
        assert bad == 1
    dev.assert_inputs_untouched()


@pytest.mark.parametrize("B,F,D", gc.ISOLATION)
def test_backward_keeps_nonfinite_values_in_their_sample(B, F, D):
    lib = _lib.load()
    clean, p, _, rows = _isolation_cases(B, F, D)
    dev = gc.Device(p)
    for name in ("dense", "padded"):
        gd, gs, _, _ = _backward(lib, dev, name)
        _assert_isolated(gd, p.dot.grads[0], clean.dot.grads[0], rows)
        _assert_isolated(gs, p.dot.grads[1], clean.dot.grads[1], rows)
    dev.assert_inputs_untouched()


@pytest.mark.parametrize("B,F,D", gc.ISOLATION)
def test_sgd_keeps_nonfinite_values_in_their_sample(B, F, D):
    """Every contribution flagged, the missing one too: the pad columns that held a poisoned sample's addresses, and the
    LDS rows that held its NaN, serve the wave's next sample."""
    lib = _lib.load()
    clean, p, _, rows = _isolation_cases(B, F, D)
    single = _all_flags(p)
    upd = p.updated(single)
    assert upd.sum() == F * B - 1
    clean_flat, want_flat = clean.sgd_flat(single), p.sgd_flat(single)
    dev = gc.Device(p)
    for name in ("dense", "padded"):
        gd, gs, _, flat = _backward(lib, dev, name, single=single)
        gc.assert_same(flat, want_flat)
        _assert_isolated(gd, p.dot.grads[0], clean.dot.grads[0], rows)
        gc.assert_same(gs, p.sgd_grad_sparse(single, CANARY))
        gc.assert_same(gs[rows], clean.sgd_grad_sparse(single, CANARY)[rows])
        for f in range(F):  # the table rows of the clean samples
            touched = p.classes[0][f][rows][upd[f][rows]]
            got = p.table(f, flat)[touched]
            assert np.isfinite(got).all()
            gc.assert_same(got, clean.table(f, clean_flat)[touched])
    dev.assert_inputs_untouched()


# ---- f. the SGD variant against the oracle, flags made by hand ---------------------------------------------------------
def _trip_flags(c, phase, value):
    """(f + trip + phase) % 2 with trip = b // sample_stride: for one LDS row, the two address slots alternate between
    "once" and "not once" over a wave's trips, and neighbouring rows differ."""
    trip = np.arange(c.B) // ic.sample_stride("bwd", c.B, c.D)
    return (((np.arange(c.F)[:, None] + trip[None, :] + phase) % 2) * value).astype(np.uint8).reshape(-1)


@pytest.mark.parametrize("name", gc.SGD_LAYOUTS)
@pytest.mark.parametrize("F", gc.SGD_F)
@pytest.mark.parametrize("D", gc.DIMS)
def test_sgd_flag_patterns_against_the_oracle(D, F, name):
    """No flag, every flag, and the two alternating patterns, with 1, 7 and 255 for "set"."""
    lib = _lib.load()
    c = gc.case(gc.LOOP_B, F, D, distinct=True)
    assert ic.trips("bwd", c.B, D) == 3
    dev = gc.Device(c)
    patterns = (_all_flags(c, 0), _all_flags(c, 1), _trip_flags(c, 0, 7), _trip_flags(c, 1, 255))
    assert [int((s != 0).sum()) for s in patterns[:2]] == [0, F * c.B]
    assert ((patterns[2] != 0) ^ (patterns[3] != 0)).all()
    for single in patterns:
        assert (c.updated(single).reshape(-1) == (single != 0)).all()  # distinct local ids: flagged means updated
        _check_sgd(lib, c, (name,), single, dev, twice=True)


@functools.lru_cache(maxsize=1)
def _flagged_misses_case(F, D):
    base = gc.case(gc.LOOP_B, F, D, distinct=True)
    lo = np.full(F, 3, dtype=np.int64)
    window = np.stack([lo, lo + base.rows + 11], axis=1)
    ids = base.ids + 3
    stride = ic.sample_stride("bwd", base.B, D)
    misses = [(0, 0, -1), (F - 1, 1, gc.ID_SKIP), (F // 2, 1 + stride, 0), (F - 1, 1 + 2 * stride, int(window[F - 1, 1])),
              (0, stride, 2), (F - 1, base.B - 1, 1 << 40), (0, base.B - 1 - stride, int(lo[0] + base.rows[0]))]
    for f, b, v in misses:
        ids[f, b] = v
    assert len({(f, b) for f, b, _ in misses}) == len(misses)
    return base.replace(ids=ids, window=window), [(f, b) for f, b, _ in misses]


@pytest.mark.parametrize("name", gc.SGD_LAYOUTS)
@pytest.mark.parametrize("F", gc.SGD_F)
@pytest.mark.parametrize("D", gc.DIMS)
def test_sgd_flagged_misses_touch_no_table(D, F, name):
    """Every flag set while a handful of ids are bad, skipped or another shard's: such a contribution goes to grad_sparse
    as usual (the gradient of a zero row) and no table element changes for it."""
    c, where = _flagged_misses_case(F, D)
    single = np.array([1, 7, 255], dtype=np.uint8)[np.arange(F * c.B) % 3]
    upd = c.updated(single)
    assert upd.sum() == F * c.B - len(where) and not any(upd[f, b] for f, b in where) and c.bad == 3
    _check_sgd(_lib.load(), c, (name,), single, twice=True)


def test_sgd_leaves_rows_touched_more_than_once_alone():
    """A batch with duplicates (1-, 3-, 1000- and 5000-row tables), flags by the numpy rule the flag kernel is tested
    against: the rows touched once are updated, every other row keeps its bits and its gradient goes to grad_sparse."""
    from test_single_row_update_gpu import _expected_flags

    B, F, D = gc.LOOP_B, 16, 128
    c = gc.case(B, F, D, rows=gc.duplicate_rows(F))
    shim = types.SimpleNamespace(F=F, B=B, rows=c.rows.tolist(), feat_window=None)
    single = _expected_flags(shim, torch.from_numpy(c.ids.reshape(-1).copy()))
    upd = c.updated(single)
    assert (upd.reshape(-1) == (single != 0)).all() and 0 < upd.sum() < F * B
    assert not upd[0].any() and not upd[1].any() and upd[3].any()  # 1 and 3 rows: none once; 5000 rows: some
    flat = _check_sgd(_lib.load(), c, ("dense", "odd"), single, twice=True)
    changed = np.zeros(c.flat.size, dtype=bool)
    for f in range(F):
        c.table(f, changed)[c.classes[0][f][upd[f]]] = True
    gc.assert_same(flat[~changed], c.flat[~changed])
