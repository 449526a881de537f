"""CPU: the two gather-interaction entry points (include/tbe_hip.h) are exported and refuse bad arguments before any
launch; the numpy lookup and the SGD expectation of tests/_gather_cases.py agree with the oracle, and its shape lists reach
what tests/test_gather_interaction_abi_gpu.py claims."""
from fractions import Fraction

import numpy as np

import _paths  # noqa: F401
import _gather_cases as gc
import _interaction_cases as ic
from fbgemm_gpu import _lib
from oracle import oracle

FWD = "tbe_dlrm_interaction_gather_forward_f32"
BWD = "tbe_dlrm_interaction_gather_backward_f32"


def test_gather_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name in (FWD, BWD):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.tbe_abi_version() == 3


def _fwd(lib, B=4, F=26, D=128, stride=479, ptr=16):
    return lib.tbe_dlrm_interaction_gather_forward_f32(ptr, ptr, ptr, None, ptr, B, F, D, ptr, stride, None, None)


def _bwd(lib, B=4, F=26, D=128, stride=479, ptr=16):
    return lib.tbe_dlrm_interaction_gather_backward_f32(ptr, ptr, ptr, None, ptr, ptr, stride, B, F, D, ptr, ptr, None, None)


def test_gather_entry_points_validate_before_any_launch():
    lib = _lib.load()
    for call in (_fwd, _bwd):
        assert call(lib, F=28) == -1 and b"F=28" in lib.tbe_last_error()
        assert call(lib, F=0) == -1
        assert call(lib, D=48) == -1 and b"D=48" in lib.tbe_last_error()
        assert call(lib, stride=478) == -1 and b"stride" in lib.tbe_last_error()
        assert call(lib, ptr=None) == -1 and b"null pointer" in lib.tbe_last_error()
        assert call(lib, ptr=20) == -1 and b"aligned" in lib.tbe_last_error()
        assert call(lib, B=0) == 0  # an empty batch launches nothing


# ---- the cases of tests/test_gather_interaction_abi_gpu.py (tests/_gather_cases.py) -----------------------------------
def test_numpy_lookup_equals_the_oracles():
    """The restatement of classify_id that every expected result of the GPU file starts from, against oracle.tbe_forward
    (pooled, one id per bag) on a windowless case with bad and skipped ids: the rows and the count.  The oracle knows no
    skip id: it counts TBE_ID_SKIP like any other negative id, so its count is the restatement's plus the skipped ids."""
    B, F, D = 300, 7, 64
    base = gc.case(B, F, D)
    ids = base.ids.copy()
    bad = [(0, 5, -1), (1, 17, 3), (2, 0, 40), (3, 299, 1 << 40), (6, 100, (1 << 63) - 1), (2, 64, -77), (6, 0, 1 << 32)]
    skipped = [(0, 9), (4, 250), (6, 299)]
    for f, b, v in bad:
        ids[f, b] = v
    for f, b in skipped:
        ids[f, b] = gc.ID_SKIP
    c = base.replace(ids=ids)
    tabs = oracle.Tables(c.rows.tolist(), [D] * F)
    tabs.weights = [np.ascontiguousarray(c.table(f)) for f in range(F)]
    pooled, counted = oracle.tbe_forward(tabs, c.ids.reshape(-1), np.arange(F * B + 1, dtype=np.int64))
    np.testing.assert_array_equal(c.sparse, pooled.reshape(B, F, D))
    assert c.bad == len(bad) and counted == c.bad + len(skipped)
    for f, b in [(f, b) for f, b, _ in bad] + skipped:
        assert not c.sparse[b, f].any()
    assert c.classes[1].sum() == F * B - len(bad) - len(skipped)


def test_numpy_lookup_with_row_windows():
    """Hand-made ids round a window whose first global row is above 2^32: what is local, silent and counted."""
    F, B, D = 2, 8, 64
    base = gc.make(B, F, D, (4, 4))
    lo = gc.BIG_LO
    ids = np.array([[lo, lo + 3, lo + 4, lo - 1, 3, -1, lo + 20, gc.ID_SKIP],
                    [0, 3, 4, 9, 10, -1, 1 << 40, gc.ID_SKIP]], dtype=np.int64)
    c = base.replace(ids=ids, window=[(lo, lo + 20), (0, 10)])
    local, is_local, counted = c.classes
    np.testing.assert_array_equal(is_local, [[1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0, 0]])
    np.testing.assert_array_equal(counted, [[0, 0, 0, 0, 0, 1, 1, 0], [0, 0, 0, 0, 1, 1, 1, 0]])
    np.testing.assert_array_equal(local[is_local], [0, 3, 0, 3])
    np.testing.assert_array_equal(c.sparse[1, 0], c.table(0)[3])
    assert c.bad == 5 and not c.sparse[2:].any()


def _is_nearest_float32(r, exact):
    """No float32 is closer to the rational `exact` than r."""
    err = abs(exact - Fraction(float(r)))
    return all(err <= abs(exact - Fraction(float(np.nextafter(r, np.float32(to))))) for to in (-np.inf, np.inf))


def test_sgd_expectation_is_one_fmaf_on_the_flagged_local_rows():
    """sgd_flat changes exactly the rows of flagged local contributions, and by fmaf(-lr, g, w): the float32 nearest to
    the exact w - lr * g (rational arithmetic), which float64 arithmetic followed by a second rounding need not give."""
    B, F, D = 40, 3, 64
    base = gc.case(B, F, D, distinct=True)
    ids = base.ids.copy()
    ids[0, 0], ids[1, 1], ids[2, 2] = -1, gc.ID_SKIP, B + 5
    c = base.replace(ids=ids)
    single = (np.arange(F * B) % 3 != 1).astype(np.uint8) * 255
    single[[0, B + 1, 2 * B + 2]] = 1  # flagged misses
    upd = c.updated(single)
    assert upd.sum() == (single != 0).sum() - 3
    flat, gs = c.sgd_flat(single), c.dot.grads[1]
    np.testing.assert_array_equal(flat, c.sgd_flat(single))
    lr = Fraction(float(np.float32(gc.LR)))
    for f in range(F):
        touched = np.zeros(c.rows[f], dtype=bool)
        for b in np.nonzero(upd[f])[0]:
            row = c.ids[f, b]
            touched[row] = True
            for got, g, w in zip(c.table(f, flat)[row], gs[b, f], c.table(f)[row]):
                assert _is_nearest_float32(got, Fraction(float(w)) - lr * Fraction(float(g)))
            assert not np.array_equal(c.table(f, flat)[row], c.table(f)[row])
        np.testing.assert_array_equal(c.table(f, flat)[~touched], c.table(f)[~touched])
    want_gs = c.sgd_grad_sparse(single, np.float32(-1.5))
    np.testing.assert_array_equal((want_gs == -1.5).all(axis=2), upd.T)
    np.testing.assert_array_equal(want_gs[~upd.T], gs[~upd.T])


def test_gather_case_lists_reach_what_the_gpu_file_claims():
    assert gc.DIMS == (64, 128) and gc.MAX_F == 27 and gc.LOOP_B == 4101
    assert all(ic.forward_kernel(D) == "glds" and ic.grid_cap(k, D) == 512 for D in gc.DIMS for k in ("fwd", "bwd"))
    # the named layouts take the scalar path (counted stores) on both sides of the second row tile, R = 16 | 17 ...
    for D in gc.DIMS:
        for F in (15, 16):
            assert F in gc.LOOP_F
            assert ic.pairs(F) % 4 == 0  # "dense" rows are 16-B rows here (the strides 248 and 200 of the older GPU file)
            for name in ("odd", "shifted"):
                _, stride, shift = ic.layout(F, D, name)
                assert name in ic.LAYOUTS and not ic.vector_path(F, D, stride, shift)
            for name in ("dense", "padded", "wide"):
                _, stride, shift = ic.layout(F, D, name)
                assert ic.vector_path(F, D, stride, shift)
    # ... and "odd", which the every-F and the id tests use, takes it at every F
    for D in gc.DIMS:
        for F in range(1, gc.MAX_F + 1):
            _, stride, shift = ic.layout(F, D, "odd")
            assert not ic.vector_path(F, D, stride, shift)
    assert "odd" in gc.EVERY_F_LAYOUTS and {"dense", "padded"} <= set(gc.EVERY_F_LAYOUTS)
    # T = ceil(P / 64) of the counted wait
    assert [ic.pair_stores(F) for F in gc.LOOP_F] == [1, 1, 2, 2, 3, 4, 5, 6]
    # trips of the longest and the shortest wave: 1, 2, 3 and 4, and every wave's end inside the id pipeline
    def trips(B, D):
        stride = ic.sample_stride("fwd", B, D)
        assert stride == ic.sample_stride("bwd", B, D)
        return ic.trips("fwd", B, D), B // stride  # the wave of sample stride - 1 is the last to start
    assert trips(gc.EVERY_F_B, 64) == (1, 0) and all(trips(B, D)[0] == 1 for B in gc.FEW_B for _, D in gc.FEW_SHAPES)
    assert [trips(B, D) for B, _, D, _ in gc.TRIP_EDGES] == [(2, 1), (4, 3)]
    assert all(trips(gc.LOOP_B, D) == (3, 2) for D in gc.DIMS)
    assert all(B == gc.LOOP_B for B, _, _ in gc.ID_EDGE_SHAPES + gc.ISOLATION)
    assert {name for *_, name in gc.TRIP_EDGES} == {"odd"} and {(F, D) for _, F, D, _ in gc.TRIP_EDGES} == {(16, 128)}
    # fewer samples than waves on both sides of the second row tile
    assert gc.FEW_B == (1, 3, 5) and set(gc.FEW_SHAPES) == {(16, 128), (15, 64)} == {(F, D) for _, F, D in gc.ISOLATION}
    # rows per table: some shared by every sample, some nearly distinct; the SGD tables leave room for distinct ids
    assert gc.row_cycle(9, 5) == (1, 3, 40, 14, 1) and set(gc.distinct_rows(9, 3)) == {14}
    c = gc.case(9, 5, 64, distinct=True)
    assert all(len(set(c.ids[f])) == 9 for f in range(5)) and c.bad == 0 and c.classes[1].all()
    assert gc.SGD_F == (1, 16, 27) and gc.SGD_LAYOUTS == ("dense", "padded", "shifted") and gc.LR == 0.05
    assert gc.BIG_LO == (1 << 33) + 5
