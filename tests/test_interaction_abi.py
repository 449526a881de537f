"""CPU: the two dense dot-interaction entry points (include/tbe_hip.h) are exported and refuse bad arguments before any
launch; the shape lists of tests/test_interaction_abi_gpu.py reach what they claim to; the oracle keeps non-finite values
inside their sample (so the GPU isolation test compares against something that has the property)."""
import numpy as np

import _paths  # noqa: F401
import _interaction_cases as ic
from fbgemm_gpu import _lib

FWD = "tbe_dlrm_interaction_forward_f32"
BWD = "tbe_dlrm_interaction_backward_f32"


def test_dense_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name in (FWD, BWD):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def _fwd(lib, B=4, F=26, D=128, stride=479, ptr=16, inp=None):
    inp = ptr if inp is None else inp
    return lib.tbe_dlrm_interaction_forward_f32(inp, inp, B, F, D, ptr, stride, None)


def _bwd(lib, B=4, F=26, D=128, stride=479, ptr=16, inp=None):
    inp = ptr if inp is None else inp
    return lib.tbe_dlrm_interaction_backward_f32(inp, inp, ptr, stride, B, F, D, inp, inp, None)


def test_dense_entry_points_validate_before_any_launch():
    lib = _lib.load()
    for call, too_many in ((_fwd, 32), (_bwd, 28)):
        assert call(lib, F=0) == -1 and b"F=0 outside" in lib.tbe_last_error()
        assert call(lib, F=too_many, stride=1 << 20) == -1 and b"F=%d outside" % too_many in lib.tbe_last_error()
        assert call(lib, D=48) == -1 and b"D=48 not in" in lib.tbe_last_error()
        assert call(lib, stride=478) == -1 and b"stride 478 <" in lib.tbe_last_error()
        assert call(lib, ptr=None) == -1 and b"null pointer" in lib.tbe_last_error()
        assert call(lib, inp=20) == -1 and b"16-B aligned" in lib.tbe_last_error()
        assert call(lib, B=-1) == -1 and b"outside" in lib.tbe_last_error()
        assert call(lib, B=0) == 0  # an empty batch launches nothing
    # the ranges differ: what the forward takes, the backward refuses
    assert _bwd(lib, D=256, stride=1 << 20) == -1 and b"D=256 not in" in lib.tbe_last_error()
    assert _bwd(lib, F=28, stride=1 << 20) == -1 and b"F=28 outside" in lib.tbe_last_error()
    assert _fwd(lib, B=0, F=31, D=256, stride=256 + 496) == 0


def test_layouts_take_the_paths_they_are_named_for():
    for D in ic.FWD_DIMS:
        for F in range(1, ic.FWD_MAX_F + 1):
            P, P4 = ic.pairs(F), ic.pairs4(F)
            lay = {name: (stride, shift) for name, stride, shift in ic.layouts(F, D)}
            assert tuple(lay) == ic.LAYOUTS
            assert all(stride >= D + P for stride, _ in lay.values())
            assert ic.vector_path(F, D, *lay["dense"]) == (P % 4 == 0)
            assert ic.vector_path(F, D, *lay["padded"]) and ic.vector_path(F, D, *lay["wide"])
            assert lay["wide"][0] > D + P4
            assert lay["odd"][0] % 4 != 0 and lay["odd"][0] > D + P and not ic.vector_path(F, D, *lay["odd"])
            assert lay["shifted"] == (D + P4, 4) and not ic.vector_path(F, D, *lay["shifted"])


def test_case_lists_cover_every_edge_of_the_kernels():
    # every R of both directions, in a register-form and an LDS-DMA forward
    assert {ic.forward_kernel(D) for D in ic.EVERY_R_DIMS} == {"register", "glds"}
    # multi-trip batches for all nine instantiations: forward 16, 32, 256 (register), 64, 128 (LDS-DMA), backward <1,2,4,8>
    assert {D for _, _, D in ic.FWD_LOOP} == set(ic.FWD_DIMS) and {D for _, _, D in ic.BWD_LOOP} == set(ic.BWD_DIMS)
    for kind, shapes in (("fwd", ic.FWD_LOOP), ("bwd", ic.BWD_LOOP)):
        for B, F, D in shapes:
            stride = ic.sample_stride(kind, B, D)
            assert stride == 4 * ic.grid_cap(kind, D) and B == 2 * stride + 5 and ic.trips(kind, B, D) == 3
    assert {B for B, _, D in ic.FWD_LOOP if D in (16, 32)} == {8197}
    assert {B for B, _, D in ic.FWD_LOOP if D in (64, 128, 256)} == {4101}
    assert {B for B, _, _ in ic.BWD_LOOP} == {4101}
    # both sides of the second row tile (R = 16 | 17) and the largest R in every instantiation
    for D in ic.FWD_DIMS:
        assert {15, 16, 31} <= {F for _, F, d in ic.FWD_LOOP if d == D}
    for D in ic.BWD_DIMS:
        assert {15, 16, 27} <= {F for _, F, d in ic.BWD_LOOP if d == D}
    # the counted wait of the LDS-DMA forward: every T = 1 .. 8 with a looping wave on a scalar-path layout
    for D in (64, 128):
        reached = set()
        for B, F, d in ic.FWD_LOOP:
            scalar = [name for name, stride, shift in ic.layouts(F, d) if not ic.vector_path(F, d, stride, shift)]
            assert {"odd", "shifted"} <= set(scalar)
            if d == D and B > 2048:
                reached.add(ic.pair_stores(F))
        assert reached == set(range(1, 9))
    # isolation: a wave that meets a poisoned sample first and clean ones after it, and one the other way round
    for B, F, D in ic.ISOLATION:
        for kind in ("fwd", "bwd") if ic.supports_backward(F, D) else ("fwd",):
            s, stride = ic.poisoned_samples(kind, B, D), ic.sample_stride(kind, B, D)
            assert {7, 7 + stride, B - 1} <= set(s) and len(s) == 4
            assert 2 in s and 2 + stride not in s and 2 + 2 * stride not in s and 2 + 2 * stride < B
            assert (B - 1) % stride not in s and (B - 1) % stride + stride not in s


def test_oracle_keeps_nonfinite_values_in_their_sample():
    B, F, D = 12, 5, 16
    clean = ic.case(B, F, D)
    samples = [2, 7, B - 1]
    p = ic.poison(clean, samples)
    rows = np.setdiff1d(np.arange(B), samples)
    for got, ref in ((p.out, clean.out), (p.grads[0], clean.grads[0]), (p.grads[1], clean.grads[1])):
        assert np.isfinite(got[rows]).all()
        np.testing.assert_array_equal(got[rows], ref[rows])
    c = ic.POISON_COL
    iu = np.triu_indices(F + 1, k=1)
    for b in samples:
        r = 1 + b % F  # the row of X that holds the NaN
        # forward: +Inf passes through, every pair with row r is NaN, no other pair is
        assert p.out[b, c] == np.inf
        np.testing.assert_array_equal(np.isnan(p.out[b, D:]), (iu[0] == r) | (iu[1] == r))
        # backward: NaN in exactly one column of every gradient row of the sample
        g = np.concatenate([p.grads[0][b][None], p.grads[1][b]])
        expect = np.zeros((F + 1, D), dtype=bool)
        expect[:, c] = True
        np.testing.assert_array_equal(np.isnan(g), expect)
