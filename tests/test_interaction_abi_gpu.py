"""GPU: the two dense dot-interaction entry points (tbe_dlrm_interaction_forward_f32 / _backward_f32, include/tbe_hip.h)
through the C ABI, bit for bit against oracle/dlrm_oracle.c at every tile and loop edge of csrc/dlrm_interaction.hip.

Every buffer sits between guard elements (tests/_guarded.py); an `out` buffer starts as canaries, so that every column a
call must not write is checked too; inputs are read back and must be what was uploaded; the `grad_out` buffer holds NaN
in every column from D + P on.  Shapes, layouts and what each of them reaches: tests/_interaction_cases.py."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _interaction_cases as ic
from _guarded import CANARY, Buf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

OK = 0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _done(lib, rc):
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()


class _Inputs:
    """dense and sparse of a case on the device, uploaded once for all layouts."""

    def __init__(self, c):
        self.c = c
        self.dense, self.sparse = Buf(c.dense.size, c.dense), Buf(c.sparse.size, c.sparse)

    def assert_untouched(self):
        np.testing.assert_array_equal(self.dense.get(self.c.dense.shape), self.c.dense)
        np.testing.assert_array_equal(self.sparse.get(self.c.sparse.shape), self.c.sparse)


def _forward(lib, x, name):
    """One forward of x.c in layout `name` -> the whole [B, stride] image of `out`."""
    c = x.c
    _, stride, shift = ic.layout(c.F, c.D, name)
    out = ic.RowBuf(c.B, stride, shift)
    _done(lib, lib.tbe_dlrm_interaction_forward_f32(x.dense.ptr, x.sparse.ptr, c.B, c.F, c.D, out.ptr, stride, _stream()))
    return out.get(), stride, shift


def _backward(lib, x, name):
    """One backward of x.c with grad_out in layout `name` -> grad_dense [B, D], grad_sparse [B, F, D]."""
    c = x.c
    _, stride, shift = ic.layout(c.F, c.D, name)
    image = ic.grad_image(c, stride)
    g = ic.RowBuf(c.B, stride, shift, image)
    gd, gs = Buf(c.B * c.D), Buf(c.B * c.F * c.D)
    _done(lib, lib.tbe_dlrm_interaction_backward_f32(x.dense.ptr, x.sparse.ptr, g.ptr, stride, c.B, c.F, c.D, gd.ptr,
                                                     gs.ptr, _stream()))
    np.testing.assert_array_equal(g.get(), image)  # grad_out is an input
    return gd.get((c.B, c.D)), gs.get((c.B, c.F, c.D))


def _check_forward(lib, c, names):
    x = _Inputs(c)
    for name in names:
        image, stride, shift = _forward(lib, x, name)
        np.testing.assert_array_equal(image, ic.expected_out(c, stride, shift), err_msg=f"F={c.F} D={c.D} {name}")
    x.assert_untouched()


def _check_backward(lib, c, names):
    x = _Inputs(c)
    for name in names:
        gd, gs = _backward(lib, x, name)
        np.testing.assert_array_equal(gd, c.grads[0], err_msg=f"F={c.F} D={c.D} {name}")
        np.testing.assert_array_equal(gs, c.grads[1], err_msg=f"F={c.F} D={c.D} {name}")
    x.assert_untouched()


# ---- 1. every R ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ic.EVERY_R_DIMS)
def test_forward_every_row_count(D):
    """F = 1 .. 31: triu_index for every R, the pad-zeroing for every P mod 4, both sides of R = 16 | 17."""
    lib = _lib.load()
    for F in range(1, ic.FWD_MAX_F + 1):
        _check_forward(lib, ic.case(ic.EVERY_R_B, F, D), ("dense", "padded"))


@pytest.mark.parametrize("D", ic.EVERY_R_DIMS)
def test_backward_every_row_count(D):
    """F = 1 .. 27: triu_row (float sqrtf + integer correction) for every pair of every R."""
    lib = _lib.load()
    for F in range(1, ic.BWD_MAX_F + 1):
        _check_backward(lib, ic.case(ic.EVERY_R_B, F, D), ("dense", "padded"))


# ---- 2. loop edges x tile edges x layouts ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,D", ic.FWD_LOOP)
def test_forward_three_trips_in_every_layout(B, F, D):
    """Two full trips of every wave's sample loop and a third of five waves: the prefetch, the reload of the dense
    pass-through, the rewrite of the wave's pair block and, in the LDS-DMA form, the counted wait for the next copy."""
    assert ic.trips("fwd", B, D) == 3
    _check_forward(_lib.load(), ic.case(B, F, D), ic.LAYOUTS)


@pytest.mark.parametrize("B,F,D", ic.BWD_LOOP)
def test_backward_three_trips_in_every_layout(B, F, D):
    assert ic.trips("bwd", B, D) == 3
    _check_backward(_lib.load(), ic.case(B, F, D), ic.LAYOUTS)


# ---- 3. fewer samples than waves -------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,D", ic.FEW_SHAPES)
@pytest.mark.parametrize("B", ic.FEW_B)
def test_fewer_samples_than_waves(B, F, D):
    """Waves with b >= B do nothing; at B = 5 the second block runs with one active wave."""
    lib = _lib.load()
    c = ic.case(B, F, D)
    _check_forward(lib, c, ic.LAYOUTS)
    _check_backward(lib, c, ic.LAYOUTS)


@pytest.mark.parametrize("F,D", ic.FEW_SHAPES)
def test_empty_batch_returns_ok_and_writes_nothing(F, D):
    lib = _lib.load()
    stride = D + ic.pairs4(F)
    x, out, g = Buf(4 * F * D), Buf(4 * stride), Buf(4 * stride)
    gd, gs = Buf(4 * D), Buf(4 * F * D)
    _done(lib, lib.tbe_dlrm_interaction_forward_f32(x.ptr, x.ptr, 0, F, D, out.ptr, stride, _stream()))
    _done(lib, lib.tbe_dlrm_interaction_backward_f32(x.ptr, x.ptr, g.ptr, stride, 0, F, D, gd.ptr, gs.ptr, _stream()))
    for b in (x, out, g, gd, gs):
        assert (b.all() == CANARY).all()


# ---- 4. isolation ----------------------------------------------------------------------------------------------------
def _assert_isolated(got, poisoned_ref, clean_ref, clean_rows):
    np.testing.assert_array_equal(got, poisoned_ref)
    assert np.isfinite(got[clean_rows]).all()
    np.testing.assert_array_equal(got[clean_rows], clean_ref[clean_rows])


@pytest.mark.parametrize("B,F,D", ic.ISOLATION)
def test_nonfinite_values_stay_in_their_sample(B, F, D):
    """A wave keeps an LDS image across samples and holds the next sample in registers: NaN and Inf of one sample must
    not reach another.  Poisoned: a sample whose wave goes on to clean ones, a sample and its wave's next, the last."""
    lib = _lib.load()
    clean = ic.case(B, F, D)
    W = D + ic.pairs(F)
    for kind in ("fwd", "bwd") if ic.supports_backward(F, D) else ("fwd",):
        samples = ic.poisoned_samples(kind, B, D)
        assert samples[0] + 2 * ic.sample_stride(kind, B, D) < B  # two clean samples follow the first poisoned one
        p = ic.poison(clean, samples)
        rows = np.setdiff1d(np.arange(B), samples)
        x = _Inputs(p)
        for name in ("dense", "padded"):
            if kind == "fwd":
                image, stride, shift = _forward(lib, x, name)
                np.testing.assert_array_equal(image, ic.expected_out(p, stride, shift))
                _assert_isolated(image[:, :W], p.out, clean.out, rows)
            else:
                gd, gs = _backward(lib, x, name)
                _assert_isolated(gd, p.grads[0], clean.grads[0], rows)
                _assert_isolated(gs, p.grads[1], clean.grads[1], rows)
        x.assert_untouched()
