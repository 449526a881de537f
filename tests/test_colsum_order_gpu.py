"""GPU: the summation ORDER of the row-block column sums, bit for bit through the C ABI (include/tbe_hip.h) against the numpy
float32 host model tests/_colsum_order.py, every output and workspace between guard elements that must stay untouched.

The inputs are ordinary float32 numbers (the weighted entry's have short significands, so that fmaf has an exact float64
model): another order of the same adds gives other bits (tests/test_colsum_order.py asserts that for these very inputs)."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _colsum_order as co
from _guarded import Buf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

OK = 0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _done(lib, rc):
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,N", co.SHAPES)
def test_relu_backward_bias_grad_and_partials(B, N):
    lib = _lib.load()
    c = co.case(B, N)["relu"]
    bgy, bact = Buf(B * N, c["gy"]), Buf(B * N, c["act"])
    # one pass
    bgx, bgb = Buf(B * N), Buf(N)
    wbytes = lib.tbe_relu_backward_bias_grad_workspace_bytes(B, N)
    bws = Buf(wbytes // 4)
    _done(lib, lib.tbe_relu_backward_bias_grad_f32(bgy.ptr, bact.ptr, B, N, bgx.ptr, bgb.ptr, bws.ptr, wbytes, _stream()))
    np.testing.assert_array_equal(bgx.get((B, N)), c["gx"])
    np.testing.assert_array_equal(bgb.get(), c["bias_grad"])
    bws.get()  # guards round the workspace
    # first stage alone
    nrb = lib.tbe_colsum_row_blocks(B, N)
    assert nrb == co.row_blocks(B, N)
    bgx, bpart = Buf(B * N), Buf(nrb * N)
    _done(lib, lib.tbe_relu_backward_bias_partials_f32(bgy.ptr, bact.ptr, B, N, bgx.ptr, bpart.ptr, 4 * nrb * N, _stream()))
    np.testing.assert_array_equal(bgx.get((B, N)), c["gx"])
    np.testing.assert_array_equal(bpart.get((nrb, N)), c["partial"])
    for b, src in ((bgy, c["gy"]), (bact, c["act"])):
        np.testing.assert_array_equal(b.get((B, N)), src)  # inputs are not modified


@pytest.mark.parametrize("B,N", co.SHAPES)
def test_weighted_colsum_and_partials(B, N):
    lib = _lib.load()
    c = co.case(B, N)["weighted"]
    bx, bw = Buf(B * N, c["x"]), Buf(B, c["w"])
    bout = Buf(N)
    wbytes = lib.tbe_weighted_colsum_workspace_bytes(B, N)
    bws = Buf(wbytes // 4)
    _done(lib, lib.tbe_weighted_colsum_f32(bx.ptr, bw.ptr, B, N, bout.ptr, bws.ptr, wbytes, _stream()))
    np.testing.assert_array_equal(bout.get(), c["out"])
    bws.get()
    nrb = lib.tbe_colsum_row_blocks(B, N)
    bpart = Buf(nrb * N)
    _done(lib, lib.tbe_weighted_colsum_partials_f32(bx.ptr, bw.ptr, B, N, bpart.ptr, 4 * nrb * N, _stream()))
    np.testing.assert_array_equal(bpart.get((nrb, N)), c["partial"])
    np.testing.assert_array_equal(bx.get((B, N)), c["x"])
    np.testing.assert_array_equal(bw.get(), c["w"])


@pytest.mark.parametrize("first", [1, 0], ids=["first", "accumulate"])
@pytest.mark.parametrize("B,N", co.SHAPES)
def test_cross_backward(B, N, first):
    lib = _lib.load()
    c = co.case(B, N)["cross"]
    bG, bx, bt = Buf(B * N, c["G"]), Buf(B * N, c["x0"]), Buf(B * N, c["t"])
    bgy, bacc, bgb = Buf(B * N), Buf(B * N, c["acc0"]), Buf(N)
    wbytes = lib.tbe_cross_backward_workspace_bytes(B, N)
    bws = Buf(wbytes // 4)
    _done(lib, lib.tbe_cross_backward_f32(bG.ptr, bx.ptr, bt.ptr, B, N, first, bgy.ptr, bacc.ptr, bgb.ptr, bws.ptr, wbytes,
                                          _stream()))
    np.testing.assert_array_equal(bgy.get((B, N)), c["gy"])
    np.testing.assert_array_equal(bacc.get((B, N)), c["acc"][first])
    np.testing.assert_array_equal(bgb.get(), c["bias_grad"])
    bws.get()
    for b, src in ((bG, c["G"]), (bx, c["x0"]), (bt, c["t"])):
        np.testing.assert_array_equal(b.get((B, N)), src)
