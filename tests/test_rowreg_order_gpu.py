"""GPU: the summation ORDERS of the row-in-registers kernels (csrc/rowreg.hpp: VectorCrossNet, SwishLayerNorm), bit for bit
through the C ABI (include/tbe_hip.h) against the numpy float32 host model tests/_rowreg_order.py, every output and workspace
between guard elements that must stay untouched.

The inputs are ordinary float32 numbers: another order of the same adds gives other bits (tests/test_rowreg_order.py asserts
that for these very inputs).  SwishLayerNorm runs with gamma = beta = 0, where the sigmoid is 0.5 and nothing else depends
on expf; the random-parameter path is held by tests/test_swish_layernorm_abi_gpu.py within its tolerance."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _rowreg_order as ro
import _swish_layernorm_ref as sr
from _guarded import Buf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

OK = 0


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("B,N,L", ro.VECTOR_SHAPES)
def test_vector_cross_is_bit_equal_to_the_order_model(B, N, L):
    """The kernels hold no transcendental and every operation is rounded on its own: out, s, grad_in and all 2 L N parameter
    gradients are the model's, the row-block partial sums in the workspace too."""
    lib = _lib.load()
    c = ro.vector_case(B, N, L)
    m = c["model"]
    bx, bw, bb, bg = Buf(B * N, c["x"]), Buf(L * N, c["w"]), Buf(L * N, c["b"]), Buf(B * N, c["g"])
    bout, bs, bgin, bgp = Buf(B * N), Buf(L * B), Buf(B * N), Buf(2 * L * N)
    rc = lib.tbe_vector_cross_forward_f32(bx.ptr, bw.ptr, bb.ptr, B, N, L, bout.ptr, bs.ptr, _stream())
    assert rc == OK, lib.tbe_last_error()
    wbytes = lib.tbe_vector_cross_backward_workspace_bytes(B, N, L)
    bws = Buf(wbytes // 4)
    rc = lib.tbe_vector_cross_backward_f32(bg.ptr, bx.ptr, bs.ptr, bw.ptr, bb.ptr, B, N, L, bgin.ptr, bgp.ptr, bws.ptr, wbytes,
                                           _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bs.get((L, B)), m["s"])
    np.testing.assert_array_equal(bout.get((B, N)), m["out"])
    np.testing.assert_array_equal(bws.get()[:m["partial"].size], m["partial"].reshape(-1))
    np.testing.assert_array_equal(bgp.get((2 * L, N)), m["grad_params"])
    np.testing.assert_array_equal(bgin.get((B, N)), m["grad_in"])
    for buf, src in ((bx, c["x"]), (bw, c["w"]), (bb, c["b"]), (bg, c["g"])):
        np.testing.assert_array_equal(buf.get(), src.reshape(-1))  # inputs are not modified


@pytest.mark.parametrize("B,N", ro.SLN_SHAPES)
def test_swish_layernorm_sums_are_bit_equal_to_the_order_model(B, N):
    """mean and rstd (two-pass row sums, IEEE division, 1 / sqrtf) hold for any input.  With gamma = beta = 0 the sigmoid is
    1 / (1 + expf(-0)): `out == y * 0.5` is asserted first, as the precondition of the rest — then grad_gamma (column sums of
    dz * n), grad_beta (column sums of dz = ((g * y) * 0.5) * 0.5) and grad_y are the model's: the column-sum finish at all
    three threads-per-row classes."""
    lib = _lib.load()
    c = ro.sln_case(B, N)
    m = c["model"]
    zeros = np.zeros(N, dtype=np.float32)
    by, bga, bbe, bg = Buf(B * N, c["y"]), Buf(N, zeros), Buf(N, zeros), Buf(B * N, c["g"])
    bout, bst, bgy, bgp = Buf(B * N), Buf(2 * B), Buf(B * N), Buf(2 * N)
    rc = lib.tbe_swish_layernorm_forward_f32(by.ptr, bga.ptr, bbe.ptr, sr.EPS, B, N, bout.ptr, bst.ptr, _stream())
    assert rc == OK, lib.tbe_last_error()
    wbytes = lib.tbe_swish_layernorm_backward_workspace_bytes(B, N)
    bws = Buf(wbytes // 4)
    rc = lib.tbe_swish_layernorm_backward_f32(bg.ptr, by.ptr, bst.ptr, bga.ptr, bbe.ptr, B, N, bgy.ptr, bgp.ptr, bws.ptr, wbytes,
                                              _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    st = bst.get((2, B))
    np.testing.assert_array_equal(st[0], m["mean"])
    np.testing.assert_array_equal(st[1], m["rstd"])
    np.testing.assert_array_equal(bout.get((B, N)), c["y"] * np.float32(0.5), err_msg="precondition: expf(-0) == 1")
    np.testing.assert_array_equal(bws.get()[:m["partial"].size], m["partial"].reshape(-1))
    np.testing.assert_array_equal(bgp.get((2, N)), m["grad_params"])
    np.testing.assert_array_equal(bgy.get((B, N)), m["grad_y"])
    for buf, src in ((by, c["y"]), (bg, c["g"])):
        np.testing.assert_array_equal(buf.get(), src.reshape(-1))
