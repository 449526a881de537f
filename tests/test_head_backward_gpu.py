"""GPU: the head backward kernel through the C ABI (include/tbe_hip.h tbe_relu_linear1_backward[_partials]_f32), bit for bit
against the numpy float32 host model tests/_head_backward.py and against the entries it replaces, chained on the same device
buffers: tbe_weighted_colsum_partials_f32(act, dy) and tbe_relu_backward_bias_partials_f32 fed torch's dy w.  Every output and
workspace sits between guard elements that must stay untouched; inputs are not modified."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _colsum_order as co
import _head_backward as hb
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
def test_head_backward_equals_the_model_and_the_entries_it_replaces(B, N):
    lib = _lib.load()
    c = hb.case(B, N)
    nrb = lib.tbe_colsum_row_blocks(B, N)
    assert nrb == co.row_blocks(B, N)
    bact, bdy, bw = Buf(B * N, c["act"]), Buf(B, c["dy"]), Buf(N, c["w"])
    # first stage alone
    bgx, bpart = Buf(B * N), Buf(nrb * 2 * N)
    _done(lib, lib.tbe_relu_linear1_backward_partials_f32(bact.ptr, bdy.ptr, bw.ptr, B, N, bgx.ptr, bpart.ptr, 4 * nrb * 2 * N,
                                                          _stream()))
    gx, part = bgx.get((B, N)), bpart.get((nrb, 2 * N))
    np.testing.assert_array_equal(gx, c["gx"])
    np.testing.assert_array_equal(part[:, :N], c["partial"][:, :N])
    np.testing.assert_array_equal(part[:, N:], c["partial"][:, N:])
    # one pass: the same first stage, finished over 2 N columns
    bgx1, bsums = Buf(B * N), Buf(2 * N)
    wbytes = lib.tbe_relu_linear1_backward_workspace_bytes(B, N)
    bws = Buf(wbytes // 4)
    _done(lib, lib.tbe_relu_linear1_backward_f32(bact.ptr, bdy.ptr, bw.ptr, B, N, bgx1.ptr, bsums.ptr, bws.ptr, wbytes, _stream()))
    np.testing.assert_array_equal(bgx1.get((B, N)), c["gx"])
    sums = bsums.get()
    np.testing.assert_array_equal(sums, c["sums"])
    bws.get()  # guards round the workspace
    # the entries it replaces, on the same device buffers
    bwpart = Buf(nrb * N)
    _done(lib, lib.tbe_weighted_colsum_partials_f32(bact.ptr, bdy.ptr, B, N, bwpart.ptr, 4 * nrb * N, _stream()))
    np.testing.assert_array_equal(bwpart.get((nrb, N)), part[:, N:])
    dev_dy = torch.from_numpy(c["dy"]).cuda()
    dev_w = torch.from_numpy(c["w"]).cuda()
    outer = dev_dy[:, None] @ dev_w[None, :]  # the K = 1 GEMM of the two-node backward
    bouter = Buf(B * N, outer.cpu().numpy())
    bgx2, bbpart, bgb = Buf(B * N), Buf(nrb * N), Buf(N)
    _done(lib, lib.tbe_relu_backward_bias_partials_f32(bouter.ptr, bact.ptr, B, N, bgx2.ptr, bbpart.ptr, 4 * nrb * N, _stream()))
    np.testing.assert_array_equal(bgx2.get((B, N)), gx)
    np.testing.assert_array_equal(bbpart.get((nrb, N)), part[:, :N])
    wb = lib.tbe_relu_backward_bias_grad_workspace_bytes(B, N)
    bws2 = Buf(wb // 4)
    _done(lib, lib.tbe_relu_backward_bias_grad_f32(bouter.ptr, bact.ptr, B, N, bgx2.ptr, bgb.ptr, bws2.ptr, wb, _stream()))
    np.testing.assert_array_equal(bgb.get(), sums[:N])
    bout = Buf(N)
    ww = lib.tbe_weighted_colsum_workspace_bytes(B, N)
    bws3 = Buf(ww // 4)
    _done(lib, lib.tbe_weighted_colsum_f32(bact.ptr, bdy.ptr, B, N, bout.ptr, bws3.ptr, ww, _stream()))
    np.testing.assert_array_equal(bout.get(), sums[N:])
    for b, src, shape in ((bact, c["act"], (B, N)), (bdy, c["dy"], None), (bw, c["w"], None)):
        np.testing.assert_array_equal(b.get(shape), src)  # inputs are not modified


def test_one_pass_of_an_empty_batch_gives_zeros():
    lib = _lib.load()
    N = 8
    bsums = Buf(2 * N)
    wbytes = lib.tbe_relu_linear1_backward_workspace_bytes(0, N)
    bws = Buf(wbytes // 4)
    _done(lib, lib.tbe_relu_linear1_backward_f32(None, None, None, 0, N, None, bsums.ptr, bws.ptr, wbytes, _stream()))
    np.testing.assert_array_equal(bsums.get(), np.zeros(2 * N, dtype=np.float32))
