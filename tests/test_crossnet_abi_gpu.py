"""GPU: csrc/crossnet.hip straight through the C ABI (include/tbe_hip.h), every output and workspace between guard
elements that must stay untouched.

tbe_cross_backward_f32 is compared bit for bit with the float32 restatement (tests/_crossnet_ref.py): the inputs are small
integers scaled by powers of two, so every product, add and column sum is exact in float32 in any order.  The vector
kernels are compared with the float64 restatement within the tolerance measured in tests/test_crossnet.py, and run twice."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _crossnet_ref as cr
from _guarded import Buf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ints(rng, shape, scale):
    return rng.integers(-4, 5, shape).astype(np.float32) * np.float32(scale)


@pytest.mark.parametrize("first", [1, 0], ids=["first", "accumulate"])
@pytest.mark.parametrize("B,N", [(1, 4), (63, 60), (65, 64), (257, 516), (300, 128)])
def test_cross_backward_is_bit_equal_to_the_float32_restatement(B, N, first):
    """(1, 4): fewer than 16 float4 columns; (63, 60) and (65, 64): a partial row block of 64 rows, 15 / 16 float4 columns;
    (257, 516): N >= 512 (256-row blocks, one row in the second) and a column-tile tail; (300, 128): five row blocks."""
    lib = _lib.load()
    rng = np.random.default_rng([B, N, first])
    G, x0, t, acc0 = _ints(rng, (B, N), 0.25), _ints(rng, (B, N), 0.5), _ints(rng, (B, N), 0.25), _ints(rng, (B, N), 0.125)
    bG, bx, bt = Buf(B * N, G), Buf(B * N, x0), Buf(B * N, t)
    bgy, bacc, bgb = Buf(B * N), Buf(B * N, acc0), Buf(N)
    wbytes = lib.tbe_cross_backward_workspace_bytes(B, N)
    assert wbytes % 4 == 0
    bws = Buf(wbytes // 4)
    rc = lib.tbe_cross_backward_f32(bG.ptr, bx.ptr, bt.ptr, B, N, first, bgy.ptr, bacc.ptr, bgb.ptr, bws.ptr, wbytes, _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    gy, acc, gb = cr.cross_backward_f32(G, x0, t, acc0, bool(first))
    np.testing.assert_array_equal(bgy.get((B, N)), gy)
    np.testing.assert_array_equal(bacc.get((B, N)), acc)
    np.testing.assert_array_equal(bgb.get(), gb)
    bws.get()  # guards round the workspace
    for b, src in ((bG, G), (bx, x0), (bt, t)):
        np.testing.assert_array_equal(b.get((B, N)), src)  # inputs are not modified


def test_cross_backward_errors_and_the_empty_batch_change_no_byte():
    lib = _lib.load()
    B, N = 8, 8
    rng = np.random.default_rng(5)
    bufs = {k: Buf(B * N, _ints(rng, (B, N), 0.5)) for k in ("G", "x0", "t", "gy", "acc")}
    bufs["gb"] = Buf(N, np.ones(N))
    wbytes = lib.tbe_cross_backward_workspace_bytes(B, N)
    bufs["ws"] = Buf(wbytes // 4, np.ones(wbytes // 4))
    before = {k: b.all().copy() for k, b in bufs.items()}

    def call(B=B, N=N, shift=0, ws_bytes=wbytes):
        rc = lib.tbe_cross_backward_f32(bufs["G"].ptr + shift, bufs["x0"].ptr, bufs["t"].ptr, B, N, 1, bufs["gy"].ptr,
                                        bufs["acc"].ptr, bufs["gb"].ptr, bufs["ws"].ptr, ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc, lib.tbe_last_error().decode()

    rc, msg = call(N=6)
    assert rc == INVALID and "multiple of 4" in msg
    rc, msg = call(shift=4)
    assert rc == INVALID and "aligned" in msg
    rc, msg = call(ws_bytes=wbytes - 4)
    assert rc == INVALID and "workspace" in msg
    for k, b in bufs.items():
        np.testing.assert_array_equal(b.all(), before[k], err_msg=k)
    # B == 0: bias_grad is zeroed, nothing else is touched
    rc, msg = call(B=0)
    assert rc == OK, msg
    np.testing.assert_array_equal(bufs["gb"].get(), np.zeros(N, dtype=np.float32))
    for k, b in bufs.items():
        if k != "gb":
            np.testing.assert_array_equal(b.all(), before[k], err_msg=k)


def _vector_run(lib, w, b, x, g):
    """One forward and one backward through the ABI; returns the results laid out like _crossnet_ref.run's."""
    (B, N), L = x.shape, w.shape[0]
    bx, bw, bb, bg = Buf(B * N, x), Buf(L * N, w), Buf(L * N, b), Buf(B * N, g)
    bout, bs, bgin, bgp = Buf(B * N), Buf(L * B), Buf(B * N), Buf(2 * L * N)
    rc = lib.tbe_vector_cross_forward_f32(bx.ptr, bw.ptr, bb.ptr, B, N, L, bout.ptr, bs.ptr, _stream())
    assert rc == OK, lib.tbe_last_error()
    wbytes = lib.tbe_vector_cross_backward_workspace_bytes(B, N, L)
    bws = Buf(wbytes // 4)
    rc = lib.tbe_vector_cross_backward_f32(bg.ptr, bx.ptr, bs.ptr, bw.ptr, bb.ptr, B, N, L, bgin.ptr, bgp.ptr, bws.ptr, wbytes,
                                           _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    bws.get()
    gp = bgp.get((2 * L, N))
    grad = {f"bias.{l}": gp[l].reshape(N, 1) for l in range(L)}
    grad.update({f"kernels.{l}": gp[L + l].reshape(N, 1) for l in range(L)})
    return {"out": bout.get((B, N)), "s": bs.get((L, B)), "grad_input": bgin.get((B, N)), "grad": grad}


@pytest.mark.parametrize("B,N,L", cr.VECTOR_GPU_SHAPES)
def test_vector_kernels_match_the_float64_restatement_and_repeat_bit_for_bit(B, N, L):
    """(1, 4, 1): one row, one float4, one layer; (5, 12, 3) and (67, 64, 2): part of a wave, four rows in flight with a
    ragged last round; (130, 260, 3): two row blocks, two float4 slots per lane, the last one partial; (64, 1028, 4): the
    smallest width on the block-per-row kernel; (3, 4096, 8): both limits."""
    lib = _lib.load()
    p, x, g = cr.gpu_case("VectorCrossNet", B, N, L)
    w = np.stack([p[f"kernels.{l}"].reshape(N) for l in range(L)])
    b = np.stack([p[f"bias.{l}"].reshape(N) for l in range(L)])
    got = _vector_run(lib, w, b, x, g)
    ref = cr.run("VectorCrossNet", p, x, g, "float64")
    errs = cr.result_errors(got, ref)
    tol = cr.gpu_tolerance()
    print(f"VectorCrossNet {B}x{N} L={L}: tolerance {tol:.3e}, errors " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= tol, errs
    again = _vector_run(lib, w, b, x, g)
    for k in ("out", "s", "grad_input"):
        np.testing.assert_array_equal(got[k], again[k], err_msg=k)
    for k in got["grad"]:
        np.testing.assert_array_equal(got["grad"][k], again["grad"][k], err_msg=k)


def test_vector_kernels_name_their_limits_and_change_no_byte():
    lib = _lib.load()
    n = 4100 * 9
    bufs = {k: Buf(n, np.ones(n)) for k in ("x", "w", "b", "g", "out", "s", "gin", "gp", "ws")}
    before = {k: b.all().copy() for k, b in bufs.items()}
    P = {k: b.ptr for k, b in bufs.items()}
    for N, L in ((4100, 1), (4096, 9)):
        rc = lib.tbe_vector_cross_forward_f32(P["x"], P["w"], P["b"], 1, N, L, P["out"], P["s"], _stream())
        assert rc == INVALID and b"N <= 4096, L <= 8" in lib.tbe_last_error()
        rc = lib.tbe_vector_cross_backward_f32(P["g"], P["x"], P["s"], P["w"], P["b"], 1, N, L, P["gin"], P["gp"], P["ws"],
                                               4 * n, _stream())
        assert rc == INVALID and b"N <= 4096, L <= 8" in lib.tbe_last_error()
    rc = lib.tbe_vector_cross_backward_f32(P["g"], P["x"], P["s"], P["w"], P["b"], 4, 64, 2, P["gin"], P["gp"], P["ws"], 16,
                                           _stream())
    assert rc == INVALID and b"workspace" in lib.tbe_last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        np.testing.assert_array_equal(b.all(), before[k], err_msg=k)
