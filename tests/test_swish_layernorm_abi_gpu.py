"""GPU: csrc/swish_layernorm.hip straight through the C ABI (include/tbe_hip.h), every output and the workspace between guard
elements that must stay untouched.  Results are compared with the float64 restatement (tests/_swish_layernorm_ref.py) within
the tolerance measured in tests/test_swish_layernorm.py, and every case runs twice: the second run repeats the first bit for
bit."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _swish_layernorm_ref as sr
from _guarded import Buf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
KEYS = ("out", "mean", "rstd", "grad_input", "grad_gamma", "grad_beta")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(lib, gamma, beta, x, g, eps=sr.EPS):
    """One forward and one backward through the ABI; the results laid out like _swish_layernorm_ref.run's."""
    B, N = x.shape
    bx, bga, bbe, bg = Buf(B * N, x), Buf(N, gamma), Buf(N, beta), Buf(B * N, g)
    bout, bst, bgy, bgp = Buf(B * N), Buf(2 * B), Buf(B * N), Buf(2 * N)
    rc = lib.tbe_swish_layernorm_forward_f32(bx.ptr, bga.ptr, bbe.ptr, eps, B, N, bout.ptr, bst.ptr, _stream())
    assert rc == OK, lib.tbe_last_error()
    wbytes = lib.tbe_swish_layernorm_backward_workspace_bytes(B, N)
    assert wbytes % 4 == 0
    bws = Buf(wbytes // 4)
    rc = lib.tbe_swish_layernorm_backward_f32(bg.ptr, bx.ptr, bst.ptr, bga.ptr, bbe.ptr, B, N, bgy.ptr, bgp.ptr, bws.ptr,
                                              wbytes, _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    bws.get()  # guards round the workspace
    for b, src in ((bx, x), (bga, gamma), (bbe, beta), (bg, g)):
        np.testing.assert_array_equal(b.get(), np.asarray(src).reshape(-1))  # inputs are not modified
    st, gp = bst.get((2, B)), bgp.get((2, N))
    return {"out": bout.get((B, N)), "mean": st[0], "rstd": st[1], "grad_input": bgy.get((B, N)), "grad_gamma": gp[0],
            "grad_beta": gp[1]}


def _check(lib, label, gamma, beta, x, g, eps=sr.EPS):
    got = _run(lib, gamma, beta, x, g, eps)
    ref = sr.run(gamma, beta, x, g, eps, "float64")
    errs = sr.result_errors(got, ref)
    tol = sr.gpu_tolerance()
    print(f"{label}: tolerance {tol:.3e}, errors " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert set(errs) == set(KEYS)
    for k in KEYS:
        assert np.isfinite(got[k]).all(), k
    assert max(errs.values()) <= tol, errs
    again = _run(lib, gamma, beta, x, g, eps)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], again[k], err_msg=k)
    return got, ref


@pytest.mark.parametrize("B,N", sr.abi_shapes())
def test_kernels_match_the_float64_restatement_and_repeat_bit_for_bit(B, N):
    """Widths (tests/_swish_layernorm_ref.py ABI_WIDTHS): both sides of 64 | 68 (16 threads per row | a wave) and of
    1024 | 1028 (a wave | the block), every float4 slot count of a thread with the first width of each count (260, 516, 772;
    2052, 3076), a partly empty slot row (60), the limits 4 and 4096.  Batches: one row, and three row blocks with a ragged
    last one (298 rows of 128, 74 of 32, 37 of 16)."""
    assert -(-B // sr.rows_per_block(N)) in (1, 3)
    _check(_lib.load(), f"swish_layernorm {B}x{N}", *sr.gpu_case(B, N))


@pytest.mark.parametrize("N", [64, 260, 1028])
def test_constant_rows_and_saturated_sigmoids_stay_finite(N):
    """Rows 0 and 3 are constant: var = 0, n = 0, rstd = 1 / sqrt(eps).  A quarter of the columns has beta = +200 and
    another -200, so |z| is near 200 on both sides there: s is exactly 1 / exactly 0, out = y / 0 and dz = 0, with no NaN from
    inf * 0.  The remaining columns keep the parameter gradients non-zero.  One width per threads-per-row class."""
    B = 9
    gamma, beta, x, g = sr.gpu_case(B, N, seed=1)
    q = N // 4 // 4 * 4
    beta[:q], beta[q:2 * q] = 200.0, -200.0
    x[0], x[3] = 1.5, -2.25
    got, ref = _check(_lib.load(), f"swish_layernorm edges {B}x{N}", gamma, beta, x, g)
    for r, v in ((0, 1.5), (3, -2.25)):
        assert got["mean"][r] == np.float32(v) and got["rstd"][r] == np.float32(1.0) / np.sqrt(np.float32(sr.EPS))
    np.testing.assert_array_equal(got["out"][:, :q], x[:, :q])           # s = 1 exactly
    np.testing.assert_array_equal(got["out"][:, q:2 * q], np.zeros((B, q), dtype=np.float32))  # s = 0 exactly
    np.testing.assert_array_equal(got["grad_gamma"][:2 * q], np.zeros(2 * q, dtype=np.float32))
    np.testing.assert_array_equal(got["grad_beta"][:2 * q], np.zeros(2 * q, dtype=np.float32))


def test_errors_and_the_empty_batch_change_no_byte():
    lib = _lib.load()
    B, N = 8, 68
    gamma, beta, x, g = sr.gpu_case(B, N)
    wbytes = lib.tbe_swish_layernorm_backward_workspace_bytes(B, N)
    bufs = {"x": Buf(B * N, x), "gamma": Buf(N, gamma), "beta": Buf(N, beta), "g": Buf(B * N, g), "out": Buf(B * N, np.ones(B * N)),
            "stats": Buf(2 * B, np.ones(2 * B)), "gy": Buf(B * N, np.ones(B * N)), "gp": Buf(2 * N, np.ones(2 * N)),
            "ws": Buf(wbytes // 4, np.ones(wbytes // 4))}
    before = {k: b.all().copy() for k, b in bufs.items()}
    P = {k: b.ptr for k, b in bufs.items()}

    def fwd(B=B, N=N, eps=sr.EPS, **kw):
        p = dict(P, **kw)
        rc = lib.tbe_swish_layernorm_forward_f32(p["x"], p["gamma"], p["beta"], eps, B, N, p["out"], p["stats"], _stream())
        torch.cuda.synchronize()
        return rc, lib.tbe_last_error().decode()

    def bwd(B=B, N=N, ws_bytes=wbytes, **kw):
        p = dict(P, **kw)
        rc = lib.tbe_swish_layernorm_backward_f32(p["g"], p["x"], p["stats"], p["gamma"], p["beta"], B, N, p["gy"], p["gp"],
                                                  p["ws"], ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc, lib.tbe_last_error().decode()

    for call in (fwd, bwd):
        for bad_n, text in ((6, "multiple of 4"), (0, "multiple of 4"), (4100, "N <= 4096")):
            rc, msg = call(N=bad_n)
            assert rc == INVALID and text in msg and "tbe_swish_layernorm" in msg, msg
        rc, msg = call(x=None)
        assert rc == INVALID and "null" in msg
        rc, msg = call(x=P["x"] + 4)
        assert rc == INVALID and "aligned" in msg
        rc, msg = call(B=(1 << 31) * 32)
        assert rc == INVALID and "row blocks" in msg
    for eps in (float("nan"), float("inf"), -1.0):
        rc, msg = fwd(eps=eps)
        assert rc == INVALID and "eps" in msg
    rc, msg = bwd(ws_bytes=wbytes - 256)
    assert rc == INVALID and "workspace" in msg
    rc, msg = bwd(ws=None)
    assert rc == INVALID and "null" in msg
    rc, msg = bwd(gp=None)
    assert rc == INVALID and "null" in msg
    for k, b in bufs.items():
        np.testing.assert_array_equal(b.all(), before[k], err_msg=k)
    # B == 0: the forward does nothing; the backward zeroes grad_params and touches nothing else
    rc, msg = fwd(B=0)
    assert rc == OK, msg
    rc, msg = bwd(B=0)
    assert rc == OK, msg
    np.testing.assert_array_equal(bufs["gp"].get(), np.zeros(2 * N, dtype=np.float32))
    for k, b in bufs.items():
        if k != "gp":
            np.testing.assert_array_equal(b.all(), before[k], err_msg=k)
