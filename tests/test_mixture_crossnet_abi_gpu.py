"""GPU: the gate kernels of LowRankMixtureCrossNet (csrc/crossnet.hip tbe_mixture_gate_forward_f32 / _backward_f32) straight
through the C ABI (include/tbe_hip.h), every output between guard elements that must stay untouched.

Forward: p against the float64 softmax within the tolerance measured in tests/test_mixture_crossnet.py; m bit for bit the
one product p_gpu * relu(a2).  Backward: bit for bit the float32 restatement (tests/_mixture_crossnet_ref.py) on inputs whose
every product and sum is exact in float32 in any order.  Both twice."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _mixture_crossnet_ref as mr
from _guarded import Buf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
SHAPES = [s + (0,) for s in mr.GATE_SHAPES] + [mr.GATE_SHAPE_OFF_GRID + (1,)]  # (B, K, r, elements off the 16-byte grid)
IDS = ["x".join(map(str, s[:3])) + ("-off-grid" if s[3] else "") for s in SHAPES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Off:
    """A guarded buffer whose payload starts `off` float32 elements into a Buf: the base leaves the 16-byte grid, the
    skipped elements join the leading guard."""

    def __init__(self, n, init=None, off=0):
        self.n, self.off = int(n), off
        self.buf = Buf(self.n + off)
        if init is not None:
            self.buf.t[64 + off:64 + off + self.n] = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).reshape(-1))
        self.ptr = self.buf.ptr + 4 * off
        self.before = self.buf.all().copy()

    def get(self, shape=None):
        a = self.buf.get()
        assert (a[:self.off] == self.before[64:64 + self.off]).all(), "guard elements overwritten"
        a = a[self.off:]
        return a.reshape(shape) if shape is not None else a

    def unchanged(self):
        return np.array_equal(self.buf.all(), self.before)


def _forward(lib, a2, logits, off=0):
    K, B, r = a2.shape
    ba, bl, bm, bp = Off(a2.size, a2, off), Off(B * K, logits, off), Off(B * K * r, None, off), Off(B * K, None, off)
    rc = lib.tbe_mixture_gate_forward_f32(ba.ptr, bl.ptr, B, K, r, bm.ptr, bp.ptr, _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    assert ba.unchanged() and bl.unchanged()  # inputs are not modified
    return bm.get((B, K * r)), bp.get((B, K))


def _backward(lib, gm, a2, p, off=0):
    K, B, r = a2.shape
    bg, ba, bp = Off(gm.size, gm, off), Off(a2.size, a2, off), Off(p.size, p, off)
    bga, bgl = Off(a2.size, None, off), Off(B * K, None, off)
    rc = lib.tbe_mixture_gate_backward_f32(bg.ptr, ba.ptr, bp.ptr, B, K, r, bga.ptr, bgl.ptr, _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    assert bg.unchanged() and ba.unchanged() and bp.unchanged()
    return bga.get((K, B, r)), bgl.get((B, K))


@pytest.mark.parametrize("B,K,r,off", SHAPES, ids=IDS)
def test_gate_forward(B, K, r, off):
    lib = _lib.load()
    a2, logits, _ = mr.gate_case(B, K, r)
    m, p = _forward(lib, a2, logits, off)
    p64 = mr.gate_forward(a2.astype(np.float64), logits.astype(np.float64))[1]
    tol = mr.softmax_tolerance()
    err, sum_err = np.abs(p - p64).max(), np.abs(p.sum(axis=1, dtype=np.float64) - 1.0).max()
    print(f"gate forward {B}x{K}x{r}: softmax tolerance {tol:.3e}, |p - p64| {err:.2e}, |sum p - 1| {sum_err:.2e}")
    assert err <= tol
    assert sum_err <= tol
    # m: ONE product of the kernel's own p with relu(a2), rounded once; -0.0 and negatives give +0.0
    want = (p.T[:, :, None] * mr.relu(a2)).transpose(1, 0, 2).reshape(B, K * r)
    assert m.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(m.view(np.uint32), want.view(np.uint32))
    if a2.size >= 64:
        assert (a2 < 0).any() and (a2 > 0).any() and np.signbit(a2[a2 == 0]).any() and not np.signbit(a2[a2 == 0]).all()
    m2, p2 = _forward(lib, a2, logits, off)
    np.testing.assert_array_equal(m2.view(np.uint32), m.view(np.uint32))
    np.testing.assert_array_equal(p2.view(np.uint32), p.view(np.uint32))


@pytest.mark.parametrize("K", [3, 16])
def test_gate_forward_has_no_nan_for_logits_2000_apart(K):
    lib = _lib.load()
    B, r = 5, 4
    logits = np.zeros((B, K), dtype=np.float32)
    logits[:, 0], logits[:, 2] = 1000.0, -1000.0
    logits[:, 3:] = np.linspace(-1000, -200, K - 3, dtype=np.float32) if K > 3 else 0  # expf(-1200) = 0, no denormal
    a2 = np.ones((K, B, r), dtype=np.float32)
    m, p = _forward(lib, a2, logits)
    want = np.zeros((B, K), dtype=np.float32)
    want[:, 0] = 1.0
    np.testing.assert_array_equal(p, want)
    np.testing.assert_array_equal(m, np.repeat(want, r, axis=1))


@pytest.mark.parametrize("K", [2, 4, 16])
def test_equal_logits_give_exactly_one_kth(K):
    lib = _lib.load()
    B, r = 6, 3
    logits = np.repeat(np.array([0.0, -3.25, 88.0, 1e4, -1e4, 0.1], dtype=np.float32)[:, None], K, axis=1)
    m, p = _forward(lib, np.full((K, B, r), 3.0, dtype=np.float32), logits)
    np.testing.assert_array_equal(p, np.float32(1.0 / K))
    np.testing.assert_array_equal(m, np.float32(3.0 / K))


@pytest.mark.parametrize("B,K,r,off", SHAPES, ids=IDS)
def test_gate_backward_is_bit_equal_to_the_float32_restatement(B, K, r, off):
    lib = _lib.load()
    gm, a2, p = mr.exact_gate_case(B, K, r)
    ga, gl = _backward(lib, gm, a2, p, off)
    want_ga, want_gl = mr.gate_backward(gm, a2, p)
    np.testing.assert_array_equal(ga, want_ga)
    np.testing.assert_array_equal(gl, want_gl)
    ga2, gl2 = _backward(lib, gm, a2, p, off)
    np.testing.assert_array_equal(ga2.view(np.uint32), ga.view(np.uint32))
    np.testing.assert_array_equal(gl2.view(np.uint32), gl.view(np.uint32))


@pytest.mark.parametrize("B,K,r", [(67, 5, 4), (130, 16, 16), (3, 4, 1028)])
def test_float4_and_scalar_paths_give_the_same_bits(B, K, r):
    """r % 4 == 0 on a 16-byte grid moves float4, the same data 4 bytes off it moves scalars: no result bit differs, on
    inputs whose row dots are NOT exact (the order of the sum is the same on both paths)."""
    lib = _lib.load()
    a2, logits, gm = mr.gate_case(B, K, r)
    m0, p0 = _forward(lib, a2, logits, 0)
    m1, p1 = _forward(lib, a2, logits, 1)
    np.testing.assert_array_equal(m0.view(np.uint32), m1.view(np.uint32))
    np.testing.assert_array_equal(p0.view(np.uint32), p1.view(np.uint32))
    ga0, gl0 = _backward(lib, gm, a2, p0, 0)
    ga1, gl1 = _backward(lib, gm, a2, p0, 1)
    np.testing.assert_array_equal(ga0.view(np.uint32), ga1.view(np.uint32))
    np.testing.assert_array_equal(gl0.view(np.uint32), gl1.view(np.uint32))
    # and the inexact case agrees with the float64 restatement to float32 rounding of an r-term dot
    ga64, gl64 = mr.gate_backward(gm.astype(np.float64), a2.astype(np.float64), p0.astype(np.float64))
    np.testing.assert_array_equal(ga0, ga64.astype(np.float32))  # one product each
    assert mr.rel_err(gl0, gl64) <= mr.gpu_tolerance()


def test_errors_and_the_empty_batch_change_no_byte():
    lib = _lib.load()
    B, K, r = 8, 4, 4
    rng = np.random.default_rng(11)
    bufs = {k: Off(B * K * r, rng.standard_normal(B * K * r)) for k in ("a2", "m", "gm", "ga2")}
    bufs.update({k: Off(B * K, rng.standard_normal(B * K)) for k in ("logits", "p", "gl")})
    P = {k: b.ptr for k, b in bufs.items()}

    def fwd(B=B, K=K, r=r, **over):
        q = dict(P, **over)
        rc = lib.tbe_mixture_gate_forward_f32(q["a2"], q["logits"], B, K, r, q["m"], q["p"], _stream())
        torch.cuda.synchronize()
        return rc, lib.tbe_last_error().decode()

    def bwd(B=B, K=K, r=r, **over):
        q = dict(P, **over)
        rc = lib.tbe_mixture_gate_backward_f32(q["gm"], q["a2"], q["p"], B, K, r, q["ga2"], q["gl"], _stream())
        torch.cuda.synchronize()
        return rc, lib.tbe_last_error().decode()

    for call, name, out in ((fwd, "tbe_mixture_gate_forward_f32", "m"), (bwd, "tbe_mixture_gate_backward_f32", "ga2")):
        for kw, word in ((dict(K=1), "K=1"), (dict(K=17), "K=17"), (dict(r=0), "r=0"), ({out: None}, "null"),
                         (dict(a2=None), "null"), ({out: P[out] + 2}, "aligned"), (dict(a2=P["a2"] + 1), "aligned")):
            rc, msg = call(**kw)
            assert rc == INVALID and name in msg and word in msg, (kw, rc, msg)
        rc, msg = call(B=0)
        assert rc == OK, msg
    for k, b in bufs.items():
        assert b.unchanged(), k
