"""Shapes, row layouts, inputs and oracle results for the tests that call the two dense dot-interaction entry points
(tbe_dlrm_interaction_forward_f32 / _backward_f32, include/tbe_hip.h) through the C ABI.

The constants below restate what csrc/dlrm_interaction.hip fixes in its source, so that the shape lists can be reasoned
about (and checked on the CPU, tests/test_interaction_abi.py) without a device:
  forward,  D = 16, 32, 256: interaction_fwd_kernel (operands in registers), grid capped at 256 * 4 blocks (256 * 2 at 256)
  forward,  D = 64, 128:     interaction_fwd_glds_kernel (LDS-DMA), 256 * 2 blocks; rows that take the scalar path are
                             stored by DS = D / 64 + T = ceil(P / 64) counted stores per sample
  backward, D = 16 .. 128:   interaction_bwd_kernel<D / 16>, 256 * 2 blocks
A block is 4 waves, a wave owns sample b, b + 4 * gridDim.x, ...; R = F + 1 rows, P = R (R - 1) / 2 pairs."""
import functools

import numpy as np

import _paths  # noqa: F401
from _guarded import CANARY, Buf
from oracle import oracle

FWD_MAX_F, BWD_MAX_F = 31, 27
FWD_DIMS, BWD_DIMS = (16, 32, 64, 128, 256), (16, 32, 64, 128)
LAYOUTS = ("dense", "padded", "wide", "odd", "shifted")


def pairs(F):
    return F * (F + 1) // 2


def pairs4(F):
    return (pairs(F) + 3) // 4 * 4


def forward_kernel(D):
    return "glds" if D in (64, 128) else "register"


def grid_cap(kind, D):
    """Largest grid of the kernel: constants of the source, not device queries."""
    return 256 * 4 if kind == "fwd" and D in (16, 32) else 256 * 2


def sample_stride(kind, B, D):
    """4 * gridDim.x: how far a wave moves between two of its samples."""
    return 4 * max(1, min((B + 3) // 4, grid_cap(kind, D)))


def trips(kind, B, D):
    """Most samples one wave visits."""
    return -(-B // sample_stride(kind, B, D))


def loop_batch(kind, D):
    """Smallest batch with two full trips of every wave and a third of five waves."""
    return 2 * 4 * grid_cap(kind, D) + 5


def pair_stores(F):
    """T: counted pair stores per sample of the LDS-DMA forward on the scalar path."""
    return -(-pairs(F) // 64)


def supports_backward(F, D):
    return F <= BWD_MAX_F and D in BWD_DIMS


def layouts(F, D):
    """(name, row stride in floats, byte shift of the `out` / `grad_out` pointer off its 16-B boundary)."""
    P, P4 = pairs(F), pairs4(F)
    yield "dense", D + P, 0
    yield "padded", D + P4, 0
    yield "wide", D + P4 + 4, 0
    yield "odd", next(s for s in (D + P + 1, D + P + 2, D + P + 3) if s % 4), 0
    yield "shifted", D + P4, 4


def layout(F, D, name):
    return next(lay for lay in layouts(F, D) if lay[0] == name)


def vector_path(F, D, stride, shift):
    """The kernels' `vec_out`: 16-B stores, pad columns [P, P4) written as zeros."""
    return stride % 4 == 0 and stride >= D + pairs4(F) and shift == 0


# ---- shape lists -----------------------------------------------------------------------------------------------------
EVERY_R_B = 9
EVERY_R_DIMS = (16, 64)  # one register-form, one LDS-DMA forward; backward<1> and <4>

GLDS_F = (1, 10, 11, 15, 16, 20, 23, 27, 28, 31)  # T = 1, 1, 2, 2, 3, 4, 5, 6, 7, 8; R = 16 | 17 at F = 15 | 16
REG_F = (1, 15, 16, 27, 31)
FWD_LOOP = [(loop_batch("fwd", D), F, D) for D in FWD_DIMS for F in (GLDS_F if forward_kernel(D) == "glds" else REG_F)]
BWD_LOOP = [(loop_batch("bwd", D), F, D) for D in BWD_DIMS for F in (GLDS_F if forward_kernel(D) == "glds" else REG_F)
            if F <= BWD_MAX_F]

FEW_B = (1, 3, 5)  # fewer samples than the waves of two blocks
FEW_SHAPES = ((16, 128), (15, 32))

ISOLATION = [(4101, 16, 128), (8197, 15, 32), (4101, 5, 256)]  # the last forward only


# ---- inputs and oracle results ---------------------------------------------------------------------------------------
class _Case:
    """float32 standard-normal dense [B, D], sparse [B, F, D], grad [B, D + P] and, computed on first use, the oracle's
    out [B, D + P] and (grad_dense [B, D], grad_sparse [B, F, D]).  Shared between tests: treat as read-only."""

    def __init__(self, B, F, D, dense, sparse, grad):
        self.B, self.F, self.D = B, F, D
        self.dense, self.sparse, self.grad = dense, sparse, grad
        for a in (dense, sparse, grad):
            a.setflags(write=False)

    @functools.cached_property
    def out(self):
        o = oracle.interaction_forward(self.dense, self.sparse)
        o.setflags(write=False)
        return o

    @functools.cached_property
    def grads(self):
        assert supports_backward(self.F, self.D)
        gd, gs = oracle.interaction_backward(self.dense, self.sparse, self.grad)
        gd.setflags(write=False)
        gs.setflags(write=False)
        return gd, gs


@functools.lru_cache(maxsize=4)  # a test asks for one shape and loops over the layouts; the big shapes are not kept
def case(B, F, D, seed=0):
    rng = np.random.default_rng([2025, B, F, D, seed])
    draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    return _Case(B, F, D, draw(B, D), draw(B, F, D), draw(B, D + pairs(F)))


def poisoned_samples(kind, B, D):
    """b = 2 (its wave goes on to clean samples), b = 7 and the sample the same wave visits next, and the last sample
    (its wave computes clean samples while the poisoned one sits in the prefetch registers)."""
    return sorted({2, 7, 7 + sample_stride(kind, B, D), B - 1})


POISON_COL = 5


def poison(c, samples):
    """A copy of case `c` with, in every sample b of `samples`: NaN in sparse[b, b % F, POISON_COL], +Inf in
    dense[b, POISON_COL] and -Inf in the gradient of the pair b % P."""
    dense, sparse, grad = c.dense.copy(), c.sparse.copy(), c.grad.copy()
    for b in samples:
        sparse[b, b % c.F, POISON_COL] = np.nan
        dense[b, POISON_COL] = np.inf
        grad[b, c.D + b % pairs(c.F)] = -np.inf
    return _Case(c.B, c.F, c.D, dense, sparse, grad)


# ---- device buffers in a row layout ------------------------------------------------------------------------------------
class RowBuf:
    """[B, stride] float32 rows in a guarded device buffer whose first row starts `shift` bytes (0 or 4) past a 16-B
    boundary: one element more is allocated and the pointer moved."""

    def __init__(self, B, stride, shift, init=None):
        assert shift in (0, 4)
        self.B, self.stride, self.skip = B, stride, shift // 4
        host = None
        if init is not None:
            host = np.full(B * stride + self.skip, CANARY, dtype=np.float32)
            host[self.skip:] = np.asarray(init, dtype=np.float32).reshape(-1)
        self.buf = Buf(B * stride + self.skip, host)
        self.ptr = self.buf.ptr + shift
        assert self.ptr % 16 == shift

    def get(self):
        """[B, stride]; asserts the guard elements (and the element in front of a shifted payload)."""
        a = self.buf.get()
        assert (a[:self.skip] == CANARY).all(), "element in front of the shifted rows overwritten"
        return a[self.skip:].reshape(self.B, self.stride)


def expected_out(c, stride, shift, out=None):
    """The image of an `out` buffer that was all CANARY before the forward."""
    D, W = c.D, c.D + pairs(c.F)
    img = np.full((c.B, stride), CANARY, dtype=np.float32)
    img[:, :W] = c.out if out is None else out
    if vector_path(c.F, D, stride, shift):
        img[:, W:D + pairs4(c.F)] = 0.0
    return img


def grad_image(c, stride):
    """grad_out rows in a layout: NaN in every column from D + P on (bit-equal results show they are never read)."""
    W = c.D + pairs(c.F)
    img = np.full((c.B, stride), np.nan, dtype=np.float32)
    img[:, :W] = c.grad
    return img
