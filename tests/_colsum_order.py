"""numpy float32 host model of the summation ORDER of the row-block column sums (csrc/colsum.hpp), the scheme shared by
tbe_relu_backward_bias_grad_f32, tbe_weighted_colsum_f32, tbe_cross_backward_f32 and their `_partials` first stages.

First stage (`first_stage`): a workgroup of 256 threads = TY rows x TX float4 columns owns `rows_per_block(N)` rows.  Thread
row ty starts from 0.0f and adds the rows ty, ty + TY, ... of its block in that order; the block's sum of a column is then
red[0] + red[1] + ... + red[TY - 1], left to right.  The weighted entry adds with fmaf(w[r], x[r, c], acc).
Second stage (`second_stage`): wave w of 4 starts from 0.0f and adds the blocks w, w + 4, ...; the result is
((a0 + a1) + a2) + a3.

Every add below is one float32 operation on numpy float32 arrays, so the model reproduces the kernels bit for bit
(tests/test_colsum_order_gpu.py); tests/test_colsum_order.py checks that the order matters for the inputs used."""
import functools

import numpy as np

# (B, N): minimum; TX 16 with a column tail and a partial block; TX 16, two blocks; TX 32, 3 blocks (fewer blocks than
# waves); TX 64, 5 blocks; 256-row blocks, one row in the second, column-tile tail; 38 blocks (past the second stage's unroll
# of 8 blocks per wave)
SHAPES = [(1, 4), (63, 60), (65, 64), (130, 128), (300, 256), (257, 516), (2373, 8)]
WAVES = 4  # of the second stage


def rows_per_block(N):
    """Rows of [B, N] per workgroup of the first stage (csrc/colsum.hpp rows_per_block)."""
    return 256 if N >= 512 else 64


def row_blocks(B, N):
    """tbe_colsum_row_blocks."""
    return 0 if B <= 0 or N <= 0 else -(-B // rows_per_block(N))


def tile_rows(N):
    """TY = 256 / TX: thread rows of a first-stage workgroup; TX = 64, 32 or 16 float4 columns."""
    vecs = N // 4
    return 256 // (64 if vecs >= 64 else 32 if vecs >= 32 else 16)


def _fma32(w, x, acc):
    """fmaf(w, x, acc) for operands whose exact w * x + acc fits a float64 (see `weighted_inputs`): one rounding."""
    return (w.astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def first_stage(a, w=None):
    """[row blocks, N] float32: the column sums of the row blocks of a [B, N]; with w [B], of w[:, None] * a through fmaf."""
    a = np.asarray(a, dtype=np.float32)
    B, N = a.shape
    rpb, TY = rows_per_block(N), tile_rows(N)
    out = np.empty((row_blocks(B, N), N), dtype=np.float32)
    for rb in range(out.shape[0]):
        row1 = min(B, (rb + 1) * rpb)
        red = np.zeros((TY, N), dtype=np.float32)
        for r0 in range(rb * rpb, row1, TY):  # thread rows 0 .. n-1 take one row each
            n = min(TY, row1 - r0)
            if w is None:
                red[:n] = red[:n] + a[r0:r0 + n]
            else:
                red[:n] = _fma32(w[r0:r0 + n, None], a[r0:r0 + n], red[:n])
        s = red[0]
        for y in range(1, TY):
            s = s + red[y]
        out[rb] = s
    return out


def second_stage(partial):
    """[N] float32 from [row blocks, N]."""
    partial = np.asarray(partial, dtype=np.float32)
    acc = np.zeros((WAVES, partial.shape[1]), dtype=np.float32)
    for rb in range(partial.shape[0]):
        acc[rb % WAVES] = acc[rb % WAVES] + partial[rb]
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def colsum(a, w=None):
    return second_stage(first_stage(a, w))


def row_order_sum(a, w=None):
    """The same sum in plain row order — what the kernels do NOT compute."""
    a = np.asarray(a, dtype=np.float32)
    acc = np.zeros(a.shape[1], dtype=np.float32)
    for r in range(a.shape[0]):
        acc = acc + a[r] if w is None else _fma32(w[r], a[r], acc)
    return acc


# ---- inputs of the tests: seeded, one set per shape ------------------------------------------------------------------------------
def _normal(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def weighted_inputs(rng, B, N):
    """x [B, N], w [B] with 11-bit integer significands (one more bit with the sign): integers below 2^11 scaled by
    2^-4 ... 2^-10.  A product is a multiple of 2^-20 below 2^14 and so is every float32 partial sum (below 2^26 for these
    shapes): w * x + acc takes at most 46 bits, a float64 holds it exactly, and rounding it to float32 once is fmaf."""
    def draw(shape):
        return (rng.integers(-2047, 2048, shape) * 2.0 ** -rng.integers(4, 11, shape)).astype(np.float32)

    return draw((B, N)), draw(B)


@functools.lru_cache(maxsize=None)
def case(B, N):
    """Inputs and expected results of one shape (computed once, shared; treat as read-only):
      relu:     gy, act -> gx, partial, bias_grad
      weighted: x, w -> partial, out
      cross:    G, x0, t, acc0 -> gy, acc[first], partial, bias_grad"""
    rng = np.random.default_rng([2024, B, N])
    c = {}
    gy, act = _normal(rng, (B, N)), _normal(rng, (B, N))
    gx = np.where(act > 0, gy, np.float32(0))
    part = first_stage(gx)
    c["relu"] = dict(gy=gy, act=act, gx=gx, partial=part, bias_grad=second_stage(part))
    x, w = weighted_inputs(rng, B, N)
    part = first_stage(x, w)
    c["weighted"] = dict(x=x, w=w, partial=part, out=second_stage(part))
    G, x0, t, acc0 = (_normal(rng, (B, N)) for _ in range(4))
    y, gt = G * x0, G * t  # each product rounded on its own
    part = first_stage(y)
    c["cross"] = dict(G=G, x0=x0, t=t, acc0=acc0, gy=y, acc={1: gt, 0: acc0 + gt}, partial=part,
                      bias_grad=second_stage(part))
    return c
