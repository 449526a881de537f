"""numpy float32 host model of the head backward kernel (csrc/mlp_epilogue.hip relu_linear1_bwd_kernel,
tbe_relu_linear1_backward[_partials]_f32), built from the column sums' order model tests/_colsum_order.py:

    g  = dy[b] * w[c]                      one float32 multiply
    gx = act[b, c] > 0 ? g : 0
    partial[rb][0:N]  = first stage of gx                  (the ReLU-backward kernel's addend)
    partial[rb][N:2N] = first stage of act weighted by dy  (fmaf(dy[b], act[b, c], acc), the weighted column sum's)
    sums = second stage over the 2 N columns

`act` and `dy` have the short significands of `weighted_inputs`, so that the fmaf has an exact float64 model; their signs are
mixed (and a few are zero), so the mask is exercised; `w` is seeded normal."""
import functools

import numpy as np

import _colsum_order as co


def model(act, dy, w):
    """(gx [B, N], partial [row blocks, 2 N], sums [2 N])."""
    act, dy, w = (np.asarray(a, dtype=np.float32) for a in (act, dy, w))
    g = dy[:, None] * w[None, :]  # float32 * float32 -> float32: one rounding per element
    gx = np.where(act > 0, g, np.float32(0))
    partial = np.concatenate([co.first_stage(gx), co.first_stage(act, dy)], axis=1)
    return gx, partial, co.second_stage(partial)


@functools.lru_cache(maxsize=None)
def case(B, N):
    """Inputs and expected results of one shape (computed once, shared; treat as read-only)."""
    rng = np.random.default_rng([2025, B, N])
    act, dy = co.weighted_inputs(rng, B, N)
    w = rng.standard_normal(N).astype(np.float32)
    gx, partial, sums = model(act, dy, w)
    return dict(act=act, dy=dy, w=w, gx=gx, partial=partial, sums=sums)
