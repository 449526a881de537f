"""CPU: the host model of the column sums' order (tests/_colsum_order.py) has teeth — for the inputs of
tests/test_colsum_order_gpu.py the pinned order gives other bits than a plain row-order sum and than numpy's pairwise sum, so
a kernel that adds in another order cannot pass there — and it agrees with the geometry the library reports."""
import numpy as np
import pytest

import _paths  # noqa: F401
import _colsum_order as co
from fbgemm_gpu import _lib


@pytest.mark.parametrize("B,N", co.SHAPES[1:])
def test_the_pinned_order_differs_from_row_order_and_from_numpys_sum(B, N):
    c = co.case(B, N)
    w, x = c["weighted"]["w"], c["weighted"]["x"]
    addends = {"relu": (c["relu"]["gx"], None, c["relu"]["bias_grad"]),
               "cross": (c["cross"]["gy"], None, c["cross"]["bias_grad"]),
               "weighted": (x, w, c["weighted"]["out"])}
    for name, (a, wt, model) in addends.items():
        rows = (model != co.row_order_sum(a, wt)).sum()
        prod = a if wt is None else wt[:, None] * a
        pairwise = (model != prod.sum(axis=0, dtype=np.float32)).sum()
        print(f"{name} {B}x{N}: {rows} / {N} columns differ from the row-order sum, {pairwise} from numpy's")
        assert rows >= 1 and pairwise >= 1, name
        # and it is a sum of the same numbers: within float32 rounding of the float64 result
        exact = a.astype(np.float64) if wt is None else wt.astype(np.float64)[:, None] * a
        ref = exact.sum(axis=0)
        bound = 2.0 ** -23 * B * np.abs(exact).sum(axis=0)  # (B - 1) roundings of 2^-24 each, with room
        assert (np.abs(model - ref) <= bound).all(), name


def test_the_fused_multiply_add_model_is_exact_for_its_inputs():
    """w * x + acc of the weighted inputs fits a float64: its significand needs at most 46 bits (tests/_colsum_order.py)."""
    for B, N in co.SHAPES:
        x, w = co.case(B, N)["weighted"]["x"], co.case(B, N)["weighted"]["w"]
        for a in (x, w):
            q = a.astype(np.float64) * 2.0 ** 10
            assert (q == np.round(q)).all() and np.abs(a).max() < 2.0 ** 7
        assert B * 2.0 ** 14 < 2.0 ** 26


def test_row_block_geometry_is_the_librarys():
    lib = _lib.load()
    for B, N in co.SHAPES + [(0, 8), (64, 512), (65536, 508), (65536, 512)]:
        assert lib.tbe_colsum_row_blocks(B, N) == co.row_blocks(B, N)
        for fn in (lib.tbe_relu_backward_bias_grad_workspace_bytes, lib.tbe_weighted_colsum_workspace_bytes,
                   lib.tbe_cross_backward_workspace_bytes):
            assert fn(B, N) >= max(1, co.row_blocks(B, N) * N * 4) and fn(B, N) % 256 == 0
