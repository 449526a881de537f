"""CPU: the host model of the head backward kernel (tests/_head_backward.py) has teeth — for the inputs of
tests/test_head_backward_gpu.py both of its column sums differ from a plain row-order sum of the same addends, so a kernel
that adds in another order cannot pass there — the mask is exercised, and the library reports the geometry it assumes."""
import numpy as np
import pytest

import _paths  # noqa: F401
import _colsum_order as co
import _head_backward as hb
from fbgemm_gpu import _lib


@pytest.mark.parametrize("B,N", co.SHAPES[1:])
def test_both_sums_differ_from_a_row_order_sum(B, N):
    c = hb.case(B, N)
    bias, weight = c["sums"][:N], c["sums"][N:]
    d_bias = (bias != co.row_order_sum(c["gx"])).sum()
    d_weight = (weight != co.row_order_sum(c["act"], c["dy"])).sum()
    print(f"{B}x{N}: {d_bias} / {N} bias columns and {d_weight} / {N} weight columns differ from the row-order sum")
    assert d_bias >= 1 and d_weight >= 1
    # sums of the same numbers: within float32 rounding of the float64 results
    for got, exact in ((bias, c["gx"].astype(np.float64)),
                       (weight, c["dy"].astype(np.float64)[:, None] * c["act"])):
        bound = 2.0 ** -23 * B * np.abs(exact).sum(axis=0)
        assert (np.abs(got - exact.sum(axis=0)) <= bound).all()


@pytest.mark.parametrize("B,N", co.SHAPES)
def test_model_shapes_and_mask(B, N):
    c = hb.case(B, N)
    nrb = co.row_blocks(B, N)
    assert c["gx"].shape == (B, N) and c["partial"].shape == (nrb, 2 * N) and c["sums"].shape == (2 * N,)
    assert ((c["act"] > 0) | (c["gx"] == 0)).all()
    if B * N >= 64:
        on = (c["act"] > 0).mean()
        assert 0.3 < on < 0.7  # both sides of the mask
    np.testing.assert_array_equal(c["partial"][:, :N], co.first_stage(c["gx"]))
    np.testing.assert_array_equal(c["partial"][:, N:], co.first_stage(c["act"], c["dy"]))


def test_workspace_holds_both_sums_of_every_row_block():
    lib = _lib.load()
    for B, N in co.SHAPES + [(0, 8), (64, 512), (65536, 256)]:
        need = lib.tbe_relu_linear1_backward_workspace_bytes(B, N)
        assert need >= max(1, co.row_blocks(B, N) * 2 * N * 4) and need % 256 == 0


def test_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    assert lib.tbe_relu_linear1_backward_partials_f32(None, None, None, 0, 8, None, None, 0, None) == -1  # B > 0
    assert lib.tbe_relu_linear1_backward_partials_f32(None, None, None, 4, 6, None, None, 0, None) == -1  # N % 4
    assert lib.tbe_relu_linear1_backward_partials_f32(None, None, None, 4, 8, None, None, 0, None) == -1  # null pointers
    assert lib.tbe_relu_linear1_backward_f32(None, None, None, 4, 8, None, None, None, 0, None) == -1
    # (16: a non-null address that is never dereferenced — the width is refused first)
    assert lib.tbe_relu_linear1_backward_f32(None, 16, None, 4, 1 << 21, None, 16, None, 0, None) == -1
    assert b"above" in lib.tbe_last_error()
