"""CPU: the host model of the row-in-registers kernels' summation orders (tests/_rowreg_order.py) has teeth — for the inputs
of tests/test_rowreg_order_gpu.py every pinned row sum gives other bits than a left-to-right sum and every pinned column sum
other bits than a row-order sum, so a kernel that adds in another order cannot pass there — and it agrees with the geometry
the library reports.

Exempt, because there the pinned order IS the plain one (asserted as such below):
  row sums     VectorCrossNet (1, 4, 1): one float4, which one thread adds x, y, z, w; the butterfly adds zeros
  column sums  one row: VectorCrossNet (1, 4, 1) and the (1, N) shapes of SwishLayerNorm (a single addend)
               VectorCrossNet (64, 1028, 4) and (3, 4096, 8): one row block of the block-per-row kernel, whose one thread group
               adds its rows in row order; (257, 1028, 2) has the three row blocks that give that kernel an order of its own"""
import numpy as np
import pytest

import _paths  # noqa: F401
import _colsum_order as co
import _rowreg_order as ro
import _swish_layernorm_ref as sr
from fbgemm_gpu import _lib

ROW_EXEMPT_VECTOR = {(1, 4, 1)}
COL_EXEMPT_VECTOR = {(1, 4, 1), (64, 1028, 4), (3, 4096, 8)}
COL_EXEMPT_SLN = {(1, N) for N in ro.SLN_WIDTHS}


def _check(label, model, row_exempt, col_exempt):
    for name, (terms, pinned) in model["row_terms"].items():
        plain = ro.left_to_right_row_sum(terms)
        differ = int((pinned != plain).sum())
        print(f"{label} row sum {name}: {differ} / {len(pinned)} rows differ from the left-to-right sum")
        assert (differ == 0) if row_exempt else (differ >= 1), name
        exact = terms.astype(np.float64)
        bound = 2.0 ** -23 * terms.shape[1] * np.abs(exact).sum(axis=1)  # a sum of the same numbers, with room
        assert (np.abs(pinned - exact.sum(axis=1)) <= bound).all(), name
    for name, (terms, pinned) in model["col_terms"].items():
        plain = co.row_order_sum(terms)
        differ = int((pinned != plain).sum())
        print(f"{label} column sum {name}: {differ} / {len(pinned)} columns differ from the row-order sum")
        assert (differ == 0) if col_exempt else (differ >= 1), name
        exact = terms.astype(np.float64)
        bound = 2.0 ** -23 * terms.shape[0] * np.abs(exact).sum(axis=0)
        assert (np.abs(pinned - exact.sum(axis=0)) <= bound).all(), name


@pytest.mark.parametrize("B,N,L", ro.VECTOR_SHAPES)
def test_vector_cross_orders_differ_from_plain_index_order(B, N, L):
    m = ro.vector_case(B, N, L)["model"]
    assert set(m["row_terms"]) == {f"{k}.{l}" for k in "sd" for l in range(L)}
    assert set(m["col_terms"]) == {f"{k}.{l}" for k in ("bias", "weight") for l in range(L)}
    _check(f"VectorCrossNet {B}x{N} L={L}", m, (B, N, L) in ROW_EXEMPT_VECTOR, (B, N, L) in COL_EXEMPT_VECTOR)


@pytest.mark.parametrize("B,N", ro.SLN_SHAPES)
def test_swish_layernorm_orders_differ_from_plain_index_order(B, N):
    m = ro.sln_case(B, N)["model"]
    assert set(m["row_terms"]) == {"mean", "var"} and set(m["col_terms"]) == {"gamma", "beta"}
    _check(f"SwishLayerNorm {B}x{N}", m, False, (B, N) in COL_EXEMPT_SLN)


def test_the_shapes_are_the_issues():
    assert ro.VECTOR_SHAPES == [(1, 4, 1), (5, 12, 3), (67, 64, 2), (130, 260, 3), (64, 1028, 4), (3, 4096, 8), (257, 1028, 2)]
    assert sorted({N for _, N in ro.SLN_SHAPES}) == [60, 64, 68, 772, 1024, 1028, 4096]
    for N in ro.SLN_WIDTHS:
        blocks = sorted(-(-B // sr.rows_per_block(N)) for B, n in ro.SLN_SHAPES if n == N)
        assert blocks == [1, 3] and all(B == 1 or B % sr.rows_per_block(N) for B, n in ro.SLN_SHAPES if n == N)
    assert -(-257 // 128) == 3 and ro.vector_tpr(1028) == 256


def test_the_zero_affine_model_is_the_restatement():
    """The model at gamma = beta = 0 against tests/_swish_layernorm_ref.py in float64: the same function, other orders."""
    B, N = 74, 772
    c = ro.sln_case(B, N)
    ref = sr.run(np.zeros(N), np.zeros(N), c["y"], c["g"], sr.EPS, "float64")
    m = c["model"]
    got = {"out": m["out"], "mean": m["mean"], "rstd": m["rstd"], "grad_input": m["grad_y"], "grad_gamma": m["grad_params"][0],
           "grad_beta": m["grad_params"][1]}
    assert max(sr.result_errors(got, ref).values()) <= sr.gpu_tolerance()


def test_workspace_geometry_is_the_librarys():
    lib = _lib.load()
    for B, N, L in ro.VECTOR_SHAPES:
        need = -(-B // 128) * 2 * L * N * 4
        got = lib.tbe_vector_cross_backward_workspace_bytes(B, N, L)
        assert need <= got < need + 256 and got % 256 == 0
    for B, N in ro.SLN_SHAPES:
        need = -(-B // sr.rows_per_block(N)) * 2 * N * 4
        got = lib.tbe_swish_layernorm_backward_workspace_bytes(B, N)
        assert need <= got < need + 256 and got % 256 == 0
