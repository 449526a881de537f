"""CPU guard of the premise tests/test_tbe_backward_runs_gpu.py rests on: for the designed inputs of tests/_bwd_abi.py the
coalesced gradient is exact in FP32 whatever the summation order, so the FP32 oracle equals a float64 sum bit for bit and a
GPU kernel may be compared with it bitwise.  Widening a value range breaks THIS test, not the GPU comparison."""
import numpy as np
import pytest

import _fused_optim_ref
import _paths  # noqa: F401
from _bwd_abi import LAYOUTS, BackwardCase, coalesced_grad_f64, make_inputs, valid_keys, with_grad
from oracle import oracle

CONFIGS = {
    "d128_sum": dict(dims=[128], weighted=False, pooling=oracle.POOL_SUM, shift=0),
    "d13_260_weighted_mean_64bit_keys": dict(dims=[13, 260], weighted=True, pooling=oracle.POOL_MEAN, shift=1 << 33),
    "d64_64_weighted_sum": dict(dims=[64, 64], weighted=True, pooling=oracle.POOL_SUM, shift=0),
}


def _cases():
    for layout in LAYOUTS:
        for name, cfg in CONFIGS.items():
            if layout == "BIG" and name != "d128_sum":
                continue  # BIG is one feature, D = 16, bags of one id
            big = layout == "BIG"
            yield pytest.param(layout, dict(cfg, dims=[16]) if big else cfg, id=f"{layout}-{'d16_sum' if big else name}")


@pytest.mark.parametrize("layout,cfg", list(_cases()))
def test_oracle_dense_gradient_equals_the_float64_sum_exactly(layout, cfg):
    inp = make_inputs(layout, cfg["dims"], weighted=cfg["weighted"])
    case = BackwardCase(inp.rows, cfg["dims"], row_base_shift=cfg["shift"], code=oracle.OPT_DENSE_GRAD)
    tabs, dense, _ = case.oracle_tables()
    bad = oracle.tbe_backward(tabs, inp.indices, inp.offsets, inp.grad, oracle.OPT_DENSE_GRAD, 0.0, inp.psw, cfg["pooling"],
                              state0=dense)
    assert bad == inp.n_bad * inp.F
    ref = coalesced_grad_f64(inp, tabs, cfg["pooling"])
    for t in range(len(inp.rows)):
        assert dense[t].dtype == np.float32
        assert np.array_equal(dense[t].astype(np.float64), ref[t]), f"table {t}"
        # the sums are multiples of 1/8 far below 2^24 / 8: every partial sum of every order is representable
        assert np.array_equal(ref[t] * 8, np.round(ref[t] * 8)) and np.abs(ref[t]).max() * 8 < 2 ** 24
        assert np.abs(ref[t]).max() > 0


CLIP = 1.5  # _fused_optim_ref.RUN_CLIP: the bound the clipping tests of the run harness use


@pytest.mark.parametrize("layout,cfg", list(_cases()))
def test_clamped_gradient_is_exact_too(layout, cfg):
    """Gradient clipping at 1.5 clamps the integer gradients to {-1.5, -1, 0, 1, 1.5}: times {0.5, 1, 2} and over {1, 2, 4}
    every term is a multiple of 1/16, so the FP32 sum of clamped terms equals the float64 one bit for bit in any order."""
    assert _fused_optim_ref.RUN_CLIP == CLIP
    base = make_inputs(layout, cfg["dims"], weighted=cfg["weighted"])
    inp = with_grad(base, np.clip(base.grad, -CLIP, CLIP))
    assert set(np.unique(inp.grad).tolist()) == {-1.5, -1.0, 0.0, 1.0, 1.5} and (np.abs(base.grad) > CLIP).mean() > 0.5
    case = BackwardCase(inp.rows, cfg["dims"], row_base_shift=cfg["shift"], code=oracle.OPT_DENSE_GRAD)
    tabs, dense, _ = case.oracle_tables()
    bad = oracle.tbe_backward(tabs, inp.indices, inp.offsets, inp.grad, oracle.OPT_DENSE_GRAD, 0.0, inp.psw, cfg["pooling"],
                              state0=dense)
    assert bad == inp.n_bad * inp.F
    ref = coalesced_grad_f64(inp, tabs, cfg["pooling"])
    unclamped = coalesced_grad_f64(base, tabs, cfg["pooling"])
    for t in range(len(inp.rows)):
        assert dense[t].dtype == np.float32
        assert np.array_equal(dense[t].astype(np.float64), ref[t]), f"table {t}"
        assert np.array_equal(ref[t] * 16, np.round(ref[t] * 16)) and np.abs(ref[t]).max() * 16 < 2 ** 24
        assert not np.array_equal(ref[t], unclamped[t])


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shift", [0, 1 << 33], ids=["keys32", "keys64"])
def test_every_designed_run_length_is_present(layout, shift):
    runs, n_bad = LAYOUTS[layout]
    dims = [16] if layout == "BIG" else [13, 260]
    inp = make_inputs(layout, dims, weighted=layout != "BIG")
    case = BackwardCase(inp.rows, dims, row_base_shift=shift)
    tabs, _, _ = case.oracle_tables()
    keys, _ = valid_keys(inp, tabs)
    uniq, count = np.unique(keys, return_counts=True)
    # runs in key order: table after table, each with the designed list
    assert count.tolist() == list(runs) * len(dims)
    assert uniq.min() >= shift and case.key_bits == (34 if shift else int(sum(inp.rows)).bit_length())
    assert (case.key_bits > 32) == bool(shift)
    assert inp.N == (sum(runs) + n_bad) * inp.F
    lengths = np.diff(inp.offsets)
    assert set(lengths.tolist()) <= {1, 2, 4} and lengths.size == inp.F * inp.B
    assert set(np.unique(inp.grad).tolist()) <= set(range(-4, 5))
    if inp.psw is not None:
        assert set(np.unique(inp.psw).tolist()) <= {0.5, 1.0, 2.0}
    if layout == "BIG":
        assert inp.N > 524288  # beyond the last N with 32-id chunks
