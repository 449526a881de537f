"""CPU half of the row-norm optimizer family (LAMB, PARTIAL_ROWWISE_ADAM, PARTIAL_ROWWISE_LAMB, LARS_SGD) and gradient
clipping: the C ABI's argument validation, which returns before anything is launched, and the margin of the numpy
restatement the GPU tests (tests/test_fused_optimizers_gpu.py) compare with."""
import ctypes
import math

import numpy as np
import pytest

import _paths  # noqa: F401
import _fused_optim_ref as fo
from fbgemm_gpu import _lib
from fbgemm_gpu._lib import OptimizerArgs, OptimizerExt

OK, INVALID, UNSUPPORTED = 0, -1, -4  # TBE_OK, TBE_ERR_INVALID_ARGUMENT, TBE_ERR_UNSUPPORTED
S0, S1 = 0x1000, 0x2000  # stand-ins for state address tables: validation only tests them against NULL


def _call(name, code, state0=S0, state1=S1, ext=None, iteration=1):
    """One backward entry with F = 1, B = 1, N = 0: every check runs, and a call that passes them has nothing to do."""
    lib = _lib.load()
    opt = OptimizerArgs(code, 0.1, 1e-8, 0.0, 0.9, 0.999, iteration)
    head = (None, None, None, None, None, state0, state1, 1, 1, 8, 4, None, 0, None, None, 0, None, None, 8, opt, 0, None, 0)
    fused, f16, ex = "fused" in name, name.endswith("f16w"), "_ex_" in name
    args = head + ((None, None) if fused else ()) + ((0, 0) if f16 else ())
    if ex:
        args += (ctypes.byref(ext) if ext is not None else None,)
    rc = getattr(lib, name)(*args, None)
    return rc, lib.tbe_last_error().decode()


OLD = ["tbe_backward_fused_f32", "tbe_backward_apply_f32", "tbe_backward_fused_f16w", "tbe_backward_apply_f16w"]
EX = ["tbe_backward_fused_ex_f32", "tbe_backward_apply_ex_f32", "tbe_backward_fused_ex_f16w", "tbe_backward_apply_ex_f16w"]


def test_the_four_ex_entries_are_exported_and_bound():
    lib = _lib.load()
    for name in EX:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert ctypes.sizeof(OptimizerExt) == 16
    assert lib.tbe_abi_version() == 3


@pytest.mark.parametrize("name", OLD)
@pytest.mark.parametrize("code", fo.NORM_FAMILY)
def test_the_old_entries_still_refuse_the_new_codes(name, code):
    rc, msg = _call(name, code)
    assert rc == UNSUPPORTED and "unknown optimizer" in msg


@pytest.mark.parametrize("name", EX)
def test_ex_entries_validate_states_iteration_and_clipping_before_any_launch(name):
    for code in fo.NORM_FAMILY:
        assert _call(name, code)[0] == OK  # both states given, N = 0: nothing to do
        rc, msg = _call(name, code, state0=None)
        assert rc == INVALID and "feat_state0" in msg
    for code in (fo.LAMB, fo.PARTIAL_ROWWISE_ADAM, fo.PARTIAL_ROWWISE_LAMB):
        rc, msg = _call(name, code, state1=None)
        assert rc == INVALID and "feat_state1" in msg
    assert _call(name, fo.LARS_SGD, state1=None)[0] == OK
    rc, msg = _call(name, fo.PARTIAL_ROWWISE_ADAM, iteration=0)
    assert rc == INVALID and "iteration" in msg
    assert _call(name, fo.PARTIAL_ROWWISE_LAMB, iteration=0)[0] == OK  # no bias correction
    for bad in (-1.0, math.nan, math.inf, -math.inf):
        for code in (fo.SGD, fo.LAMB):
            rc, msg = _call(name, code, ext=OptimizerExt(0.0, 0.0, bad, 1))
            assert rc == INVALID and "max_gradient" in msg, (bad, code)
    assert _call(name, fo.SGD, ext=OptimizerExt(0.0, 0.0, -1.0, 0))[0] == OK  # the bound is not read without the switch
    assert _call(name, fo.SGD, ext=OptimizerExt(0.0, 0.0, 0.0, 1))[0] == OK
    assert _call(name, fo.SGD, state0=None, state1=None)[0] == OK  # ext = NULL, an old code: the twin
    for code in (8, 99, -1):
        rc, msg = _call(name, code)
        assert rc == UNSUPPORTED and "unknown optimizer" in msg


def test_dense_grad_with_fp16_tables_stays_unsupported_through_the_ex_entries():
    for name in ("tbe_backward_fused_ex_f16w", "tbe_backward_apply_ex_f16w"):
        assert _call(name, 100)[0] == UNSUPPORTED
    assert _call("tbe_backward_fused_ex_f32", 100)[0] == OK


@pytest.mark.parametrize("cfg", fo.GPU_CONFIGS, ids=[f"{n}-{fo.OPT_NAMES[c]}-wd{wd}-clip{mg}" for n, c, wd, mg in fo.GPU_CONFIGS])
def test_restatement_in_float32_agrees_with_float64_within_the_gpu_tolerance(cfg):
    """The GPU tests' tolerance (rtol = atol = 2e-5, the project's own for fused-optimizer results) is not tighter than
    FP32 arithmetic allows on the very inputs they use: the same restatement run in float32 stays inside it."""
    name, code, wd, mg = cfg
    r64 = fo.reference(name, code, wd, mg, "float64")
    r32 = fo.reference(name, code, wd, mg, "float32")
    for t in range(len(r64.rows)):
        assert r32.w[t].dtype == np.float32 and r64.w[t].dtype == np.float64
        np.testing.assert_allclose(r32.w[t], r64.w[t], rtol=fo.RTOL, atol=fo.ATOL)
        for s32, s64 in zip(r32.state, r64.state):
            if s64 is not None:
                np.testing.assert_allclose(s32[t], s64[t], rtol=fo.RTOL, atol=fo.ATOL)


@pytest.mark.parametrize("code", (fo.LAMB, fo.PARTIAL_ROWWISE_LAMB, fo.LARS_SGD))
def test_guard_inputs_reach_both_guards_and_stay_finite(code):
    """The guard input set does what it is for: row 0 starts with |w| = 0, row 1 sees |g| = 0 (so |u| = 0), and the
    restatement's guarded forms keep both finite; row 1 is touched yet unchanged."""
    c = fo.guard_case()
    assert not c.weights[0][0].any()
    ref = fo.Ref(c.rows, c.dims, None, c.weights, code, **fo.hyper(code))
    G, touched = ref.coalesce(*[c.batches[0][i] for i in (0, 1, 3)], psw=None, pooling=c.pooling)
    assert touched[0][[0, 1, 2, 3]].all() and not touched[0][[4, 5]].any()
    assert not G[0][1].any() and G[0][0].any()
    done = fo.reference("guards", code)
    assert all(np.isfinite(a).all() for a in done.w + [s[0] for s in done.state if s is not None])
    np.testing.assert_array_equal(done.w[0][1], c.weights[0][1].astype(np.float64))
    assert np.abs(done.w[0][0]).min() > 0
