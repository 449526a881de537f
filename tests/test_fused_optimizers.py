"""CPU half of the row-norm optimizer family (LAMB, PARTIAL_ROWWISE_ADAM, PARTIAL_ROWWISE_LAMB, LARS_SGD) and gradient
clipping: the C ABI's argument validation, which returns before anything is launched, and the margin of the numpy
restatement the GPU tests (tests/test_fused_optimizers_gpu.py) compare with; for the run harness
(tests/test_fused_optimizers_runs_gpu.py) also where its tolerance comes from and that a wrong norm leaves it."""
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


# ---- the run harness: tolerance and sensitivity --------------------------------------------------------------------------
def _run_case(cfg):
    from _bwd_abi import BackwardCase, finishing_paths

    layout, dims, payload, code, wd, clip = cfg
    inp = fo.run_inputs(layout, dims, payload)
    case = BackwardCase(inp.rows, list(dims), code=code)  # the initial arrays the GPU test starts from
    return inp, case, finishing_paths(inp, case.oracle_tables()[0])


def _arrays(ref, t):
    return [("weights", ref.w[t])] + [(f"state{k}", s[t]) for k, s in enumerate(ref.state) if s is not None]


@pytest.mark.parametrize("cfg", fo.RUN_CONFIGS, ids=fo.run_config_id)
def test_run_harness_float32_restatement_is_within_an_eighth_of_the_tolerance(cfg):
    """NORM_TOL = 8 x NORM_F32_ERROR, and NORM_F32_ERROR bounds max |r32 - r64| / (1 + |r64|) of the restatement run in
    float32 on exactly the GPU configurations (worst measured: 4.257e-7, the weights of PARTIAL_ROWWISE_ADAM at [2048]).  A configuration
    added to RUN_CONFIGS that needs more fails here, not on the GPU."""
    inp, case, _ = _run_case(cfg)
    r64, r32 = fo.run_reference(cfg, case.init), fo.run_reference(cfg, case.init, np.float32)
    assert fo.NORM_TOL == 8 * fo.NORM_F32_ERROR and fo.NORM_TOL <= fo.RTOL
    for t in range(len(inp.rows)):
        for (what, a32), (_, a64) in zip(_arrays(r32, t), _arrays(r64, t)):
            assert a32.dtype == np.float32 and a64.dtype == np.float64
            err = fo.norm_error(a32, a64).max() * 8  # in units of NORM_F32_ERROR
            assert err <= 1.0, f"{what} of table {t}: float32 is {err:.3f} x NORM_F32_ERROR away from float64"
            R = inp.touched[t]
            assert (a64[R] != np.asarray(case.init[what][t], dtype=np.float64)[R]).reshape(R.size, -1).any(axis=1).all()


@pytest.mark.parametrize("code", fo.RUN_GUARD_CODES, ids=lambda c: fo.OPT_NAMES[c])
def test_run_harness_guard_rows_are_finished_by_the_block_fixup_and_reach_both_guards(code):
    from _bwd_abi import BLOCK_FIXUP, BackwardCase, coalesced_grad_f64, finishing_paths

    cfg, inp, init, zero_g, zero_w = fo.run_guard_case(code)
    tabs = BackwardCase(inp.rows, [128]).oracle_tables()[0]
    paths = finishing_paths(inp, tabs)[0]
    assert zero_g != zero_w and paths[zero_g] == paths[zero_w] == BLOCK_FIXUP
    G = coalesced_grad_f64(inp, tabs, fo.POOL_SUM)[0]
    assert not G[zero_g].any() and G[zero_w].any() and not init["weights"][0][zero_w].any()
    assert np.array_equal(G * 8, np.round(G * 8))  # zeroed bags keep the sums exact
    r64, r32 = fo.run_guard_reference(code), fo.run_guard_reference(code, np.float32)
    for (what, a32), (_, a64) in zip(_arrays(r32, 0), _arrays(r64, 0)):
        assert np.isfinite(a64).all()
        assert fo.norm_error(a32, a64).max() * 8 <= 1.0
        np.testing.assert_array_equal(a64[zero_g], np.asarray(init[what][0][zero_g], dtype=np.float64))  # |g| = |u| = 0: no move
    assert r64.w[0][zero_w].any()  # |w| = 0: the ratio is 1 and the row moves


SENSITIVITY_CONFIGS = [cfg for cfg in fo.RUN_CONFIGS if cfg[0] == "MIXED" and cfg[5] is None]


@pytest.mark.parametrize("cfg", SENSITIVITY_CONFIGS, ids=fo.run_config_id)
def test_a_column_missing_from_any_one_norm_leaves_the_run_harness_tolerance(cfg):
    """The condition NORM_TOL has to meet: a kernel that drops the last valid column from ONE of the optimizer's sums of
    squares (|w|, |g|, |u|, the mean(g^2) of v) gives, in every table and on EVERY finishing path, at least one row that a
    comparison at NORM_TOL rejects — for every optimizer and every dispatch class, D = 2048 included.  The smallest
    margin is |g| of LARS_SGD at [2048] on the wave fix-up's rows: 3.09 x NORM_TOL.  At rtol = atol = 2e-5 that change is
    0.53 x the tolerance (0.91 x on the in-chunk rows) and this test fails."""
    from _bwd_abi import PATH_NAMES

    inp, case, paths = _run_case(cfg)
    code = cfg[3]
    good = fo.run_reference(cfg, case.init)
    for which in fo.NORMS[code]:
        bad = fo.run_reference(cfg, case.init, drop=which)
        for t in range(len(inp.rows)):
            err = np.max([fo.norm_error(b, g).reshape(inp.rows[t], -1).max(axis=1)
                          for (_, b), (_, g) in zip(_arrays(bad, t), _arrays(good, t))], axis=0)
            assert not err[paths[t] < 0].any()  # rows no id names do not move at all
            for p, name in PATH_NAMES.items():
                assert (paths[t] == p).any()
                worst = err[paths[t] == p].max()
                assert worst > 1.0, (f"dropping a column from {which!r}: table {t}, rows finished {name}: the largest "
                                     f"change is {worst:.3f} x NORM_TOL — the comparison would not see it")
