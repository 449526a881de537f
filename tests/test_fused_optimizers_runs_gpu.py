"""The row-norm optimizer family (LAMB, PARTIAL_ROWWISE_ADAM, PARTIAL_ROWWISE_LAMB, LARS_SGD; `apply_row_norm` of
csrc/tbe_backward_impl.hpp) and gradient clipping on the run/chunk harness of tests/test_tbe_backward_runs_gpu.py: through
the C ABI's tbe_backward_*_ex_* entries, every dispatch class of run_apply, rows finished inside a chunk, by the per-wave
and by the whole-workgroup fix-up in ONE launch, 32- and 64-bit sort keys, FP16 tables, guard bytes round every array.

The designed inputs (tests/_bwd_abi.py) make the coalesced gradient exact in FP32 in any order, so what is left between a
kernel and the float64 restatement (tests/_fused_optim_ref.py `restate`) is the optimizer's own arithmetic, and the
comparison runs at rtol = atol = NORM_TOL = 8 x the measured float32-vs-float64 error of the restatement (3.44e-6; the
project's 2e-5 cannot see a column missing from a norm at D = 2048).  tests/test_fused_optimizers.py holds the CPU side:
the float32 margin over exactly RUN_CONFIGS and the dropped-column condition.  Failures report the worst
error / tolerance and its row per finishing path.  Set TBE_RUNS_REPORT=1 to print those figures for passing cases too."""
import os

import numpy as np
import pytest

import _paths  # noqa: F401
import _fused_optim_ref as fo
from _bwd_abi import (BLOCK_FIXUP, FLAG_UNIFORM_ALIGNED, IN_CHUNK, ROUND_STOCHASTIC, WAVE_FIXUP, BackwardCase,
                      finishing_paths, opt_args, opt_ext)
from oracle import oracle
from test_tbe_backward_runs_gpu import _assert_all_same, _assert_same_bits, _bits, _untouched, _worst_row_per_path

pytestmark = pytest.mark.gpu

SGD, DENSE = oracle.OPT_EXACT_SGD, oracle.OPT_DENSE_GRAD
KINDS = ("weights", "state0", "state1")
REPORT = os.environ.get("TBE_RUNS_REPORT") == "1"


def _case(inp, dims, code, shift=0, dtype="float32", init=None):
    # [40, 12]: the second table lies 4 B off the 16-B grid in all of its arrays: scalar loads and stores of w, m1, m2
    return BackwardCase(inp.rows, list(dims), None, shift, dtype, code, misalign=(1,) if list(dims) == [40, 12] else (), init=init)


def _opt(code, wd, clip=None):
    """(tbe_optimizer_args, tbe_optimizer_ext or None) of fo.run_hyper: ext only where the call needs one, so that the
    family also runs with ext = NULL."""
    h = fo.run_hyper(code, wd)
    opt = opt_args(code, h["learning_rate"], h["eps"], h["weight_decay"], h["beta1"], h["beta2"], fo.RUN_ITERATION)
    ext = opt_ext(h["momentum"], h["eta"], clip) if (code == fo.LARS_SGD or clip is not None) else None
    return opt, ext


def _got(res):
    return {"weights": res.weights, "state0": res.state0, "state1": res.state1}


def _want(ref):
    return {"weights": ref.w, "state0": ref.state[0], "state1": ref.state[1]}


def _assert_matches_restatement(inp, case, res, ref, paths, what):
    """Weights and every state against the float64 restatement at NORM_TOL, rows no id names bit-identical to the start."""
    got, want = _got(res), _want(ref)
    for kind in KINDS:
        assert (got[kind] is None) == (want[kind] is None) == (case.init[kind] is None), kind
        if got[kind] is None:
            continue
        for t in range(len(inp.rows)):
            assert got[kind][t].dtype == np.float32 and np.isfinite(got[kind][t]).all()
            un = _untouched(inp, t)
            _assert_same_bits(got[kind][t][un], case.init[kind][t][un], f"{what}: {kind} of table {t}, rows no id names")
            worst = _worst_row_per_path(got[kind][t], want[kind][t], paths[t], fo.NORM_TOL)
            if REPORT:
                print(f"REPORT {what} {kind} t{t} " + " ".join(f"{n}={e:.4f}@{r}" for n, (e, r) in worst.items()))
            assert all(e <= 1.0 for e, _ in worst.values()), \
                f"{what}: {kind} of table {t}: worst (error / NORM_TOL, row) per finishing path: {worst}"


def _run_and_compare(cfg, shift=0):
    layout, dims, payload, code, wd, clip = cfg
    inp = fo.run_inputs(layout, dims, payload)  # unclamped: the kernel clamps
    case = _case(inp, dims, code, shift)
    opt, ext = _opt(code, wd, clip)
    res = case.run(inp, opt, fo.RUN_PAYLOADS[payload][1], ext=ext)
    paths = finishing_paths(inp, case.oracle_tables()[0])
    _assert_matches_restatement(inp, case, res, fo.run_reference(cfg, case.init), paths, fo.run_config_id(cfg))
    assert res.guards_ok, "bytes outside the tables and states were written"
    return inp, res, paths


# ---- a. every finishing path, every dispatch class ---------------------------------------------------------------------
A_CONFIGS = [cfg for cfg in fo.RUN_CONFIGS if cfg[0] == "MIXED" and cfg[5] is None]
A64_CONFIGS = [cfg for cfg in A_CONFIGS if list(cfg[1]) in ([128], [13, 260], [1024])]


@pytest.mark.parametrize("cfg", A_CONFIGS, ids=fo.run_config_id)
def test_row_norm_family_matches_the_restatement_on_every_finishing_path(cfg):
    inp, res, paths = _run_and_compare(cfg)
    for t in range(len(inp.rows)):
        assert {IN_CHUNK, WAVE_FIXUP, BLOCK_FIXUP} <= set(paths[t].tolist())  # MIXED finishes rows all three ways
    assert res.bounds == 0


@pytest.mark.parametrize("cfg", A64_CONFIGS, ids=fo.run_config_id)
def test_row_norm_family_with_64_bit_sort_keys(cfg):
    inp, res, paths = _run_and_compare(cfg, shift=1 << 33)
    assert all({IN_CHUNK, WAVE_FIXUP, BLOCK_FIXUP} <= set(p.tolist()) for p in paths) and res.bounds == 0


# ---- b. other layouts --------------------------------------------------------------------------------------------------
B_CONFIGS = [cfg for cfg in fo.RUN_CONFIGS if cfg[0] != "MIXED"]


@pytest.mark.parametrize("cfg", B_CONFIGS, ids=fo.run_config_id)
def test_row_norm_family_on_aligned_runs_an_open_tail_and_invalid_ids(cfg):
    """ALIGNED: every run starts and ends on the chunk grid; OPEN_TAIL: a long chain ends at N, N % 32 != 0; INVALID_TAIL:
    out-of-range ids share the last chunks with a real run — counted, and never part of a norm or a state."""
    inp, res, paths = _run_and_compare(cfg)
    assert res.bounds == inp.n_bad * inp.F and (inp.n_bad > 0) == (cfg[0] == "INVALID_TAIL")
    assert inp.N % 32 != 0 or cfg[0] != "OPEN_TAIL"


# ---- c. header contracts of the _ex entries ----------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [[128], [64, 64]], ids=["d128", "d64_64"])
@pytest.mark.parametrize("code", fo.NORM_FAMILY, ids=lambda c: fo.OPT_NAMES[c])
def test_ex_split_phases_flags0_and_a_second_call_give_the_same_bits(code, dims):
    """include/tbe_hip.h: `fused_ex` == `prepare` followed by `apply_ex`; flags 0 is always correct; no float atomics."""
    inp = fo.run_inputs("MIXED", dims, "narrow_sum")
    case = _case(inp, dims, code)
    assert case.uniform_aligned(inp.grad.shape[1])
    opt, ext = _opt(code, 0.01)
    first = case.run(inp, opt, ext=ext)  # TBE_FLAG_UNIFORM_ALIGNED
    for kind in KINDS:
        if case.init[kind] is not None:
            assert all((_bits(a) != _bits(b)).any() for a, b in zip(_got(first)[kind], case.init[kind])), kind
    others = {"a second identical call": case.run(inp, opt, ext=ext), "prepare + apply_ex": case.run(inp, opt, mode="split", ext=ext),
              "flags = 0": case.run(inp, opt, flags=0, ext=ext)}
    for what, r in others.items():
        for kind in KINDS:
            _assert_all_same(_got(r)[kind], _got(first)[kind], f"{what}: {kind}")
        assert r.guards_ok and r.bounds == 0
    assert first.guards_ok and first.bounds == 0


# ---- d. clipping at the chunk edges ------------------------------------------------------------------------------------
# name -> (dims, payload, flags: None = UNIFORM_ALIGNED where it holds)
CLIP_SHAPES = {"d128_fast_kernel_shape": ([128], "narrow_sum"), "d13_260": ([13, 260], "wide_mean")}


@pytest.mark.parametrize("shape", list(CLIP_SHAPES))
@pytest.mark.parametrize("code", [DENSE, SGD], ids=["dense_grad", "sgd"])
def test_clipped_dense_grad_and_sgd_are_bit_exact(code, shape):
    """The clamp sends a launch that TBE_FLAG_UNIFORM_ALIGNED would give a FAST kernel to the generic one; the clamped
    terms are exact (tests/test_backward_run_inputs.py), so the result equals the FP32 oracle fed the clamped gradient."""
    dims, payload = CLIP_SHAPES[shape]
    weighted, pooling = fo.RUN_PAYLOADS[payload]
    inp = fo.run_inputs("MIXED", dims, payload)
    assert (np.abs(inp.grad) > fo.RUN_CLIP).mean() > 0.5
    case = _case(inp, dims, code)
    lr = 0.0 if code == DENSE else 0.05
    flags = None
    if shape == "d128_fast_kernel_shape":
        assert case.uniform_aligned(inp.grad.shape[1])
        flags = FLAG_UNIFORM_ALIGNED
    res = case.run(inp, opt_args(code, lr), pooling, flags=flags, ext=opt_ext(max_gradient=fo.RUN_CLIP))
    clamped = fo.run_inputs("MIXED", dims, payload, fo.RUN_CLIP)
    tabs, s0, _ = case.oracle_tables()
    bad = oracle.tbe_backward(tabs, clamped.indices, clamped.offsets, clamped.grad, code, lr, clamped.psw, pooling, state0=s0)
    assert res.bounds == bad == 0
    _assert_all_same(res.weights, tabs.weights, "weights")
    _assert_all_same(res.state0, s0, "dense gradient")
    after, before = (res.state0, case.init["state0"]) if code == DENSE else (res.weights, case.init["weights"])
    for t in range(len(dims)):
        changed = (_bits(after[t]) != _bits(before[t])).reshape(inp.rows[t], -1).any(axis=1)
        assert not changed[_untouched(inp, t)].any() and changed[inp.touched[t]].all()
    unclamped = case.run(inp, opt_args(code, lr), pooling, flags=flags)
    assert any((_bits(a) != _bits(b)).any() for a, b in zip(after, unclamped.state0 if code == DENSE else unclamped.weights))
    assert res.guards_ok and unclamped.guards_ok


@pytest.mark.parametrize("code", [DENSE, SGD, fo.LAMB, fo.PARTIAL_ROWWISE_ADAM],
                         ids=["dense_grad", "sgd", "LAMB", "PARTIAL_ROWWISE_ADAM"])
def test_a_bound_no_gradient_exceeds_is_bit_identical_to_no_clipping(code):
    dims = [128]
    inp = fo.run_inputs("MIXED", dims, "narrow_sum")
    assert np.abs(inp.grad).max() == 4.0
    case = _case(inp, dims, code)
    if code in fo.NORM_FAMILY:
        opt, _ = _opt(code, 0.01)
    else:
        opt = opt_args(code, 0.0 if code == DENSE else 0.05)
    plain = case.run(inp, opt)  # old codes: the twin entry and its FAST kernel
    wide = case.run(inp, opt, ext=opt_ext(max_gradient=4.0))
    for kind in KINDS:
        _assert_all_same(_got(wide)[kind], _got(plain)[kind], kind)
    assert plain.guards_ok and wide.guards_ok and plain.bounds == wide.bounds == 0


D_CONFIGS = [cfg for cfg in fo.RUN_CONFIGS if cfg[5] is not None]


@pytest.mark.parametrize("cfg", D_CONFIGS, ids=fo.run_config_id)
def test_clipped_row_norm_optimizers_match_the_restatement(cfg):
    inp, res, paths = _run_and_compare(cfg)
    assert res.bounds == 0
    unclipped = fo.run_reference(cfg[:5] + (None,), BackwardCase(inp.rows, list(cfg[1]), code=cfg[3]).init)
    assert fo.norm_error(res.weights[0], unclipped.w[0])[inp.touched[0]].max() > 100  # the clamp did something


# ---- e. FP16 tables ----------------------------------------------------------------------------------------------------
F16_CONFIGS = {"d128_8B_rows": ([128], "narrow_sum"), "d13_260_scalar_rows": ([13, 260], "wide_mean"), "d1024": ([1024], "narrow_sum")}
F16_CODES = (fo.LAMB, fo.PARTIAL_ROWWISE_LAMB)


def _f16_pair(code, config):
    dims, payload = F16_CONFIGS[config]
    inp = fo.run_inputs("MIXED", dims, payload)
    case = _case(inp, dims, code, dtype="float16")
    twin = case.twin_f32()
    opt, ext = _opt(code, 0.01)
    pooling = fo.RUN_PAYLOADS[payload][1]
    ref = twin.run(inp, opt, pooling, ext=ext)  # the _ex_f32 entry on the up-cast table
    assert ref.guards_ok
    return inp, case, opt, ext, pooling, ref


@pytest.mark.parametrize("config", list(F16_CONFIGS))
@pytest.mark.parametrize("code", F16_CODES, ids=lambda c: fo.OPT_NAMES[c])
def test_fp16_tables_nearest_even_is_the_rounded_ex_f32_result(code, config):
    """The arithmetic, norms included, is the _ex_f32 arithmetic on float(w16); only the final store converts."""
    inp, case, opt, ext, pooling, ref = _f16_pair(code, config)
    res = case.run(inp, opt, pooling, ext=ext)
    for t in range(len(case.dims)):
        assert res.weights[t].dtype == np.float16
        _assert_same_bits(res.weights[t], ref.weights[t].astype(np.float16), f"weights of table {t}")
        un = _untouched(inp, t)
        _assert_same_bits(res.weights[t][un], case.init["weights"][t][un], f"weights of table {t}, rows no id names")
    _assert_all_same(res.state0, ref.state0, "state0")
    _assert_all_same(res.state1, ref.state1, "state1")
    assert res.guards_ok and res.bounds == 0


@pytest.mark.parametrize("config", list(F16_CONFIGS))
@pytest.mark.parametrize("code", F16_CODES, ids=lambda c: fo.OPT_NAMES[c])
def test_fp16_tables_stochastic_rounding_stores_a_neighbour_of_the_ex_f32_result(code, config):
    inp, case, opt, ext, pooling, ref = _f16_pair(code, config)
    res = case.run(inp, opt, pooling, rounding=ROUND_STOCHASTIC, seed=1234, ext=ext)
    split = case.run(inp, opt, pooling, mode="split", rounding=ROUND_STOCHASTIC, seed=1234, ext=ext)
    for kind in KINDS:
        _assert_all_same(_got(split)[kind], _got(res)[kind], f"prepare + apply_ex: {kind}")
    _assert_all_same(res.state0, ref.state0, "state0")  # the states never see the rounding
    _assert_all_same(res.state1, ref.state1, "state1")
    up = down = 0
    for t in range(len(case.dims)):
        x = ref.weights[t]
        near = x.astype(np.float16)
        lo = np.where(near.astype(np.float32) <= x, near, np.nextafter(near, np.float16(-np.inf)))
        hi = np.where(near.astype(np.float32) >= x, near, np.nextafter(near, np.float16(np.inf)))
        got = res.weights[t]
        ok = (got == lo) | (got == hi)
        assert ok.all(), f"table {t}: {int((~ok).sum())} stored halves are no neighbour of the f32 result, first at {np.argwhere(~ok)[0]}"
        up += int(((got == hi) & (lo != hi)).sum())
        down += int(((got == lo) & (lo != hi)).sum())
    assert up > 0 and down > 0  # it does round both ways
    assert res.guards_ok and split.guards_ok and res.bounds == 0


# ---- f. the trust-ratio guards on rows the block fix-up finishes -------------------------------------------------------
@pytest.mark.parametrize("code", fo.RUN_GUARD_CODES, ids=lambda c: fo.OPT_NAMES[c])
def test_trust_ratio_guards_on_rows_finished_by_the_block_fixup(code):
    """A row with an exactly zero coalesced gradient (|g| = |u| = 0) and a row of zero weights (|w| = 0), both at the end of
    chains longer than kLongChain chunks: finite, the first unchanged bit for bit, both as the restatement has them."""
    cfg, inp, init, zero_g, zero_w = fo.run_guard_case(code)
    case = _case(inp, cfg[1], code, init=init)
    paths = finishing_paths(inp, case.oracle_tables()[0])
    assert paths[0][zero_g] == paths[0][zero_w] == BLOCK_FIXUP
    opt, ext = _opt(code, 0.0)
    res = case.run(inp, opt, ext=ext)
    _assert_matches_restatement(inp, case, res, fo.run_guard_reference(code), paths, f"guards-{fo.OPT_NAMES[code]}")
    for kind in KINDS:
        if init[kind] is not None:
            _assert_same_bits(_got(res)[kind][0][zero_g], init[kind][0][zero_g], f"{kind} of the zero-gradient row")
    assert res.weights[0][zero_w].any()
    assert res.guards_ok and res.bounds == 0
