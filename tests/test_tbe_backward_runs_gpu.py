"""The fused embedding backward (csrc/tbe_backward_impl.hpp) where a run of equal row keys meets the chunk grid, through the
C ABI and against the oracle: every (lane group, vectors per lane) class, both payload widths, 32- and 64-bit sort keys
(`row_base_shift` 2^33 — the Python module would need 2^32 rows), the generic and the FAST update kernel, rows finished
inside a chunk, by the per-wave fix-up and by the whole-workgroup fix-up.

The inputs (tests/_bwd_abi.py) make the coalesced gradient exact in FP32 in any summation order — guarded on the CPU by
tests/test_backward_run_inputs.py — so DENSE_GRAD (a store) and EXACT_SGD (one fmaf) must match the oracle BIT FOR BIT at
any run length; the stateful optimizers get the exact gradient too and differ from the oracle by their own arithmetic only."""
import numpy as np
import pytest

import _paths  # noqa: F401
from _bwd_abi import (BLOCK_FIXUP, IN_CHUNK, PATH_NAMES, ROUND_STOCHASTIC, WAVE_FIXUP, BackwardCase, finishing_paths,
                      make_inputs, opt_args)
from _util import oracle_backward_mixed
from oracle import oracle

pytestmark = pytest.mark.gpu

SGD, ROWWISE, ADAM, ADAGRAD, DENSE = (oracle.OPT_EXACT_SGD, oracle.OPT_EXACT_ROWWISE_ADAGRAD, oracle.OPT_ADAM,
                                      oracle.OPT_EXACT_ADAGRAD, oracle.OPT_DENSE_GRAD)
LR = 0.05
SHIFTS = [pytest.param(0, id="keys32"), pytest.param(1 << 33, id="keys64")]
# sort payload: the bag number alone (narrow) or (bag, position) (wide: per-sample weights)
PAYLOADS = {"narrow_sum": (False, oracle.POOL_SUM), "wide_sum": (True, oracle.POOL_SUM), "wide_mean": (True, oracle.POOL_MEAN)}
# one per dispatch class of run_apply (max_D <= 64, 128, 256, 512, 1024, 2048) + odd dims under a larger max_D
DIMS_ALL = [[64], [128], [256], [512], [1024], [2048], [7, 13], [13, 260], [40, 12]]
DIMS_FEW = [[128], [13, 260], [1024]]


def _bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _assert_same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    diff = _bits(got) != _bits(want)
    if diff.any():
        rows = np.unique(np.nonzero(diff.reshape(got.shape[0], -1))[0])
        i = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} elements differ in rows {rows[:12].tolist()}"
                             f"{'...' if rows.size > 12 else ''}; first at {i}: got {got[i]!r}, want {want[i]!r}")


def _assert_all_same(got, want, what):
    assert (got is None) == (want is None), what
    for t in range(len(got or [])):
        _assert_same_bits(got[t], want[t], f"{what}, table {t}")


def _untouched(inp, t):
    m = np.ones(inp.rows[t], dtype=bool)
    m[inp.touched[t]] = False
    return m


def _case(inp, dims, shift, code, dtype="float32", ftm=None):
    # [40, 12]: both dims are multiples of 4; moving the second table 4 B off the 16-B grid sends it down the scalar path
    return BackwardCase(inp.rows, dims, ftm, shift, dtype, code, misalign=(1,) if dims == [40, 12] else ())


def _id(layout, dims, payload):
    return f"{layout}-d{'_'.join(map(str, dims))}-{payload}"


# ---- a. coalescing -----------------------------------------------------------------------------------------------------
A_CASES = [pytest.param(lay, d, p, id=_id(lay, d, p))
           for lay, dd in (("MIXED", DIMS_ALL), ("ALIGNED", DIMS_FEW), ("OPEN_TAIL", DIMS_FEW), ("INVALID_TAIL", DIMS_FEW))
           for d in dd for p in PAYLOADS]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("layout,dims,payload", A_CASES)
def test_coalesced_gradient_is_bit_exact(layout, dims, payload, shift):
    weighted, pooling = PAYLOADS[payload]
    inp = make_inputs(layout, dims, weighted=weighted)
    case = _case(inp, dims, shift, DENSE)
    res = case.run(inp, opt_args(DENSE, 0.0), pooling)
    tabs, dense, _ = case.oracle_tables()
    bad = oracle.tbe_backward(tabs, inp.indices, inp.offsets, inp.grad, DENSE, 0.0, inp.psw, pooling, state0=dense)
    assert res.bounds == bad == inp.n_bad * inp.F
    for t in range(len(dims)):
        _assert_same_bits(res.state0[t], dense[t], f"dense gradient of table {t}")
        assert not res.state0[t][_untouched(inp, t)].any(), "a row no id names received a gradient"
        assert np.abs(res.state0[t][inp.touched[t]]).max() > 0
        _assert_same_bits(res.weights[t], case.init["weights"][t], f"weights of table {t} (DENSE_GRAD must not touch them)")
    assert res.guards_ok, "bytes outside the tables were written"


# ---- b. PoolingMode.NONE -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("code", [DENSE, SGD], ids=["dense_grad", "sgd"])
@pytest.mark.parametrize("D", [64, 256])
def test_pooling_none_is_bit_exact(D, code, shift):
    dims = [D, D]  # two features: the position -> feature search of the unpooled linearize has something to find
    inp = make_inputs("MIXED", dims, nobag=True)
    case = _case(inp, dims, shift, code)
    res = case.run(inp, opt_args(code, LR), oracle.POOL_NONE)
    tabs, s0, _ = case.oracle_tables()
    bad = oracle.tbe_backward(tabs, inp.indices, inp.offsets, inp.grad, code, LR, None, oracle.POOL_NONE, state0=s0)
    assert res.bounds == bad == 0
    _assert_all_same(res.weights, tabs.weights, "weights")
    _assert_all_same(res.state0, s0, "dense gradient")
    for t in range(2):
        changed = (_bits(res.state0[t] if code == DENSE else res.weights[t])
                   != _bits(case.init["state0" if code == DENSE else "weights"][t])).reshape(inp.rows[t], -1).any(axis=1)
        assert not changed[_untouched(inp, t)].any() and changed[inp.touched[t]].all()
    assert res.guards_ok


# ---- c. SGD ------------------------------------------------------------------------------------------------------------
# name -> (dims, feature_table_map, payload, flags: None = UNIFORM_ALIGNED where it holds)
SGD_CONFIGS = {
    "d128_fast_kernel": ([128], None, "narrow_sum", None),
    "d128_flags0": ([128], None, "narrow_sum", 0),
    "d13_260": ([13, 260], None, "wide_mean", None),
    "d2048": ([2048], None, "wide_sum", None),
    "two_features_one_table": ([128], [0, 0], "narrow_sum", None),
}


def _assert_sgd_matches(inp, case, res, tabs, bad):
    assert res.bounds == bad == inp.n_bad * inp.F
    _assert_all_same(res.weights, tabs.weights, "weights")
    for t in range(len(inp.rows)):
        un = _untouched(inp, t)
        _assert_same_bits(res.weights[t][un], case.init["weights"][t][un], f"rows of table {t} no id names")
        moved = (_bits(res.weights[t]) != _bits(case.init["weights"][t])).reshape(inp.rows[t], -1).any(axis=1)
        assert moved[inp.touched[t]].all()
    assert res.guards_ok


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("config", list(SGD_CONFIGS))
@pytest.mark.parametrize("layout", ["MIXED", "OPEN_TAIL"])
def test_sgd_is_bit_exact(layout, config, shift):
    dims, ftm, payload, flags = SGD_CONFIGS[config]
    weighted, pooling = PAYLOADS[payload]
    inp = make_inputs(layout, dims, ftm=ftm, weighted=weighted)
    case = _case(inp, dims, shift, SGD, ftm=ftm)
    if config == "d128_fast_kernel":
        assert case.uniform_aligned(inp.grad.shape[1])  # the flag really is passed
    res = case.run(inp, opt_args(SGD, LR), pooling, flags=flags)
    tabs, _, _ = case.oracle_tables()
    bad = oracle.tbe_backward(tabs, inp.indices, inp.offsets, inp.grad, SGD, LR, inp.psw, pooling)
    _assert_sgd_matches(inp, case, res, tabs, bad)


@pytest.mark.parametrize("shift", SHIFTS)
def test_sgd_sum_and_mean_features_in_one_call_is_bit_exact(shift):
    dims, feat_mean = [128, 36], [False, True]
    inp = make_inputs("MIXED", dims, weighted=True)
    case = _case(inp, dims, shift, SGD)
    res = case.run(inp, opt_args(SGD, LR), oracle.POOL_MEAN, feat_pooling=[int(m) for m in feat_mean])
    tabs, _, _ = case.oracle_tables()
    oracle_backward_mixed(tabs, inp.indices, inp.offsets, inp.grad, SGD, LR, inp.psw, feat_mean)
    _assert_sgd_matches(inp, case, res, tabs, 0)


# ---- d. stateful optimizers through every finishing path ---------------------------------------------------------------
OPTS = {
    "rowwise_adagrad": (ROWWISE, dict(eps=1e-3)),
    "rowwise_adagrad_weight_decay": (ROWWISE, dict(eps=1e-3, weight_decay=0.01)),
    "adagrad": (ADAGRAD, dict(eps=1e-3)),
    "adam_weight_decay_iteration3": (ADAM, dict(eps=1e-3, weight_decay=0.02, iteration=3)),
}
STATEFUL_CONFIGS = {"d128": ([128], "narrow_sum"), "d13_260": ([13, 260], "wide_mean"), "d1024": ([1024], "wide_sum")}
TOL = 2e-5  # rtol = atol of test_tbe_gpu.py::test_backward_fused_vs_oracle; the gradient itself is exact here


def _worst_row_per_path(got, want, paths, tol=TOL):
    """{path name: (|got - want| / (atol + rtol |want|) of its worst row, that row)} over the rows ids name, for every
    finishing path the layout has."""
    err = np.abs(got.astype(np.float64) - want) / (tol + tol * np.abs(want.astype(np.float64)))
    err = err.reshape(got.shape[0], -1).max(axis=1)
    out = {}
    for p, name in PATH_NAMES.items():
        rows = np.nonzero(paths == p)[0]
        if rows.size == 0:
            continue
        worst = rows[np.argmax(err[rows])]
        out[name] = (float(err[worst]), int(worst))
    return out


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("config", list(STATEFUL_CONFIGS))
@pytest.mark.parametrize("optname", list(OPTS))
def test_stateful_optimizers_agree_with_the_oracle_on_every_finishing_path(optname, config, shift):
    code, kw = OPTS[optname]
    dims, payload = STATEFUL_CONFIGS[config]
    weighted, pooling = PAYLOADS[payload]
    inp = make_inputs("MIXED", dims, weighted=weighted)
    case = _case(inp, dims, shift, code)
    res = case.run(inp, opt_args(code, LR, **kw), pooling)
    tabs, s0, s1 = case.oracle_tables()
    oracle.tbe_backward(tabs, inp.indices, inp.offsets, inp.grad, code, LR, inp.psw, pooling, state0=s0, state1=s1, **kw)
    paths = finishing_paths(inp, tabs)
    arrays = [("weights", res.weights, tabs.weights, "weights"), ("state0", res.state0, s0, "state0")]
    if s1 is not None:
        arrays.append(("state1", res.state1, s1, "state1"))
    for t in range(len(dims)):
        assert {IN_CHUNK, WAVE_FIXUP, BLOCK_FIXUP} <= set(paths[t].tolist())  # MIXED finishes rows all three ways
        un = _untouched(inp, t)
        for what, got, want, kind in arrays:
            _assert_same_bits(got[t][un], case.init[kind][t][un], f"{what} of table {t}, rows no id names")
            worst = _worst_row_per_path(got[t], want[t], paths[t])
            assert all(e <= 1.0 for e, _ in worst.values()), \
                f"{what} of table {t}: worst (error / tolerance, row) per finishing path: {worst}"
    assert res.bounds == 0 and res.guards_ok


# ---- e. header contracts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("dims", [[128], [64, 64]], ids=["d128", "d64_64"])
@pytest.mark.parametrize("optname", ["sgd"] + list(OPTS))
def test_split_phases_flags0_and_a_second_call_give_the_same_bits(optname, dims, shift):
    """include/tbe_hip.h: `fused` == `prepare` followed by `apply`; flags 0 is always correct; no float atomics."""
    code, kw = OPTS.get(optname, (SGD, {}))
    inp = make_inputs("MIXED", dims)
    case = _case(inp, dims, shift, code)
    assert case.uniform_aligned(inp.grad.shape[1])
    opt = opt_args(code, LR, **kw)
    first = case.run(inp, opt)  # TBE_FLAG_UNIFORM_ALIGNED
    assert (_bits(first.weights[0]) != _bits(case.init["weights"][0])).any()
    others = {"a second identical call": case.run(inp, opt), "prepare + apply": case.run(inp, opt, mode="split"),
              "flags = 0": case.run(inp, opt, flags=0)}
    for what, r in others.items():
        _assert_all_same(r.weights, first.weights, f"{what}: weights")
        _assert_all_same(r.state0, first.state0, f"{what}: state0")
        _assert_all_same(r.state1, first.state1, f"{what}: state1")
        assert r.guards_ok and r.bounds == 0


# ---- f. FP16 tables ----------------------------------------------------------------------------------------------------
F16_CONFIGS = {"d128_8B_rows": ([128], "narrow_sum"), "d13_260_scalar_rows": ([13, 260], "wide_mean"), "d1024": ([1024], "narrow_sum")}
F16_OPTS = {"sgd": (SGD, {}), "rowwise_adagrad": (ROWWISE, dict(eps=1e-3))}


def _f16_pair(optname, config, shift):
    code, kw = F16_OPTS[optname]
    dims, payload = F16_CONFIGS[config]
    weighted, pooling = PAYLOADS[payload]
    inp = make_inputs("MIXED", dims, weighted=weighted)
    case = _case(inp, dims, shift, code, dtype="float16")
    twin = case.twin_f32()
    opt = opt_args(code, LR, **kw)
    ref = twin.run(inp, opt, pooling)  # the _f32 entry on the up-cast table
    assert ref.guards_ok
    return inp, case, opt, pooling, ref


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("config", list(F16_CONFIGS))
@pytest.mark.parametrize("optname", list(F16_OPTS))
def test_fp16_tables_nearest_even_is_the_rounded_f32_result(optname, config, shift):
    """The arithmetic is the _f32 arithmetic on float(w16); only the final store converts."""
    inp, case, opt, pooling, ref = _f16_pair(optname, config, shift)
    res = case.run(inp, opt, pooling)
    for t in range(len(case.dims)):
        assert res.weights[t].dtype == np.float16
        _assert_same_bits(res.weights[t], ref.weights[t].astype(np.float16), f"weights of table {t}")
    _assert_all_same(res.state0, ref.state0, "state0")
    assert res.guards_ok and res.bounds == 0


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("config", list(F16_CONFIGS))
@pytest.mark.parametrize("optname", list(F16_OPTS))
def test_fp16_tables_stochastic_rounding_stores_a_neighbour_of_the_f32_result(optname, config, shift):
    inp, case, opt, pooling, ref = _f16_pair(optname, config, shift)
    res = case.run(inp, opt, pooling, rounding=ROUND_STOCHASTIC, seed=1234)
    split = case.run(inp, opt, pooling, mode="split", rounding=ROUND_STOCHASTIC, seed=1234)
    _assert_all_same(split.weights, res.weights, "prepare + apply: weights")
    _assert_all_same(split.state0, res.state0, "prepare + apply: state0")
    _assert_all_same(res.state0, ref.state0, "state0")  # the state never sees the rounding
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


# ---- g. the 64-id chunk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [DENSE, SGD], ids=["dense_grad", "sgd"])
def test_big_batch_with_64_id_chunks_is_bit_exact(code):
    dims = [16]
    inp = make_inputs("BIG", dims)
    assert inp.N > 524288 and inp.B == inp.N
    case = _case(inp, dims, 0, code)
    assert case.key_bits <= 32
    res = case.run(inp, opt_args(code, LR))
    tabs, s0, _ = case.oracle_tables()
    bad = oracle.tbe_backward(tabs, inp.indices, inp.offsets, inp.grad, code, LR, None, oracle.POOL_SUM, state0=s0)
    assert res.bounds == bad == 0
    _assert_all_same(res.weights, tabs.weights, "weights")
    _assert_all_same(res.state0, s0, "dense gradient")
    un = _untouched(inp, 0)
    after, before = (res.state0, case.init["state0"]) if code == DENSE else (res.weights, case.init["weights"])
    _assert_same_bits(after[0][un], before[0][un], "rows no id names")
    assert res.guards_ok
