"""CPU half of LowRankMixtureCrossNet (torchrec_amd/modules/crossnet.py, the gate kernels of csrc/crossnet.hip): the new
symbols, the numpy restatement in the folded layout (tests/_mixture_crossnet_ref.py) against the reference's recorded runs
(tests/golden/mixture_crossnet.npz, written by tests/golden/make_mixture_crossnet_golden.py from torchrec/modules/
crossnet.py itself), the module's fall-back path against the same, where the GPU tests' two tolerances come from, and that
the faults such kernels can have leave them."""
import os
import re

import numpy as np
import pytest
import torch

import _paths
import _mixture_crossnet_ref as mr
from fbgemm_gpu import _lib

NEW_SYMBOLS = ["tbe_mixture_gate_forward_f32", "tbe_mixture_gate_backward_f32"]
INVALID = -1


def test_new_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(_paths.ROOT, "include", "tbe_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    assert "torchrec/modules/crossnet.py:271-446" in hdr
    assert lib.tbe_abi_version() == 3
    from torchrec_amd.distributed import _device_ops  # noqa: F401

    assert hasattr(torch.ops.tbe_hip, "mixture_gate_forward") and hasattr(torch.ops.tbe_hip, "mixture_gate_backward")
    import torchrec_amd.modules as modules

    assert modules.LowRankMixtureCrossNet is modules.crossnet.LowRankMixtureCrossNet


def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    ok = 0x1000
    entries = {
        "tbe_mixture_gate_forward_f32": lambda B, K, r, first=ok, last=ok: lib.tbe_mixture_gate_forward_f32(
            first, ok, B, K, r, ok, last, None),
        "tbe_mixture_gate_backward_f32": lambda B, K, r, first=ok, last=ok: lib.tbe_mixture_gate_backward_f32(
            first, ok, ok, B, K, r, ok, last, None),
    }
    for name, call in entries.items():
        for K, r, word in ((1, 4, b"K=1"), (17, 4, b"K=17"), (4, 0, b"r=0"), (4, -1, b"r=-1")):
            assert call(8, K, r) == INVALID
            msg = lib.tbe_last_error()
            assert name.encode() in msg and word in msg, msg
        assert call(-1, 4, 4) == INVALID and name.encode() in lib.tbe_last_error()
        for kw in (dict(first=None), dict(last=None)):
            assert call(8, 4, 4, **kw) == INVALID
            assert name.encode() in lib.tbe_last_error() and b"null" in lib.tbe_last_error()
        for kw in (dict(first=ok + 2), dict(last=ok + 1)):
            assert call(8, 4, 4, **kw) == INVALID
            assert name.encode() in lib.tbe_last_error() and b"aligned" in lib.tbe_last_error()
        assert call(0, 4, 4, first=None, last=None) == 0  # the empty batch: success, nothing is looked at
        assert call(0, 1, 4) == INVALID  # but its K and r are still checked


@pytest.mark.parametrize("case", list(mr.CASES))
def test_float64_restatement_equals_the_reference_in_float64(case):
    fx = mr.fixture(case)
    got = mr.run(fx["params"], fx["x"], fx["g"], "float64")
    errs = mr.result_errors(got, fx["f64"])
    assert max(errs.values()) <= 1e-12, errs
    for name, ref in [("out", fx["f64"]["out"]), ("grad_input", fx["f64"]["grad_input"])] + \
            [("grad." + n, a) for n, a in fx["f64"]["grad"].items()]:
        mine = got[name] if not name.startswith("grad.") else got["grad"][name[5:]]
        np.testing.assert_allclose(mine, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    # the softmax weights: the reference recorded them in float32 only
    np.testing.assert_allclose(got["p"], fx["f32"]["p"], rtol=0, atol=1e-6)


def _module(case):
    from torchrec_amd.modules import LowRankMixtureCrossNet

    B, N, L, K, r = mr.CASES[case]
    return LowRankMixtureCrossNet(N, L, num_experts=K, low_rank=r)


@pytest.mark.parametrize("case", list(mr.CASES))
def test_module_on_cpu_loads_the_reference_state_dict_and_reproduces_it(case):
    fx = mr.fixture(case)
    B, N, L, K, r = mr.CASES[case]
    m = _module(case)
    sd = m.state_dict()
    assert list(sd.keys()) == mr.param_names(L, K)  # the reference's keys, in its registration order
    assert list(sd.keys()) == list(fx["params"].keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: v.shape for k, v in fx["params"].items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == mr.param_shapes(N, L, K, r)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in fx["params"].items()}, strict=True)
    x = torch.from_numpy(fx["x"].copy()).requires_grad_()
    out = m(x)
    out.backward(torch.from_numpy(fx["g"].copy()))
    tol = dict(rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(out.detach().numpy(), fx["f32"]["out"], **tol)
    np.testing.assert_allclose(x.grad.numpy(), fx["f32"]["grad_input"], **tol)
    for n, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), fx["f32"]["grad"][n], err_msg=n, **tol)


def test_constructor_assertions_initialisers_and_key_order_are_the_references():
    from torchrec_amd.modules import LowRankMixtureCrossNet

    with pytest.raises(AssertionError, match="num_experts must be larger or equal to 1"):
        LowRankMixtureCrossNet(8, 2, num_experts=0)
    with pytest.raises(AssertionError, match="Low rank must be larger or equal to 1"):
        LowRankMixtureCrossNet(8, 2, num_experts=2, low_rank=0)
    d = LowRankMixtureCrossNet(in_features=8, num_layers=2)
    assert (d._num_experts, d._low_rank, d._activation) == (1, 1, torch.relu) and d.gates is None
    assert list(d.state_dict()) == ["U_kernels.0", "U_kernels.1", "V_kernels.0", "V_kernels.1", "bias.0", "bias.1",
                                    "C_kernels.0", "C_kernels.1"]
    torch.manual_seed(0)
    N, L, K, r = 64, 2, 4, 16
    m = LowRankMixtureCrossNet(N, L, num_experts=K, low_rank=r, activation=torch.nn.ReLU())
    assert list(m.state_dict()) == mr.param_names(L, K)
    # an nn.Module activation registers between the gates and C_kernels, as in the reference
    assert [n for n, _ in m.named_children()] == ["U_kernels", "V_kernels", "bias", "gates", "_activation", "C_kernels"]
    assert isinstance(m.gates, torch.nn.ModuleList) and len(m.gates) == K
    for gate in m.gates:
        assert isinstance(gate, torch.nn.Linear) and gate.bias is None and tuple(gate.weight.shape) == (1, N)
        assert float(gate.weight.detach().abs().max()) <= N ** -0.5  # Linear's own: uniform within 1 / sqrt(fan_in)
    for group in (m.U_kernels, m.V_kernels, m.bias, m.C_kernels):
        assert isinstance(group, torch.nn.ParameterList) and len(group) == L
    for n, p in m.named_parameters():
        if n.startswith("bias"):
            assert not p.any()  # zeros_
        elif not n.startswith("gates"):
            # xavier_normal_ on a 3-D tensor: fan_in = size(1) * size(2), fan_out = size(0) * size(2)
            want = (2.0 / (p.shape[1] * p.shape[2] + p.shape[0] * p.shape[2])) ** 0.5
            assert 0.8 * want < float(p.std()) < 1.25 * want, (n, float(p.std()), want)


def test_the_two_gpu_tolerances_are_measured_not_chosen():
    """gpu_tolerance: 8 x the worst float32-vs-float64 rel_err of the reference's three fixtures and of the float32
    restatement on TRAIN_SHAPES.  Measured when this was written: reference 2.7e-7 ... 1.9e-6 (70x64), restatement 3e-7 ...
    6e-7, tolerance 1.5e-5.  softmax_tolerance: 8 x the worst |p32 - p64| over the gate kernels' shapes, measured 1.4e-7,
    tolerance 1.1e-6.  The host's BLAS and libm move the last digit, hence bands instead of numbers."""
    errs = mr.measured_errors()
    assert len(errs) == len(mr.CASES) + len(mr.TRAIN_SHAPES)
    worst = max(errs.values())
    assert all(e > 0 for e in errs.values()), errs
    assert mr.gpu_tolerance() == 8.0 * worst
    serrs = mr.measured_softmax_errors()
    assert len(serrs) == len(mr.GATE_SHAPES) + 1
    assert mr.softmax_tolerance() == 8.0 * max(serrs.values())
    print(f"gpu_tolerance {mr.gpu_tolerance():.3e} from {errs}")
    print(f"softmax_tolerance {mr.softmax_tolerance():.3e} from {serrs}")
    assert 1e-7 < worst < 1e-5, errs  # float32 rounding over a few hundred addends, nothing else
    assert 2.0 ** -25 <= max(serrs.values()) < 2.0 ** -20, serrs  # a few ulps of numbers below 1


@pytest.mark.parametrize("fault", mr.FAULTS)
def test_every_fault_leaves_the_gpu_tolerance_on_every_train_shape(fault):
    """The premise of the GPU tests: a kernel or a backward with one of these faults could not pass them."""
    tol = mr.gpu_tolerance()
    tried = 0
    for shape in mr.TRAIN_SHAPES:
        B, N, L, K, r = shape
        if fault in mr.GATE_FAULTS and K < 2:
            continue
        p, x, g = mr.gpu_case(*shape)
        errs = mr.result_errors(mr.run(p, x, g, "float64", fault), mr.run(p, x, g, "float64"))
        assert max(errs.values()) > 10 * tol, (fault, shape, errs)
        tried += 1
    assert tried == len(mr.TRAIN_SHAPES)
    # and on the fixtures the module tests compare with (37x20 has no gates; 3x10 is the fall-back, checked all the same)
    for case, (B, N, L, K, r) in mr.CASES.items():
        if fault in mr.GATE_FAULTS and K < 2:
            continue
        fx = mr.fixture(case)
        errs = mr.result_errors(mr.run(fx["params"], fx["x"], fx["g"], "float64", fault), fx["f64"])
        assert max(errs.values()) > 10 * tol, (fault, case, errs)


@pytest.mark.parametrize("shape", mr.GATE_SHAPES + [mr.GATE_SHAPE_OFF_GRID], ids=str)
def test_gate_backward_restatement_is_exact_for_the_abi_tests_inputs(shape):
    """tests/test_mixture_crossnet_abi_gpu.py feeds small integers times powers of two and p in eighths: every product and
    sum is exact in float32, so float32 in two summation orders equals float64 and the comparison there is bit for bit."""
    gm, a2, p = mr.exact_gate_case(*shape)
    assert gm.dtype == a2.dtype == p.dtype == np.float32
    np.testing.assert_array_equal(p.sum(axis=1, dtype=np.float64), 1.0)
    np.testing.assert_array_equal(p * 8, np.round(p * 8))
    assert a2.size < 64 or ((a2 > 0).any() and (a2 < 0).any() and (a2 == 0).any())
    ga, gl = mr.gate_backward(gm, a2, p)
    assert ga.dtype == gl.dtype == np.float32
    ga_r, gl_r = mr.gate_backward(gm, a2, p, reverse=True)
    ga64, gl64 = mr.gate_backward(gm.astype(np.float64), a2.astype(np.float64), p.astype(np.float64))
    for a in (ga, ga_r):
        np.testing.assert_array_equal(a, ga64)
    for a in (gl, gl_r):
        np.testing.assert_array_equal(a, gl64)


def test_gate_forward_restatement_special_values():
    """What the ABI test asks of the kernel holds for the float32 restatement: no NaN for logits 2000 apart, exactly 1 / K
    for equal logits, +0 for a2 <= 0 (a -0.0 included)."""
    a2 = np.array([-1.0, 0.0, -0.0, 2.0], dtype=np.float32).reshape(1, 1, 4).repeat(3, axis=0)
    m, p = mr.gate_forward(a2, np.array([[1000.0, 0.0, -1000.0]], dtype=np.float32))
    np.testing.assert_array_equal(p, [[1.0, 0.0, 0.0]])
    np.testing.assert_array_equal(m[0, :4], [0.0, 0.0, 0.0, 2.0])
    assert not np.signbit(m).any()
    for K in (2, 4, 16):
        _, p = mr.gate_forward(np.ones((K, 2, 1), dtype=np.float32), np.full((2, K), 3.25, dtype=np.float32))
        np.testing.assert_array_equal(p, np.float32(1.0 / K))
