"""CPU half of SwishLayerNorm (torchrec_amd/modules/activation.py, csrc/swish_layernorm.hip) and of the activations MLP
accepts (torchrec_amd/modules/mlp.py, utils.py): the new symbols, the module's fall-back path and MLP("swish_layernorm")
against the reference's recorded runs (tests/golden/swish_layernorm.npz, written by
tests/golden/make_swish_layernorm_golden.py from torchrec/modules/activation.py and mlp.py themselves), the reference's
activation contract of MLP, the numpy restatement (tests/_swish_layernorm_ref.py) against the same fixtures, where the GPU
tests' tolerance comes from, and that the faults such kernels can have leave it."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import _paths
import _swish_layernorm_ref as sr
from fbgemm_gpu import _lib

NEW_SYMBOLS = ["tbe_swish_layernorm_forward_f32", "tbe_swish_layernorm_backward_f32",
               "tbe_swish_layernorm_backward_workspace_bytes"]
INVALID = -1


def _t(a):
    return torch.from_numpy(np.array(a))


def test_new_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(_paths.ROOT, "include", "tbe_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    assert "torchrec/modules/activation.py:18-55" in hdr
    assert lib.tbe_abi_version() == 3


def test_entries_refuse_bad_arguments_before_any_launch():
    """No device is needed: every check precedes the first launch, so made-up addresses are never touched."""
    lib = _lib.load()
    P = 0x1000

    def fwd(B=4, N=64, eps=1e-5, y=P, stats=P):
        return lib.tbe_swish_layernorm_forward_f32(y, P, P, eps, B, N, P, stats, None), lib.tbe_last_error()

    def bwd(B=4, N=64, g=P, gp=P, ws=P, ws_bytes=1 << 20):
        return lib.tbe_swish_layernorm_backward_f32(g, P, P, P, P, B, N, P, gp, ws, ws_bytes, None), lib.tbe_last_error()

    for call in (fwd, bwd):
        for N in (0, -4, 6):
            rc, msg = call(N=N)
            assert rc == INVALID and b"multiple of 4" in msg, (N, msg)
        rc, msg = call(N=4100)
        assert rc == INVALID and b"N <= 4096" in msg
        rc, msg = call(B=-1)
        assert rc == INVALID
        # more row blocks than a grid dimension allows: 2^31 blocks of 128 rows (N <= 64) / 16 rows (N > 1024)
        for N, rows in ((4, 128), (4096, 16)):
            rc, msg = call(B=(1 << 31) * rows, N=N)
            assert rc == INVALID and b"row blocks" in msg
    for eps in (float("nan"), float("inf"), -1e-5):
        rc, msg = fwd(eps=eps)
        assert rc == INVALID and b"eps" in msg, eps
    rc, msg = fwd(y=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = fwd(y=P + 4)
    assert rc == INVALID and b"aligned" in msg
    rc, msg = fwd(stats=P + 2)
    assert rc == INVALID and b"aligned" in msg
    rc, msg = bwd(gp=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = bwd(g=None)
    assert rc == INVALID and b"null" in msg
    rc, msg = bwd(g=P + 8)
    assert rc == INVALID and b"aligned" in msg
    rc, msg = bwd(ws=P + 4)
    assert rc == INVALID and b"aligned" in msg
    need = lib.tbe_swish_layernorm_backward_workspace_bytes(70, 68)
    assert need >= 3 * 2 * 68 * 4  # three row blocks of 32 rows, two sums per column
    rc, msg = bwd(B=70, N=68, ws_bytes=need - 256)
    assert rc == INVALID and b"workspace" in msg
    for (B, N) in sr.abi_shapes():
        blocks = -(-B // sr.rows_per_block(N))
        assert lib.tbe_swish_layernorm_backward_workspace_bytes(B, N) >= blocks * 2 * N * 4
    assert fwd(B=0)[0] == 0  # the empty batch launches nothing


# ---- the module on its fall-back path ------------------------------------------------------------------------------------------
def _module(case):
    from torchrec_amd.modules import SwishLayerNorm

    lead, dims = sr.CASES[case]
    return SwishLayerNorm(dims[0] if len(dims) == 1 else dims)


@pytest.mark.parametrize("case", list(sr.CASES))
def test_module_on_cpu_loads_the_reference_state_dict_and_reproduces_it(case):
    """The fall-back is the reference's expression on the same torch: when this was written the output and the input
    gradient came out bit for bit and the gamma / beta gradients within 3.1e-7 (torch's CPU layer norm sums the rows of its
    parameter gradients in an order that depends on its thread count and build), so the assertion allows `gpu_tolerance()`.
    The printed errors say what it was."""
    fx = sr.fixture(case)
    m = _module(case)
    assert isinstance(m.norm, nn.Sequential) and isinstance(m.norm[0], nn.LayerNorm) and isinstance(m.norm[1], nn.Sigmoid)
    assert list(m.state_dict().keys()) == ["norm.0.weight", "norm.0.bias"]
    m.load_state_dict({k: _t(v) for k, v in fx["params"].items()}, strict=True)
    x = _t(fx["x"]).requires_grad_()
    out = m(x)
    assert out.shape == x.shape
    out.backward(_t(fx["g"]))
    got = {"out": out.detach().numpy(), "grad_input": x.grad.numpy(),
           "grad": {n: p.grad.numpy() for n, p in m.named_parameters()}}
    errs = sr.result_errors(sr.flat(case, got), sr.flat(case, fx["f32"]))
    print(f"{case}: errors against the reference's float32 run {errs}")
    assert max(errs.values()) <= sr.gpu_tolerance(), errs


def test_double_backward_runs_through_the_module():
    m = _module("37x20").double()
    x = torch.randn(5, 20, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradgradcheck(m, (x,))


# ---- MLP's activations ---------------------------------------------------------------------------------------------------------
def test_mlp_with_swish_layernorm_matches_the_reference():
    from torchrec_amd.modules.activation import SwishLayerNorm
    from torchrec_amd.modules.mlp import MLP

    fx = sr.mlp_fixture()
    m = MLP(*sr.MLP_ARGS, activation="swish_layernorm")
    assert list(m.state_dict().keys()) == sr.mlp_keys()
    acts = [p._activation_fn for p in m._mlp]
    assert all(isinstance(a, SwishLayerNorm) for a in acts) and len({id(a) for a in acts}) == 3
    assert [a.norm[0].normalized_shape for a in acts] == [(16,), (8,), (4,)]
    m.load_state_dict({k: _t(v) for k, v in fx["params"].items()}, strict=True)
    x = _t(fx["x"]).requires_grad_()
    out = m(x)
    out.backward(_t(fx["g"]))
    tol = sr.gpu_tolerance()
    ref = fx["f32"]
    errs = {"out": sr.rel_err(out.detach().numpy(), ref["out"]), "grad_input": sr.rel_err(x.grad.numpy(), ref["grad_input"])}
    for n, p in m.named_parameters():
        errs[n] = sr.rel_err(p.grad.numpy(), ref["grad"][n])
    print(f"MLP swish_layernorm: errors against the reference's float32 run {errs}")
    assert max(errs.values()) <= tol, errs


def test_mlp_calls_a_module_factory_once_per_layer():
    from torchrec_amd.modules.mlp import MLP

    m = MLP(40, [16, 8, 4], activation=nn.ReLU)
    acts = [p._activation_fn for p in m._mlp]
    assert all(isinstance(a, nn.ReLU) for a in acts) and len({id(a) for a in acts}) == 3
    x = torch.randn(3, 40)
    out = m(x)
    assert out.shape == (3, 4) and bool((out >= 0).all())
    twin = MLP(40, [16, 8, 4], activation="relu")
    twin.load_state_dict(m.state_dict(), strict=True)  # a parameter-free activation module adds no keys
    assert torch.equal(out, twin(x))


def test_torch_relu_and_other_tensor_callables_come_back_as_the_same_object():
    """Perceptron's fused ReLU path and relu_linear1_head test `_activation_fn is torch.relu`."""
    from torchrec_amd.modules import extract_module_or_tensor_callable
    from torchrec_amd.modules.mlp import MLP

    assert extract_module_or_tensor_callable(torch.relu) is torch.relu
    for name, fn in (("relu", torch.relu), ("sigmoid", torch.sigmoid)):
        for m in (MLP(8, [4, 4], activation=fn), MLP(8, [4, 4], activation=name)):
            assert all(p._activation_fn is fn for p in m._mlp)
    assert all(p._activation_fn is torch.relu for p in MLP(8, [4, 4])._mlp)
    lam = lambda t: t * 2  # noqa: E731
    inst = nn.Tanh()
    for act in (lam, inst):  # a module INSTANCE is shared by the layers, as in the reference
        assert all(p._activation_fn is act for p in MLP(8, [4, 4], activation=act)._mlp)


def test_factory_contract():
    from torchrec_amd.modules.mlp import MLP
    from torchrec_amd.modules.utils import extract_module_or_tensor_callable

    assert isinstance(extract_module_or_tensor_callable(lambda: nn.Sigmoid()), nn.Sigmoid)
    with pytest.raises(ValueError, match="torch.nn.Module"):
        extract_module_or_tensor_callable(lambda: 3)
    with pytest.raises(ValueError, match="torch.nn.Module"):
        MLP(8, [4], activation=lambda: torch.relu)

    def broken():
        raise TypeError("something else")

    with pytest.raises(TypeError, match="something else"):
        extract_module_or_tensor_callable(broken)
    with pytest.raises(ValueError, match="swish_layernorm"):
        MLP(8, [4], activation="gelu")


# ---- the restatement and the tolerance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(sr.CASES))
def test_restatement_equals_the_reference(case):
    fx = sr.fixture(case)
    e64 = sr.result_errors(sr.run_fixture(case, "float64"), sr.flat(case, fx["f64"]))
    assert max(e64.values()) <= 1e-12, e64
    got32 = sr.run_fixture(case, "float32")
    assert all(v.dtype == np.float32 for v in got32.values())
    e32 = sr.result_errors(got32, sr.flat(case, fx["f64"]))
    assert max(e32.values()) <= sr.gpu_tolerance(), e32


def test_the_gpu_tolerance_is_measured_not_chosen():
    """8 x the worst float32-vs-float64 error of the reference's own fixtures and of the float32 restatement on the GPU
    tests' shapes.  Measured when this was written: reference 1.6e-7 ... 6.8e-7 (37 x 20), restatement 1.3e-7 ... 4.2e-7,
    tolerance 5.5e-6; numpy's summation order moves the last digit, hence the band instead of a number."""
    errs = sr.measured_errors()
    assert len(errs) == len(sr.CASES) + len(sr.gpu_test_shapes())
    assert all(N > 1 for _, N in sr.gpu_test_shapes())
    worst = max(errs.values())
    print(f"measured float32 errors {min(errs.values()):.2e} ... {worst:.2e}; tolerance {sr.gpu_tolerance():.3e}")
    assert all(e > 0 for e in errs.values()), errs
    assert 1e-7 < worst < 2e-6, errs
    assert sr.gpu_tolerance() == 8.0 * worst


@pytest.mark.parametrize("fault", sr.FAULTS)
def test_every_fault_leaves_the_gpu_tolerance_on_the_gpu_test_shapes(fault):
    """The premise of the GPU tests: a kernel that drops one column from one of its four row reductions, or one row from
    one of its two column sums, could not pass them at any of their shapes."""
    tol = sr.gpu_tolerance()
    for B, N in sr.gpu_test_shapes():
        c = sr.gpu_case(B, N)
        errs = sr.result_errors(sr.run(*c, fault=fault), sr.run(*c))
        assert max(errs.values()) > tol, (B, N, errs)
    for case in sr.CASES:  # and on the fixtures the module tests compare with
        errs = sr.result_errors(sr.run_fixture(case, fault=fault), sr.flat(case, sr.fixture(case)["f64"]))
        assert max(errs.values()) > tol, (case, errs)
