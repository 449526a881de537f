"""CPU half of the cross networks (torchrec_amd/modules/crossnet.py, csrc/crossnet.hip): the new symbols, the numpy
restatement (tests/_crossnet_ref.py) against the reference's recorded runs (tests/golden/crossnet.npz, written by
tests/golden/make_crossnet_golden.py from torchrec/modules/crossnet.py itself), the modules' fall-back path against the
same, where the GPU tests' tolerance comes from, and that the faults such kernels can have leave it."""
import os
import re

import numpy as np
import pytest
import torch

import _paths
import _crossnet_ref as cr
from fbgemm_gpu import _lib

NEW_SYMBOLS = ["tbe_cross_backward_f32", "tbe_cross_backward_workspace_bytes", "tbe_vector_cross_forward_f32",
               "tbe_vector_cross_backward_f32", "tbe_vector_cross_backward_workspace_bytes"]
ALL = [(k, c) for k in cr.KINDS for c in cr.CASES]
IDS = [f"{k}-{c}" for k, c in ALL]


def test_new_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(_paths.ROOT, "include", "tbe_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    assert "torchrec/modules/crossnet.py:" in hdr
    assert lib.tbe_abi_version() == 3


def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    INVALID = -1
    assert lib.tbe_cross_backward_f32(None, None, None, 4, 6, 1, None, None, 0x1000, None, 0, None) == INVALID
    assert b"multiple of 4" in lib.tbe_last_error()
    assert lib.tbe_cross_backward_f32(None, None, None, 65536 * 64, 4, 1, 0x1000, 0x1000, 0x1000, None, 0, None) == INVALID
    for N, L in ((4100, 1), (64, 9)):
        for rc in (lib.tbe_vector_cross_forward_f32(None, None, None, 4, N, L, None, None, None),
                   lib.tbe_vector_cross_backward_f32(None, None, None, None, None, 4, N, L, None, None, None, 0, None)):
            assert rc == INVALID
            msg = lib.tbe_last_error()
            assert b"N <= 4096" in msg and b"L <= 8" in msg
    # more row blocks than a grid dimension allows
    ws = lib.tbe_cross_backward_workspace_bytes(65536 * 64, 4)
    assert lib.tbe_cross_backward_f32(0x1000, 0x1000, 0x1000, 65536 * 64, 4, 1, 0x1000, 0x1000, 0x1000, 0x1000, ws,
                                      None) == INVALID
    assert b"row blocks" in lib.tbe_last_error()
    assert lib.tbe_cross_backward_workspace_bytes(65, 64) >= 2 * 64 * 4
    assert lib.tbe_cross_backward_workspace_bytes(257, 516) >= 2 * 516 * 4
    assert lib.tbe_vector_cross_backward_workspace_bytes(130, 260, 3) >= 2 * (2 * 3 * 260) * 4


@pytest.mark.parametrize("kind,case", ALL, ids=IDS)
def test_float64_restatement_equals_the_reference_in_float64(kind, case):
    fx = cr.fixture(kind, case)
    got = cr.run(kind, fx["params"], fx["x"], fx["g"], "float64")
    errs = cr.result_errors(got, fx["f64"])
    assert max(errs.values()) <= 1e-12, errs
    for name, ref in [("out", fx["f64"]["out"]), ("grad_input", fx["f64"]["grad_input"])] + \
            [("grad." + n, a) for n, a in fx["f64"]["grad"].items()]:
        mine = got[name] if not name.startswith("grad.") else got["grad"][name[5:]]
        np.testing.assert_allclose(mine, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("kind,case", ALL, ids=IDS)
def test_float32_restatement_is_bit_equal_where_no_reduction_is_involved(kind, case):
    """Given the reference's recorded per-layer GEMM results (row dots), the element-wise part of every layer in float32
    — the operation order csrc/crossnet.hip follows — reproduces the reference's float32 output bit for bit."""
    fx = cr.fixture(kind, case)
    B, N, L, r = cr.CASES[case]
    x0 = fx["x"]
    assert x0.dtype == np.float32 and fx["y"].dtype == np.float32
    x_l = x0
    for l in range(L):
        b = fx["params"][f"bias.{l}"].reshape(N)
        if kind == "VectorCrossNet":
            x_l = cr.vector_layer_from_s(x0, x_l, fx["y"][l], b)
        else:
            x_l = cr.layer_from_y(x0, x_l, fx["y"][l], b)
        assert x_l.dtype == np.float32
    np.testing.assert_array_equal(x_l, fx["f32"]["out"])


def _module(kind, N, L, r):
    from torchrec_amd.modules import crossnet

    if kind == "LowRankCrossNet":
        return crossnet.LowRankCrossNet(N, L, low_rank=r)
    return getattr(crossnet, kind)(N, L)


@pytest.mark.parametrize("kind,case", ALL, ids=IDS)
def test_modules_on_cpu_load_the_reference_state_dict_and_reproduce_it(kind, case):
    fx = cr.fixture(kind, case)
    B, N, L, r = cr.CASES[case]
    m = _module(kind, N, L, r)
    sd = m.state_dict()
    assert list(sd.keys()) == cr.param_names(kind, L)  # the reference's keys, in its order
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: v.shape for k, v in fx["params"].items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == cr.param_shapes(kind, N, L, r)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in fx["params"].items()}, strict=True)
    x = torch.from_numpy(fx["x"].copy()).requires_grad_()
    out = m(x)
    out.backward(torch.from_numpy(fx["g"].copy()))
    tol = dict(rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(out.detach().numpy(), fx["f32"]["out"], **tol)
    np.testing.assert_allclose(x.grad.numpy(), fx["f32"]["grad_input"], **tol)
    for n, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), fx["f32"]["grad"][n], err_msg=n, **tol)


def test_constructors_and_initialisers_are_the_references():
    from torchrec_amd.modules import CrossNet, LowRankCrossNet, VectorCrossNet

    with pytest.raises(AssertionError, match="Low rank must be larger or equal to 1"):
        LowRankCrossNet(8, 2, low_rank=0)
    assert LowRankCrossNet(in_features=8, num_layers=2)._low_rank == 1
    torch.manual_seed(0)
    for m in (CrossNet(in_features=64, num_layers=2), LowRankCrossNet(64, 2, 16), VectorCrossNet(64, 2)):
        assert isinstance(m.bias, torch.nn.ParameterList) and len(m.bias) == 2
        for n, p in m.named_parameters():
            if n.startswith("bias"):
                assert not p.any()  # zeros_
            else:  # xavier_normal_: std = sqrt(2 / (fan_in + fan_out))
                want = (2.0 / sum(p.shape)) ** 0.5
                assert 0.6 * want < float(p.std()) < 1.4 * want, (n, float(p.std()), want)


def test_the_gpu_tolerance_is_measured_not_chosen():
    """8 x the worst float32-vs-float64 error of the reference's own fixtures and of the float32 restatement on the GPU
    tests' shapes.  Measured when this was written: reference 1.0e-7 ... 3.4e-7, restatement 5.8e-8 ... 6.2e-7 (the
    low-rank net at 130 x 260), tolerance 5.0e-6; summation order of the host's BLAS moves the last
    digit, hence the band instead of a number."""
    errs = cr.measured_errors()
    assert len(errs) == 9 + len(cr.VECTOR_GPU_SHAPES) + 3
    worst = max(errs.values())
    assert all(e > 0 for k, e in errs.items()), errs
    assert 1e-7 < worst < 2e-6, errs
    assert cr.gpu_tolerance() == 8.0 * worst
    for k, e in errs.items():
        if k.startswith("reference"):
            assert 5e-8 < e < 6e-7, (k, e)


def _premise_shapes():
    for B, N, L in cr.VECTOR_GPU_SHAPES:
        yield "VectorCrossNet", B, N, L, 1
    for kind in cr.KINDS:
        yield (kind,) + cr.TRAIN_SHAPE


@pytest.mark.parametrize("fault", cr.FAULTS)
def test_every_fault_leaves_the_gpu_tolerance_on_the_gpu_test_shapes(fault):
    """The premise of the GPU tests: a kernel with one of these faults could not pass them.  A fault is tried wherever the
    net has the operation: row dots only in VectorCrossNet, an accumulated acc only from two layers on."""
    tol = cr.gpu_tolerance()
    tried = 0
    for kind, B, N, L, r in _premise_shapes():
        if fault == "dot_last_col" and kind != "VectorCrossNet":
            continue
        if fault == "acc_overwrite" and L < 2:
            continue
        p, x, g = cr.gpu_case(kind, B, N, L, r)
        errs = cr.result_errors(cr.run(kind, p, x, g, "float64", fault), cr.run(kind, p, x, g, "float64"))
        assert max(errs.values()) > 10 * tol, (kind, B, N, L, errs)
        tried += 1
    assert tried >= 6
    # and on the fixtures the module tests compare with (N = 10 is the fall-back, checked all the same)
    for kind, case in ALL:
        if fault == "dot_last_col" and kind != "VectorCrossNet":
            continue
        fx = cr.fixture(kind, case)
        errs = cr.result_errors(cr.run(kind, fx["params"], fx["x"], fx["g"], "float64", fault), fx["f64"])
        assert max(errs.values()) > 10 * tol, (kind, case, errs)


def test_cross_backward_restatement_is_exact_for_the_abi_tests_inputs():
    """tests/test_crossnet_abi_gpu.py feeds small integers scaled by powers of two: every product, add and column sum is
    exact in float32, so the comparison there is bit for bit in any summation order."""
    from _crossnet_ref import cross_backward_f32

    rng = np.random.default_rng(3)
    B, N = 300, 128
    G, x0, t, acc = (rng.integers(-4, 5, (B, N)).astype(np.float32) * s for s in (0.25, 0.5, 0.25, 0.125))
    for first in (True, False):
        gy, a, gb = cross_backward_f32(G, x0, t, acc, first)
        gy64, gt64 = G.astype(np.float64) * x0, G.astype(np.float64) * t
        np.testing.assert_array_equal(gy, gy64)
        np.testing.assert_array_equal(a, gt64 if first else acc + gt64)
        np.testing.assert_array_equal(gb, gy64.sum(0))
        np.testing.assert_array_equal(gb, gy[::-1].sum(0, dtype=np.float32))
