"""CPU: torchrec_amd.modules.loss — the float64 restatement the GPU tests compare with (tests/_cross_entropy_ref.py), the
measured float32 error of torch's own cross_entropy that sets their tolerance, the torch fallback, and the edge values
(all rows ignored, R = 0, -inf entries) as torch gives them."""
import inspect

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _paths  # noqa: F401
import _cross_entropy_ref as cr
from torchrec_amd.modules.loss import CrossEntropyLoss, cross_entropy


@pytest.mark.parametrize("reduction", cr.REDUCTIONS)
def test_the_restatement_is_torchs_cross_entropy_in_float64(reduction):
    for R, V, share in ((1, 1, 1.0), (7, 5, 1.0), (40, 65, 0.15), (9, 1025, 0.5)):
        x, target = cr.gpu_case(R, V, share)
        g = cr.grad_out_for(R, reduction)
        e = cr.result_errors(cr.run(x, target, cr.IGNORE, reduction, g),
                             cr.torch_run(x, target, cr.IGNORE, reduction, g, dtype=torch.float64))
        assert max(e.values()) <= 1e-13, (R, V, e)


def test_premise_a_restatement_that_reads_ignored_rows_or_forgets_the_one_hot_is_far_outside_the_tolerance():
    tol = cr.gpu_tolerance()
    x, target = cr.gpu_case(40, 65, 0.15)
    g = cr.grad_out_for(40, "mean")
    want = cr.run(x, target, cr.IGNORE, "mean", g)
    counted = cr.run(x, np.where(target == cr.IGNORE, 0, target), cr.IGNORE, "mean", g)  # ignored rows counted as label 0
    assert cr.result_errors(counted, want)["loss"] > 1e3 * tol["loss"]
    no_onehot = dict(want, grad=want["grad"] + (np.arange(65)[None, :] == target[:, None]) * (g / want["n_valid"]))
    assert cr.result_errors(no_onehot, want)["grad"] > 1e3 * tol["grad"]


def test_measured_float32_error_of_torch_on_the_gpu_tests_inputs():
    """The tolerance of the GPU tests is 8 x these two numbers; here they are printed and bracketed by what float32 can
    give: not below a tenth of an ulp (the comparison would be vacuous), not above 64 ulp of the scale."""
    err = cr.measured_errors()
    print(f"F.cross_entropy float32 vs float64 on the GPU tests' inputs: loss {err['loss']:.3e}, grad {err['grad']:.3e}; "
          f"tolerance {cr.gpu_tolerance()}")
    eps = 2.0 ** -24
    for k in ("loss", "grad"):
        assert 0.1 * eps <= err[k] <= 64 * eps, err


@pytest.mark.parametrize("reduction", cr.REDUCTIONS)
def test_cpu_tensors_take_torch_bit_for_bit(reduction):
    x, target = cr.gpu_case(33, 65, 0.5)
    target = np.where(target == cr.IGNORE, 0, target)  # the reference's ignore_index = 0
    leaves = [torch.from_numpy(x).clone().requires_grad_() for _ in range(2)]
    t = torch.from_numpy(target)
    g = torch.from_numpy(np.asarray(cr.grad_out_for(33, reduction)))
    ours = CrossEntropyLoss(ignore_index=0, reduction=reduction)(leaves[0], t)
    theirs = F.cross_entropy(leaves[1], t, ignore_index=0, reduction=reduction)
    ours.backward(g)
    theirs.backward(g)
    assert torch.equal(ours, theirs) and torch.equal(leaves[0].grad, leaves[1].grad)
    assert torch.equal(cross_entropy(leaves[0], t, 0, reduction), theirs)


def test_everything_outside_the_kernel_conditions_is_torchs_result():
    x = torch.randn(4, 6, 5)
    t3 = torch.randint(0, 6, (4, 5))
    assert torch.equal(cross_entropy(x, t3), F.cross_entropy(x, t3))                      # rank 3
    probs = torch.softmax(torch.randn(4, 6), 1)
    assert torch.equal(cross_entropy(x[:, :, 0], probs), F.cross_entropy(x[:, :, 0], probs))  # probability targets, stride 5
    xd = torch.randn(4, 6, dtype=torch.float64)
    t = torch.randint(0, 6, (4,))
    assert torch.equal(cross_entropy(xd, t), F.cross_entropy(xd, t))                      # another dtype
    with pytest.raises(ValueError):
        cross_entropy(torch.randn(4, 6), t, reduction="median")


def test_weight_and_label_smoothing_are_not_parameters():
    for fn in (CrossEntropyLoss.__init__, cross_entropy):
        names = set(inspect.signature(fn).parameters)
        assert "weight" not in names and "label_smoothing" not in names
        assert {"ignore_index", "reduction"} <= names
    with pytest.raises(TypeError):
        CrossEntropyLoss(weight=torch.ones(3))
    with pytest.raises(TypeError):
        CrossEntropyLoss(label_smoothing=0.1)
    with pytest.raises(ValueError):
        CrossEntropyLoss(reduction="median")
    ce = CrossEntropyLoss()
    assert (ce.ignore_index, ce.reduction) == (-100, "mean") and "ignore_index=-100" in repr(ce)


@pytest.mark.parametrize("R", [0, 6])
def test_all_rows_ignored_or_no_rows_mean_is_nan_with_a_zero_gradient(R):
    """What torch gives, and what the restatement (and with it the kernel tests) pins."""
    x = torch.randn(R, 5, requires_grad=True)
    t = torch.zeros(R, dtype=torch.int64)
    loss = cross_entropy(x, t, ignore_index=0, reduction="mean")
    loss.backward()
    assert bool(torch.isnan(loss)) and torch.equal(x.grad, torch.zeros(R, 5))
    ref = cr.run(x.detach().numpy(), t.numpy(), 0, "mean", np.float32(1.0))
    assert np.isnan(ref["loss"]) and not ref["grad"].any() and ref["n_valid"] == 0
    for red, want in (("sum", 0.0), ("none", np.zeros(R))):
        got = cross_entropy(x.detach(), t, ignore_index=0, reduction=red)
        np.testing.assert_array_equal(got.numpy(), np.asarray(want, dtype=np.float32))
        np.testing.assert_array_equal(cr.run(x.detach().numpy(), t.numpy(), 0, red, cr.grad_out_for(R, red))["loss"], want)


def test_minus_inf_entries_are_ordinary_values():
    """A masked logit has probability 0 and gradient 0; the rest of the row is the cross-entropy of the unmasked entries."""
    x, target = cr.gpu_case(9, 12)
    masked = x.copy()
    cols = np.array([1, 4, 5, 10])
    target = np.where(np.isin(target, cols), 0, target)
    masked[:, cols] = -np.inf
    keep = np.setdiff1d(np.arange(12), cols)
    g = cr.grad_out_for(9, "mean")
    full = cr.run(masked, target, cr.IGNORE, "mean", g)
    small = cr.run(x[:, keep], np.searchsorted(keep, target), cr.IGNORE, "mean", g)
    np.testing.assert_allclose(full["loss"], small["loss"], rtol=1e-14)
    assert not full["grad"][:, cols].any()
    np.testing.assert_allclose(full["grad"][:, keep], small["grad"], rtol=1e-12, atol=1e-15)
    got = cr.torch_run(masked, target, cr.IGNORE, "mean", g)
    assert np.isfinite(got["loss"]) and not got["grad"][:, cols].any()
    assert max(cr.result_errors(got, full).values()) <= 64 * 2.0 ** -24
