"""GPU: torchrec_amd.modules.loss on the kernel path against F.cross_entropy in float64 on the same values, within the
tolerance of tests/test_cross_entropy_abi_gpu.py; autograd plumbing, HIP graph capture with a changing number of valid rows,
peak memory, and two BERT4Rec training steps against nn.CrossEntropyLoss."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _cross_entropy_ref as cr
from torchrec_amd.modules import loss as L
from torchrec_amd.modules.loss import CrossEntropyLoss, cross_entropy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _on_kernel_path(t):
    return type(t.grad_fn).__name__ == L._CrossEntropy.__name__ + "Backward"


def _module_run(x, target, ignore, reduction, g):
    """The module's loss and gradient for a device tensor x (any strides)."""
    leaf = x.detach().requires_grad_()
    loss = CrossEntropyLoss(ignore_index=ignore, reduction=reduction)(leaf, target)
    assert _on_kernel_path(loss)  # not the fallback
    loss.backward(torch.from_numpy(np.asarray(g)).to(DEV))
    return {"loss": loss.detach().cpu().numpy(), "grad": leaf.grad.cpu().numpy()}


@pytest.mark.parametrize("reduction", cr.REDUCTIONS)
@pytest.mark.parametrize("R,V,share", [(300, 1025, 0.15), (37, 65, 1.0), (5, 26746, 1.0)])
def test_module_matches_torch_in_float64(R, V, share, reduction):
    x, target = cr.gpu_case(R, V, share)
    g = cr.grad_out_for(R, reduction)
    want = cr.torch_run(x, target, cr.IGNORE, reduction, g, dtype=torch.float64, device=DEV)
    got = _module_run(torch.from_numpy(x).to(DEV), torch.from_numpy(target).to(DEV), cr.IGNORE, reduction, g)
    errs, tol = cr.result_errors(got, want), cr.gpu_tolerance()
    print(f"module {R}x{V}@{share} {reduction}: tolerance {tol}, errors {errs}")
    assert errs["loss"] <= tol["loss"] and errs["grad"] <= tol["grad"]


def test_rows_of_a_wider_buffer_go_in_as_they_are():
    R, V = 37, 1025
    x, target = cr.gpu_case(R, V, 0.5)
    wide = torch.full((R, V + 7), float("nan"), device=DEV)
    wide[:, 3:3 + V] = torch.from_numpy(x).to(DEV)
    view = wide[:, 3:3 + V]
    assert not view.is_contiguous() and view.stride() == (V + 7, 1)
    t = torch.from_numpy(target).to(DEV)
    a = _module_run(view, t, cr.IGNORE, "mean", np.float32(1.0))
    b = _module_run(torch.from_numpy(x).to(DEV), t, cr.IGNORE, "mean", np.float32(1.0))
    np.testing.assert_array_equal(a["loss"].view(np.uint32), b["loss"].view(np.uint32))
    np.testing.assert_array_equal(a["grad"].view(np.uint32), b["grad"].view(np.uint32))
    # a non-unit inner stride takes torch
    xt = torch.from_numpy(x).to(DEV).t().contiguous().t().requires_grad_()
    assert xt.stride(1) != 1
    assert not _on_kernel_path(cross_entropy(xt, t))


def test_requires_grad_false_and_no_grad_keep_nothing():
    x, target = cr.gpu_case(37, 65, 0.5)
    xt, t = torch.from_numpy(x).to(DEV), torch.from_numpy(target).to(DEV)
    plain = cross_entropy(xt, t)
    assert not plain.requires_grad and plain.grad_fn is None
    leaf = xt.clone().requires_grad_()
    with torch.no_grad():
        quiet = cross_entropy(leaf, t)
    assert not quiet.requires_grad and quiet.grad_fn is None
    tracked = cross_entropy(leaf, t)
    assert torch.equal(plain, quiet) and torch.equal(plain, tracked.detach())
    assert torch.equal(plain.cpu(), torch.from_numpy(_module_run(xt, t, cr.IGNORE, "mean", np.float32(1.0))["loss"]))
    # double backward goes through differentiable torch operations
    (gx,) = torch.autograd.grad(tracked, leaf, create_graph=True)
    gx.square().sum().backward()
    assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all())


def test_captured_step_follows_labels_overwritten_in_place():
    """Forward + backward captured on one stream; the replay after the labels changed IN PLACE, to a different number of
    valid rows, gives the new loss and gradient: the divisor is read on the device."""
    R, V = 64, 1025
    x, first = cr.gpu_case(R, V, 0.15, seed=1)
    _, second = cr.gpu_case(R, V, 0.6, seed=2)
    assert (first != cr.IGNORE).sum() != (second != cr.IGNORE).sum()
    leaf = torch.from_numpy(x).to(DEV).requires_grad_()
    labels = torch.from_numpy(first).to(DEV)

    def step():
        loss = cross_entropy(leaf, labels, ignore_index=cr.IGNORE)
        return loss, torch.autograd.grad(loss, leaf)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for lab in (first, second, first):
        labels.copy_(torch.from_numpy(lab).to(DEV))
        for t in captured:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])
        want = cr.run(x, lab, cr.IGNORE, "mean", np.float32(1.0))
        errs = cr.result_errors({"loss": captured[0].detach().cpu().numpy(), "grad": captured[1].detach().cpu().numpy()}, want)
        tol = cr.gpu_tolerance()
        assert errs["loss"] <= tol["loss"] and errs["grad"] <= tol["grad"]


def test_peak_memory_is_one_gradient():
    """A condition derived from shapes: forward + backward at (512, 3708) allocate the gradient [R, V] and O(R) more — no
    second [R, V] tensor.  The allowance of 4 MiB is two allocator blocks."""
    R, V = 512, 3708
    x, target = cr.gpu_case(R, V, 0.15)
    leaf = torch.from_numpy(x).to(DEV).requires_grad_()
    t = torch.from_numpy(target).to(DEV)
    peak = None
    for _ in range(2):  # the second round counts: everything is warm
        leaf.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        cross_entropy(leaf, t, ignore_index=cr.IGNORE).backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above the start: {peak / 2**20:.2f} MiB; one [R, V] float32 tensor {R * V * 4 / 2**20:.2f} MiB")
    assert peak <= R * V * 4 + (4 << 20)


def test_two_bert4rec_training_steps_against_nn_cross_entropy_loss():
    """The "train" configuration of tests/_bert4rec_golden.py with this loss and with nn.CrossEntropyLoss(ignore_index=0),
    at the tolerances of tests/test_bert4rec_model_gpu.py's training test."""
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from test_bert4rec_model_gpu import build_model
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor
    import _bert4rec_golden as G

    z, pre = G.load(), "model|train|"
    fused = {"optimizer": EmbOptimType.EXACT_SGD, "learning_rate": 0.05}
    models = [build_model("train", fused_params=dict(fused)) for _ in range(2)]
    losses_fn = [CrossEntropyLoss(ignore_index=0), torch.nn.CrossEntropyLoss(ignore_index=0)]
    dense = lambda m: [p for n, p in m.named_parameters() if not n.startswith("history.ec.")]  # noqa: E731
    opts = [torch.optim.SGD(dense(m), lr=0.05) for m in models]
    vocab, max_len = int(z[pre + "config"][0]), int(z[pre + "config"][1])
    B = len(z[pre + "lengths"])
    rng = np.random.default_rng(3)
    for step in range(2):
        labels = rng.integers(1, vocab, size=(B, max_len))
        labels[rng.random((B, max_len)) < 0.7] = 0  # most positions carry ignore_index, as in the masked-item task
        labels[0, 0] = 1 + step
        target = torch.from_numpy(labels).to(DEV)
        got = []
        for m, fn, opt in zip(models, losses_fn, opts):
            kjt = KeyedJaggedTensor.from_lengths_sync(keys=["item"], values=torch.from_numpy(z[pre + "values"]).to(DEV),
                                                      lengths=torch.from_numpy(z[pre + "lengths"]).to(DEV))
            opt.zero_grad()
            logits = m(kjt)
            loss = fn(logits.reshape(-1, vocab), target.reshape(-1))
            loss.backward()
            opt.step()
            got.append(loss.detach())
        torch.testing.assert_close(got[0], got[1], rtol=1e-4, atol=1e-5)
    torch.cuda.synchronize()
    torch.testing.assert_close(models[0].history.ec.table_weights()["item_embedding"],
                               models[1].history.ec.table_weights()["item_embedding"], rtol=1e-3, atol=2e-5)
    for (n, a), b in zip(((n, p) for n, p in models[0].named_parameters() if not n.startswith("history.ec.")), dense(models[1])):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-3, atol=2e-5, msg=lambda s, n=n: f"{n}: {s}")
