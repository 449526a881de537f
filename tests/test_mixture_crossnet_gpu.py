"""GPU: LowRankMixtureCrossNet (torchrec_amd/modules/crossnet.py) on its kernel path (the folded experts, the gate kernels of
csrc/crossnet.hip) against the reference's recorded runs (tests/golden/mixture_crossnet.npz) and the float64 restatement
(tests/_mixture_crossnet_ref.py), within the tolerance measured in tests/test_mixture_crossnet.py."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _mixture_crossnet_ref as mr

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["x".join(map(str, s)) for s in mr.TRAIN_SHAPES]
# two steps of these move the float64 restatement's parameters by 0.65 / 0.55 of their scale (measured on the CPU)
SGD_LR = {mr.TRAIN_SHAPES[0]: 1e-3, mr.TRAIN_SHAPES[1]: 3e-3}
GROUPS = ("bias", "U_", "V_", "C_", "gates")


def _module(N, L, K, r, params=None, **kw):
    from torchrec_amd.modules import LowRankMixtureCrossNet

    m = LowRankMixtureCrossNet(N, L, num_experts=K, low_rank=r, **kw)
    if params is not None:
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()}, strict=True)
    return m.cuda()


def _run(m, x, g):
    """out, input gradient, parameter gradients as numpy, laid out like _mixture_crossnet_ref.run's result."""
    m.zero_grad(set_to_none=True)
    xi = x.detach().requires_grad_()  # a leaf on x's own storage: a strided x stays strided
    out = m(xi)
    out.backward(g)
    return {"out": out.detach().cpu().numpy(), "grad_input": xi.grad.cpu().numpy(),
            "grad": {n: p.grad.cpu().numpy() for n, p in m.named_parameters()}}


def _case(shape, **kw):
    B, N, L, K, r = shape
    p, x, g = mr.gpu_case(*shape)
    return _module(N, L, K, r, p, **kw), p, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), x, g


def _assert_same(a, b):
    assert torch.equal(torch.as_tensor(a["out"]), torch.as_tensor(b["out"]))
    assert torch.equal(torch.as_tensor(a["grad_input"]), torch.as_tensor(b["grad_input"]))
    for n in a["grad"]:
        assert torch.equal(torch.as_tensor(a["grad"][n]), torch.as_tensor(b["grad"][n])), n


def _on_kernel_path(m, x):
    """The module's own routing, spied on: the call reaches _MixtureCross / _mixture_forward, not the torch expression."""
    from torchrec_amd.modules import crossnet

    seen = []
    orig = crossnet._mixture_forward

    def spy(*a, **k):
        seen.append(1)
        return orig(*a, **k)

    crossnet._mixture_forward = spy
    try:
        m(x)
    finally:
        crossnet._mixture_forward = orig
    return bool(seen)


@pytest.mark.parametrize("case", list(mr.CASES))
def test_module_reproduces_the_reference_fixtures(case):
    """3x10: N is no multiple of 4, the fall-back, which must match all the same.  37x20: K = 1 — the kernel path without a
    gate launch.  70x64: four experts."""
    fx = mr.fixture(case)
    B, N, L, K, r = mr.CASES[case]
    m = _module(N, L, K, r, fx["params"])
    x = torch.from_numpy(fx["x"]).cuda()
    assert _on_kernel_path(m, x) == (N % 4 == 0)
    got = _run(m, x, torch.from_numpy(fx["g"]).cuda())
    errs = mr.result_errors(got, fx["f64"])
    tol = mr.gpu_tolerance()
    print(f"{case}: tolerance {tol:.3e}, errors " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= tol, errs
    assert max(mr.result_errors(got, fx["f32"]).values()) <= tol


def test_a_reference_state_dict_round_trips():
    fx = mr.fixture("70x64")
    B, N, L, K, r = mr.CASES["70x64"]
    m = _module(N, L, K, r, fx["params"])
    sd = m.state_dict()
    assert list(sd) == mr.param_names(L, K)
    for k, v in fx["params"].items():
        assert sd[k].is_cuda and sd[k].shape == v.shape
        np.testing.assert_array_equal(sd[k].cpu().numpy(), v)


@pytest.mark.parametrize("shape", mr.TRAIN_SHAPES, ids=SHAPE_IDS)
def test_two_sgd_steps_follow_the_float64_restatement(shape):
    m, p, x, g, xn, gn = _case(shape)
    assert _on_kernel_path(m, x)
    lr = SGD_LR[shape]
    ref = mr.sgd_steps(p, xn, gn, lr, 2)
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        (m(x) * g).sum().backward()
        opt.step()
    tol = mr.gpu_tolerance()
    moved = []
    for n, q in m.named_parameters():
        err = mr.rel_err(q.detach().cpu().numpy(), ref[n])
        print(f"{n}: {err:.2e}")
        assert err <= tol, (n, err, tol)
        moved.append(np.abs(ref[n] - p[n]).max() / np.abs(p[n]).max())
    assert max(moved) > 0.3  # the steps are no rounding-sized nudges: a wrong gradient would show


@pytest.mark.parametrize("shape", mr.TRAIN_SHAPES, ids=SHAPE_IDS)
def test_grad_flags(shape):
    """Input without grad; each parameter group frozen; everything below the last layer (gates included) frozen: the
    remaining gradients are bit-equal to the full run's, the frozen ones None."""
    m, p, x, g, _, _ = _case(shape)
    full = _run(m, x, g)

    def grads(frozen, x_grad):
        for n, q in m.named_parameters():
            q.requires_grad_(not frozen(n))
        m.zero_grad(set_to_none=True)
        xi = x.detach().clone().requires_grad_(x_grad)
        m(xi).backward(g)
        return xi.grad, {n: (None if q.grad is None else q.grad.cpu().numpy()) for n, q in m.named_parameters()}

    gx, gp = grads(lambda n: False, False)
    assert gx is None
    for n in gp:
        np.testing.assert_array_equal(gp[n], full["grad"][n], err_msg=n)
    for group in GROUPS:
        assert any(n.startswith(group) for n in full["grad"])
        for x_grad in (True, False):
            gx, gp = grads(lambda n: n.startswith(group), x_grad)
            if x_grad:
                np.testing.assert_array_equal(gx.cpu().numpy(), full["grad_input"])
            else:
                assert gx is None
            for n in gp:
                if n.startswith(group):
                    assert gp[n] is None, n
                else:
                    np.testing.assert_array_equal(gp[n], full["grad"][n], err_msg=(group, x_grad, n))
    # everything below the last layer frozen, gates included, and no input gradient: the chain stops early
    L = shape[2]
    last = lambda n: n.endswith(f".{L - 1}") and not n.startswith("gates")  # noqa: E731
    gx, gp = grads(lambda n: not last(n), False)
    assert gx is None
    for n in gp:
        if last(n):
            np.testing.assert_array_equal(gp[n], full["grad"][n], err_msg=n)
        else:
            assert gp[n] is None, n
    # one gate alone
    gx, gp = grads(lambda n: n != "gates.1.weight", False)
    for n in gp:
        if n == "gates.1.weight":
            np.testing.assert_array_equal(gp[n], full["grad"][n])
        else:
            assert gp[n] is None, n


@pytest.mark.parametrize("shape", mr.TRAIN_SHAPES, ids=SHAPE_IDS)
def test_no_grad_forward_equals_the_training_forward_bit_for_bit(shape):
    m, p, x, g, _, _ = _case(shape)
    out = m(x.clone().requires_grad_())
    with torch.no_grad():
        out2 = m(x)
    assert not out2.requires_grad and torch.equal(out.detach(), out2)
    for q in m.parameters():
        q.requires_grad_(False)
    out3 = m(x)  # grad mode on, nothing requires grad
    assert not out3.requires_grad and torch.equal(out3, out2)


@pytest.mark.parametrize("shape", mr.TRAIN_SHAPES, ids=SHAPE_IDS)
def test_non_contiguous_input_gives_the_result_of_its_contiguous_copy(shape):
    m, p, x, g, _, _ = _case(shape)
    wide = torch.zeros(x.shape[0], x.shape[1] + 12, device="cuda")
    wide[:, 4:4 + x.shape[1]] = x
    view = wide[:, 4:4 + x.shape[1]]
    assert not view.is_contiguous()
    a, b = _run(m, view, g), _run(m, x, g)
    _assert_same(a, b)
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous()
    _assert_same(_run(m, xt, g), b)


@pytest.mark.parametrize("shape", mr.TRAIN_SHAPES, ids=SHAPE_IDS)
def test_forward_and_backward_are_bit_identical_across_two_runs(shape):
    m, p, x, g, _, _ = _case(shape)
    _assert_same(_run(m, x, g), _run(m, x, g))


@pytest.mark.parametrize("shape", mr.TRAIN_SHAPES, ids=SHAPE_IDS)
def test_forward_and_backward_capture_into_one_hip_graph(shape):
    """Captured on a single stream, replayed twice on new input values: bit for bit what the eager run gives."""
    m, p, x, g, _, _ = _case(shape)
    params = list(m.parameters())
    sx, sg = x.clone().requires_grad_(), g.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the capture: library handles, workspaces, autograd's buffers
        for _ in range(2):
            torch.autograd.grad(m(sx), [sx] + params, sg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(sx)
        grads = torch.autograd.grad(out, [sx] + params, sg)
    gen = torch.Generator(device="cuda").manual_seed(7)
    for _ in range(2):
        nx = torch.randn(x.shape, device="cuda", generator=gen)
        ng = torch.randn(g.shape, device="cuda", generator=gen)
        with torch.no_grad():
            sx.copy_(nx)
            sg.copy_(ng)
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(m, nx, ng)
        assert torch.equal(out.detach().cpu(), torch.as_tensor(eager["out"]))
        assert torch.equal(grads[0].cpu(), torch.as_tensor(eager["grad_input"]))
        for (n, _), gr in zip(m.named_parameters(), grads[1:]):
            assert torch.equal(gr.cpu(), torch.as_tensor(eager["grad"][n])), n


@pytest.mark.parametrize("what", ["tanh", "K=17", "N=10"])
def test_fall_backs_equal_the_torch_composition_bit_for_bit(what):
    from torchrec_amd.modules import crossnet

    B, N, L, K, r = {"tanh": (33, 64, 2, 3, 4), "K=17": (33, 64, 2, 17, 2), "N=10": (33, 10, 2, 3, 4)}[what]
    p, x, g = mr.gpu_case(B, N, L, K, r)
    m = _module(N, L, K, r, p, **({"activation": torch.tanh} if what == "tanh" else {}))
    x, g = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    assert not _on_kernel_path(m, x)
    got = _run(m, x, g)
    m.zero_grad(set_to_none=True)
    xi = x.detach().requires_grad_()
    out = crossnet._low_rank_mixture_cross_torch(xi, list(m.U_kernels), list(m.V_kernels), list(m.bias),
                                                 [gate.weight for gate in m.gates], list(m.C_kernels), m._activation)
    out.backward(g)
    want = {"out": out.detach().cpu().numpy(), "grad_input": xi.grad.cpu().numpy(),
            "grad": {n: q.grad.cpu().numpy() for n, q in m.named_parameters()}}
    _assert_same(got, want)


@pytest.mark.parametrize("act", ["functional", "module"])
def test_every_spelling_of_relu_takes_the_kernel_path(act):
    shape = mr.TRAIN_SHAPES[1]
    activation = torch.nn.functional.relu if act == "functional" else torch.nn.ReLU()
    m, p, x, g, _, _ = _case(shape, activation=activation)
    assert _on_kernel_path(m, x)
    m0 = _case(shape)[0]
    _assert_same(_run(m, x, g), _run(m0, x, g))


def _peak_above_start(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def test_the_expert_stack_never_exists():
    """(B, N, L, K, r) = (2048, 512, 2, 16, 2): one layer's [B, N, K] stack is 64 MiB.  The peak of a forward + backward
    above the level before it stays below that on the kernel path — measured 35.3 MiB — and exceeds it on
    the torch composition (measured 329.4 MiB), so the bound tells the two apart."""
    from torchrec_amd.modules import crossnet

    B, N, L, K, r = 2048, 512, 2, 16, 2
    bound = B * N * K * 4
    p, x, g = mr.gpu_case(B, N, L, K, r)
    m = _module(N, L, K, r, p)
    x, g = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    assert _on_kernel_path(m, x)

    def kernel_path():
        m.zero_grad(set_to_none=True)
        xi = x.detach().requires_grad_()
        m(xi).backward(g)

    def torch_path():
        m.zero_grad(set_to_none=True)
        xi = x.detach().requires_grad_()
        crossnet._low_rank_mixture_cross_torch(xi, list(m.U_kernels), list(m.V_kernels), list(m.bias),
                                               [gate.weight for gate in m.gates], list(m.C_kernels)).backward(g)

    kernel_path()  # warm-up: library handles and workspaces
    m.zero_grad(set_to_none=True)
    peak = _peak_above_start(kernel_path)
    m.zero_grad(set_to_none=True)
    torch_path()
    m.zero_grad(set_to_none=True)
    torch_peak = _peak_above_start(torch_path)
    print(f"peak above start: kernel path {peak / 2**20:.1f} MiB, torch composition {torch_peak / 2**20:.1f} MiB, "
          f"one layer's stack {bound / 2**20:.0f} MiB")
    assert peak < bound
    assert torch_peak > bound
