"""GPU: CrossNet, LowRankCrossNet and VectorCrossNet (torchrec_amd/modules/crossnet.py) on their kernel paths
(csrc/crossnet.hip) against the reference's recorded runs (tests/golden/crossnet.npz) and the float64 restatement
(tests/_crossnet_ref.py), within the tolerance measured in tests/test_crossnet.py."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _crossnet_ref as cr

pytestmark = pytest.mark.gpu

ALL = [(k, c) for k in cr.KINDS for c in cr.CASES]
SGD_LR = {"CrossNet": 1e-3, "LowRankCrossNet": 1e-3, "VectorCrossNet": 3e-5}  # updates about as large as the parameters


def _module(kind, N, L, r, params=None):
    from torchrec_amd.modules import crossnet

    m = crossnet.LowRankCrossNet(N, L, low_rank=r) if kind == "LowRankCrossNet" else getattr(crossnet, kind)(N, L)
    if params is not None:
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()}, strict=True)
    return m.cuda()


def _run(m, x, g):
    """out, input gradient, parameter gradients as numpy, laid out like _crossnet_ref.run's result."""
    m.zero_grad(set_to_none=True)
    xi = x.detach().requires_grad_()  # a leaf on x's own storage: a strided x stays strided
    out = m(xi)
    out.backward(g)
    return {"out": out.detach().cpu().numpy(), "grad_input": xi.grad.cpu().numpy(),
            "grad": {n: p.grad.cpu().numpy() for n, p in m.named_parameters()}}


def _case(kind, shape=cr.TRAIN_SHAPE):
    B, N, L, r = shape
    p, x, g = cr.gpu_case(kind, B, N, L, r)
    return _module(kind, N, L, r, p), p, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), x, g


def _assert_same(a, b):
    assert torch.equal(torch.as_tensor(a["out"]), torch.as_tensor(b["out"]))
    assert torch.equal(torch.as_tensor(a["grad_input"]), torch.as_tensor(b["grad_input"]))
    for n in a["grad"]:
        assert torch.equal(torch.as_tensor(a["grad"][n]), torch.as_tensor(b["grad"][n])), n


@pytest.mark.parametrize("kind,case", ALL, ids=[f"{k}-{c}" for k, c in ALL])
def test_modules_reproduce_the_reference_fixtures(kind, case):
    """N = 10 is no multiple of 4: the fall-back, which must match all the same."""
    fx = cr.fixture(kind, case)
    B, N, L, r = cr.CASES[case]
    m = _module(kind, N, L, r, fx["params"])
    got = _run(m, torch.from_numpy(fx["x"]).cuda(), torch.from_numpy(fx["g"]).cuda())
    errs = cr.result_errors(got, fx["f64"])
    tol = cr.gpu_tolerance()
    print(f"{kind} {case}: tolerance {tol:.3e}, errors " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= tol, errs
    assert max(cr.result_errors(got, fx["f32"]).values()) <= tol


@pytest.mark.parametrize("kind", cr.KINDS)
def test_a_reference_state_dict_round_trips(kind):
    fx = cr.fixture(kind, "70x64")
    B, N, L, r = cr.CASES["70x64"]
    m = _module(kind, N, L, r, fx["params"])
    sd = m.state_dict()
    assert list(sd) == cr.param_names(kind, L)
    for k, v in fx["params"].items():
        assert sd[k].is_cuda and sd[k].shape == v.shape
        np.testing.assert_array_equal(sd[k].cpu().numpy(), v)


@pytest.mark.parametrize("kind", cr.KINDS)
def test_two_sgd_steps_follow_the_float64_restatement(kind):
    m, p, x, g, xn, gn = _case(kind)
    lr = SGD_LR[kind]
    ref = cr.sgd_steps(kind, p, xn, gn, lr, 2)
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        (m(x) * g).sum().backward()
        opt.step()
    tol = cr.gpu_tolerance()
    moved = []
    for n, q in m.named_parameters():
        err = cr.rel_err(q.detach().cpu().numpy(), ref[n])
        assert err <= tol, (n, err, tol)
        moved.append(np.abs(ref[n] - p[n]).max() / np.abs(p[n]).max())
    assert max(moved) > 0.3  # the steps are no rounding-sized nudges: a wrong gradient would show


@pytest.mark.parametrize("kind", cr.KINDS)
def test_grad_flags(kind):
    """Input without grad, frozen bias, frozen kernels: the remaining gradients are unchanged, the frozen ones None."""
    m, p, x, g, _, _ = _case(kind)
    full = _run(m, x, g)

    def grads(freeze, x_grad):
        for n, q in m.named_parameters():
            q.requires_grad_(not n.startswith(freeze) if freeze else True)
        m.zero_grad(set_to_none=True)
        xi = x.detach().clone().requires_grad_(x_grad)
        m(xi).backward(g)
        out = {n: (None if q.grad is None else q.grad.cpu().numpy()) for n, q in m.named_parameters()}
        return xi.grad, out

    gx, gp = grads(None, False)
    assert gx is None
    for n in gp:
        np.testing.assert_array_equal(gp[n], full["grad"][n], err_msg=n)
    for freeze in ("bias", "kernels", "W_kernels", "V_kernels"):
        if not any(n.startswith(freeze) for n in full["grad"]):
            continue
        gx, gp = grads(freeze, True)
        np.testing.assert_array_equal(gx.cpu().numpy(), full["grad_input"])
        for n in gp:
            if n.startswith(freeze):
                assert gp[n] is None, n
            else:
                np.testing.assert_array_equal(gp[n], full["grad"][n], err_msg=n)
    # everything below the last layer frozen and no input gradient: the chain stops early, the rest is unchanged
    L = cr.TRAIN_SHAPE[2]
    for n, q in m.named_parameters():
        q.requires_grad_(n.endswith(f".{L - 1}"))
    m.zero_grad(set_to_none=True)
    m(x).backward(g)
    for n, q in m.named_parameters():
        if n.endswith(f".{L - 1}"):
            np.testing.assert_array_equal(q.grad.cpu().numpy(), full["grad"][n], err_msg=n)
        else:
            assert q.grad is None


@pytest.mark.parametrize("kind", cr.KINDS)
def test_no_grad_forward_equals_the_training_forward_bit_for_bit(kind):
    m, p, x, g, _, _ = _case(kind)
    out = m(x.clone().requires_grad_())
    with torch.no_grad():
        out2 = m(x)
    assert not out2.requires_grad and torch.equal(out.detach(), out2)
    for q in m.parameters():
        q.requires_grad_(False)
    assert torch.equal(m(x), out2)  # grad mode on, nothing requires grad


@pytest.mark.parametrize("kind", cr.KINDS)
def test_non_contiguous_input_gives_the_result_of_its_contiguous_copy(kind):
    m, p, x, g, _, _ = _case(kind)
    wide = torch.zeros(x.shape[0], x.shape[1] + 12, device="cuda")
    wide[:, 4:4 + x.shape[1]] = x
    view = wide[:, 4:4 + x.shape[1]]
    assert not view.is_contiguous()
    a, b = _run(m, view, g), _run(m, x, g)
    _assert_same(a, b)
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous()
    _assert_same(_run(m, xt, g), b)


@pytest.mark.parametrize("kind", cr.KINDS)
def test_forward_and_backward_are_bit_identical_across_two_runs(kind):
    m, p, x, g, _, _ = _case(kind)
    _assert_same(_run(m, x, g), _run(m, x, g))


@pytest.mark.parametrize("kind", cr.KINDS)
def test_forward_and_backward_capture_into_one_hip_graph(kind):
    """Captured on a single stream, replayed twice on new input values: bit for bit what the eager run gives."""
    m, p, x, g, _, _ = _case(kind)
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
