"""GPU: SwishLayerNorm (torchrec_amd/modules/activation.py) and MLP(activation="swish_layernorm") on the device against the
reference's recorded runs and a float64 torch twin.  What the kernels alone produce is held to the tolerance measured in
tests/test_swish_layernorm.py (8 x the reference's own float32 error); what passes through a GEMM to the tolerance
tests/test_dlrm_e2e_gpu.py uses (tests/_deepfm_ref.py GEMM_TOL, as tests/test_deepfm_gpu.py's model test)."""
import copy

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _swish_layernorm_ref as sr
from _deepfm_ref import GEMM_TOL

pytestmark = pytest.mark.gpu

KERNEL_CASES = {"3x100": True, "37x20": True, "70x64": True, "5x3x4x8": True, "9x10": False}  # 10 % 4 != 0: the fall-back


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _module(dims, params=None):
    from torchrec_amd.modules import SwishLayerNorm

    m = SwishLayerNorm(dims)
    if params is not None:
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()}, strict=True)
    return m.cuda()


def _on_kernel_path(out):
    """Whether `out` comes from the autograd node of the kernels (behind a view, when the input has more than two dims)."""
    fn = out.grad_fn
    if "View" in type(fn).__name__:
        fn = fn.next_functions[0][0]
    return "_SwishLayerNorm" in type(fn).__name__


def _run(m, x, g):
    m.zero_grad(set_to_none=True)
    xi = x.detach().requires_grad_()  # a leaf on x's own storage: a strided x stays strided
    out = m(xi)
    out.backward(g)
    return {"out": out.detach().cpu().numpy(), "grad_input": xi.grad.cpu().numpy(),
            "grad": {n: p.grad.cpu().numpy() for n, p in m.named_parameters()}}, out


def _case(B=70, N=64):
    gamma, beta, x, g = sr.gpu_case(B, N)
    m = _module(N, {"norm.0.weight": gamma, "norm.0.bias": beta})
    return m, _dev(x), _dev(g)


def _assert_same(a, b):
    np.testing.assert_array_equal(a["out"], b["out"])
    np.testing.assert_array_equal(a["grad_input"], b["grad_input"])
    for n in a["grad"]:
        np.testing.assert_array_equal(a["grad"][n], b["grad"][n], err_msg=n)


@pytest.mark.parametrize("case", list(sr.CASES))
def test_module_reproduces_the_reference_fixtures(case):
    """3x100, 37x20, 70x64 and the two-dim normalised shape under two leading dims run on the kernels (N % 4 == 0);
    9x10 is the fall-back, which must match all the same."""
    fx = sr.fixture(case)
    lead, dims = sr.CASES[case]
    m = _module(dims[0] if len(dims) == 1 else dims, fx["params"])
    sd = m.state_dict()
    assert list(sd) == sr.SLN_KEYS and all(v.is_cuda for v in sd.values())
    got, out = _run(m, _dev(fx["x"]), _dev(fx["g"]))
    assert got["out"].shape == fx["x"].shape
    assert _on_kernel_path(out) == KERNEL_CASES[case], out.grad_fn
    tol = sr.gpu_tolerance()
    for prec in ("f64", "f32"):
        errs = sr.result_errors(sr.flat(case, got), sr.flat(case, fx[prec]))
        print(f"{case} against {prec}: tolerance {tol:.3e}, errors " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= tol, (prec, errs)


@pytest.mark.parametrize("dims", [[32], [4, 8]], ids=["1d", "2d"])
def test_an_input_without_leading_dims_is_one_row(dims):
    """x of exactly the normalised shape (B = 1): the bits of the same row inside a batch."""
    gamma, beta, x, g = sr.gpu_case(3, 32)
    m = _module(dims[0] if len(dims) == 1 else dims, {"norm.0.weight": gamma.reshape(dims), "norm.0.bias": beta.reshape(dims)})
    batch, _ = _run(m, _dev(x.reshape([3] + dims)), _dev(g.reshape([3] + dims)))
    one, out = _run(m, _dev(x[1].reshape(dims)), _dev(g[1].reshape(dims)))
    assert _on_kernel_path(out) and one["out"].shape == tuple(dims)
    np.testing.assert_array_equal(one["out"], batch["out"][1])
    np.testing.assert_array_equal(one["grad_input"], batch["grad_input"][1])


def test_a_strided_input_gives_the_result_of_its_contiguous_copy():
    m, x, g = _case()
    wide = torch.zeros(x.shape[0], x.shape[1] + 12, device="cuda")
    wide[:, 4:4 + x.shape[1]] = x
    view = wide[:, 4:4 + x.shape[1]]
    assert not view.is_contiguous()
    b, _ = _run(m, x, g)
    _assert_same(_run(m, view, g)[0], b)
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous()
    _assert_same(_run(m, xt, g)[0], b)
    _assert_same(_run(m, x, g.t().contiguous().t())[0], b)  # and a strided output gradient
    _assert_same(_run(m, x, g)[0], b)  # two runs, the same bits


def test_no_grad_forward_saves_nothing_and_equals_the_training_forward():
    m, x, g = _case(B=4096, N=1024)
    out = m(x.clone().requires_grad_()).detach().clone()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        out2 = m(x)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - base <= out2.numel() * 4 + 512  # the output alone: the row statistics are gone
    assert out2.grad_fn is None and not out2.requires_grad and torch.equal(out, out2)
    for q in m.parameters():
        q.requires_grad_(False)
    out3 = m(x)  # grad mode on, nothing requires grad
    assert out3.grad_fn is None and torch.equal(out3, out2)


def test_grad_flags():
    """Input without grad, frozen gamma, frozen beta: the remaining gradients are unchanged, the frozen ones None."""
    m, x, g = _case()
    full, _ = _run(m, x, g)

    def grads(freeze, x_grad):
        for n, q in m.named_parameters():
            q.requires_grad_(n != freeze)
        m.zero_grad(set_to_none=True)
        xi = x.detach().clone().requires_grad_(x_grad)
        m(xi).backward(g)
        return xi.grad, {n: (None if q.grad is None else q.grad.cpu().numpy()) for n, q in m.named_parameters()}

    gx, gp = grads(None, False)
    assert gx is None
    for n in gp:
        np.testing.assert_array_equal(gp[n], full["grad"][n], err_msg=n)
    for freeze in sr.SLN_KEYS:
        gx, gp = grads(freeze, True)
        np.testing.assert_array_equal(gx.cpu().numpy(), full["grad_input"])
        for n in gp:
            if n == freeze:
                assert gp[n] is None, n
            else:
                np.testing.assert_array_equal(gp[n], full["grad"][n], err_msg=n)


def test_double_backward_takes_differentiable_torch_operations():
    from torchrec_amd.modules.activation import _swish_layernorm_torch

    m, x, g = _case(B=15, N=32)

    def second_order(fn):
        xi = x.detach().clone().requires_grad_()
        (gx,) = torch.autograd.grad(fn(xi), xi, g, create_graph=True)
        (ggx,) = torch.autograd.grad((gx * gx).sum(), xi)
        return gx.detach(), ggx

    gx, ggx = second_order(m)
    gx_t, ggx_t = second_order(lambda t: _swish_layernorm_torch(t, m.norm))
    torch.testing.assert_close(gx, gx_t, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(ggx, ggx_t, rtol=1e-4, atol=1e-5)


def test_two_sgd_steps_of_an_mlp_follow_a_float64_twin():
    from torchrec_amd.modules.activation import SwishLayerNorm
    from torchrec_amd.modules.mlp import MLP

    torch.manual_seed(3)
    width, sizes = 64, list(sr.TRAIN_WIDTHS)
    m = MLP(width, sizes, activation="swish_layernorm", device=torch.device("cuda"))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm.0." in n:
                p.add_(0.5 * torch.randn_like(p))
    twin = copy.deepcopy(m).double()
    rng = np.random.default_rng(11)
    x = _dev((0.5 + 2.0 * rng.standard_normal((sr.TRAIN_BATCH, width))).astype(np.float32))
    g = _dev(rng.standard_normal((sr.TRAIN_BATCH, sizes[-1])).astype(np.float32))
    h = m._mlp[0](x)
    assert isinstance(m._mlp[0]._activation_fn, SwishLayerNorm) and _on_kernel_path(h)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    lr = 0.005  # two steps move the Linear weights by about their own size and gamma / beta by several per cent
    for net, xx, gg in ((m, x, g), (twin, x.double(), g.double())):
        opt = torch.optim.SGD(net.parameters(), lr=lr)
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            (net(xx) * gg).sum().backward()
            opt.step()
    moved = []
    for (n, p), q in zip(m.named_parameters(), twin.parameters()):
        torch.testing.assert_close(p.detach().double(), q.detach(), msg=lambda s, n=n: f"{n}: {s}", **GEMM_TOL)
        moved.append(float((p.detach() - before[n]).abs().max() / before[n].abs().max()))
    assert min(moved) > 0.01, moved  # the steps are no rounding-sized nudges: a wrong gradient would show


def test_forward_and_backward_capture_into_one_hip_graph():
    """Captured on a single stream, replayed twice on new input values: bit for bit what the eager run gives."""
    m, x, g = _case()
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
        eager, _ = _run(m, nx, ng)
        np.testing.assert_array_equal(out.detach().cpu().numpy(), eager["out"])
        np.testing.assert_array_equal(grads[0].cpu().numpy(), eager["grad_input"])
        for (n, _), gr in zip(m.named_parameters(), grads[1:]):
            np.testing.assert_array_equal(gr.cpu().numpy(), eager["grad"][n], err_msg=n)


def test_the_forward_keeps_two_floats_per_row_where_torch_keeps_a_second_matrix():
    """Derived, not measured: after a forward with grad the allocator holds the output [B, N] and the row statistics [2, B]
    (4 B bytes each for mean and rstd, rounded up to the allocator's 512-byte blocks) plus 1024 bytes of slack; the input is
    the caller's.  The torch composition keeps sigmoid(...) as a second [B, N] tensor: it must exceed the same bound, so this
    test cannot pass vacuously."""
    from torchrec_amd.modules.activation import _swish_layernorm_torch

    B, N = 4096, 1024
    m, x, g = _case(B, N)
    x.requires_grad_()
    bound = B * N * 4 + 2 * ((4 * B + 511) // 512 * 512) + 1024

    def grown(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        out = fn(x)
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated() - base, out

    mine, out = grown(m)
    assert _on_kernel_path(out)
    theirs, out_t = grown(lambda t: _swish_layernorm_torch(t, m.norm))
    print(f"forward with grad at {B}x{N}: kernel path keeps {mine} bytes, torch {theirs}; bound {bound}")
    assert mine <= bound < theirs
