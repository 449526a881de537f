"""GPU parity (bit-exact): torch.ops.fbgemm.permute_pooled_embs(_auto_grad) and PermutePooledEmbeddings against
torch.cat of column slices, forward and backward, at the smallest shapes that reach every branch of
csrc/permute_pooled.hip (16-B path, scalar path, misaligned pointer, grid-stride wrap, empty batch, graph replay)."""
from itertools import accumulate

import pytest
import torch

import _paths  # noqa: F401
import fbgemm_gpu  # noqa: F401
from fbgemm_gpu.permute_pooled_embedding_modules import PermutePooledEmbeddings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def reference(x, dims, permute):
    off = [0] + list(accumulate(dims))
    return torch.cat([x[:, off[p]:off[p + 1]] for p in permute], dim=1)


def inverse(permute):
    inv = [0] * len(permute)
    for i, p in enumerate(permute):
        inv[p] = i
    return inv


def index_tensors(dims, permute):
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)  # noqa: E731
    return (t([0] + list(accumulate(dims))), t(permute), t([0] + list(accumulate(dims[p] for p in permute))),
            t(inverse(permute)))


def check(dims, permute, B, x=None):
    if x is None:
        x = torch.randn(B, sum(dims), device=DEV, generator=torch.Generator(DEV).manual_seed(B + len(dims)))
    want = reference(x, dims, permute)
    # the plain op, from bare index tensors (the 16-B precondition is read from the lists)
    got = torch.ops.fbgemm.permute_pooled_embs(x, *index_tensors(dims, permute))
    assert got.shape == want.shape and torch.equal(got, want)
    # the module = the differentiable op
    mod = PermutePooledEmbeddings(dims, permute, device=torch.device(DEV))
    xg = x.detach().clone().requires_grad_(True)
    out = mod(xg)
    assert torch.equal(out.detach(), want)
    grad_out = torch.randn_like(want)
    (grad_in,) = torch.autograd.grad(out, xg, grad_out)
    dims_p = [dims[p] for p in permute]
    assert torch.equal(grad_in, reference(grad_out, dims_p, inverse(permute)))
    return got


@pytest.mark.parametrize("B", [1, 3, 257])
def test_vector_path(B):
    check([4, 8, 12], [2, 0, 1], B)


@pytest.mark.parametrize("B", [1, 3, 257])
def test_scalar_path(B):
    check([3, 5, 1, 7], [3, 1, 0, 2], B)


def test_identity_permutation():
    check([4, 8, 12], [0, 1, 2], 5)
    check([3, 5, 1, 7], [0, 1, 2, 3], 5)


def test_single_segment():
    check([16], [0], 7)
    check([5], [0], 7)


def test_empty_batch():
    out = check([4, 8, 12], [2, 0, 1], 0)
    assert out.shape == (0, 24)


def test_misaligned_view_takes_the_scalar_path():
    dims, permute, B = [4, 8, 12], [2, 0, 1], 9
    flat = torch.randn(B * 24 + 1, device=DEV)
    x = flat[1:].view(B, 24)  # contiguous, 4 bytes past a 16-B boundary
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    check(dims, permute, B, x=x)


def test_grid_stride_loop_wraps():
    # the grid is capped at 8 192 blocks of 256 lanes = 2 097 152 elements per sweep.  70 000 x [32, 32] is 1 120 000
    # 16-B vectors (one sweep, just under the cap's block count); the same batch wraps on the scalar path (4 480 000
    # elements, dims [31, 33]) and, with four 32-wide segments, on the vector path (2 240 000 vectors)
    check([32, 32], [1, 0], 70000)
    check([31, 33], [1, 0], 70000)
    check([32, 32, 32, 32], [3, 1, 0, 2], 70000)


def test_too_many_segments_is_refused():
    T = 8000
    with pytest.raises(RuntimeError, match="too many segments"):
        torch.ops.fbgemm.permute_pooled_embs(torch.zeros(2, T, device=DEV), *index_tensors([1] * T, list(range(T))))


def test_capture_and_replay_in_a_hip_graph():
    dims, permute, B = [4, 8, 12], [2, 0, 1], 33
    mod = PermutePooledEmbeddings(dims, permute, device=torch.device(DEV))
    static_in = torch.randn(B, 24, device=DEV)
    stream = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        mod(static_in)  # warm-up on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        static_out = mod(static_in)
    fresh = torch.randn(B, 24, device=DEV)
    static_in.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, reference(fresh, dims, permute))


def test_non_permutation_raises_in_the_constructor():
    with pytest.raises(ValueError, match="not a permutation"):
        PermutePooledEmbeddings([4, 8, 12], [0, 0, 1], device=torch.device(DEV))
    with pytest.raises(ValueError, match="not a permutation"):
        PermutePooledEmbeddings([4, 8, 12], [0, 1], device=torch.device(DEV))


def test_module_follows_to_device():
    mod = PermutePooledEmbeddings([4, 8, 12], [2, 0, 1], device=torch.device("cpu")).to(device=torch.device(DEV))
    x = torch.randn(3, 24, device=DEV)
    assert torch.equal(mod(x), reference(x, [4, 8, 12], [2, 0, 1]))
