"""Cross-entropy over class indices with `ignore_index`: the loss of the BERT4Rec trainer
(examples/bert4rec/bert4rec_main.py:278-295, `nn.CrossEntropyLoss(ignore_index=0)` over `logits.view(B * T, V)`).

    from torchrec_amd.modules.loss import CrossEntropyLoss
    ce = CrossEntropyLoss(ignore_index=0)
    loss = ce(logits.view(-1, V), labels.view(-1)); loss.backward()

On a HIP device, for a float32 `input` [R, V] with inner stride 1 and any row stride >= V, an int64 `target` [R] and
`reduction` in mean | sum | none, forward and backward are the kernels of csrc/cross_entropy.hip (`tbe_cross_entropy_forward_f32`
/ `_backward_f32`): a row whose label is `ignore_index` is never read, no [R, V] intermediate exists, and autograd keeps the
logits, the labels, two floats per row (maximum and log-sum) and the device-side count of valid rows — nothing waits for
the host, so a step captures into a HIP graph.  Results depend on (R, V) and the values only; two runs are bit-identical.

Everything else silently takes `torch.nn.functional.cross_entropy`, as the other modules here fall back: CPU tensors, other
dtypes, class-probability targets, inputs of rank other than 2, a non-unit inner stride, double backward.

`weight=` and `label_smoothing=` are NOT parameters of `CrossEntropyLoss` / `cross_entropy` here: the reference does not use
them, and they are not accepted rather than ignored.

Deliberate differences on the kernel path: NaN or Inf inside an ignored row reaches neither the loss nor the gradient (torch's
log_softmax backward turns that row's gradient into NaN); a label outside [0, V) that is not `ignore_index` gives NaN in that
row's loss and gradient row (and in a mean / sum loss) where torch aborts the process with a device-side assertion."""
import torch
from torch import nn
from torch.nn import functional as F

from fbgemm_gpu import _lib
from fbgemm_gpu._lib import check, ptr, stream_ptr

__all__ = ["CrossEntropyLoss", "cross_entropy"]

_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}


def _row_stride(input: torch.Tensor) -> int:
    R, V = input.shape
    return input.stride(0) if R > 1 else V


def _forward(input, target, ignore_index, reduction):
    """(loss, state) of one forward on the current stream.  state: float32 [2 + 2 R] — the valid-row count as one int64 in
    the first 8 bytes, then the ABI's stats [2, R] (row maxima, log-sums): all the backward needs besides the logits and the
    labels."""
    R, V = input.shape
    dev = input.device
    lib = _lib.load()
    red = _REDUCTIONS[reduction]
    state = torch.empty(2 + 2 * R, dtype=torch.float32, device=dev)
    loss = torch.empty((R,) if red == 2 else (), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = None if red == 2 else _lib.workspace(lib.tbe_cross_entropy_workspace_bytes(R), dev)
        check(lib.tbe_cross_entropy_forward_f32(
            ptr(input), _row_stride(input), ptr(target), R, V, ignore_index, red, state.data_ptr() + 8, ptr(loss),
            state.data_ptr(), ptr(ws), 0 if ws is None else ws.numel(), stream_ptr(dev)), "tbe_cross_entropy_forward_f32")
    return loss, state


class _CrossEntropy(torch.autograd.Function):
    """input [R, V] float32 on a HIP device with inner stride 1; target [R] int64, contiguous."""

    @staticmethod
    def forward(ctx, input, target, ignore_index, reduction):
        loss, state = _forward(input, target, ignore_index, reduction)
        ctx.ignore_index, ctx.reduction = ignore_index, reduction
        ctx.save_for_backward(input, target, state)
        return loss

    @staticmethod
    def backward(ctx, G):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        input, target, state = ctx.saved_tensors
        if torch.is_grad_enabled():  # create_graph: the same gradient from differentiable torch operations
            out = F.cross_entropy(input, target, ignore_index=ctx.ignore_index, reduction=ctx.reduction)
            return torch.autograd.grad(out, input, G, create_graph=True)[0], None, None, None
        R, V = input.shape
        dev = input.device
        G = G.to(torch.float32).contiguous()
        grad = torch.empty((R, V), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(_lib.load().tbe_cross_entropy_backward_f32(
                ptr(G), ptr(input), _row_stride(input), ptr(target), state.data_ptr() + 8, state.data_ptr(), R, V,
                ctx.ignore_index, _REDUCTIONS[ctx.reduction], ptr(grad), V, stream_ptr(dev)), "tbe_cross_entropy_backward_f32")
        return grad, None, None, None


def _kernel_path(input: torch.Tensor, target: torch.Tensor, reduction: str) -> bool:
    return (input.is_cuda and input.dtype == torch.float32 and input.dim() == 2 and input.shape[1] >= 1
            and input.stride(1) == 1 and (input.shape[0] <= 1 or input.stride(0) >= input.shape[1])
            and target.dtype == torch.int64 and target.dim() == 1 and target.shape[0] == input.shape[0]
            and target.device == input.device and reduction in _REDUCTIONS)


def cross_entropy(input: torch.Tensor, target: torch.Tensor, ignore_index: int = -100, reduction: str = "mean") -> torch.Tensor:
    """`torch.nn.functional.cross_entropy(input, target, ignore_index=..., reduction=...)` (module docstring: what runs on
    the kernels and what falls back)."""
    if not _kernel_path(input, target, reduction):
        return F.cross_entropy(input, target, ignore_index=ignore_index, reduction=reduction)
    target = target.contiguous()
    ignore_index = int(ignore_index)
    if torch.is_grad_enabled() and input.requires_grad:
        return _CrossEntropy.apply(input, target, ignore_index, reduction)
    return _forward(input.detach(), target, ignore_index, reduction)[0]  # nothing is kept


class CrossEntropyLoss(nn.Module):
    """`nn.CrossEntropyLoss(ignore_index=..., reduction=...)` for class-index targets; no `weight`, no `label_smoothing`."""

    def __init__(self, ignore_index: int = -100, reduction: str = "mean") -> None:
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError(f"{reduction} is not a valid value for reduction")
        self.ignore_index = int(ignore_index)
        self.reduction = reduction

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return cross_entropy(input, target, self.ignore_index, self.reduction)

    def extra_repr(self) -> str:
        return f"ignore_index={self.ignore_index}, reduction={self.reduction!r}"
