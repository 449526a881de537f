"""DeepFM modules with the reference's constructors and results (torchrec/modules/deepfm.py: _get_flatten_input :28-32,
DeepFM :35-130, FactorizationMachine :133-215).

On a HIP device, for float32 inputs of one batch size whose inner dimension is contiguous, FactorizationMachine runs as
ONE autograd.Function over csrc/deepfm.hip (`torch.ops.tbe_hip.fm_forward` / `fm_backward`): the inputs are handed to the
kernel as column segments of one logical row, never concatenated; list neighbours that are adjacent column slices of one
buffer (the per-feature views of a KeyedTensor) count as one segment, and only a list that still has more than 8 segments
is concatenated first.  Every input gets its own gradient; an input that does not require grad gets none.

Everything else (CPU tensors, other dtypes, an inner dimension that is not contiguous, double backward) silently takes the
reference's torch expression, as the cross networks do.  DeepFM is dense_module(cat(...)) and needs no kernel of its own;
`fm_and_cat` is the fused form FMInteractionArch (models/deepfm.py) uses: the concatenated row and the FM term from one
read."""
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

MAX_SEGMENTS = 8  # include/tbe_hip.h TBE_FM_MAX_SEGMENTS


# ---- the reference's expressions in plain torch: the fall-back, and what tools/fmbench.py times as "torch" ---------------
def _get_flatten_input(inputs: List[torch.Tensor]) -> torch.Tensor:
    return torch.cat([input.flatten(1) for input in inputs], dim=1)


def _fm_torch(fm_input: torch.Tensor) -> torch.Tensor:
    sum_of_input = torch.sum(fm_input, dim=1, keepdim=True)
    sum_of_square = torch.sum(fm_input * fm_input, dim=1, keepdim=True)
    square_of_sum = sum_of_input * sum_of_input
    cross_term = square_of_sum - sum_of_square
    return torch.sum(cross_term, dim=1, keepdim=True) * 0.5  # [B, 1]


def _kernel_inputs(inputs: Sequence[torch.Tensor]) -> Optional[List[torch.Tensor]]:
    """The inputs as float32 [B, w] column blocks for the kernels, or None where the fall-back applies."""
    if len(inputs) == 0:
        return None
    flat = []
    for x in inputs:
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2
                and x.device == inputs[0].device and x.shape[0] == inputs[0].shape[0]):
            return None
        if x.dim() > 2:
            if not x.is_contiguous():
                return None
            x = x.flatten(1)  # a view
        if x.shape[1] < 1 or (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
            return None
        flat.append(x)
    return flat


def _squeeze_segments(flat: List[torch.Tensor]) -> List[torch.Tensor]:
    from ..distributed import _device_ops

    if len(_device_ops.fm_segments(flat)) > MAX_SEGMENTS:
        return [torch.cat(flat, dim=1)]
    return flat


class _FM(torch.autograd.Function):
    """(fm [B, 1], cat [B, N] or an empty tensor) of the column blocks xs; one kernel each way."""

    @staticmethod
    def forward(ctx, want_cat, *xs):
        fm, row_sum, cat = torch.ops.tbe_hip.fm_forward(list(xs), want_cat)
        ctx.want_cat = want_cat
        ctx.save_for_backward(row_sum, *xs)
        if not want_cat:
            ctx.mark_non_differentiable(cat)
        return fm, cat

    @staticmethod
    def backward(ctx, grad_fm, grad_cat):
        row_sum, *xs = ctx.saved_tensors
        wanted = list(ctx.needs_input_grad[1:])
        if torch.is_grad_enabled():  # create_graph: the same gradient from differentiable torch operations
            s = torch.sum(torch.cat(list(xs), dim=1), dim=1, keepdim=True)
            grads, col = [], 0
            for x, w in zip(xs, wanted):
                g = None
                if w:
                    g = grad_fm * (s - x) if grad_fm is not None else torch.zeros_like(x)
                    if ctx.want_cat and grad_cat is not None:
                        g = g + grad_cat[:, col:col + x.shape[1]]
                grads.append(g)
                col += x.shape[1]
            return (None, *grads)
        if grad_fm is None:
            grad_fm = torch.zeros((row_sum.shape[0], 1), dtype=torch.float32, device=row_sum.device)
        gcat = grad_cat if ctx.want_cat else None
        grads = torch.ops.tbe_hip.fm_backward(list(xs), grad_fm, row_sum, gcat, wanted)
        return (None, *[g if w else None for g, w in zip(grads, wanted)])


def fm_and_cat(flat: List[torch.Tensor], want_cat: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(fm [B, 1], the concatenated row [B, N] or None) of kernel-ready column blocks (see _kernel_inputs)."""
    from ..distributed import _device_ops  # noqa: F401  (registers torch.ops.tbe_hip.*)

    flat = _squeeze_segments(flat)
    if torch.is_grad_enabled() and any(x.requires_grad for x in flat):
        fm, cat = _FM.apply(want_cat, *flat)
    else:
        fm, _, cat = torch.ops.tbe_hip.fm_forward([x.detach() for x in flat], want_cat)
    return fm, (cat if want_cat else None)


class DeepFM(nn.Module):
    """dense_module(cat of the flattened embeddings): the deep component (torchrec/modules/deepfm.py:35-130)."""

    def __init__(self, dense_module: nn.Module) -> None:
        super().__init__()
        self.dense_module = dense_module

    def forward(self, embeddings: List[torch.Tensor]) -> torch.Tensor:
        return self.dense_module(_get_flatten_input(embeddings))


class FactorizationMachine(nn.Module):
    """0.5 * ((sum x)^2 - sum x^2) over the flattened, concatenated embeddings, [B, 1] (torchrec/modules/deepfm.py:133-215)."""

    def __init__(self) -> None:
        super().__init__()

    def forward(self, embeddings: List[torch.Tensor]) -> torch.Tensor:
        flat = _kernel_inputs(embeddings)
        if flat is None:
            return _fm_torch(_get_flatten_input(embeddings))
        return fm_and_cat(flat, False)[0]
