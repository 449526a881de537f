"""SwishLayerNorm with the reference's constructor and module tree (torchrec/modules/activation.py:18-55):
`Y = X * Sigmoid(LayerNorm(X))`, parameters `norm.0.weight` / `norm.0.bias`, so a reference state_dict loads unchanged.

On a HIP device, for a float32 input whose trailing dims are the normalised shape with N = prod(input_dims) a multiple of 4
and at most 4096, forward and backward are one kernel each (csrc/swish_layernorm.hip through
`torch.ops.tbe_hip.swish_layernorm_forward` / `_backward`): leading dims are flattened to B, the normalised dims to N; the
backward keeps the input and two floats per row, nothing else of size [B, N].

Everything else (CPU tensors, other dtypes, another N, parameters elsewhere or without affine, double backward) silently
takes `_swish_layernorm_torch`, the reference's expression, as LinearOut and the cross nets do."""
import math
from typing import List, Optional, Union

import torch
from torch import nn

MAX_FEATURES = 4096  # csrc/swish_layernorm.hip kSlnMaxN


def _swish_layernorm_torch(input: torch.Tensor, norm: nn.Module) -> torch.Tensor:
    """The reference's formula in plain torch: the fall-back, and what tools/swishbench.py times as "torch"."""
    return input * norm(input)


class _SwishLayerNorm(torch.autograd.Function):
    """y [B, N] contiguous float32; gamma, beta [N]."""

    @staticmethod
    def forward(ctx, y, gamma, beta, eps):
        from ..distributed import _device_ops  # noqa: F401  (registers torch.ops.tbe_hip.*)

        out, stats = torch.ops.tbe_hip.swish_layernorm_forward(y, gamma, beta, eps)
        ctx.eps = eps
        ctx.save_for_backward(y, stats, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, G):
        y, stats, gamma, beta = ctx.saved_tensors
        need = ctx.needs_input_grad[:3]
        if torch.is_grad_enabled():  # create_graph: the same gradients from differentiable torch operations
            wanted = [t for t, w in zip((y, gamma, beta), need) if w]
            z = nn.functional.layer_norm(y, (y.shape[1],), gamma, beta, ctx.eps)
            grads = iter(torch.autograd.grad(y * torch.sigmoid(z), wanted, G, create_graph=True))
            return (*[next(grads) if w else None for w in need], None)
        gy, gp = torch.ops.tbe_hip.swish_layernorm_backward(G.contiguous(), y, stats, gamma, beta)
        return gy if need[0] else None, gp[0] if need[1] else None, gp[1] if need[2] else None, None


class SwishLayerNorm(nn.Module):
    """`Y = X * Sigmoid(LayerNorm(X))` over the trailing `input_dims` (torchrec/modules/activation.py:18-55)."""

    def __init__(self, input_dims: Union[int, List[int], torch.Size], device: Optional[torch.device] = None) -> None:
        super().__init__()
        self.norm: nn.Sequential = nn.Sequential(nn.LayerNorm(input_dims, device=device), nn.Sigmoid())

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        ln = self.norm[0]
        shape = tuple(ln.normalized_shape)
        N = math.prod(shape)
        gamma, beta = ln.weight, ln.bias
        if not (input.is_cuda and input.dtype == torch.float32 and input.dim() >= len(shape)
                and tuple(input.shape[input.dim() - len(shape):]) == shape and N % 4 == 0 and 0 < N <= MAX_FEATURES
                and gamma is not None and beta is not None
                and all(p.dtype == torch.float32 and p.device == input.device for p in (gamma, beta))):
            return _swish_layernorm_torch(input, self.norm)
        y = input.contiguous()
        if len(shape) != 1:
            gamma, beta = gamma.view(N), beta.view(N)
        if y.dim() != 2 or len(shape) != 1:  # the usual [B, N] with [N] parameters passes as it is: no view nodes for autograd
            y = y.view(-1, N)
        if torch.is_grad_enabled() and (y.requires_grad or gamma.requires_grad or beta.requires_grad):
            out = _SwishLayerNorm.apply(y, gamma, beta, ln.eps)
        else:
            from ..distributed import _device_ops  # noqa: F401

            out = torch.ops.tbe_hip.swish_layernorm_forward(y, gamma.detach(), beta.detach(), ln.eps)[0]
        return out if out.shape == input.shape else out.view(input.shape)
