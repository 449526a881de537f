"""Cross networks with the reference's constructors, parameter containers, names, shapes and initialisers
(torchrec/modules/crossnet.py: CrossNet :19-89, LowRankCrossNet :92-188, VectorCrossNet :191-268), so a reference
state_dict loads unchanged (`kernels.{i}`, `W_kernels.{i}`, `V_kernels.{i}`, `bias.{i}`).

On a HIP device, for a 2-D float32 input whose width is a multiple of 4:

* CrossNet / LowRankCrossNet run as ONE autograd.Function over all layers.  Forward per layer: the bias rides in the GEMM
  (torch.addmm) and x_0 * t + x_l is one torch.addcmul.  Backward per layer: one pass of csrc/crossnet.hip
  (`torch.ops.tbe_hip.cross_backward`: g_y = G * x_0, acc (+)= G * t, bias gradient), the weight gradients as batched
  split-K GEMMs (modules/mlp.py), G_l by a beta = 1 addmm; the input gradient is G_0 + acc.
* VectorCrossNet runs all layers in one forward and one backward kernel (`vector_cross_forward` / `_backward`).

Everything else (CPU tensors, other dtypes or ranks, a width that is no multiple of 4, VectorCrossNet beyond N = 4096 or
8 layers) silently takes the plain torch expression of the reference's formula, as LinearOut and Perceptron do."""
from typing import List, Sequence

import torch
from torch import nn

from .mlp import _DeferredWgrad, _wgrad_chunks

VECTOR_MAX_FEATURES = 4096  # csrc/crossnet.hip kVecMaxN / kVecMaxL
VECTOR_MAX_LAYERS = 8


# ---- the reference's formulas in plain torch: the fall-back, and what tools/crossbench.py times as "torch" ----------------
def _cross_torch(x: torch.Tensor, kernels: Sequence[torch.Tensor], bias: Sequence[torch.Tensor]) -> torch.Tensor:
    x_l = x
    for k, b in zip(kernels, bias):
        x_l = x * (x_l @ k.t() + b.view(-1)) + x_l
    return x_l


def _low_rank_cross_torch(x: torch.Tensor, w_kernels: Sequence[torch.Tensor], v_kernels: Sequence[torch.Tensor],
                          bias: Sequence[torch.Tensor]) -> torch.Tensor:
    x_l = x
    for w, v, b in zip(w_kernels, v_kernels, bias):
        x_l = x * ((x_l @ v.t()) @ w.t() + b.view(-1)) + x_l
    return x_l


def _vector_cross_torch(x: torch.Tensor, kernels: Sequence[torch.Tensor], bias: Sequence[torch.Tensor]) -> torch.Tensor:
    # x_0 * s_l: on the CPU as the reference's batched [N, 1] x [1, 1] matmul, whose backward forms the row dot G . x_0 in
    # the BLAS's order — the broadcast product's sum kernel orders it otherwise, which moves small elements of the
    # gradients by 3e-6 against the reference's float32 run.  On a GPU the broadcast product is the faster composition.
    batched = x.dim() == 2 and not x.is_cuda
    x_l = x
    for k, b in zip(kernels, bias):
        s = x_l @ k  # [B, 1]
        xs = torch.bmm(x.unsqueeze(2), s.unsqueeze(2)).squeeze(2) if batched else x * s
        x_l = xs + b.view(-1) + x_l
    return x_l


def _kernel_path(x: torch.Tensor, params: Sequence[torch.Tensor]) -> bool:
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.shape[1] % 4 == 0
            and all(p.dtype == torch.float32 and p.device == x.device for p in params))


def _any_grad(x: torch.Tensor, params: Sequence[torch.Tensor]) -> bool:
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))


class _GemmCross(torch.autograd.Function):
    """All layers of CrossNet (params = kernels + bias) or LowRankCrossNet (W_kernels + V_kernels + bias)."""

    @staticmethod
    def forward(ctx, x0, low_rank, num_layers, *params):
        L = num_layers
        bias = params[-L:]
        xs, ts, vs = [x0], [], []
        x_l = x0
        for l in range(L):
            b = bias[l].view(-1)
            if low_rank:
                v = x_l @ params[L + l].t()  # [B, r]
                t = torch.addmm(b, v, params[l].t())
                vs.append(v)
            else:
                t = torch.addmm(b, x_l, params[l].t())
            ts.append(t)
            x_l = torch.addcmul(x_l, x0, t)
            if l + 1 < L:
                xs.append(x_l)
        ctx.low_rank, ctx.L = low_rank, L
        ctx.save_for_backward(*params, *xs, *ts, *vs)
        return x_l

    @staticmethod
    def backward(ctx, G):
        from ..distributed import _device_ops  # noqa: F401  (registers torch.ops.tbe_hip.*)

        L, low = ctx.L, ctx.low_rank
        P = (3 if low else 2) * L
        saved = ctx.saved_tensors
        params, xs, ts, vs = saved[:P], saved[P:P + L], saved[P + L:P + 2 * L], saved[P + 2 * L:]
        need = ctx.needs_input_grad
        need_x, need_p = need[0], need[3:]
        grads: List = [None] * P
        x0 = xs[0]
        B, N = x0.shape
        G = G.contiguous()
        acc = torch.empty_like(x0)
        for l in reversed(range(L)):
            gy, gb = torch.ops.tbe_hip.cross_backward(G, x0, ts[l], acc, l == L - 1)
            if need_p[P - L + l]:
                grads[P - L + l] = gb.view(N, 1)
            # does anything below this layer still need G_l?
            below = need_x or any(need_p[i * L + j] for i in range(P // L) for j in range(l))
            if low:
                W, V = params[l], params[L + l]
                r = W.shape[1]
                if need_p[l]:
                    grads[l] = _DeferredWgrad.compute(gy, vs[l], _wgrad_chunks(B, N, r))
                if need_p[L + l] or below:
                    gv = gy @ W
                    if need_p[L + l]:
                        grads[L + l] = _DeferredWgrad.compute(gv, xs[l], _wgrad_chunks(B, r, N))
                    if below:
                        G = torch.addmm(G, gv, V)
            else:
                if need_p[l]:
                    grads[l] = _DeferredWgrad.compute(gy, xs[l], _wgrad_chunks(B, N, N))
                if below:
                    G = torch.addmm(G, gy, params[l])
            if not below:
                break
        gx = G + acc if need_x else None
        return (gx, None, None, *grads)


class _VectorCross(torch.autograd.Function):
    """All layers of VectorCrossNet; params = kernels + bias, each [N, 1]."""

    @staticmethod
    def forward(ctx, x0, num_layers, *params):
        from ..distributed import _device_ops  # noqa: F401

        L = num_layers
        w = torch.stack([p.view(-1) for p in params[:L]])
        b = torch.stack([p.view(-1) for p in params[L:]])
        out, s = torch.ops.tbe_hip.vector_cross_forward(x0, w, b)
        ctx.L = L
        ctx.save_for_backward(x0, s, w, b)
        return out

    @staticmethod
    def backward(ctx, G):
        L = ctx.L
        x0, s, w, b = ctx.saved_tensors
        gin, gp = torch.ops.tbe_hip.vector_cross_backward(G.contiguous(), x0, s, w, b)
        N = x0.shape[1]
        need_p = ctx.needs_input_grad[2:]
        gw = [gp[L + l].view(N, 1) if need_p[l] else None for l in range(L)]
        gb = [gp[l].view(N, 1) if need_p[L + l] else None for l in range(L)]
        return (gin if ctx.needs_input_grad[0] else None, None, *gw, *gb)


def _param_list(shape, num_layers: int, init) -> nn.ParameterList:
    return nn.ParameterList([nn.Parameter(init(torch.empty(*shape))) for _ in range(num_layers)])


class CrossNet(nn.Module):
    """x_{l+1} = x_0 * (W_l x_l + b_l) + x_l with full-rank W_l [N, N] (torchrec/modules/crossnet.py:19-89)."""

    def __init__(self, in_features: int, num_layers: int) -> None:
        super().__init__()
        self._num_layers = num_layers
        self.kernels: nn.Module = _param_list((in_features, in_features), num_layers, nn.init.xavier_normal_)
        self.bias: nn.Module = _param_list((in_features, 1), num_layers, nn.init.zeros_)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        params = [*self.kernels, *self.bias]
        if self._num_layers == 0 or not _kernel_path(input, params):
            return _cross_torch(input, list(self.kernels), list(self.bias))
        return _GemmCross.apply(input.contiguous(), False, self._num_layers, *params)


class LowRankCrossNet(nn.Module):
    """x_{l+1} = x_0 * (W_l (V_l x_l) + b_l) + x_l with W_l [N, r], V_l [r, N] (torchrec/modules/crossnet.py:92-188)."""

    def __init__(self, in_features: int, num_layers: int, low_rank: int = 1) -> None:
        super().__init__()
        assert low_rank >= 1, "Low rank must be larger or equal to 1"
        self._num_layers = num_layers
        self._low_rank = low_rank
        self.W_kernels: nn.Module = _param_list((in_features, low_rank), num_layers, nn.init.xavier_normal_)
        self.V_kernels: nn.Module = _param_list((low_rank, in_features), num_layers, nn.init.xavier_normal_)
        self.bias: nn.Module = _param_list((in_features, 1), num_layers, nn.init.zeros_)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        params = [*self.W_kernels, *self.V_kernels, *self.bias]
        if self._num_layers == 0 or not _kernel_path(input, params):
            return _low_rank_cross_torch(input, list(self.W_kernels), list(self.V_kernels), list(self.bias))
        return _GemmCross.apply(input.contiguous(), True, self._num_layers, *params)


class VectorCrossNet(nn.Module):
    """x_{l+1} = x_0 * (w_l . x_l) + b_l + x_l with a vector w_l [N, 1] — DCN (torchrec/modules/crossnet.py:191-268)."""

    def __init__(self, in_features: int, num_layers: int) -> None:
        super().__init__()
        self._num_layers = num_layers
        self.kernels: nn.Module = _param_list((in_features, 1), num_layers, nn.init.xavier_normal_)
        self.bias: nn.Module = _param_list((in_features, 1), num_layers, nn.init.zeros_)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        params = [*self.kernels, *self.bias]
        L = self._num_layers
        if (not 1 <= L <= VECTOR_MAX_LAYERS or not _kernel_path(input, params)
                or input.shape[1] > VECTOR_MAX_FEATURES):
            return _vector_cross_torch(input, list(self.kernels), list(self.bias))
        x = input.contiguous()
        if _any_grad(x, params):
            return _VectorCross.apply(x, L, *params)
        from ..distributed import _device_ops  # noqa: F401

        w = torch.stack([p.detach().view(-1) for p in self.kernels])
        b = torch.stack([p.detach().view(-1) for p in self.bias])
        return torch.ops.tbe_hip.vector_cross_forward(x, w, b)[0]
