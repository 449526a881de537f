"""Cross networks with the reference's constructors, parameter containers, names, shapes and initialisers
(torchrec/modules/crossnet.py: CrossNet :19-89, LowRankCrossNet :92-188, VectorCrossNet :191-268), so a reference
state_dict loads unchanged (`kernels.{i}`, `W_kernels.{i}`, `V_kernels.{i}`, `bias.{i}`).

On a HIP device, for a 2-D float32 input whose width is a multiple of 4:

* CrossNet / LowRankCrossNet run as ONE autograd.Function over all layers.  Forward per layer: the bias rides in the GEMM
  (torch.addmm) and x_0 * t + x_l is one torch.addcmul.  Backward per layer: one pass of csrc/crossnet.hip
  (`torch.ops.tbe_hip.cross_backward`: g_y = G * x_0, acc (+)= G * t, bias gradient), the weight gradients as batched
  split-K GEMMs (modules/mlp.py), G_l by a beta = 1 addmm; the input gradient is G_0 + acc.
* VectorCrossNet runs all layers in one forward and one backward kernel (`vector_cross_forward` / `_backward`).
* LowRankMixtureCrossNet (:271-446; `U_kernels.{i}`, `V_kernels.{i}`, `bias.{i}`, `gates.{k}.weight`, `C_kernels.{i}`) folds
  its K experts into one low-rank layer of rank K r and runs like LowRankCrossNet, with one narrow pass between the GEMMs
  (`mixture_gate_forward` / `_backward`); see the class.

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


# ---- LowRankMixtureCrossNet ---------------------------------------------------------------------------------------------------
MIXTURE_MAX_EXPERTS = 16  # csrc/crossnet.hip kMixMaxK


def _low_rank_mixture_cross_torch(x: torch.Tensor, u_kernels: Sequence[torch.Tensor], v_kernels: Sequence[torch.Tensor],
                                  bias: Sequence[torch.Tensor], gate_weights: Sequence[torch.Tensor],
                                  c_kernels: Sequence[torch.Tensor], activation=torch.relu) -> torch.Tensor:
    """The reference's forward op for op (torchrec/modules/crossnet.py:400-446): the [B, N, K] expert stack, softmax over
    dim 1 of the stacked gate logits, matmul.  gate_weights: K tensors [1, N], or none for K = 1."""
    K = u_kernels[0].shape[0] if len(u_kernels) else 0
    x_0 = x.unsqueeze(2)  # (B, N, 1)
    x_l = x_0
    for u, v, b, c in zip(u_kernels, v_kernels, bias, c_kernels):
        if K > 1:
            gating = torch.stack([torch.nn.functional.linear(x_l.squeeze(2), w) for w in gate_weights], 1)  # (B, K, 1)
        experts = []
        for i in range(K):
            expert = torch.matmul(v[i], x_l)  # (B, r, 1)
            expert = torch.matmul(c[i], activation(expert))  # (B, r, 1)
            expert = torch.matmul(u[i], activation(expert))  # (B, N, 1)
            expert = x_0 * (expert + b)  # (B, N, 1)
            experts.append(expert.squeeze(2))  # (B, N)
        experts = torch.stack(experts, 2)  # (B, N, K)
        if K > 1:
            x_l = torch.matmul(experts, torch.nn.functional.softmax(gating, 1)) + x_l  # (B, N, 1)
        else:
            x_l = experts + x_l
    return torch.squeeze(x_l, dim=2)


def _is_relu(activation) -> bool:
    return activation is torch.relu or activation is torch.nn.functional.relu or isinstance(activation, nn.ReLU)


def _ucat(u: torch.Tensor) -> torch.Tensor:
    """Ucat [N, K r] with Ucat[n, k r + j] = U[k, n, j]: the K experts' U side by side (a view for K = 1)."""
    K, N, r = u.shape
    return u.view(N, r) if K == 1 else u.permute(1, 0, 2).reshape(N, K * r)


def _mixture_forward(x0, L, K, params, wg, keep):
    """The folded forward (module docstring).  Returns x_L and, with `keep`, what the backward needs per layer:
    (x_l, t, h1, a2, m, p)."""
    from ..distributed import _device_ops  # noqa: F401  (registers torch.ops.tbe_hip.*)

    U, V, bias, C = params[:L], params[L:2 * L], params[2 * L:3 * L], params[len(params) - L:]
    B, N = x0.shape
    r = U[0].shape[2]
    kept = []
    x_l = x0
    for l in range(L):
        a1 = x_l @ V[l].view(K * r, N).t()  # [B, K r]
        logits = x_l @ wg.t() if K > 1 else None  # [B, K]
        h1 = torch.relu_(a1)
        a2 = torch.bmm(h1.view(B, K, r).transpose(0, 1), C[l].transpose(1, 2))  # [K, B, r]
        if K > 1:
            m, p = torch.ops.tbe_hip.mixture_gate_forward(a2, logits)
        else:
            m, p = torch.relu(a2).view(B, r), None
        t = torch.addmm(bias[l].view(-1), m, _ucat(U[l]).t())
        if keep:
            kept.append((x_l, t, h1, a2, m, p))
        x_l = torch.addcmul(x_l, x0, t)
    return x_l, kept


class _MixtureCross(torch.autograd.Function):
    """All layers of LowRankMixtureCrossNet; params = U_kernels + V_kernels + bias + gate weights (K, none for K = 1) +
    C_kernels, the module's registration order."""

    @staticmethod
    def forward(ctx, x0, num_layers, num_experts, *params):
        L, K = num_layers, num_experts
        wg = torch.cat(params[3 * L:len(params) - L]) if K > 1 else None  # [K, N]: the gates are shared by the layers
        out, kept = _mixture_forward(x0, L, K, params, wg, True)
        ctx.L, ctx.K = L, K
        flat = [a for layer in kept for a in layer if a is not None]
        ctx.save_for_backward(x0, *params, *([wg] if K > 1 else []), *flat)
        return out

    @staticmethod
    def backward(ctx, G):
        L, K = ctx.L, ctx.K
        saved = ctx.saved_tensors
        x0 = saved[0]
        P = 4 * L + (K if K > 1 else 0)
        params = saved[1:1 + P]
        U, V, C = params[:L], params[L:2 * L], params[P - L:]
        pos = 1 + P
        wg = None
        if K > 1:
            wg, pos = saved[pos], pos + 1
        per = 6 if K > 1 else 5
        layers = [saved[pos + per * l:pos + per * (l + 1)] for l in range(L)]
        need = ctx.needs_input_grad
        need_x, need_p = need[0], need[3:]
        need_gates = K > 1 and any(need_p[3 * L:3 * L + K])
        groups = (0, L, 2 * L, P - L)  # first index of U, V, bias, C
        grads: List = [None] * P
        B, N = x0.shape
        r = U[0].shape[2]
        G = G.contiguous()
        acc = torch.empty_like(x0)
        g_wg = None
        for l in reversed(range(L)):
            x_l, t, h1, a2, m = layers[l][:5]
            p = layers[l][5] if K > 1 else None
            gy, gb = torch.ops.tbe_hip.cross_backward(G, x0, t, acc, l == L - 1)
            if need_p[2 * L + l]:
                grads[2 * L + l] = gb.view(N, 1)
            if need_p[l]:
                gu = _DeferredWgrad.compute(gy, m, _wgrad_chunks(B, N, K * r))  # [N, K r]
                grads[l] = gu.view(1, N, r) if K == 1 else gu.view(N, K, r).permute(1, 0, 2).contiguous()
            # does anything below this layer still need G_l?
            below = need_x or (need_gates and l > 0) or any(need_p[g + j] for g in groups for j in range(l))
            if not (below or need_gates or need_p[L + l] or need_p[P - L + l]):
                break
            gm = gy @ _ucat(U[l])  # [B, K r]
            if K > 1:
                ga2, gl = torch.ops.tbe_hip.mixture_gate_backward(gm, a2, p)
            else:
                ga2, gl = torch.ops.aten.threshold_backward(gm.view(1, B, r), a2, 0), None
            if need_p[P - L + l]:
                grads[P - L + l] = torch.bmm(ga2.transpose(1, 2), h1.view(B, K, r).transpose(0, 1))  # [K, r, r]
            if need_gates:
                gw = gl.t() @ x_l  # [K, N], summed over the layers: the gates are shared
                g_wg = gw if g_wg is None else g_wg.add_(gw)
            if need_p[L + l] or below:
                gh1 = torch.bmm(ga2, C[l])  # [K, B, r]
                ga1 = torch.empty_like(h1)  # [B, K r]
                torch.ops.aten.threshold_backward.grad_input(gh1.transpose(0, 1), h1.view(B, K, r), 0,
                                                             grad_input=ga1.view(B, K, r))  # torch's ReLU mask, into [B, K r]
                if need_p[L + l]:
                    grads[L + l] = _DeferredWgrad.compute(ga1, x_l, _wgrad_chunks(B, K * r, N)).view(K, r, N)
                if below:
                    G = torch.addmm(G, ga1, V[l].view(K * r, N))
                    if K > 1:
                        G.addmm_(gl, wg)
            if not below:
                break
        if need_gates:
            for k in range(K):
                if need_p[3 * L + k]:
                    grads[3 * L + k] = g_wg[k:k + 1]
        gx = G + acc if need_x else None
        return (gx, None, None, *grads)


class LowRankMixtureCrossNet(nn.Module):
    """DCN-v2 with a mixture of K low-rank experts (torchrec/modules/crossnet.py:271-446):

        x_{l+1} = sum_k p_k x_0 * (U_lk g(C_lk g(V_lk x_l)) + b_l) + x_l,   p = softmax_k(gate_k . x_l)

    with U_l [K, N, r], V_l [K, r, N], C_l [K, r, r], b_l [N, 1] and K gates Linear(N, 1, bias=False) shared by all layers
    (none for K = 1, where the sum is its only term).

    On a HIP device — a 2-D float32 input with N % 4 == 0, float32 parameters, num_layers >= 1, K <= 16, ReLU as the
    activation — the [B, N, K] expert stack is never built: the softmax weights sum to 1, so the layer is
    x_0 * ([p_1 h_1 | ... | p_K h_K] Ucat^T + b) + x_l with h_k = relu(C_k relu(V_k x_l)) and Ucat[n, k r + j] = U[k, n, j],
    i.e. a LowRankCrossNet layer of rank K r: one GEMM [B, N] x [N, K r] (and the K gate logits), one batched r x r GEMM, one
    narrow pass over [B, K r] (`torch.ops.tbe_hip.mixture_gate_forward`: softmax, ReLU, scale, layout), one GEMM with the
    bias riding in it, one addcmul — as ONE autograd.Function over all layers, whose backward is `cross_backward` plus the
    mirror of the narrow pass (`mixture_gate_backward`) per layer.  Everything else silently takes the reference's formula
    in plain torch (`_low_rank_mixture_cross_torch`)."""

    def __init__(self, in_features: int, num_layers: int, num_experts: int = 1, low_rank: int = 1,
                 activation=torch.relu) -> None:
        super().__init__()
        assert num_experts >= 1, "num_experts must be larger or equal to 1"
        assert low_rank >= 1, "Low rank must be larger or equal to 1"
        self._num_layers = num_layers
        self._num_experts = num_experts
        self._low_rank = low_rank
        self._in_features = in_features
        K, N, r = num_experts, in_features, low_rank
        self.U_kernels: nn.Module = _param_list((K, N, r), num_layers, nn.init.xavier_normal_)
        self.V_kernels: nn.Module = _param_list((K, r, N), num_layers, nn.init.xavier_normal_)
        self.bias: nn.Module = _param_list((N, 1), num_layers, nn.init.zeros_)
        self.gates = nn.ModuleList([nn.Linear(N, 1, bias=False) for _ in range(K)]) if K > 1 else None
        self._activation = activation
        self.C_kernels: nn.Module = _param_list((K, r, r), num_layers, nn.init.xavier_normal_)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        gate_w = [g.weight for g in self.gates] if self.gates is not None else []
        params = [*self.U_kernels, *self.V_kernels, *self.bias, *gate_w, *self.C_kernels]
        L, K = self._num_layers, self._num_experts
        if L == 0 or K > MIXTURE_MAX_EXPERTS or not _is_relu(self._activation) or not _kernel_path(input, params):
            return _low_rank_mixture_cross_torch(input, list(self.U_kernels), list(self.V_kernels), list(self.bias), gate_w,
                                                 list(self.C_kernels), self._activation)
        x = input.contiguous()
        if _any_grad(x, params):
            return _MixtureCross.apply(x, L, K, *params)
        params = [p.detach() for p in params]
        return _mixture_forward(x, L, K, params, torch.cat(params[3 * L:3 * L + K]) if K > 1 else None, False)[0]
