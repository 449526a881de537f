"""Perceptron / MLP with the reference's module and parameter names
(torchrec/modules/mlp.py:14-170) so state_dict keys match (`_mlp.{i}._linear.weight`), and with its activation forms:
"relu" / "sigmoid" / "swish_layernorm", a tensor function, a module instance (shared), a zero-argument module factory (called
once per layer)."""
import contextlib
from typing import Callable, List, Optional, Tuple, Union

import torch
from torch import nn
from torch.autograd import Variable

from .activation import SwishLayerNorm
from .utils import extract_module_or_tensor_callable


class _DeferredWgrad:
    """Weight gradients set aside while a backward is being CAPTURED (distributed/hip_graph.py capture_backward(defer_wgrad=
    True)): the capture of the input-gradient chain ends first, and the weight-gradient GEMMs are captured into a second
    graph that the owner replays AFTER it has started the embedding-gradient all-to-all — dW is needed by nobody until the
    optimizer, the all-to-all by the embedding backward (models/dlrm.py explicit step).  `pending` is a list while such a
    capture is running, else None; entries are ("w", weight parameter, dY, X, split-K chunks) or — with `partials_ok`, i.e.
    when the segment's parameter gradients go into a flat buffer (param_grad_sinks) — ("p", parameter, partial sums
    [chunks, *parameter shape]): bias gradients as the row-block sums of the ReLU-backward kernel, the one-output layer's
    weight gradient as the row-block sums of its column-sum kernel.  The capture then finishes EVERY gradient of the segment
    — split-K chunk sums, row-block sums, complete gradients — with one `multi_chunk_sum` launch into the flat buffer."""

    pending: Optional[list] = None
    partials_ok: bool = False

    @classmethod
    def compute(cls, gy: torch.Tensor, x: torch.Tensor, c: int) -> torch.Tensor:
        B = x.shape[0]
        if c > 1 and B % c == 0:
            return torch.bmm(gy.view(c, B // c, -1).transpose(1, 2), x.view(c, B // c, -1)).sum(dim=0)
        return gy.t() @ x

    @classmethod
    def compute_partials(cls, gy: torch.Tensor, x: torch.Tensor, c: int) -> torch.Tensor:
        """[chunks, out, in] whose sum over dim 0 is dY^T X (the batched GEMM of `compute` without its reduction)."""
        B = x.shape[0]
        if c > 1 and B % c == 0:
            return torch.bmm(gy.view(c, B // c, -1).transpose(1, 2), x.view(c, B // c, -1))
        return (gy.t() @ x).unsqueeze(0)

    @classmethod
    def stashing(cls, t: torch.Tensor) -> bool:
        return cls.pending is not None and t.is_cuda and torch.cuda.is_current_stream_capturing()


class _EagerFinish:
    """Column-sum gradients of an EAGER backward, finished by ONE launch at its end.  Every bias gradient of a ReLU layer (and
    the one-output layer's weight gradient) is the sum of its kernel's row-block sums; finished per layer that is one
    `colsum_partials_kernel` launch each, eight per DLRM step, to add up a few hundred KB.  While `enabled` was set during the
    forward (DLRM.forward sets it round its dense stacks on the one-rank eager step, `DLRM.deferred_dense_finish`) and the
    backward is neither capturing nor building a graph of itself, the backward nodes below keep the row-block sums, return
    None for those gradients and `add` (parameters, sums) here.  The first `add` of a backward queues `_flush` on the autograd
    engine; at the end of the backward it cuts the parameters' `.grad` out of one flat buffer and fills them with one
    `multi_chunk_sum` launch in the second stage's own order (csrc/colsum.hpp): the same bits as the per-layer launches.
    Only a leaf parameter without `.grad` and without hooks is left to it (`takes`): accumulation into an existing
    gradient and hooks see the gradient at once, as before.  The gradients exist when `backward()` returns; a caller of
    `torch.autograd.grad` on these parameters turns the switch off."""

    enabled: bool = False
    flushes = 0  # finishing launches / gradients that went through them so far (tests)
    deferred = 0
    _pending: Optional[list] = None  # [(parameters, row-block sums [row blocks, sum of their numel])] of the backward `_task`
    _task: int = -1
    _stream: int = 0

    @classmethod
    @contextlib.contextmanager
    def enable(cls, on: bool):
        prev, cls.enabled = cls.enabled, bool(on)
        try:
            yield
        finally:
            cls.enabled = prev

    @classmethod
    def takes(cls, wanted: bool, t: torch.Tensor, *params: Optional[torch.Tensor]) -> bool:
        """True inside a backward whose node may leave the gradients of `params` to the finishing launch (`t`: its dY; an
        empty batch has no row blocks to keep: the one-pass entries give its zeros)."""
        if not (wanted and t.is_cuda and t.shape[0] > 0) or torch.is_grad_enabled() or torch.cuda.is_current_stream_capturing():
            return False
        task = torch._C._current_graph_task_id()
        if task < 0:
            return False
        waiting = cls._pending if cls._task == task and cls._pending else ()
        for p in params:
            if (p is None or not p.is_leaf or p.grad is not None or p._backward_hooks
                    or getattr(p, "_post_accumulate_grad_hooks", None)
                    or any(p is q for qs, _ in waiting for q in qs)):  # used twice in one graph: the second use accumulates
                return False
        return True

    @classmethod
    def add(cls, params: Tuple[torch.Tensor, ...], part: torch.Tensor) -> None:
        from fbgemm_gpu._lib import stream_ptr

        task = torch._C._current_graph_task_id()
        if cls._pending is None or cls._task != task:  # (a list left by a backward that raised belongs to another task)
            cls._pending, cls._task, cls._stream = [], task, stream_ptr(part.device)
            Variable._execution_engine.queue_callback(cls._flush)
        cls._pending.append((params, part))

    @classmethod
    def _flush(cls) -> None:
        from fbgemm_gpu._lib import stream_ptr
        from ..distributed._device_ops import finish_row_block_sums

        pend, cls._pending = cls._pending, None
        if not pend:
            return
        dev = pend[0][1].device
        if stream_ptr(dev) != cls._stream:  # the callback's stream is the caller's: order it behind the backward's
            cur = torch.cuda.current_stream(dev)
            cur.wait_stream(torch.cuda.ExternalStream(cls._stream, device=dev))
            for _, part in pend:
                part.record_stream(cur)
        segs, total = [], 0
        for _, part in pend:
            segs.append((part, total))
            total += (part.shape[1] + 63) // 64 * 64  # 256-B aligned slices
        flat = finish_row_block_sums(segs, torch.empty(total, dtype=torch.float32, device=dev))
        for (params, _), (_, off) in zip(pend, segs):
            for p in params:
                g = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
                p.grad = g if p.grad is None else p.grad + g
                cls.deferred += 1
        cls.flushes += 1


def _input_and_weight_grads(ctx, gy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor):
    """(dX, dW) of y = x W^T for a backward node whose inputs 0 and 1 are x and W, given dY (contiguous): the input-gradient
    GEMM, then the weight gradient as a batched GEMM over `ctx.chunks` batch slices — or, in a capture that defers the weight
    gradients, its stash (dW = None)."""
    gx = None
    if ctx.needs_input_grad[0]:
        if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) > x.shape[1] and x.stride(0) % 4 == 0:
            # the input is a row-padded view (16-B aligned rows, e.g. the 479-wide interaction output inside a 480-wide
            # buffer): give its gradient the same layout, so that the consumer reads aligned rows too
            gx = gy.new_empty((x.shape[0], x.stride(0)))[:, :x.shape[1]]
            torch.mm(gy, weight, out=gx)
        else:
            gx = gy @ weight
    c = ctx.chunks
    w = ctx.weight_param
    if w is not None and ctx.needs_input_grad[1] and _DeferredWgrad.stashing(gy):
        _DeferredWgrad.pending.append(("w", w, gy, x, c))  # captured later, into the segment's second backward graph
        gw = None
    else:
        gw = _DeferredWgrad.compute(gy, x, c)
    return gx, gw


class _LinearSplitKWgrad(torch.autograd.Function):
    """y = x W^T + b with the weight gradient computed as a batched GEMM over batch chunks.

    dW = dY^T X has a tiny output (out x in, e.g. 256 x 512) and a huge reduction dimension (the
    batch, 65 536): a plain GEMM launches ~50 workgroups on a 256-CU chip.  Splitting the batch
    into `chunks` slices turns it into one batched GEMM with `chunks` x more workgroups plus a
    small sum — the split-K the BLAS heuristic does not pick for this shape.  fp32 throughout;
    only the summation order of the batch reduction changes."""

    @staticmethod
    def forward(ctx, x, weight, bias, chunks, fuse_relu):
        ctx.chunks = chunks
        ctx.has_bias = bias is not None
        ctx.fuse_relu = fuse_relu
        ctx.defer_finish = _EagerFinish.enabled
        ctx.weight_param = weight if (weight.is_leaf and weight.requires_grad) else None
        ctx.bias_param = bias if (bias is not None and bias.is_leaf and bias.requires_grad) else None
        if fuse_relu:
            # bias + ReLU in the GEMM epilogue (hipBLASLt): no separate activation kernel
            out = torch._addmm_activation(bias, x, weight.t(), use_gelu=False)
            ctx.save_for_backward(x, weight, out)
            return out
        ctx.save_for_backward(x, weight)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, gy):
        gb = None
        gb_deferred = False
        if ctx.fuse_relu:
            x, weight, out = ctx.saved_tensors
            if ctx.has_bias and gy.dtype == torch.float32 and out.shape[1] % 4 == 0:
                # ReLU backward + bias gradient in one pass over [B, out] (csrc/mlp_epilogue.hip)
                from ..distributed import _device_ops  # noqa: F401  (registers torch.ops.tbe_hip.*)
                if (_DeferredWgrad.partials_ok and ctx.bias_param is not None and ctx.needs_input_grad[2]
                        and _DeferredWgrad.stashing(gy)):
                    # the row-block sums are finished later, together with every other gradient of the segment
                    gy, part = torch.ops.tbe_hip.relu_backward_bias_partials(gy, out)
                    _DeferredWgrad.pending.append(("p", ctx.bias_param, part))
                    gb_deferred = True
                elif _EagerFinish.takes(ctx.defer_finish and ctx.needs_input_grad[2], gy, ctx.bias_param):
                    gy, part = torch.ops.tbe_hip.relu_backward_bias_partials(gy, out)
                    _EagerFinish.add((ctx.bias_param,), part)
                    gb_deferred = True
                else:
                    gy, gb = torch.ops.tbe_hip.relu_backward_bias_grad(gy, out)
            else:
                gy = torch.ops.aten.threshold_backward(gy.contiguous(), out, 0.0)
        else:
            x, weight = ctx.saved_tensors
            gy = gy.contiguous()
        gx, gw = _input_and_weight_grads(ctx, gy, x, weight)
        if gb is None and ctx.has_bias and not gb_deferred:
            gb = gy.sum(dim=0)
        return gx, gw, gb, None, None


class _LinearOneOutput(torch.autograd.Function):
    """y = x W^T + b for a Linear with ONE output feature.  Its weight gradient dW[0, c] = sum_b dy[b] x[b, c]
    is a GEMM with N = 1, which the BLAS libraries run at ~1 % of HBM speed (86 us for [65536, 256] with the
    best of all hipBLASLt / rocBLAS solutions); here it is one pass over x (csrc/mlp_epilogue.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.weight_param = weight if (weight.is_leaf and weight.requires_grad) else None
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, gy):
        from ..distributed import _device_ops  # noqa: F401  (registers torch.ops.tbe_hip.*)

        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gy @ weight if ctx.needs_input_grad[0] else None
        if _DeferredWgrad.partials_ok and ctx.weight_param is not None and _DeferredWgrad.stashing(gy):
            part = torch.ops.tbe_hip.weighted_colsum_partials(x, gy.view(-1))  # [row blocks, in]
            _DeferredWgrad.pending.append(("p", ctx.weight_param, part.view(part.shape[0], 1, -1)))
            gw = None
        else:
            gw = torch.ops.tbe_hip.weighted_colsum(x, gy.view(-1)).view(1, -1)
        gb = gy.sum(dim=0) if ctx.has_bias else None
        return gx, gw, gb


class _ReluLinearOneOutput(torch.autograd.Function):
    """h = relu(x W^T + b), y = h w^T + c with ONE output: a hidden layer and the one-output Linear behind it (the last two
    layers of DLRM's over arch) as one node.  Forward: the two calls of _LinearSplitKWgrad and _LinearOneOutput.  Backward:
    those two ran dy w (a K = 1 GEMM that writes [B, N]), a pass over h for dw, and a pass over both for the masked
    gradient and db; here ONE pass over h gives all three (csrc/mlp_epilogue.hip relu_linear1_bwd_kernel), bit for bit."""

    @staticmethod
    def forward(ctx, x, weight, bias, chunks, weight_out, bias_out):
        ctx.chunks = chunks
        ctx.has_bias_out = bias_out is not None
        ctx.defer_finish = _EagerFinish.enabled
        ctx.weight_param = weight if (weight.is_leaf and weight.requires_grad) else None
        ctx.sum_params = (bias, weight_out)
        h = torch._addmm_activation(bias, x, weight.t(), use_gelu=False)
        ctx.save_for_backward(x, weight, h, weight_out)
        return torch.nn.functional.linear(h, weight_out, bias_out)

    @staticmethod
    def backward(ctx, gy):
        from ..distributed import _device_ops  # noqa: F401  (registers torch.ops.tbe_hip.*)

        x, weight, h, weight_out = ctx.saved_tensors
        gy = gy.contiguous()
        N = h.shape[1]
        if _EagerFinish.takes(ctx.defer_finish and ctx.needs_input_grad[2] and ctx.needs_input_grad[4], gy, *ctx.sum_params):
            g, part = torch.ops.tbe_hip.relu_linear1_backward_partials(h, gy.view(-1), weight_out)
            _EagerFinish.add(ctx.sum_params, part)  # [row blocks, db | dw]
            gb = gw_out = None
        else:
            g, sums = torch.ops.tbe_hip.relu_linear1_backward(h, gy.view(-1), weight_out)
            gb, gw_out = sums[:N], sums[N:].view(1, N)
        gb_out = gy.sum(dim=0) if ctx.has_bias_out else None
        gx, gw = _input_and_weight_grads(ctx, g, x, weight)
        return gx, gw, gb, None, gw_out, gb_out


class LinearOut(nn.Linear):
    """nn.Linear (same parameters / state_dict keys) whose one-output case uses _LinearOneOutput on a HIP device."""

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if (self.out_features == 1 and input.is_cuda and input.dim() == 2 and input.dtype == torch.float32
                and self.in_features % 4 == 0 and torch.is_grad_enabled() and self.weight.requires_grad):
            return _LinearOneOutput.apply(input, self.weight, self.bias)
        return super().forward(input)


def _wgrad_chunks(batch: int, out_f: int, in_f: int) -> int:
    """Chunks for the split-K weight gradient: enough (128 x 128)-tile workgroups to fill 256 CUs."""
    tiles = max(1, (out_f + 127) // 128) * max(1, (in_f + 127) // 128)
    c = 1
    while tiles * c < 256 and c < 32 and batch % (2 * c) == 0 and batch // (2 * c) >= 1024:
        c *= 2
    return c


class Perceptron(nn.Module):
    def __init__(self, in_size: int, out_size: int, bias: bool = True,
                 activation: Union[nn.Module, Callable[[torch.Tensor], torch.Tensor]] = torch.relu,
                 device: Optional[torch.device] = None) -> None:
        super().__init__()
        self._in_size, self._out_size = in_size, out_size
        self._linear = nn.Linear(in_size, out_size, bias=bias, device=device)
        self._activation_fn = activation

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        lin = self._linear
        if input.is_cuda and input.dim() == 2 and torch.is_grad_enabled() and lin.weight.requires_grad:
            c = _wgrad_chunks(input.shape[0], self._out_size, self._in_size)
            relu = self._activation_fn is torch.relu and lin.bias is not None
            if c > 1 or relu:
                y = _LinearSplitKWgrad.apply(input, lin.weight, lin.bias, c, relu)
                return y if relu else self._activation_fn(y)
        return self._activation_fn(lin(input))


def relu_linear1_head(hidden: Perceptron, out: nn.Linear, input: torch.Tensor) -> Optional[torch.Tensor]:
    """out(hidden(input)) as ONE autograd node (_ReluLinearOneOutput) where that applies — float32 on a HIP device, `hidden`
    with bias + ReLU and a width that is a multiple of 4, `out` with one output, training (every parameter wants its
    gradient), not inside a graph capture — else None: the caller runs the two modules."""
    lin = hidden._linear
    if not (out.out_features == 1 and input.is_cuda and input.dim() == 2 and input.dtype == torch.float32
            and hidden._activation_fn is torch.relu and lin.bias is not None and hidden._out_size % 4 == 0
            and hidden._out_size <= 1 << 20 and torch.is_grad_enabled()
            and all(p.requires_grad and p.dtype == torch.float32 for p in (lin.weight, lin.bias, out.weight))
            and (out.bias is None or out.bias.requires_grad) and not torch.cuda.is_current_stream_capturing()):
        return None
    c = _wgrad_chunks(input.shape[0], hidden._out_size, hidden._in_size)
    return _ReluLinearOneOutput.apply(input, lin.weight, lin.bias, c, out.weight, out.bias)


class MLP(nn.Module):
    def __init__(self, in_size: int, layer_sizes: List[int], bias: bool = True,
                 activation: Union[str, Callable] = torch.relu, device: Optional[torch.device] = None) -> None:
        super().__init__()
        if activation == "relu":
            activation = torch.relu
        elif activation == "sigmoid":
            activation = torch.sigmoid
        sizes = [in_size] + list(layer_sizes)
        if activation == "swish_layernorm":  # one module per layer (torchrec/modules/mlp.py:145-157)
            def layer_activation(i):
                return SwishLayerNorm(layer_sizes[i], device=device)
        elif isinstance(activation, str):
            raise ValueError(f"MLP supports the activation strings relu, sigmoid and swish_layernorm, got {activation!r}")
        else:  # a zero-argument factory is called once per layer; torch.relu comes back as torch.relu (:131-143)
            def layer_activation(i):
                return extract_module_or_tensor_callable(activation)
        self._mlp = nn.Sequential(*[
            Perceptron(sizes[i], sizes[i + 1], bias=bias, activation=layer_activation(i), device=device)
            for i in range(len(layer_sizes))])

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return self._mlp(input)
