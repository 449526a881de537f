"""BERT4Rec with the reference's constructors, assertions, module tree and registration order
(examples/bert4rec/models/bert4rec.py): `history.positional`, `history.layernorm.*`,
`transformer_blocks.<i>.attention.linear_layers.<k>.*`, `...output_linear.*`, `out.*` load from a reference state_dict; the
item table keeps this package's EmbeddingCollection naming, as under DLRM and SimpleDeepFMNN.

What runs differently:
  * MultiHeadedAttention, on a HIP device with float32 inputs, a supported (L, d_k) and no mask or a key-padding mask:
    the three projections stay torch's nn.Linear, their outputs go to one fused kernel each way (csrc/attention.hip) where
    they are, and its [B, L, H * d_k] result goes straight into output_linear.  No [B, H, L, L] tensor exists; autograd keeps
    the three projections and one float per row.  An (L, d_k) the LDS-resident kernels cannot hold — (200, 128), every L
    above 256 up to 4096 — takes the tiled kernels of csrc/attention_tiled.hip in the same way (`last_kernel` says which;
    `prefer_tiled = True` sends every supported shape there); their backward also reads the result that output_linear keeps
    for its own backward.  Everything else silently takes `_attention_torch`, the reference's
    expression op for op: CPU tensors, other dtypes, an unsupported (L, d_k), a materialised or per-query mask, p >= 1,
    active dropout under stream capture (the per-call counter is host state and would freeze in a graph).  Double backward
    (create_graph=True) of a kernel-path forward recomputes the gradients from differentiable torch operations when the
    kernel's dropout was inactive, and raises RuntimeError when it was active: the kernel's mask exists in no tensor.
  * The kernel's dropout mask is its own counter-based draw (include/tbe_hip.h), not torch's generator: seed =
    torch.initial_seed(), call = a per-module counter that advances once per training forward, below a high word that is
    0 for a stand-alone module and 1 + the layer index inside BERT4Rec.
  * TransformerBlock, on a HIP device with float32 [B, L, N], N % 4 == 0, 4 <= N <= 4096 and affine LayerNorms: everything
    between the GEMMs and the attention kernel is three launches of one kernel and one of another each way
    (csrc/residual_layernorm.hip):  n1 = LN1(x);  x1, n2 = x + drop(attention(n1)), LN2(x1);  h = drop(relu(w_1(n2)));
    x2 = drop(x1 + drop(w_2(h))) and, inside BERT4Rec, the next block's LN1(x2) with it (`_forward_chained`).  Autograd keeps
    the residual streams and two floats per row: no dropout mask, no copy of a LayerNorm's input.  The dropouts draw as the
    attention kernel's does, under a domain tag of their own, with `site` 0 = input_sublayer.dropout, 1 =
    output_sublayer.dropout, 2 = the block's dropout, 3 = feed_forward.dropout and a per-block call counter.  Everything
    else silently takes the torch expression: `kernel_path = False`, CPU tensors, other dtypes, other N,
    elementwise_affine=False, p >= 1, active dropout under stream capture.  Double backward of a kernel-path forward
    recomputes from differentiable torch operations with dropout inactive and raises RuntimeError with it active.
    SublayerConnection and PositionwiseFeedForward called on their own are the reference's expressions.
  * HistoryArch, when the batch's keys are the collection's one feature, the item table is one float32 DEVICE table without
    a row cache behind either TBE class, (history_len, emb_dim) is supported (emb_dim % 4 == 0, 4 <= emb_dim <= 2048,
    history_len * emb_dim <= 32 768), `positional` and the affine LayerNorm are float32 on the device and p < 1: lookup, padding, positional add,
    LayerNorm over [history_len, emb_dim] and dropout are one launch each way (csrc/history_arch.hip).  Autograd keeps the
    ids, the offsets and two floats per sample; the backward hands the jagged [N, emb_dim] gradient to the table's own
    backward (fused optimizer, or the dense gradient of `.weights`).  The dropout draws as the blocks' do, with site 4, the
    high word 0 and a per-module call counter.  Everything else silently takes the torch expression: `kernel_path = False`,
    FP16 tables, several features, CPU parameters, elementwise_affine=False, p >= 1, active dropout under stream capture.
    Double backward of a kernel-path forward raises RuntimeError.  So does a backward that finds the fused table updated
    since its forward (two forwards, then two backwards): it recomputes xhat from the live rows, and the saved statistics
    no longer belong to them.  The torch expression keeps the embeddings and has no such limit.
  * BERT4Rec.forward builds the mask with .expand (stride 0 along the queries) where the reference uses .repeat, and
    HistoryArch adds `positional` by broadcasting.
  * HistoryArch and BERT4Rec take a keyword-only `fused_params` for the EmbeddingCollection (the fused ADAM of
    examples/bert4rec/bert4rec_main.py:488-491; there is no EmbeddingCollectionSharder here)."""
import copy
import math
from typing import Callable, Optional, Tuple

import torch
import torch.nn as nn

from ..modules.embedding_configs import EmbeddingConfig
from ..modules.embedding_modules import EmbeddingCollection
from ..sparse.jagged_tensor import KeyedJaggedTensor


def clones(module: nn.Module, N: int) -> nn.ModuleList:
    """N deep copies of `module` (examples/bert4rec/models/bert4rec.py:20-31)."""
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


def _scaled_dot_product(query, key, value, mask, dropout) -> Tuple[torch.Tensor, torch.Tensor]:
    """examples/bert4rec/models/bert4rec.py:72-82, op for op."""
    scores = torch.matmul(query, key.transpose(-2, -1)) / math.sqrt(query.size(-1))
    if mask is not None:
        scores = scores.masked_fill(mask == 0, -1e9)
    p_attn = nn.functional.softmax(scores, dim=-1)
    if dropout is not None:
        p_attn = dropout(p_attn)
    return torch.matmul(p_attn, value), p_attn


def _attention_torch(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], num_heads: int,
                     dropout: Optional[nn.Module]) -> torch.Tensor:
    """The reference's attention between the projections q, k, v [B, L, H * d_k] and output_linear's input
    (examples/bert4rec/models/bert4rec.py:152-170) in plain torch: the fall-back, and what tools/attnbench.py times as
    "torch"."""
    B, d_k = q.size(0), q.size(-1) // num_heads
    q, k, v = [t.view(B, -1, num_heads, d_k).transpose(1, 2) for t in (q, k, v)]
    x, _ = _scaled_dot_product(q, k, v, mask, dropout)
    return x.transpose(1, 2).contiguous().view(B, -1, num_heads * d_k)


def key_padding_mask(mask: Optional[torch.Tensor], B: int, L: int) -> Tuple[bool, Optional[torch.Tensor]]:
    """(recognised, key_valid): whether `mask` is None or a key-padding mask in the reference's shape — [B, 1, L, L] or
    broadcastable to it, the same for every query row BY CONSTRUCTION (size 1 or stride 0 along the head and query
    dimensions; the values of a materialised mask are not inspected: that would be a device-to-host copy) — and then the
    kernel's key_valid: None, or uint8 [B, L] = mask[:, 0, 0, :] != 0."""
    if mask is None:
        return True, None
    if mask.dim() != 4 or mask.shape[0] not in (1, B) or mask.shape[3] != L:
        return False, None
    for dim, size in ((1, 1), (2, L)):
        if not (mask.shape[dim] == 1 or (mask.shape[dim] == size and mask.stride(dim) == 0)):
            return False, None
    valid = (mask[:, 0, 0, :] != 0).expand(B, L).contiguous()
    return True, valid.view(torch.uint8)


class _FusedAttention(torch.autograd.Function):
    """q, k, v: the projections [B, L, H * d_k] float32 (any batch / row strides) -> [B, L, H * d_k] contiguous."""

    @staticmethod
    def forward(ctx, q, k, v, key_valid, H, p, seed, call):
        from ..distributed._device_ops import attention_forward

        out, lse = attention_forward(q, k, v, key_valid, H, p, seed, call)
        ctx.save_for_backward(q, k, v, lse)
        ctx.key_valid, ctx.args = key_valid, (H, p, seed, call)
        return out

    @staticmethod
    def backward(ctx, G):
        from ..distributed._device_ops import attention_backward

        q, k, v, lse = ctx.saved_tensors
        H, p, seed, call = ctx.args
        need = ctx.needs_input_grad[:3]
        if torch.is_grad_enabled():
            return (*_attention_grads_by_torch(ctx, G, q, k, v), None, None, None, None, None)
        dq, dk, dv = attention_backward(G.contiguous(), q, k, v, ctx.key_valid, lse, H, p, seed, call, need)
        return dq, dk, dv, None, None, None, None, None


def _attention_grads_by_torch(ctx, G, q, k, v):
    """create_graph: the gradients of a kernel-path forward from differentiable torch operations."""
    H, p, _, _ = ctx.args
    need = ctx.needs_input_grad[:3]
    if p != 0.0:
        raise RuntimeError("MultiHeadedAttention: double backward through the fused kernel's dropout is not supported")
    mask = None if ctx.key_valid is None else ctx.key_valid[:, None, None, :]
    wanted = [t for t, w in zip((q, k, v), need) if w]
    grads = iter(torch.autograd.grad(_attention_torch(q, k, v, mask, H, None), wanted, G, create_graph=True))
    return [next(grads) if w else None for w in need]


class _TiledAttention(torch.autograd.Function):
    """_FusedAttention through the tiled kernels (csrc/attention_tiled.hip).  It also keeps its result, from which the backward
    takes D = dO . O; output_linear keeps that tensor for its own backward anyway."""

    @staticmethod
    def forward(ctx, q, k, v, key_valid, H, p, seed, call):
        from ..distributed._device_ops import attention_tiled_forward

        out, lse = attention_tiled_forward(q, k, v, key_valid, H, p, seed, call)
        ctx.save_for_backward(q, k, v, lse, out)
        ctx.key_valid, ctx.args = key_valid, (H, p, seed, call)
        return out

    @staticmethod
    def backward(ctx, G):
        from ..distributed._device_ops import attention_tiled_backward

        q, k, v, lse, out = ctx.saved_tensors
        H, p, seed, call = ctx.args
        if torch.is_grad_enabled():
            return (*_attention_grads_by_torch(ctx, G, q, k, v), None, None, None, None, None)
        dq, dk, dv = attention_tiled_backward(G.contiguous(), out, q, k, v, ctx.key_valid, lse, H, p, seed, call,
                                              ctx.needs_input_grad[:3])
        return dq, dk, dv, None, None, None, None, None


class Attention(nn.Module):
    """'Scaled Dot Product Attention' (examples/bert4rec/models/bert4rec.py:34-82): returns (output, p_attn) through the
    torch expression.  The reference's public class; nothing on the model's kernel path calls it."""

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, mask: Optional[torch.Tensor] = None,
                dropout: Optional[nn.Dropout] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        return _scaled_dot_product(query, key, value, mask, dropout)


class MultiHeadedAttention(nn.Module):
    """Multi-headed attention block (examples/bert4rec/models/bert4rec.py:85-171).

    Args:
        num_heads (int): number of attention heads
        dim_model (int): input/output dimensionality
        dropout (float): the dropout probability
        device: (Optional[torch.device]).
    """

    def __init__(self, num_heads: int, dim_model: int, dropout: float = 0.1, device: Optional[torch.device] = None) -> None:
        super().__init__()
        assert dim_model % num_heads == 0
        # We assume d_v always equals d_k
        self.d_k: int = dim_model // num_heads
        self.num_heads = num_heads
        self.linear_layers = nn.ModuleList([nn.Linear(dim_model, dim_model, device=device) for _ in range(3)])
        self.output_linear = nn.Linear(dim_model, dim_model, device=device)
        self.attention = Attention()
        self.dropout = nn.Dropout(p=dropout)
        self.kernel_path = True     # False: always `_attention_torch` (tests and tools compare the two)
        self.last_path = None       # "kernel" / "torch": what the last forward took
        self.last_kernel = None     # "resident" / "tiled" (csrc/attention.hip / attention_tiled.hip), None on the torch path
        self.prefer_tiled = False   # True: the tiled kernels also where the resident ones would do (tools and tests compare)
        # The high word of the kernel dropout's `call`: 0 for a module built on its own, 1 + the layer index inside BERT4Rec,
        # so that the layers of a model do not drop the same (b, h, i, j).  No process state enters: two stand-alone modules
        # under the same seed draw the same masks call for call.
        self._dropout_salt = 0
        self._dropout_calls = 0     # training forwards with active kernel dropout so far

    def _kernel_inputs(self, q, k, v, mask, p):
        """(kernel, key_valid): "resident" / "tiled" when this call may take that kernel, else None."""
        if not (self.kernel_path and q.is_cuda and q.dtype == torch.float32 and q.dim() == 3 and k.shape == q.shape
                and v.shape == q.shape and k.dtype == q.dtype and v.dtype == q.dtype and q.shape[0] > 0 and 0.0 <= p < 1.0):
            return None, None
        from ..distributed._device_ops import attention_supported, attention_tiled_supported

        if attention_supported(q.shape[1], self.d_k) and not self.prefer_tiled:
            kernel = "resident"
        elif attention_tiled_supported(q.shape[1], self.d_k):
            kernel = "tiled"
        else:
            return None, None
        if p > 0.0 and torch.cuda.is_current_stream_capturing():
            return None, None
        ok, key_valid = key_padding_mask(mask, q.shape[0], q.shape[1])
        if not ok or (key_valid is not None and key_valid.device != q.device):
            return None, None
        return kernel, key_valid

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        # 1) the linear projections dim_model => num_heads x d_k, left as [B, L, H * d_k]
        q, k, v = [layer(x) for layer, x in zip(self.linear_layers, (query, key, value))]
        p = float(self.dropout.p) if self.training else 0.0
        kernel, key_valid = self._kernel_inputs(q, k, v, mask, p)
        self.last_kernel = kernel
        if kernel is None:
            self.last_path = "torch"
            return self.output_linear(_attention_torch(q, k, v, mask, self.num_heads, self.dropout))
        self.last_path = "kernel"
        # 2) attention over all heads in one launch; 3) the heads are already side by side for the final linear
        seed = call = 0
        if p > 0.0:
            seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
            call = (self._dropout_salt << 32) | (self._dropout_calls & 0xFFFFFFFF)
            self._dropout_calls += 1
        if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
            fn = _TiledAttention if kernel == "tiled" else _FusedAttention
            x = fn.apply(q, k, v, key_valid, self.num_heads, p, seed, call)
        else:
            from ..distributed._device_ops import attention_forward, attention_tiled_forward

            fwd = attention_tiled_forward if kernel == "tiled" else attention_forward
            x = fwd(q, k, v, key_valid, self.num_heads, p, seed, call)[0]
        return self.output_linear(x)


class _ResidualLayerNorm(torch.autograd.Function):
    """(y, n) = (drop_out(x + drop_in(s)), LayerNorm(y)) over [R, N] float32 in one launch each way
    (csrc/residual_layernorm.hip).  s may be None; gamma None: no LayerNorm, n is None; want_y False (no dropout active, s
    None): y is x itself and None is returned for it.  drop = (p_in, site_in, p_out, site_out, seed, call).  Kept for the
    backward: y, two floats per row and gamma — no mask, no copy of the LayerNorm's input."""

    @staticmethod
    def forward(ctx, x, s, gamma, beta, eps, drop, want_y):
        from ..distributed._device_ops import residual_layernorm_forward

        y, n, stats = residual_layernorm_forward(x, s, gamma, beta, eps, drop, want_y)
        ctx.save_for_backward(y if want_y else x, stats, gamma, beta)
        ctx.eps, ctx.drop = eps, drop
        ctx.set_materialize_grads(False)
        return y, n

    @staticmethod
    def backward(ctx, g_y, g_n):
        from ..distributed._device_ops import residual_layernorm_backward

        y, stats, gamma, beta = ctx.saved_tensors
        need_x, need_s, need_gamma, need_beta = ctx.needs_input_grad[:4]
        if (g_y is None and g_n is None) or not any(ctx.needs_input_grad[:4]):
            return (None,) * 7
        if torch.is_grad_enabled():  # create_graph: the same gradients from differentiable torch operations on the saved y
            if ctx.drop[0] > 0.0 or ctx.drop[2] > 0.0:
                raise RuntimeError("TransformerBlock: double backward through the fused kernel's dropout is not supported")
            grads = {0: g_y}
            if g_n is not None:
                wrt = [(i, t) for i, t in enumerate((y, gamma, beta)) if t.requires_grad]
                n = nn.functional.layer_norm(y, y.shape[-1:], gamma, beta, ctx.eps)
                got = torch.autograd.grad(n, [t for _, t in wrt], g_n, create_graph=True)
                grads.update({i: v for (i, _), v in zip(wrt, got)})
                if g_y is not None and y.requires_grad:
                    grads[0] = g_y + grads[0]
            g = grads.get(0)
            return (g if need_x else None, g if need_s else None, grads.get(1) if need_gamma else None,
                    grads.get(2) if need_beta else None, None, None, None)
        want_params = g_n is not None and (need_gamma or need_beta)
        g_x, g_s, gp = residual_layernorm_backward(
            None if g_y is None else g_y.contiguous(), None if g_n is None else g_n.contiguous(), y, stats, gamma, ctx.drop,
            need_s, want_params)
        return (g_x if need_x else None, g_s, gp[0] if want_params and need_gamma else None,
                gp[1] if want_params and need_beta else None, None, None, None)


class _ReluDropout(torch.autograd.Function):
    """dropout(relu(a)) in one launch each way (csrc/residual_layernorm.hip); the backward reads the result alone."""

    @staticmethod
    def forward(ctx, a, p, site, seed, call):
        from ..distributed._device_ops import relu_dropout_forward

        h = relu_dropout_forward(a, p, site, seed, call)
        ctx.save_for_backward(h)
        ctx.p = p
        return h

    @staticmethod
    def backward(ctx, g_h):
        from ..distributed._device_ops import relu_dropout_backward

        (h,) = ctx.saved_tensors
        if torch.is_grad_enabled():
            if ctx.p > 0.0:
                raise RuntimeError("TransformerBlock: double backward through the fused kernel's dropout is not supported")
            return g_h * (h > 0).to(g_h.dtype), None, None, None, None
        return relu_dropout_backward(g_h.contiguous(), h, ctx.p), None, None, None, None


def _residual_layernorm(x, s, norm, drop, want_y=True):
    """_ResidualLayerNorm where a gradient may be wanted, the forward launch alone elsewhere (nothing is kept)."""
    gamma, beta, eps = (norm.weight, norm.bias, norm.eps) if norm is not None else (None, None, 0.0)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, s, gamma, beta)):
        return _ResidualLayerNorm.apply(x, s, gamma, beta, eps, drop, want_y)
    from ..distributed._device_ops import residual_layernorm_forward

    return residual_layernorm_forward(x, s, gamma, beta, eps, drop, want_y)[:2]


def _fusable_norm(norm: nn.Module, N: int) -> bool:
    return (isinstance(norm, nn.LayerNorm) and tuple(norm.normalized_shape) == (N,) and norm.elementwise_affine
            and norm.bias is not None and norm.weight.is_cuda and norm.weight.dtype == torch.float32
            and norm.weight.data_ptr() % 16 == 0 and norm.bias.data_ptr() % 16 == 0)


class PositionwiseFeedForward(nn.Module):
    """Feed-forward block (examples/bert4rec/models/bert4rec.py:174-214).

    Args:
        dim_model (int): input/output dimensionality
        d_ff (int): hidden dimensionality
        dropout (float): the dropout probability
        device: (Optional[torch.device]).
    """

    def __init__(self, dim_model: int, d_ff: int, dropout: float = 0.1, device: Optional[torch.device] = None) -> None:
        super().__init__()
        self.w_1 = nn.Linear(dim_model, d_ff, device=device)
        self.w_2 = nn.Linear(d_ff, dim_model, device=device)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.w_2(self.dropout(nn.functional.relu(self.w_1(x))))


class SublayerConnection(nn.Module):
    """A residual connection followed by a layer norm (examples/bert4rec/models/bert4rec.py:217-257).

    Args:
        size (int): layerNorm size
        dropout (float): the dropout probability
        device: (Optional[torch.device]).
    """

    def __init__(self, size: int, dropout: float, device: Optional[torch.device] = None) -> None:
        super().__init__()
        self.norm = nn.LayerNorm(size, device=device)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x: torch.Tensor, sublayer: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
        return x + self.dropout(sublayer(self.norm(x)))


class TransformerBlock(nn.Module):
    """Transformer = MultiHead_Attention + Feed_Forward with sublayer connection
    (examples/bert4rec/models/bert4rec.py:260-320).

    Args:
        hidden (int): hidden size of transformer
        attn_heads (int): head sizes of multi-head attention
        feed_forward_hidden (int): feed_forward_hidden, usually 4*hidden_size
        dropout (float): the dropout probability
        device: (Optional[torch.device]).
    """

    def __init__(self, hidden: int, attn_heads: int, feed_forward_hidden: int, dropout: float,
                 device: Optional[torch.device] = None) -> None:
        super().__init__()
        self.attention = MultiHeadedAttention(num_heads=attn_heads, dim_model=hidden, dropout=dropout, device=device)
        self.feed_forward = PositionwiseFeedForward(dim_model=hidden, d_ff=feed_forward_hidden, dropout=dropout, device=device)
        self.input_sublayer = SublayerConnection(size=hidden, dropout=dropout, device=device)
        self.output_sublayer = SublayerConnection(size=hidden, dropout=dropout, device=device)
        self.dropout = nn.Dropout(p=dropout)
        self.kernel_path = True     # False: always the torch expression (tests and tools compare the two)
        self.last_path = None       # "kernel" / "torch": what the last forward took
        # the kernel dropouts' `call`, as in MultiHeadedAttention: high word 0 for a block built on its own, 1 + the layer
        # index inside BERT4Rec; the low word counts the training forwards with active kernel dropout
        self._dropout_salt = 0
        self._dropout_calls = 0

    def _dropout_ps(self) -> Tuple[float, float, float, float]:
        """p of the sites 0 .. 3: input_sublayer.dropout, output_sublayer.dropout, the block's dropout, feed_forward.dropout."""
        drops = (self.input_sublayer.dropout, self.output_sublayer.dropout, self.dropout, self.feed_forward.dropout)
        return tuple(float(d.p) if self.training else 0.0 for d in drops)

    def _kernel_ok(self, x: torch.Tensor, ps, next_norm: Optional[nn.Module]) -> bool:
        if not (self.kernel_path and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.numel() > 0):
            return False
        N, ff = x.shape[-1], self.feed_forward
        if N % 4 or not 4 <= N <= 4096 or x.numel() // N >= 2 ** 31 or (x.is_contiguous() and x.data_ptr() % 16):
            return False
        if not (isinstance(ff.w_1, nn.Linear) and isinstance(ff.w_2, nn.Linear) and ff.w_1.weight.dtype == torch.float32
                and (x.numel() // N * ff.w_1.out_features) % 4 == 0):  # relu_dropout moves 16 bytes at a time
            return False
        if not all(_fusable_norm(m, N) for m in (self.input_sublayer.norm, self.output_sublayer.norm)):
            return False
        if next_norm is not None and not _fusable_norm(next_norm, N):
            return False
        if not all(0.0 <= p < 1.0 for p in ps):
            return False
        return not (max(ps) > 0.0 and torch.cuda.is_current_stream_capturing())  # the call counter is host state

    def forward(self, x: torch.Tensor, mask: torch.BoolTensor) -> torch.Tensor:
        return self._forward_chained(x, mask, None, None)[0]

    def _forward_chained(self, x: torch.Tensor, mask: torch.BoolTensor, n1: Optional[torch.Tensor],
                         next_norm: Optional[nn.Module]) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(the block's output, LayerNorm `next_norm` of it or None).  `n1`: this block's input_sublayer.norm(x) when the
        block before has made it already.  The second result is None whenever this call takes the torch expression."""
        ps = self._dropout_ps()
        if not self._kernel_ok(x, ps, next_norm):
            self.last_path = "torch"
            x = self.input_sublayer(x, lambda _x: self.attention.forward(_x, _x, _x, mask=mask))
            x = self.output_sublayer(x, self.feed_forward)
            return self.dropout(x), None
        self.last_path = "kernel"
        seed = call = 0
        if max(ps) > 0.0:
            seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
            call = (self._dropout_salt << 32) | (self._dropout_calls & 0xFFFFFFFF)
            self._dropout_calls += 1
        shape, N = x.shape, x.shape[-1]
        x = x.contiguous().view(-1, N)
        if n1 is None:  # launch A: n1 = LN1(x); no y is written
            n1 = _residual_layernorm(x, None, self.input_sublayer.norm, (0.0, 0, 0.0, 0, 0, 0), want_y=False)[1]
        n1 = n1.view(shape)
        a = self.attention.forward(n1, n1, n1, mask=mask)
        # launch A: x1 = x + drop(a), n2 = LN2(x1)
        x1, n2 = _residual_layernorm(x, a.contiguous().view(-1, N), self.output_sublayer.norm, (ps[0], 0, 0.0, 0, seed, call))
        # GEMM + launch B: h = drop(relu(w_1(n2)))
        h = self.feed_forward.w_1(n2).contiguous()
        if torch.is_grad_enabled() and h.requires_grad:
            h = _ReluDropout.apply(h, ps[3], 3, seed, call)
        else:
            from ..distributed._device_ops import relu_dropout_forward

            h = relu_dropout_forward(h, ps[3], 3, seed, call)
        # GEMM + launch A: x2 = drop_blk(x1 + drop(w_2(h))), and the next block's LN1 of it
        f = self.feed_forward.w_2(h).contiguous()
        x2, n_next = _residual_layernorm(x1, f, next_norm, (ps[1], 1, ps[2], 2, seed, call))
        return x2.view(shape), None if n_next is None else n_next.view(shape)


class _HistoryKernel(torch.autograd.Function):
    """HistoryArch in one launch each way (csrc/history_arch.hip) behind either TBE class of the EmbeddingCollection.  `anchor`
    is what the table's lookup hangs its backward on: the fused class's placeholder (the optimizer runs inside the
    backward, no gradient comes back) or the dense class's `.weights` (its gradient is returned).  Kept for the backward:
    the ids, the offsets and two floats per sample — no embeddings, no LayerNorm input, no mask."""

    @staticmethod
    def forward(ctx, anchor, positional, gamma, beta, tbe, ids, offsets, B, prepare, eps, drop):
        from ..distributed._device_ops import history_forward

        y, stats = history_forward(tbe.sequence_table(), ids, offsets, positional, gamma, beta, eps, drop, tbe._errors_ptr())
        ctx.save_for_backward(ids, offsets, stats, positional, gamma)
        ctx.tbe, ctx.B, ctx.drop = tbe, B, drop
        ctx.iter = getattr(tbe, "iter", None)  # fused class: the updates its table has had
        ctx.prepared = tbe._prepare_backward(ids, offsets, B) if prepare else None
        return y

    @staticmethod
    def backward(ctx, g_y):
        from fbgemm_gpu.split_table_batched_embeddings_ops import _OPT_DENSE_GRAD, OptimizerArgs

        from ..distributed._device_ops import history_backward

        if torch.is_grad_enabled():
            raise RuntimeError("HistoryArch: double backward through the fused kernel is not supported "
                               "(kernel_path = False gives the torch expression)")
        ids, offsets, stats, positional, gamma = ctx.saved_tensors
        tbe, need = ctx.tbe, ctx.needs_input_grad
        if getattr(tbe, "iter", None) != ctx.iter:
            raise RuntimeError("HistoryArch: the item table has been updated since this forward (another backward of the fused "
                               "table ran in between), and the kernel's backward recomputes from the live rows: run one "
                               "forward per backward, or set kernel_path = False")
        want = (1 if need[1] else 0) | (2 if need[2] else 0) | (4 if need[3] else 0)
        # before the table's update: it reads the rows the update rewrites (same stream)
        grad_emb, gp = history_backward(g_y.contiguous(), tbe.sequence_table(), ids, offsets, positional, gamma, stats,
                                        ctx.drop, want)
        grad_w = None
        if hasattr(tbe, "placeholder_autograd_tensor"):  # as _FusedLookup.backward
            tbe.iter += 1
            tbe._backward_impl(grad_emb, ids, offsets, None, ctx.B, tbe._optimizer_struct(), prepared=ctx.prepared,
                               ext=tbe._optimizer_ext())
        elif need[0]:  # as _DenseLookup.backward
            grad_w = torch.zeros_like(tbe.weights)
            tbe._backward_impl(grad_emb, ids, offsets, None, ctx.B, OptimizerArgs(_OPT_DENSE_GRAD, 0.0, 0.0, 0.0, 0.0, 0.0, 1),
                               state0_override=tbe._dense_grad_ptrs(grad_w), state0_aligned=grad_w.data_ptr() % 16 == 0)
        ctx.prepared = None
        return (grad_w, gp[0] if need[1] else None, gp[1] if need[2] else None, gp[2] if need[3] else None,
                None, None, None, None, None, None, None)


class HistoryArch(torch.nn.Module):
    """The input embedding layer of BERT4Rec (examples/bert4rec/models/bert4rec.py:323-409): an item embedding table of
    vocab_size vectors through EmbeddingCollection, padded / truncated to history_len rows by jagged_2d_to_dense, plus a
    positional table, LayerNorm over [history_len, emb_dim] and dropout.

    Args:
        vocab_size (int): the item count including mask and padding
        history_len (int): the max length
        emb_dim (int): embedding dimension
        dropout (float): the dropout probability
        device: (Optional[torch.device]).
        fused_params (Optional[dict]): keyword-only, handed to EmbeddingCollection (fused optimizer in the backward).
    """

    def __init__(self, vocab_size: int, history_len: int, emb_dim: int, dropout: float = 0.1,
                 device: Optional[torch.device] = None, *, fused_params: Optional[dict] = None) -> None:
        super().__init__()
        self.emb_dim = emb_dim
        self.history_len = history_len
        self.positional = nn.Parameter(torch.randn(history_len, emb_dim, device=device))
        self.layernorm = torch.nn.LayerNorm([history_len, emb_dim], device=device)
        self.dropout = torch.nn.Dropout(p=dropout)
        item_embedding_config = EmbeddingConfig(
            name="item_embedding", embedding_dim=emb_dim, num_embeddings=vocab_size, feature_names=["item"],
            weight_init_max=1.0, weight_init_min=-1.0)
        self.ec = EmbeddingCollection(tables=[item_embedding_config], device=device, fused_params=fused_params)
        self.kernel_path = True     # False: always the torch expression (tests and tools compare the two)
        self.last_path = None       # "kernel" / "torch": what the last forward took
        # the kernel dropout's `call`, as in TransformerBlock: the high word stays 0 (the blocks of a BERT4Rec use 1 + layer)
        self._dropout_salt = 0
        self._dropout_calls = 0

    def _kernel_inputs(self, features: KeyedJaggedTensor, p: float):
        """(tbe, table) when this call may take the kernel, else None."""
        tbe, ln, pos = self.ec._tbe, self.layernorm, self.positional
        if not (self.kernel_path and list(features.keys()) == list(self.ec._feature_names) and len(self.ec._feature_names) == 1
                and pos.is_cuda and pos.dtype == torch.float32 and pos.is_contiguous() and pos.data_ptr() % 16 == 0
                and tuple(pos.shape) == (self.history_len, self.emb_dim) and 0.0 <= p < 1.0):
            return None
        if not (isinstance(ln, nn.LayerNorm) and ln.elementwise_affine and ln.bias is not None
                and tuple(ln.normalized_shape) == tuple(pos.shape)
                and all(t.device == pos.device and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
                        for t in (ln.weight, ln.bias))):
            return None
        if tbe.current_device != pos.device or (p > 0.0 and torch.cuda.is_current_stream_capturing()):
            return None  # the call counter is host state
        from ..distributed._device_ops import history_supported

        if not history_supported(self.history_len, self.emb_dim):
            return None
        table = tbe.sequence_table()
        return None if table is None else (tbe, table)

    def _forward_torch(self, id_list_features: KeyedJaggedTensor) -> torch.Tensor:
        jt_dict = self.ec(id_list_features)
        padded_embeddings = [
            torch.ops.fbgemm.jagged_2d_to_dense(
                values=jt_dict[e].values(), offsets=jt_dict[e].offsets(), max_sequence_length=self.history_len,
            ).view(-1, self.history_len, self.emb_dim)
            for e in id_list_features.keys()
        ]
        item_output = padded_embeddings[0] if len(padded_embeddings) == 1 else torch.cat(padded_embeddings, dim=1)
        x = item_output + self.positional  # broadcast over the batch (the reference repeats it)
        return self.dropout(self.layernorm(x))

    def forward(self, id_list_features: KeyedJaggedTensor) -> torch.Tensor:
        p = float(self.dropout.p) if self.training else 0.0
        found = self._kernel_inputs(id_list_features, p)
        if found is None:
            self.last_path = "torch"
            return self._forward_torch(id_list_features)
        self.last_path = "kernel"
        tbe, table = found
        fused = hasattr(tbe, "placeholder_autograd_tensor")
        # what the lookup starts with on the plain path: the input checks and, for the fused class, whether the backward's
        # sort goes on the side stream
        if fused:
            ids, offsets, _, B, prepare = tbe._begin_lookup(id_list_features.values(), id_list_features.offsets(), None,
                                                            torch.is_grad_enabled())
        else:
            ids, offsets, _, B = tbe._check_inputs(id_list_features.values(), id_list_features.offsets(), None)
            prepare = False
        seed = call = 0
        if p > 0.0:
            seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
            call = (self._dropout_salt << 32) | (self._dropout_calls & 0xFFFFFFFF)
            self._dropout_calls += 1
        drop, ln = (p, 4, seed, call), self.layernorm
        anchor = tbe.placeholder_autograd_tensor if fused else tbe.weights
        if torch.is_grad_enabled() and any(t.requires_grad for t in (anchor, self.positional, ln.weight, ln.bias)):
            y = _HistoryKernel.apply(anchor, self.positional, ln.weight, ln.bias, tbe, ids, offsets, B, prepare, ln.eps, drop)
        else:
            from ..distributed._device_ops import history_forward

            y = history_forward(table, ids, offsets, self.positional, ln.weight, ln.bias, ln.eps, drop, tbe._errors_ptr())[0]
        if fused:
            tbe._enforce_bounds_check_mode()
        return y


class BERT4Rec(nn.Module):
    """The overall arch of the BERT4Rec paper (https://arxiv.org/abs/1904.06690;
    examples/bert4rec/models/bert4rec.py:412-500).

    Args:
        vocab_size (int): the item count including mask and padding
        max_len (int): the max length
        emb_dim (int): embedding dimension
        nhead (int): number of the transformation headers
        num_layers (int): number of the transformation layers
        dropout (float): the dropout probability
        device: (Optional[torch.device]).
        fused_params (Optional[dict]): keyword-only, handed to the item table's EmbeddingCollection.

    Example::

        input_kjt = KeyedJaggedTensor.from_lengths_sync(
            keys=["item"], values=torch.tensor([2, 4, 3, 4, 5]), lengths=torch.tensor([2, 3])).to(device)
        bert4rec = BERT4Rec(vocab_size=6, max_len=3, emb_dim=4, nhead=4, num_layers=4, device=device)
        logits = bert4rec(input_kjt)
    """

    def __init__(self, vocab_size: int, max_len: int, emb_dim: int, nhead: int, num_layers: int, dropout: float = 0.1,
                 device: Optional[torch.device] = None, *, fused_params: Optional[dict] = None) -> None:
        super().__init__()
        self.vocab_size = vocab_size
        self.emb_dim = emb_dim
        self.max_len = max_len
        self.history = HistoryArch(vocab_size, max_len, emb_dim, dropout=dropout, device=device, fused_params=fused_params)
        self.transformer_blocks = nn.ModuleList(
            [TransformerBlock(emb_dim, nhead, emb_dim * 4, dropout, device=device) for _ in range(num_layers)])
        for i, block in enumerate(self.transformer_blocks):
            block.attention._dropout_salt = block._dropout_salt = 1 + i
        # as in the reference: a linear output layer, not the paper's product with the embedding table
        self.out = nn.Linear(self.emb_dim, self.vocab_size, device=device)

    def forward(self, input: KeyedJaggedTensor) -> torch.Tensor:
        dense_tensor = input["item"].to_padded_dense(desired_length=self.max_len, pad_from_beginning=False)
        B, L = dense_tensor.shape
        # [B, 1, L, L] with stride 0 along the queries (the reference materialises it with .repeat)
        mask = (dense_tensor > 0)[:, None, None, :].expand(B, 1, L, L)
        x = self.history(input)
        # the last launch of block i also makes block i + 1's first LayerNorm (None when either takes the torch expression)
        blocks, n1 = list(self.transformer_blocks), None
        for i, transformer in enumerate(blocks):
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            next_norm = None
            if nxt is not None and nxt.kernel_path and _fusable_norm(nxt.input_sublayer.norm, x.shape[-1]):
                next_norm = nxt.input_sublayer.norm
            x, n1 = transformer._forward_chained(x, mask, n1, next_norm)
        return self.out(x)
