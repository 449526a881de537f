"""BERT4Rec with the reference's constructors, assertions, module tree and registration order
(examples/bert4rec/models/bert4rec.py): `history.positional`, `history.layernorm.*`,
`transformer_blocks.<i>.attention.linear_layers.<k>.*`, `...output_linear.*`, `out.*` load from a reference state_dict; the
item table keeps this package's EmbeddingCollection naming, as under DLRM and SimpleDeepFMNN.

What runs differently:
  * MultiHeadedAttention, on a HIP device with float32 inputs, a supported (L, d_k) and no mask or a key-padding mask:
    the three projections stay torch's nn.Linear, their outputs go to one fused kernel each way (csrc/attention.hip) where
    they are, and its [B, L, H * d_k] result goes straight into output_linear.  No [B, H, L, L] tensor exists; autograd keeps
    the three projections and one float per row.  Everything else silently takes `_attention_torch`, the reference's
    expression op for op: CPU tensors, other dtypes, an unsupported (L, d_k), a materialised or per-query mask, p >= 1,
    active dropout under stream capture (the per-call counter is host state and would freeze in a graph).  Double backward
    (create_graph=True) of a kernel-path forward recomputes the gradients from differentiable torch operations when the
    kernel's dropout was inactive, and raises RuntimeError when it was active: the kernel's mask exists in no tensor.
  * The kernel's dropout mask is its own counter-based draw (include/tbe_hip.h), not torch's generator: seed =
    torch.initial_seed(), call = a per-module counter that advances once per training forward, below a high word that is
    0 for a stand-alone module and 1 + the layer index inside BERT4Rec.
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
        if torch.is_grad_enabled():  # create_graph: the same gradients from differentiable torch operations
            if p != 0.0:
                raise RuntimeError("MultiHeadedAttention: double backward through the fused kernel's dropout is not supported")
            mask = None if ctx.key_valid is None else ctx.key_valid[:, None, None, :]
            wanted = [t for t, w in zip((q, k, v), need) if w]
            grads = iter(torch.autograd.grad(_attention_torch(q, k, v, mask, H, None), wanted, G, create_graph=True))
            return (*[next(grads) if w else None for w in need], None, None, None, None, None)
        dq, dk, dv = attention_backward(G.contiguous(), q, k, v, ctx.key_valid, lse, H, p, seed, call, need)
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
        # The high word of the kernel dropout's `call`: 0 for a module built on its own, 1 + the layer index inside BERT4Rec,
        # so that the layers of a model do not drop the same (b, h, i, j).  No process state enters: two stand-alone modules
        # under the same seed draw the same masks call for call.
        self._dropout_salt = 0
        self._dropout_calls = 0     # training forwards with active kernel dropout so far

    def _kernel_inputs(self, q, k, v, mask, p):
        """(True, key_valid) when this call may take the kernel."""
        if not (self.kernel_path and q.is_cuda and q.dtype == torch.float32 and q.dim() == 3 and k.shape == q.shape
                and v.shape == q.shape and k.dtype == q.dtype and v.dtype == q.dtype and q.shape[0] > 0 and 0.0 <= p < 1.0):
            return False, None
        from ..distributed._device_ops import attention_supported

        if not attention_supported(q.shape[1], self.d_k):
            return False, None
        if p > 0.0 and torch.cuda.is_current_stream_capturing():
            return False, None
        ok, key_valid = key_padding_mask(mask, q.shape[0], q.shape[1])
        if ok and key_valid is not None and key_valid.device != q.device:
            return False, None
        return ok, key_valid

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        # 1) the linear projections dim_model => num_heads x d_k, left as [B, L, H * d_k]
        q, k, v = [layer(x) for layer, x in zip(self.linear_layers, (query, key, value))]
        p = float(self.dropout.p) if self.training else 0.0
        ok, key_valid = self._kernel_inputs(q, k, v, mask, p)
        if not ok:
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
            x = _FusedAttention.apply(q, k, v, key_valid, self.num_heads, p, seed, call)
        else:
            from ..distributed._device_ops import attention_forward

            x = attention_forward(q, k, v, key_valid, self.num_heads, p, seed, call)[0]
        return self.output_linear(x)


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

    def forward(self, x: torch.Tensor, mask: torch.BoolTensor) -> torch.Tensor:
        x = self.input_sublayer(x, lambda _x: self.attention.forward(_x, _x, _x, mask=mask))
        x = self.output_sublayer(x, self.feed_forward)
        return self.dropout(x)


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

    def forward(self, id_list_features: KeyedJaggedTensor) -> torch.Tensor:
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
            block.attention._dropout_salt = 1 + i
        # as in the reference: a linear output layer, not the paper's product with the embedding table
        self.out = nn.Linear(self.emb_dim, self.vocab_size, device=device)

    def forward(self, input: KeyedJaggedTensor) -> torch.Tensor:
        dense_tensor = input["item"].to_padded_dense(desired_length=self.max_len, pad_from_beginning=False)
        B, L = dense_tensor.shape
        # [B, 1, L, L] with stride 0 along the queries (the reference materialises it with .repeat)
        mask = (dense_tensor > 0)[:, None, None, :].expand(B, 1, L, L)
        x = self.history(input)
        for transformer in self.transformer_blocks:
            x = transformer.forward(x, mask)
        return self.out(x)
