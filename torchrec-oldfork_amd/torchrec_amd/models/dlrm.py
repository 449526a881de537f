"""DLRM dense side + model wrapper (torchrec/models/dlrm.py:36-406,
examples/dlrm/modules/dlrm_train.py).  Module and parameter names follow the reference so
state_dict keys are interchangeable (`dense_arch.model._mlp.0._linear.weight`,
`over_arch.model.1.bias`, ...).  The dense MLPs and the dot interaction are the only MFMA
users of the path (rocBLAS/hipBLASLt fp32 GEMMs)."""
import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist  # called as dist.all_reduce(...): distributed/_rehearsal.py replaces the module's functions
from fbgemm_gpu import _lib
from fbgemm_gpu._lib import check, ptr, stream_ptr
from torch import nn

from ..modules.mlp import MLP, LinearOut, _EagerFinish, relu_linear1_head
from ..profiling import label
from ..sparse.jagged_tensor import KeyedJaggedTensor, KeyedTensor


class SparseArch(nn.Module):
    """models/dlrm.py:36-113: pooled embeddings -> [B, F, D]."""

    def __init__(self, embedding_bag_collection: nn.Module) -> None:
        super().__init__()
        self.embedding_bag_collection = embedding_bag_collection
        cfgs = embedding_bag_collection.embedding_bag_configs
        assert cfgs, "Embedding bag collection cannot be empty!"
        self.D: int = cfgs[0].embedding_dim
        self._sparse_feature_names: List[str] = [n for c in cfgs for n in c.feature_names]
        self.F: int = len(self._sparse_feature_names)

    def start(self, features: KeyedJaggedTensor):
        """Issues the lookup (and, when sharded, the pooled all-to-all) and returns without waiting."""
        return self.embedding_bag_collection(features)

    def finish(self, pending) -> torch.Tensor:
        sparse_features = pending.wait() if hasattr(pending, "wait") else pending
        B = sparse_features.values().shape[0]
        if sparse_features.keys() == self._sparse_feature_names:
            return sparse_features.values().reshape(B, self.F, self.D)
        sparse: Dict[str, torch.Tensor] = sparse_features.to_dict()
        return torch.cat([sparse[n] for n in self._sparse_feature_names], dim=1).reshape(B, self.F, self.D)

    def forward(self, features: KeyedJaggedTensor) -> torch.Tensor:
        return self.finish(self.start(features))

    @property
    def sparse_feature_names(self) -> List[str]:
        return self._sparse_feature_names


# flat mode: capture the head segment's weight-gradient GEMMs into a second backward graph (0: one graph as before)
_DEFER_WGRAD = os.environ.get("TORCHREC_AMD_DEFER_WGRAD", "1") != "0"
# Two half-batches per step when the pooled embeddings cross links (DLRMTrain.capture_hip_graphs(half_batches=)):
# "auto" = on for per-rank batches of at least this many samples — N = 2 at the global batch of 65 536, where the exchange
# takes ~1.5 ms per pass over the one link pair and only half of the forward one stays exposed.  Measured with emulated
# link times: 7.01 -> 6.30 ms per step at 32 768 per rank; a tie at 16 384 (3.40 / 3.38) and a loss at 8192
# (1.86 -> 2.01): two half-size passes cost 0.2 - 0.3 ms more kernel time (GEMMs at half M, kernels at their latency floor).
# "1" / "0" force it.
# Flat-gradient graph mode under a pipeline that prefetches the next lookup: the weight / bias gradients of the head's FIRST
# this-many Linear layers are captured into a third graph that the explicit step replays AFTER it has started the NEXT step's
# lookup + pooled all-to-all (the rest stays behind this step's gradient all-to-all).  The forward all-to-all then has the
# same kind of cover the gradient all-to-all always had, instead of the bottom MLP's forward only.  0 = off.
# "auto" (default): 2 layers at per-rank batches of 16 384 .. 32 767 (N = 4 at the global batch of 65 536), none otherwise.
# Why not everywhere: the late layers' gradients are all-reduced at the very end of the step, in front of the dense
# optimizer and the next bottom MLP, and that all-reduce takes the same time at every batch size while the GEMMs that are
# supposed to hide the all-to-all shrink with it.  With emulated link AND all-reduce times 0 / 2 / 3 late
# layers measure 2.08 / 2.32 / 2.33 ms at 8192 per rank, 3.71 / 3.50 / 3.60 at 16 384; without the all-reduce time
# 1.87 / 1.71 / 1.72 and 3.38 / 3.18 / 3.11.  A number forces it.
_WGRAD_LATE_LAYERS = os.environ.get("TORCHREC_AMD_WGRAD_LATE_LAYERS", "auto")


def _late_layers(batch: int, halves: bool) -> int:
    if _WGRAD_LATE_LAYERS != "auto":
        return int(_WGRAD_LATE_LAYERS)
    return 2 if (not halves and 16384 <= batch < 32768) else 0


# Where the split-off graph of those layers runs: "late" (default) = behind the next step's prefetched lookup, as above;
# "early" = FIRST in the backward window, and every piece of the flat gradient is all-reduced as soon as it exists, the
# largest first (replicated tables, the split-off head layers, the other head layers; the bottom MLP's small slice last).
# Opt-in: bit-identical, four collectives per step instead of two, and with emulated link + all-reduce times within noise of
# no split at all (2.02 vs 2.05 ms at 8192 per rank; 3.71 vs 3.49 for "late" at 16 384).
_WGRAD_SPLIT_MODE = os.environ.get("TORCHREC_AMD_WGRAD_SPLIT_MODE", "late")


# whole-batch explicit step with an exchange: unpack / pack captured into the head segment's graphs instead of two eager
# launches (persistent receive / send buffers).  Opt-in: bit-identical, the two launch gaps (8 + 7 us) do disappear, and the
# step gets no faster — 1.732 vs 1.695 ms at 8192 per rank, 2.849 vs 2.854 at 16 384 (the host, freed earlier, starts the
# next input dist earlier, and its kernels then share the chip with the head's forward GEMMs: + 50 us of GEMM time)
_GRAPH_EXCHANGE = os.environ.get("TORCHREC_AMD_GRAPH_EXCHANGE", "0") == "1"
_HALF_BATCHES = os.environ.get("TORCHREC_AMD_HALF_BATCHES", "auto")
_HALF_BATCH_MIN = int(os.environ.get("TORCHREC_AMD_HALF_BATCH_MIN", "32768"))


class DenseArch(nn.Module):
    def __init__(self, in_features: int, layer_sizes: List[int], device: Optional[torch.device] = None) -> None:
        super().__init__()
        self.model = MLP(in_features, layer_sizes, bias=True, activation="relu", device=device)

    def forward(self, features: torch.Tensor) -> torch.Tensor:
        return self.model(features)


def _interaction_row(F: int, D: int, pad_rows: bool = False) -> Tuple[int, int]:
    """(width, stride) of the interaction's result rows: D + F (F + 1) / 2 floats; pad_rows rounds the pairs up to 4 floats."""
    pairs = (F + 1) * F // 2
    return D + pairs, (D + (pairs + 3) // 4 * 4) if pad_rows else D + pairs


def _readable_grad_out(grad_out: torch.Tensor, B: int, width: int) -> torch.Tensor:
    """The gradient of the interaction's result as the backward kernels read it: float32 rows of unit stride."""
    if grad_out.shape != (B, width):
        raise RuntimeError(f"dot interaction backward: grad_out {tuple(grad_out.shape)} has the wrong shape")
    if grad_out.dtype != torch.float32 or grad_out.stride(1) != 1 or grad_out.stride(0) < width:
        return grad_out.float().contiguous()
    return grad_out  # padded rows (stride >= width) are read in place


class _FusedDotInteraction(torch.autograd.Function):
    """One HIP kernel each way (csrc/dlrm_interaction.hip, fp32 MFMA) instead of the reference's
    cat + bmm + index + cat chain and its autograd backward (models/dlrm.py:206-219).

    `pad_rows`: the result [B, D + P] is a view of a [B, S] buffer with S = D + P rounded up to a multiple of 4 (479 ->
    480 floats): rows start 16-B aligned, so the kernel stores 16 B per lane and the GEMMs of the next layer read aligned
    rows (lda = S, K = D + P; tools/gemm_probe.py).  Values and shapes are those of the dense result."""

    @staticmethod
    def forward(ctx, dense, sparse, pad_rows=False, grad_sinks=None):
        dense, sparse = dense.contiguous(), sparse.contiguous()
        B, F, D = sparse.shape
        if dense.shape != (B, D) or sparse.device != dense.device:
            raise RuntimeError(f"dot interaction: dense {tuple(dense.shape)} does not match sparse {tuple(sparse.shape)} "
                               "(same batch, same embedding dim, same device required)")
        width, stride = _interaction_row(F, D, pad_rows)
        buf = torch.empty((B, stride), dtype=torch.float32, device=dense.device)
        with torch.cuda.device(dense.device):
            check(_lib.load().tbe_dlrm_interaction_forward_f32(ptr(dense), ptr(sparse), B, F, D, ptr(buf), stride,
                                                               stream_ptr(dense.device)),
                  "tbe_dlrm_interaction_forward_f32")
        ctx.save_for_backward(dense, sparse)
        # (d dense, d sparse) buffers of the caller instead of fresh allocations: a captured backward then writes e.g. its
        # half of a whole-batch gradient buffer in place (DLRMTrain.capture_hip_graphs(half_batches=True))
        ctx.grad_sinks = grad_sinks
        return buf if stride == width else buf[:, :width]

    @staticmethod
    def backward(ctx, grad_out):
        dense, sparse = ctx.saved_tensors
        B, F, D = sparse.shape
        grad_out = _readable_grad_out(grad_out, B, _interaction_row(F, D)[0])
        if ctx.grad_sinks is not None:
            gd, gs = ctx.grad_sinks
            if (gd.shape != dense.shape or gs.shape != sparse.shape or not gd.is_contiguous() or not gs.is_contiguous()
                    or gd.dtype != torch.float32 or gs.dtype != torch.float32 or gd.device != dense.device):
                raise RuntimeError("dot interaction backward: gradient sinks do not match the inputs")
        else:
            gd, gs = torch.empty_like(dense), torch.empty_like(sparse)
        with torch.cuda.device(dense.device):
            check(_lib.load().tbe_dlrm_interaction_backward_f32(ptr(dense), ptr(sparse), ptr(grad_out), grad_out.stride(0),
                                                                B, F, D, ptr(gd), ptr(gs), stream_ptr(dense.device)),
                  "tbe_dlrm_interaction_backward_f32")
        return gd, gs, None, None


class _FusedGatherInteraction(torch.autograd.Function):
    """_FusedDotInteraction with the pooling-factor-1 lookup folded in (csrc/dlrm_interaction.hip gather kernels): the
    interaction reads the table rows itself, the pooled [B, F, D] buffer is neither written nor read.  `lookup` is the
    collection's DeferredLookup; backward hands the rows' gradient to its fused backward and returns d(dense).
    `placeholder` (the embedding module's zero-size leaf) keeps this node in the graph when `dense` needs no gradient.
    `single_row_sgd`: where the lookup's module allows it (exact SGD on fp32 tables, sort prepared: DeferredLookup
    .begin_single_row_sgd) the backward kernel writes the updated row of every contribution that alone touches its row
    straight into the table, and the fused backward leaves those contributions out."""

    @staticmethod
    def forward(ctx, dense, placeholder, lookup, pad_rows=False, single_row_sgd=False):
        dense = dense.contiguous()
        B, F, D = lookup.B, lookup.F, lookup.D
        if dense.shape != (B, D) or dense.dtype != torch.float32 or dense.device != lookup.module.current_device:
            raise RuntimeError(f"dot interaction: dense {tuple(dense.shape)} {dense.dtype} on {dense.device} does not match "
                               f"the lookup (batch {B}, dim {D}, float32 on {lookup.module.current_device})")
        width, stride = _interaction_row(F, D, pad_rows)
        buf = torch.empty((B, stride), dtype=torch.float32, device=dense.device)
        with torch.cuda.device(dense.device):
            check(_lib.load().tbe_dlrm_interaction_gather_forward_f32(
                ptr(dense), ptr(lookup.feat_weights), ptr(lookup.feat_rows), ptr(lookup.feat_window),
                ptr(lookup.rec.indices), B, F, D, ptr(buf), stride, lookup.module._errors_ptr(), stream_ptr(dense.device)),
                "tbe_dlrm_interaction_gather_forward_f32")
        ctx.save_for_backward(dense)
        ctx.lookup = lookup
        ctx.single_row_sgd = single_row_sgd
        return buf if stride == width else buf[:, :width]

    @staticmethod
    def backward(ctx, grad_out):
        (dense,) = ctx.saved_tensors
        lookup, ctx.lookup = ctx.lookup, None
        B, F, D = lookup.B, lookup.F, lookup.D
        grad_out = _readable_grad_out(grad_out, B, _interaction_row(F, D)[0])
        gd = torch.empty_like(dense)
        gs = torch.empty((B, F * D), dtype=torch.float32, device=dense.device)
        with torch.cuda.device(dense.device):
            # (flags, optimizer struct), the stream waiting for the sort behind the flags; None = the plain pair of calls
            opened = lookup.begin_single_row_sgd() if ctx.single_row_sgd else None
            # the ids were counted by the forward: no counter here (include/tbe_hip.h)
            if opened is not None:
                check(_lib.load().tbe_dlrm_interaction_gather_backward_sgd_f32(
                    ptr(dense), ptr(lookup.feat_weights), ptr(lookup.feat_rows), ptr(lookup.feat_window),
                    ptr(lookup.rec.indices), ptr(grad_out), grad_out.stride(0), B, F, D, ptr(gd), ptr(gs), None,
                    ptr(opened[0]), opened[1].learning_rate, stream_ptr(dense.device)),
                    "tbe_dlrm_interaction_gather_backward_sgd_f32")
            else:
                check(_lib.load().tbe_dlrm_interaction_gather_backward_f32(
                    ptr(dense), ptr(lookup.feat_weights), ptr(lookup.feat_rows), ptr(lookup.feat_window),
                    ptr(lookup.rec.indices), ptr(grad_out), grad_out.stride(0), B, F, D, ptr(gd), ptr(gs), None,
                    stream_ptr(dense.device)),
                    "tbe_dlrm_interaction_gather_backward_f32")
        lookup.backward(gs, opened)
        return gd, None, None, None, None


def _fused_interaction_ok(dense: torch.Tensor, sparse: torch.Tensor) -> bool:
    F, D = sparse.shape[1], sparse.shape[2]
    return (dense.is_cuda and dense.dtype == torch.float32 and sparse.dtype == torch.float32
            and 1 <= F <= 27 and D in (16, 32, 64, 128))


class InteractionArch(nn.Module):
    """models/dlrm.py:193-219: [dense | upper-triangle of (dense,sparse)x(dense,sparse)^T]."""

    def __init__(self, num_sparse_features: int) -> None:
        super().__init__()
        self.F = num_sparse_features
        self.fused = True
        # 16-B aligned output rows (a strided [B, D + P] view of a [B, 480] buffer at F = 26, D = 128); the first
        # over-arch layer keeps the alignment for its input gradient (modules/mlp.py).  Off by default: measured on
        # MI355X it buys nothing — the recorded GEMM choices run the 479-wide layer as fast at lda = 479 as at 480
        # (0.481 / 0.464 / 0.439 ms vs 0.479 / 0.464 / 0.445 ms) and the interaction kernels are not store-bound.
        self.pad_rows = os.environ.get("TORCHREC_AMD_PAD_INTERACTION", "0") == "1"
        self.grad_sinks = None  # (d dense, d sparse) buffers the fused backward writes into; read at forward time
        self.register_buffer("triu_indices", torch.triu_indices(self.F + 1, self.F + 1, offset=1), persistent=False)

    def forward(self, dense_features: torch.Tensor, sparse_features: torch.Tensor) -> torch.Tensor:
        if self.F <= 0:
            return dense_features
        if self.fused and _fused_interaction_ok(dense_features, sparse_features):
            return _FusedDotInteraction.apply(dense_features, sparse_features, self.pad_rows, self.grad_sinks)
        # generic shapes: the reference's formulation on torch ops
        combined = torch.cat((dense_features.unsqueeze(1), sparse_features), dim=1)
        interactions = torch.bmm(combined, combined.transpose(1, 2))
        flat = interactions[:, self.triu_indices[0], self.triu_indices[1]]
        return torch.cat((dense_features, flat), dim=1)


class OverArch(nn.Module):
    def __init__(self, in_features: int, layer_sizes: List[int], device: Optional[torch.device] = None) -> None:
        super().__init__()
        if len(layer_sizes) <= 1:
            raise ValueError("OverArch must have multiple layers.")
        self.model = nn.Sequential(
            MLP(in_features, layer_sizes[:-1], bias=True, activation="relu", device=device),
            LinearOut(layer_sizes[-2], layer_sizes[-1], bias=True, device=device))
        # The last hidden layer and a one-output last layer run as one autograd node whose backward is one pass over the
        # hidden activation (modules/mlp.py relu_linear1_head).  False = the two modules' own nodes (tests).  While it is
        # on, forward() calls the Perceptrons and the last layer one by one — also when relu_linear1_head declines — so
        # forward hooks on `self.model`, on its MLP (and its nn.Sequential) do not fire, and where the node applies neither do
        # those of the last Perceptron and the LinearOut; same results.  Whoever hooks these modules sets it to False.
        self.fused_head = True

    def forward(self, features: torch.Tensor) -> torch.Tensor:
        if self.fused_head:
            layers, last = self.model[0]._mlp, self.model[1]
            for i in range(len(layers) - 1):
                features = layers[i](features)
            out = relu_linear1_head(layers[-1], last, features)
            return out if out is not None else last(layers[-1](features))
        return self.model(features)


class DLRM(nn.Module):
    def __init__(self, embedding_bag_collection: nn.Module, dense_in_features: int,
                 dense_arch_layer_sizes: List[int], over_arch_layer_sizes: List[int],
                 dense_device: Optional[torch.device] = None) -> None:
        super().__init__()
        cfgs = embedding_bag_collection.embedding_bag_configs
        assert len(cfgs) > 0, "At least one embedding bag is required"
        D = cfgs[0].embedding_dim
        assert all(c.embedding_dim == D for c in cfgs), "All EmbeddingBagConfigs must have the same dimension"
        if dense_arch_layer_sizes[-1] != D:
            raise ValueError(f"embedding_bag_collection dimension ({D}) and final dense arch layer size "
                             f"({dense_arch_layer_sizes[-1]}) must match.")
        self.sparse_arch = SparseArch(embedding_bag_collection)
        F = self.sparse_arch.F
        self.dense_arch = DenseArch(dense_in_features, dense_arch_layer_sizes, device=dense_device)
        self.inter_arch = InteractionArch(F)
        over_in = D + (F + 1) * F // 2
        self.over_arch = OverArch(over_in, over_arch_layer_sizes, device=dense_device)
        if dense_device is not None:
            self.inter_arch.to(dense_device)
        # At a pooling factor of 1 the lookup is a copy of table rows into a buffer the interaction reads straight back:
        # the interaction then gathers the rows itself (_FusedGatherInteraction) whenever the collection can hand out a
        # DeferredLookup (one rank, no exchange: embeddingbag.py deferred_lookup_supported).  False = always materialise.
        self.fused_lookup = True
        self.fused_lookup_steps = 0  # forwards that took the gather path (tests)
        # On the gather path with exact SGD the interaction backward also writes the updated row of every contribution
        # that alone touches its row (_FusedGatherInteraction single_row_sgd).  False = the plain pair of calls (tests).
        self.fused_single_row_update = True
        # On the gather path (one rank, eager) the dense stacks' bias gradients and the one-output layer's weight gradient
        # are finished by ONE launch at the end of backward instead of one per layer (modules/mlp.py _EagerFinish): their
        # `.grad` is set when backward() returns, not by the engine's accumulation.  False = one launch per layer; a
        # DistributedDataParallel wrapper, whose reducer waits for the engine, turns it off (model_parallel.py).  Set it to
        # False before torch.autograd.grad(..., these parameters): with it on that call gets None for them and their
        # `.grad` is set as a side effect.  The pending list is class state (one backward at a time, any thread) keyed by
        # the engine's graph-task id (torch._C._current_graph_task_id, a private name).
        self.deferred_dense_finish = True

    def _deferred_lookup(self, dense_features: torch.Tensor, sparse_features: KeyedJaggedTensor):
        """The collection's DeferredLookup for this batch, or None (nothing consumed) when the gather path cannot serve it."""
        sa = self.sparse_arch
        ebc = sa.embedding_bag_collection
        if not (self.fused_lookup and self.inter_arch.fused and 1 <= sa.F <= 27 and sa.D in (64, 128)
                and dense_features.is_cuda and dense_features.dtype == torch.float32
                and hasattr(ebc, "deferred_lookup_supported")
                and list(getattr(ebc, "_feature_names", ())) == list(sa.sparse_feature_names)):
            return None
        piped = getattr(ebc, "_pipelined", None)  # a train pipeline's forward on this collection (queued input dist)
        if piped is not None:
            return piped.compute_deferred(sparse_features)
        if not ebc.deferred_lookup_supported(sparse_features):
            return None
        return ebc.compute_deferred(ebc.input_dist(sparse_features).wait())

    def forward(self, dense_features: torch.Tensor, sparse_features: KeyedJaggedTensor) -> torch.Tensor:
        lookup = self._deferred_lookup(dense_features, sparse_features)
        if lookup is not None:
            with _EagerFinish.enable(self.deferred_dense_finish):
                embedded_dense = self.dense_arch(dense_features)
                concatenated = _FusedGatherInteraction.apply(embedded_dense, lookup.module.placeholder_autograd_tensor, lookup,
                                                             self.inter_arch.pad_rows, self.fused_single_row_update)
                self.fused_lookup_steps += 1
                return self.over_arch(concatenated)
        # The reference runs dense_arch, then sparse_arch (models/dlrm.py:400-401).  Here the lookup and
        # the pooled all-to-all are issued first so that the exchange overlaps the bottom MLP on the
        # collective's own HIP stream; the two branches are independent, results are identical.
        pending = self.sparse_arch.start(sparse_features)
        embedded_dense = self.dense_arch(dense_features)
        embedded_sparse = self.sparse_arch.finish(pending)
        concatenated = self.inter_arch(dense_features=embedded_dense, sparse_features=embedded_sparse)
        return self.over_arch(concatenated)


# nn.BCEWithLogitsLoss (mean) as ONE kernel for loss + gradient (csrc/mlp_epilogue.hip bce_with_logits_kernel) instead of 8
# element-wise / reduce kernels forward and 5 backward


class _FusedBCEWithLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        from ..distributed import _device_ops  # noqa: F401  (registers torch.ops.tbe_hip.*)

        loss, dlogits = torch.ops.tbe_hip.bce_with_logits(logits, labels)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (dlogits,) = ctx.saved_tensors
        return dlogits * grad_out, None


def bce_with_logits_mean(loss_fn: nn.Module, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """`loss_fn(logits, labels.float())` for the train wrapper's nn.BCEWithLogitsLoss (examples/dlrm/modules/dlrm_train.py);
    on a HIP device, for the plain mean-reduced loss over float32 logits [B], one fused kernel (labels int64 or float)."""
    if (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 1 and labels.shape == logits.shape
            and type(loss_fn) is nn.BCEWithLogitsLoss and loss_fn.reduction == "mean" and loss_fn.weight is None
            and loss_fn.pos_weight is None and logits.numel() > 0 and labels.dtype in (torch.float32, torch.int64)):
        return _FusedBCEWithLogits.apply(logits, labels)
    return loss_fn(logits, labels.float())


class _Head(nn.Module):
    """interaction + over arch + loss as ONE static-shape segment (inputs: bottom-MLP output, pooled
    embeddings [B, F, D], labels as they come: int64 or float) -> (loss, logits)."""

    def __init__(self, inter_arch: nn.Module, over_arch: nn.Module, loss_fn: nn.Module) -> None:
        super().__init__()
        self.inter_arch, self.over_arch, self.loss_fn = inter_arch, over_arch, loss_fn

    def forward(self, embedded_dense: torch.Tensor, embedded_sparse: torch.Tensor, labels: torch.Tensor):
        logits = self.over_arch(self.inter_arch(dense_features=embedded_dense, sparse_features=embedded_sparse)).squeeze(-1)
        # the logits leave the segment for metrics only: detached, so that the captured backward has ONE root (no zero
        # gradient buffer for a second output, no add of the two contributions to d logits)
        return bce_with_logits_mean(self.loss_fn, logits, labels), logits.detach()


def _flat_layout(head, dense, rest) -> Tuple[List[int], int]:
    """[head | pad | bottom MLP | pad | rest | pad] in a flat float32 buffer: the segments' offsets and the total, in elements.
    The flat parameter AND gradient buffers are cut from this one result (optim/flat.py walks them with one index).  Segments
    start on 256-B boundaries (the head ends with a 1-element bias: unpadded, what follows would sit at 4 mod 16 bytes)."""
    offsets, total = [], 0
    for seg in (head, dense, rest):
        offsets.append(total)
        total = (total + sum(q.numel() for q in seg) + 63) // 64 * 64
    return offsets, total


def _views(buffer: torch.Tensor, params, offset: int) -> List[torch.Tensor]:
    """Consecutive slices of the flat `buffer` from `offset` on, one per parameter and shaped like it."""
    out = []
    for q in params:
        out.append(buffer[offset:offset + q.numel()].view_as(q))
        offset += q.numel()
    return out


def _fold_grads(pairs, scale: float) -> None:
    """(parameter, its view of the flat gradient buffer) pairs: brings what autograd left in `.grad` into the view, scaled."""
    for q, v in pairs:
        if q.grad is None:
            v.zero_()
        elif q.grad.data_ptr() != v.data_ptr():
            torch.mul(q.grad, scale, out=v)
        elif scale != 1.0:
            v.mul_(scale)  # autograd accumulated in place (zero_grad(set_to_none=False))


class _FlatDenseGrads:
    """The flat dense-gradient buffer of capture_hip_graphs(flat_grads=True) and the protocol that all-reduces it piece by
    piece while a step runs.  Set once per capture: buffers, parameters and their views, slice bounds (`n_late`: 0 until the
    backward graphs exist), process group.  Per step: the collectives in flight and the flags wait_and_attach() clears."""

    __slots__ = ("flat", "flat_param", "params", "views", "extras", "n_head", "n_dense", "n_late", "pg", "world", "scale",
                 "reduce", "split_mode", "works", "head_replayed", "dense_replayed", "extras_folded", "rest_started",
                 "pieces_done")

    def __init__(self, segments, offsets, total: int, flat_param, dev, process_group, split_mode: str) -> None:
        head, dense, extras = segments  # (with their _flat_layout, and the parameter buffer cut from the same layout)
        world = dist.get_world_size(process_group) if process_group is not None else 1
        # TORCHREC_AMD_FORCE_DENSE_REDUCE=1 (rehearsal of the N > 1 path on one rank): issue the dense all-reduces — and
        # create their communicator — although a one-rank group needs none
        reduce = world > 1 or (process_group is not None and os.environ.get("TORCHREC_AMD_FORCE_DENSE_REDUCE") == "1")
        pg = process_group
        if reduce and dist.get_backend(process_group) == "nccl" and os.environ.get("TORCHREC_AMD_DENSE_PG", "1") == "1":
            # the dense all-reduces get a communicator (and stream) of their own: on the collection's they would queue
            # behind a pooled all-to-all that is waiting for its links (the prefetched one, above all)
            from ..distributed.comm import new_rccl_group

            pg = new_rccl_group(process_group)
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_param = flat_param  # None: the parameters are not all float32 on one device and stayed where they were
        self.params = list(head) + list(dense) + list(extras)
        self.views = [v for seg, off in zip(segments, offsets) for v in _views(self.flat, seg, off)]
        # every trainable dense parameter outside the graphed segments (the replicated tiny tables of a sharded
        # collection): its gradient arrives through autograd and joins the flat buffer after backward
        self.extras = list(zip(extras, self.views[len(head) + len(dense):]))
        self.n_head, self.n_dense, self.n_late = offsets[1], offsets[2] - offsets[1], 0
        self.pg, self.world, self.scale, self.reduce, self.split_mode = pg, world, 1.0 / world, reduce, split_mode
        self.works = []
        # both graphed segments ran their backward replays this step: finish_dense_grads() tells a replayed step from an
        # eager one (another batch size, eval) by these
        self.head_replayed = self.dense_replayed = False
        self.extras_folded = self.rest_started = self.pieces_done = False

    def _all_reduce(self, lo: int, hi: int) -> None:
        if self.reduce:
            self.works.append(dist.all_reduce(self.flat[lo:hi], group=self.pg, async_op=True))

    def head_done(self, early: bool = False) -> None:
        """The head's backward runs first: its slice overlaps the rest of backward."""
        self.head_replayed = True
        # with a late part (its gradients do not exist yet) what is left of the head's slice is two small layers: they ride
        # with the rest of the buffer (start_rest) instead of paying for a collective of their own
        if not self.n_late:
            self._all_reduce(0, self.n_head)
        elif early:  # "early" split mode: the late part is on its way (reduce_late), the slice behind it follows at once
            self._all_reduce(self.n_late, self.n_head)
            self.pieces_done = True

    def dense_done(self) -> None:
        self.dense_replayed = True

    def reduce_late(self) -> None:
        if self.n_late:
            self._all_reduce(0, self.n_late)

    def fold_extras(self) -> None:
        if not self.extras_folded:
            _fold_grads(self.extras, self.scale)
            self.extras_folded = True

    def early_extras(self) -> None:
        """"early" split mode, behind the embedding collection's start_backward: the replicated tables' slice."""
        self.fold_extras()
        self._all_reduce(self.n_head + self.n_dense, self.flat.numel())

    def start_rest(self) -> None:
        """Graph-replayed step: folds the autograd / explicit gradients of the non-graphed dense parameters (the replicated
        tiny tables) into the flat buffer and starts the all-reduce of everything behind the head's slice (bottom MLP +
        those).  The explicit step calls this as soon as the bottom MLP's backward graph is enqueued — before the fused
        embedding backward and before the next step's prefetched lookup + pooled all-to-all, so that on the collective
        stream the (small) dense reduction is queued AHEAD of that all-to-all and overlaps the embedding update."""
        if self.rest_started:
            return
        self.fold_extras()
        if self.pieces_done:  # "early" split mode: head and replicated tables are on their way, the bottom MLP is left
            self._all_reduce(self.n_head, self.n_head + self.n_dense)
        else:
            self._all_reduce(self.n_late or self.n_head, self.flat.numel())  # (see head_done)
        self.rest_started = True
        self.pieces_done = False

    def fold_all_and_reduce(self) -> None:
        """This step ran eagerly (another batch size, ...): every gradient came through autograd; all are folded and reduced."""
        for w in self.works:
            w.wait()
        self.works.clear()
        _fold_grads(zip(self.params, self.views), self.scale)
        self._all_reduce(0, self.flat.numel())

    def wait_and_attach(self) -> None:
        self.rest_started = self.extras_folded = False
        for w in self.works:
            w.wait()
        self.works.clear()
        for q, v in zip(self.params, self.views):
            q.grad = v


class _Captured:
    """What one capture_hip_graphs() call produced; DLRMTrain._graphs.  `dense`: the bottom-MLP segment; `heads`: the head
    segment, or one per half batch (heads[-1] holds the parameter-gradient sinks of the flat buffer either way); `half`:
    the whole-batch buffers those two share by halves, or None.  Not sub-modules: state_dict keys unchanged."""

    __slots__ = ("batch", "dense", "heads", "half", "graph_exchange", "loss_grad_ready")

    def __init__(self, batch: int, dense, heads, half, graph_exchange: bool) -> None:
        self.batch, self.dense, self.heads, self.half, self.graph_exchange = batch, dense, heads, half, graph_exchange
        self.loss_grad_ready = False  # the explicit step fills d(loss) into the heads' grad-output buffers (zeros) once


class DLRMTrain(nn.Module):
    """examples/dlrm/modules/dlrm_train.py: BCEWithLogits wrapper used by the train pipeline."""

    def __init__(self, embedding_bag_collection: nn.Module, dense_in_features: int,
                 dense_arch_layer_sizes: List[int], over_arch_layer_sizes: List[int],
                 dense_device: Optional[torch.device] = None) -> None:
        super().__init__()
        self.model = DLRM(embedding_bag_collection, dense_in_features, dense_arch_layer_sizes,
                          over_arch_layer_sizes, dense_device)
        self.loss_fn = nn.BCEWithLogitsLoss()
        self._graphs: Optional[_Captured] = None  # (`_flat_dense` exists only once a flat capture has assigned it: _flat())
        # per-step hand-offs of the explicit step (set_between_forward_and_backward, take_backward_done)
        self._between = self._prefetch = self._prefetched = None
        self._backward_done = False
        self.explicit_steps = self.half_batch_steps = self.prefetched_lookups = 0  # for tests / bench.py's line

    def _flat(self) -> Optional[_FlatDenseGrads]:
        return self.__dict__.get("_flat_dense")

    def capture_hip_graphs(self, batch_size: int, flat_grads: bool = False, process_group=None,
                           half_batches: Optional[bool] = None) -> None:
        """Captures the two collective-free dense segments of a train step — bottom MLP; interaction
        + top MLP + loss — as HIP graphs for this per-rank batch size (distributed/hip_graph.py).
        Steps with another batch size, eval mode or no_grad run eagerly as before.

        flat_grads: the backward graphs write the parameter gradients, already divided by the world
        size, into ONE flat buffer; the head's slice is all-reduced asynchronously as soon as its backward
        replay is enqueued, the rest (bottom segment + the model's remaining dense parameters, i.e. the
        replicated tiny tables) by `finish_dense_grads()`, which also attaches the slices as `.grad`.
        This replaces DistributedDataParallel altogether (its forward wrapper alone cost 0.43 ms of host
        time per step, plus 16 per-parameter bucket copies — the per-rank step of an N > 1 run is
        host-bound); DistributedModelParallel.init_data_parallel() broadcasts rank 0's values instead."""
        # the graphs share one memory pool: the order of the captures, and of what is allocated before, inside and between
        # them, decides addresses (distributed/hip_graph.py write_sinks records what a misplaced allocation did)
        m = self.model
        dev, B = next(m.dense_arch.parameters()).device, batch_size
        head = _Head(m.inter_arch, m.over_arch, self.loss_fn)
        ebc = m.sparse_arch.embedding_bag_collection
        ebc = getattr(ebc, "sharded", ebc)
        segments, offsets, total, flat_param = self._flatten_parameters(head, dev) if flat_grads else (None,) * 4
        if half_batches is None:
            half_batches = _HALF_BATCHES == "1" or (_HALF_BATCHES == "auto" and B >= _HALF_BATCH_MIN)
        halves = bool(half_batches and flat_grads and B % 2 == 0 and getattr(ebc, "_exchange", False)
                      and hasattr(ebc, "set_half_batch_exchange"))
        cap, hooks = self._capture_forward(head, ebc, B, dev, flat_grads, halves)
        st = None
        if flat_grads:  # the flat gradient buffer, and who is told when a segment's backward has written its slice
            st = _FlatDenseGrads(segments, offsets, total, flat_param, dev, process_group,
                                 _WGRAD_SPLIT_MODE if cap.half is None else "late")
            if hasattr(ebc, "set_replicated_grad_sink"):
                dp = getattr(ebc, "_dp_module", None)
                ebc.set_replicated_grad_sink(next((v for q, v in st.extras if dp is not None and q is dp.weights), None))
            if cap.half is None:  # (the half-batch step tells it itself, once for both head segments)
                cap.heads[-1].after_backward = st.head_done
            cap.dense.after_backward = st.dense_done
            self._flat_dense = st
        self._capture_backward(cap, st, ebc, hooks, dev)
        self._graphs = cap

    def _flatten_parameters(self, head: nn.Module, dev):
        """The trainable dense parameters as (head, bottom MLP, the rest), their _flat_layout, and ONE flat buffer of that layout
        they move into before anything captures their addresses (or None): optim/flat.py updates them with one kernel."""
        seg_head = [q for q in head.parameters() if q.requires_grad]
        seg_dense = [q for q in self.model.dense_arch.parameters() if q.requires_grad]
        seen = {id(q) for q in seg_head + seg_dense}
        segments = (seg_head, seg_dense, [q for q in self.parameters() if q.requires_grad and id(q) not in seen])
        offsets, total = _flat_layout(*segments)
        flat_param = None
        if all(q.dtype == torch.float32 and q.device == dev for seg in segments for q in seg):
            flat_param = torch.zeros(total, dtype=torch.float32, device=dev)
            with torch.no_grad():
                for seg, off in zip(segments, offsets):
                    for q, view in zip(seg, _views(flat_param, seg, off)):
                        view.copy_(q)
                        q.data = view
        return segments, offsets, total, flat_param

    def _capture_forward(self, head: nn.Module, ebc, B: int, dev, flat_grads: bool, halves: bool):
        """The forward graphs: bottom MLP, then head (whole, or per half batch).  Returns (_Captured, exchange hooks or None)."""
        from ..distributed.hip_graph import GraphedSegment

        m = self.model
        F, D = m.sparse_arch.F, m.sparse_arch.D
        g_dense = GraphedSegment(m.dense_arch, [torch.randn(B, m.dense_arch.model._mlp[0]._in_size, device=dev)])
        if halves:
            if hasattr(ebc, "set_graph_exchange"):
                ebc.set_graph_exchange(None)
            # whole-batch buffers the two head segments share by halves: pooled embeddings (the collection's output
            # buffer), labels, and the gradients w.r.t. the bottom-MLP output / the pooled embeddings
            Bh = B // 2
            Dd = g_dense.static_outputs[0].shape[1]
            half = {"pooled": torch.zeros(B, F, D, device=dev), "labels": torch.zeros(B, dtype=torch.int64, device=dev),
                    "gd": torch.zeros(B, Dd, device=dev), "gs": torch.zeros(B, F, D, device=dev), "Bh": Bh}
            heads = []
            for h in range(2):
                rows = slice(h * Bh, (h + 1) * Bh)
                m.inter_arch.grad_sinks = (half["gd"][rows], half["gs"][rows])
                try:
                    heads.append(GraphedSegment(
                        head, [g_dense.static_outputs[0][rows].detach().requires_grad_(True),
                               half["pooled"][rows].detach().requires_grad_(True), half["labels"][rows]],
                        input_buffers=[g_dense.static_outputs[0][rows], half["pooled"][rows], half["labels"][rows]],
                        pool=g_dense._pool))
                finally:
                    m.inter_arch.grad_sinks = None
            return _Captured(B, g_dense, heads, half, False), None
        # static-exchange mode (flat gradients + explicit step + a collection that exchanges): the unpack of the pooled
        # all-to-all's receive buffer is the FIRST kernel of the head's forward graph and the pack of the gradient
        # into the send buffer the LAST of its backward graph, instead of two eager launches per step
        hooks = None
        if (flat_grads and _GRAPH_EXCHANGE and getattr(ebc, "_exchange", False)
                and hasattr(ebc, "set_graph_exchange")):
            pooled = torch.zeros(B, F, D, device=dev)
            ebc.set_output_buffer(pooled)
            hooks = ebc.set_graph_exchange(B)
        elif hasattr(ebc, "set_graph_exchange"):
            ebc.set_graph_exchange(None)
        g_head = GraphedSegment(
            head, [g_dense.static_outputs[0].detach().requires_grad_(True),
                   torch.randn(B, F, D, device=dev).requires_grad_(True),
                   torch.randint(0, 2, (B,), device=dev)],  # int64, as the data loader delivers them
            input_buffers=[g_dense.static_outputs[0], pooled if hooks is not None else None, None], pool=g_dense._pool,
            pre_forward=hooks[0] if hooks is not None else None)
        return _Captured(B, g_dense, [g_head], None, hooks is not None), hooks

    def _capture_backward(self, cap: _Captured, st: Optional[_FlatDenseGrads], ebc, hooks, dev) -> None:
        """The backward graphs: the head's (of both halves), then the bottom MLP's."""
        g_dense, g_head, half, flat = cap.dense, cap.heads[-1], cap.half, st is not None
        n = len(g_head._params)
        head_sinks = st.views[:n] if flat else None
        dense_sinks = st.views[n:n + len(g_dense._params)] if flat else None
        scale = st.scale if flat else 1.0
        late = 0
        if flat and _DEFER_WGRAD and getattr(ebc, "_exchange", False):
            # (weight, bias) of the over arch's first layers: the leading parameters of the head segment
            n_lin = sum(1 for q in g_head._params if q.dim() == 2)
            late = 2 * min(_late_layers(cap.batch, half is not None), max(n_lin - 1, 0))
            if late and not all(g_head._params[j].dim() == (2 if j % 2 == 0 else 1) for j in range(late)):
                late = 0  # not a plain (weight, bias) sequence: keep everything in the second graph
        # the embedding collection writes its pooled output straight into the head segment's static input
        if hasattr(ebc, "set_half_batch_exchange"):
            ebc.set_half_batch_exchange(half is not None)
        if half is not None:
            ebc.set_output_buffer(half["pooled"])
            # half 0's parameter gradients go to a buffer of their own and are added to half 1's (which sit in the flat
            # buffer) by one launch after both weight-gradient graphs
            half["tmp"] = torch.zeros(st.n_head, dtype=torch.float32, device=dev)
            tmp_sinks = _views(half["tmp"], g_head._params, 0)
            half["n_used"] = sum(q.numel() for q in g_head._params)
            for h, gh in enumerate(cap.heads):
                gh.capture_backward(param_grad_sinks=tmp_sinks if h == 0 else head_sinks, sink_scale=scale,
                                    defer_wgrad=_DEFER_WGRAD, late_params=late)
                rows = slice(h * half["Bh"], (h + 1) * half["Bh"])
                if (gh.static_grad_inputs[0].data_ptr() != half["gd"][rows].data_ptr()
                        or gh.static_grad_inputs[1].data_ptr() != half["gs"][rows].data_ptr()):
                    raise RuntimeError("capture_hip_graphs(half_batches=True): the head segment's input gradients did not land "
                                       "in the shared whole-batch buffers (is the fused dot interaction in use?)")
            grad_out = half["gd"]
        else:
            if hasattr(ebc, "set_output_buffer") and hooks is None:
                ebc.set_output_buffer(g_head.static_input(1).detach())
            # flat mode: the head's weight gradients go into a second graph that the explicit step replays after it has
            # started the embedding-gradient all-to-all (modules/mlp.py _DeferredWgrad)
            g_head.capture_backward(param_grad_sinks=head_sinks, sink_scale=scale, defer_wgrad=flat and _DEFER_WGRAD,
                                    late_params=late,
                                    post_backward=(lambda gin: hooks[1](gin[1])) if hooks is not None else None)
            grad_out = g_head.static_grad_inputs[0]
        # the head's gradient w.r.t. the bottom-MLP output doubles as the bottom segment's grad_output buffer
        g_dense.capture_backward([grad_out], param_grad_sinks=dense_sinks, sink_scale=scale, defer_wgrad=flat and _DEFER_WGRAD)
        if flat and g_head.bwd_graph3 is not None:
            st.n_late = sum(q.numel() for q in g_head._params[:late])

    def dense_optimizer(self, params, lr: float, momentum: float = 0.0, weight_decay: float = 0.0) -> torch.optim.Optimizer:
        """SGD for the dense parameters (what examples/dlrm/dlrm_main.py:536-540 builds with torch.optim.SGD): one
        kernel over the flat parameter / gradient buffers when capture_hip_graphs(flat_grads=True) has laid them out
        (optim/flat.py), torch.optim.SGD otherwise — same hyper-parameters, same arithmetic.  Call it AFTER
        capture_hip_graphs (a later capture moves the parameters into NEW flat buffers)."""
        params = list(params)
        st = self._flat()
        if (st is not None and st.flat_param is not None and {id(q) for q in st.params} <= {id(q) for q in params}
                and os.environ.get("TORCHREC_AMD_FLAT_SGD", "1") != "0"):
            from ..optim.flat import FlatSGD

            return FlatSGD(params, lr, flat_param=st.flat_param, flat_grad=st.flat, covered=st.params,
                           grad_views=st.views, momentum=momentum, weight_decay=weight_decay)
        return torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)

    def flat_grad_parameters(self) -> List[nn.Parameter]:
        """Parameters whose gradients travel through the flat buffer (kept out of DDP)."""
        st = self._flat()
        return list(st.params) if st is not None else []

    def finish_dense_grads(self) -> None:
        """After backward: folds the autograd gradients of the non-graphed dense parameters into the flat
        buffer, all-reduces the rest of it (bottom segment + those), waits, and attaches the slices as
        `.grad` (every rank then holds the rank-averaged gradient, as under DistributedDataParallel)."""
        st = self._flat()
        if st is None:
            return
        replayed = st.head_replayed and st.dense_replayed
        st.head_replayed = st.dense_replayed = False
        if replayed:
            st.start_rest()
        else:
            st.fold_all_and_reduce()
        st.wait_and_attach()

    # ---- explicit train step (HIP-graph + flat-gradient mode): forward AND backward without the autograd engine --------
    def set_between_forward_and_backward(self, fn, prefetch=None) -> None:
        """A callable the explicit step runs once between its forward and its backward (the train pipeline starts the
        next batch's input dist there, as it does between `model(batch)` and `loss.backward()` otherwise).

        `prefetch`: a callable the explicit step runs right behind its LAST backward launch (the fused embedding
        backward): it returns (next batch's KeyedJaggedTensor, its ExplicitLookupStep) or None.  The next step's lookup
        and pooled all-to-all depend on the tables this step's embedding backward has just updated and on nothing else
        — not on the dense optimizer, the dense gradient all-reduce or the host's step-boundary work — so they are
        enqueued here and the GPU has work while the host does that (the step boundary was the largest idle gap of the
        per-rank step: 98 us of 1.99 ms, profiles/r02_rehearsal_b8192_explicit_gaps.txt)."""
        self._between, self._prefetch = fn, prefetch

    @property
    def wants_lookup_prefetch(self) -> bool:
        """True when the captured head segment keeps part of its weight gradients for the window behind the next step's
        prefetched lookup (capture_hip_graphs, TORCHREC_AMD_WGRAD_LATE_LAYERS): the pipeline then prefetches by default."""
        g, st = self._graphs, self._flat()
        return bool(g is not None and g.heads[-1].bwd_graph3 is not None and (st is None or st.split_mode == "late"))

    def take_backward_done(self) -> bool:
        """True (once) when the latest forward() already ran the backward: the caller must not call loss.backward()."""
        done, self._backward_done = self._backward_done, False
        return done

    def _explicit_lookup(self, batch):
        """The collection's ExplicitLookupStep for this batch: the one prefetched at the end of the previous step, or a
        new one on the pipeline's queued input dist (or on its own).  None if the collection cannot run it."""
        ebc = self.model.sparse_arch.embedding_bag_collection
        if not hasattr(ebc, "compute_explicit"):
            return None
        inner = getattr(ebc, "sharded", ebc)
        if list(inner._feature_names) != list(self.model.sparse_arch.sparse_feature_names):
            return None
        kjt = batch.sparse_features
        pre, self._prefetched = self._prefetched, None
        if pre is not None and pre[0] is kjt and getattr(pre[1], "epoch", 0) != getattr(inner, "_weights_epoch", 0):
            # the tables were rewritten (load_state_dict) after the prefetch: look up again, on the same distributed ids
            pre[1].discard()
            pre = (kjt, inner.compute_explicit(pre[1].d))
            self.prefetched_lookups -= 1
        if pre is not None and pre[0] is kjt:
            self.prefetched_lookups += 1
            return pre[1]  # looked up (and its all-to-all started) at the end of the previous step
        if pre is not None:
            raise RuntimeError("DLRMTrain: a lookup was prefetched for another batch than the one this step received; the "
                               "owner of the pipeline must feed the batches in the order it announced them")
        piped = getattr(ebc, "_pipelined", None)  # a train pipeline's forward on this collection (queued input dist)
        if piped is not None:
            return piped.compute_explicit(kjt)
        return ebc.compute_explicit(ebc.input_dist(kjt).wait()) if ebc.explicit_step_supported(kjt.stride()) else None

    def _explicit_step(self, batch, g: _Captured):
        """One train step of the graphed configuration driven by hand: lookup -> all-to-all || bottom-MLP graph ->
        head graph (forward + backward replays) -> gradient all-to-all || bottom-MLP backward graph -> embedding
        backward.  Same kernels, same order of the dependent work as the autograd path; what disappears is the engine
        (its worker thread, ~12 Python Function nodes and their hand-offs: ~0.25 ms of host time per step, which is the
        bottleneck of the N > 1 per-rank step on a slow host).  Returns None if the collection cannot run it."""
        step = self._explicit_lookup(batch)
        if step is None:
            return None
        if g.half is not None:
            return self._explicit_step_halves(batch, step, g)
        st, g_dense, g_head = self._flat(), g.dense, g.heads[0]
        early = g_head.bwd_graph3 is not None and st.split_mode == "early"
        with torch.no_grad():
            self._bottom_forward(batch, g_dense)
            pooled = step.finish()  # written into the head segment's static input by the collection
            if pooled.data_ptr() != g_head.static_inputs[1].data_ptr():
                g_head.static_inputs[1].copy_(pooled.view_as(g_head.static_inputs[1]))
            g_head.static_inputs[2].copy_(batch.labels)
            g_head.fwd_graph.replay()
            self._between()
            with label("## backward ##"):  # train_pipeline.py:546
                if not g.loss_grad_ready:
                    g_head.static_grad_outputs[0].fill_(1.0)  # d(loss) = 1
                    g.loss_grad_ready = True
                g_head.bwd_graph.replay()  # ends with the gradient of the pooled embeddings
                step.start_backward(g_head.static_grad_inputs[1].view(g.batch, -1))  # pack + gradient all-to-all (+ replicated tables)
                if early:
                    st.early_extras()  # (_WGRAD_SPLIT_MODE; start_backward above has written the replicated tables' gradients)
                    g_head.bwd_graph3.replay()
                    st.reduce_late()
                if g_head.bwd_graph2 is not None:
                    g_head.bwd_graph2.replay()  # the head's weight gradients, while the all-to-all is in flight
                st.head_done(early)  # all-reduce of the head's slice of the flat gradient
                self._bottom_backward(step, g_dense, st)
            self._end_step(g, st, late=not early)
        loss, logits = g_head.static_outputs
        return loss.detach(), (loss.detach(), logits.detach(), batch.labels.detach())

    def _explicit_step_halves(self, batch, step, g: _Captured):
        """The explicit step with the exchange in two half-batches (capture_hip_graphs(half_batches=True)); the head's part:
            half 0: wait, unpack, head forward, head backward (input gradients), pack, gradient all-to-all 0
            half 1: the same — its embeddings crossed the links during half 0's work, half 0's gradients cross during this
            weight gradients of both halves (gradient all-to-all 1 in flight)."""
        if not getattr(step, "halves", False):
            raise RuntimeError("DLRMTrain: the head segments were captured for half-batch exchanges, the collection did "
                               "not start one")
        st, g_dense, half, heads = self._flat(), g.dense, g.half, g.heads
        Bh, gs_all = half["Bh"], half["gs"].view(g.batch, -1)
        with torch.no_grad():
            self._bottom_forward(batch, g_dense)
            half["labels"].copy_(batch.labels)
            if not g.loss_grad_ready:
                for gh in heads:
                    gh.static_grad_outputs[0].fill_(0.5)  # loss = (mean of half 0 + mean of half 1) / 2
                g.loss_grad_ready = True
            with label("## backward ##"):  # train_pipeline.py:546 (the halves' forwards are inside: they alternate)
                for h, gh in enumerate(heads):
                    step.finish_half(h)  # into the rows of the pooled buffer this segment reads
                    gh.fwd_graph.replay()
                    if h == 0:
                        self._between()
                    gh.bwd_graph.replay()  # ends with the gradients of this half's pooled embeddings / bottom-MLP output
                    step.start_backward_half(h, gs_all[h * Bh:(h + 1) * Bh], grad_out=gs_all if h == 1 else None)
                for gh in heads:
                    if gh.bwd_graph2 is not None:
                        gh.bwd_graph2.replay()  # weight gradients, while the gradient all-to-alls are in flight
                st.flat[st.n_late:half["n_used"]].add_(half["tmp"][st.n_late:half["n_used"]])
                st.head_done()  # all-reduce of the head's slice of the flat gradient (without the late part)
                self._bottom_backward(step, g_dense, st)
            self._end_step(g, st, late=True)
            loss = (heads[0].static_outputs[0] + heads[1].static_outputs[0]) * 0.5
            logits = torch.cat([heads[0].static_outputs[1], heads[1].static_outputs[1]])
        self.half_batch_steps += 1
        return loss.detach(), (loss.detach(), logits.detach(), batch.labels.detach())

    def _bottom_forward(self, batch, g_dense) -> None:
        """Both steps' prologue: the bottom MLP (graph), while the pooled all-to-all is in flight."""
        if batch.dense_features.data_ptr() != g_dense.static_inputs[0].data_ptr():
            g_dense.static_inputs[0].copy_(batch.dense_features)
        g_dense.fwd_graph.replay()

    def _bottom_backward(self, step, g_dense, st: _FlatDenseGrads) -> None:
        """Both steps' epilogue inside the backward label: the bottom MLP's backward, then the embedding backward."""
        g_dense.bwd_graph.replay()  # its grad_output buffer IS the head's gradient w.r.t. the bottom-MLP output
        if g_dense.bwd_graph2 is not None:
            g_dense.bwd_graph2.replay()  # its weight / bias gradients, finished into the flat buffer
        st.dense_done()
        st.start_rest()  # ahead of the embedding update and of the next step's all-to-all
        step.finish_backward()

    def _end_step(self, g: _Captured, st: _FlatDenseGrads, late: bool) -> None:
        """Both steps' epilogue behind the embedding backward."""
        if self._prefetch is not None:
            self._prefetched = self._prefetch()  # (kjt, ExplicitLookupStep) of the NEXT batch, or None
        if late and g.heads[-1].bwd_graph3 is not None:
            # the late part of the head's weight gradients: behind the NEXT step's lookup + (first half-batch) pooled
            # all-to-all when the owner prefetches (its cover on the links), right here otherwise
            for gh in g.heads:
                gh.bwd_graph3.replay()
            if g.half is not None:
                st.flat[:st.n_late].add_(g.half["tmp"][:st.n_late])
            st.reduce_late()
        self._backward_done = True
        self.explicit_steps += 1

    def forward(self, batch) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        g = self._graphs
        if (g is not None and self.training and torch.is_grad_enabled()
                and batch.dense_features.shape[0] == g.batch and batch.dense_features.is_cuda):
            if self._flat() is not None and self._between is not None:
                # only under an owner that asked for it (set_between_forward_and_backward) and will skip loss.backward()
                out = self._explicit_step(batch, g)
                self._between = self._prefetch = None
                if out is not None:
                    return out
            if g.half is not None:
                raise RuntimeError("DLRMTrain: graphs captured with half_batches=True serve the explicit step only (run the "
                                   "model under TrainPipelineSparseDist, or capture with half_batches=False)")
            if g.graph_exchange:
                raise RuntimeError("DLRMTrain: these graphs unpack / pack the pooled exchange themselves and serve the explicit "
                                   "step only (run the model under TrainPipelineSparseDist, or set TORCHREC_AMD_GRAPH_EXCHANGE=0)")
            g_head = g.heads[0]
            pending = self.model.sparse_arch.start(batch.sparse_features)
            embedded_dense = g.dense(batch.dense_features)
            embedded_sparse = self.model.sparse_arch.finish(pending)
            g.loss_grad_ready = False  # autograd writes whatever d(loss) the caller backpropagates
            loss, logits = g_head(embedded_dense, embedded_sparse, batch.labels.to(g_head.static_inputs[2].dtype))
            return loss, (loss.detach(), logits.detach(), batch.labels.detach())
        logits = self.model(batch.dense_features, batch.sparse_features).squeeze(-1)
        loss = bce_with_logits_mean(self.loss_fn, logits, batch.labels)
        return loss, (loss.detach(), logits.detach(), batch.labels.detach())
