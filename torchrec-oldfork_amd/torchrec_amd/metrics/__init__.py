"""Evaluation metrics of the DLRM trainer on the device: exact binary AUROC and accuracy.

The reference's `_evaluate` (examples/dlrm/dlrm_main.py:209-269) feeds `sigmoid(logits)` and the labels of every
validation / test batch into `torchmetrics.AUROC(compute_on_step=False)` and `torchmetrics.Accuracy(compute_on_step=
False)` and reads both at the end.  `AUROC` and `Accuracy` here take those two lines' place (`.to(device)`, call per
batch, `.compute().item()`), and `evaluate` is `_evaluate` itself.

`update` appends to device buffers; `compute` makes ONE call into the HIP library (`tbe_auroc_counts_f32`: key
transform, the package's pair sort, a tie-aware integer reduction — csrc/auroc.hip) on the current stream, reads six
integer counters back in one copy and divides them as Python integers.  The result is therefore exact (the correctly
rounded float64 of the rational value), the same on every run and on every rank.  Out of scope: sample weights,
multiclass, max_fpr, ROC curves, binned approximations.

`recalls_and_ndcgs_for_ks` (ranking.py) is the BERT4Rec evaluation's Recall@k / NDCG@k on the device."""
from typing import Any, Iterator, List, Optional, Tuple

import itertools

import torch
import torch.distributed as dist
from fbgemm_gpu import _lib
from fbgemm_gpu._lib import check, ptr, require_gpu, stream_ptr

from .ranking import recalls_and_ndcgs_for_ks

__all__ = ["AUROC", "Accuracy", "evaluate", "MAX_SAMPLES", "recalls_and_ndcgs_for_ks"]

MAX_SAMPLES = 1 << 29  # tbe_auroc_counts_f32 takes fewer samples than this (the pair sort's limit)
_MIN_CAPACITY = 1024
# the queue depth of the reference's pipeline (examples/dlrm/dlrm_main.py:58): what its _evaluate takes from next_iterator
TRAIN_PIPELINE_STAGES = 3


def _counts(preds: torch.Tensor, labels: torch.Tensor, threshold: float) -> List[int]:
    """[2U, P, N, n_correct, n_nan, n_bad_label] of float32 preds [n] and float32 / int64 labels [n] on one device:
    one C call on the current stream, one device-to-host copy."""
    n = preds.numel()
    if n >= MAX_SAMPLES:
        raise ValueError(f"{n} samples accumulated; the device-side AUROC takes fewer than 2^29 = {MAX_SAMPLES}")
    dev = require_gpu(preds, labels)
    lib = _lib.load()
    nbytes = lib.tbe_auroc_workspace_bytes(n)
    ws = _lib.workspace(nbytes, dev)
    counts = torch.empty(6, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.tbe_auroc_counts_f32(ptr(preds), ptr(labels), labels.element_size(), n, float(threshold), ptr(counts),
                                       ptr(ws), ws.numel(), stream_ptr(dev)), "tbe_auroc_counts_f32")
    out = [int(v) for v in counts.tolist()]  # the one D2H copy (waits for the stream)
    _lib.raise_on_faults("torchrec_amd.metrics")
    return out


class _BinaryMetric(torch.nn.Module):
    """State shared by AUROC and Accuracy: every (pred, label) pair seen since the last reset, in two device buffers that
    double when full."""

    def __init__(self, compute_on_step: bool = False, process_group: Optional[Any] = None) -> None:
        super().__init__()
        if compute_on_step:
            raise ValueError("compute_on_step=True is not supported: the reference evaluates with compute_on_step=False "
                             "(examples/dlrm/dlrm_main.py:252-253) and reads the metric once, with compute()")
        self.process_group = process_group
        # persistent=False: the accumulated samples are no part of a checkpoint; being buffers makes .to(device) move them
        self.register_buffer("_preds", torch.empty(0, dtype=torch.float32), persistent=False)
        self.register_buffer("_labels", torch.empty(0, dtype=torch.float32), persistent=False)
        self._count = 0

    def reset(self) -> None:
        self._count = 0

    def _reserve(self, dev: torch.device, label_dtype: torch.dtype, total: int) -> None:
        if self._preds.device != dev or self._labels.dtype != label_dtype:
            if self._count and self._preds.device != dev:
                raise RuntimeError(f"update on {dev} after updates on {self._preds.device}")
            self._preds = self._preds.to(dev)
            lab = self._labels.to(dev)
            if lab.dtype != label_dtype and self._count:
                raise RuntimeError(f"targets of dtype class {label_dtype} after targets stored as {lab.dtype}: keep one "
                                   "kind of target (integer / bool, or floating point) between two resets")
            self._labels = lab.to(label_dtype)
        cap = self._preds.numel()
        if total <= cap:
            return
        new_cap = max(_MIN_CAPACITY, cap)
        while new_cap < total:
            new_cap *= 2
        for name in ("_preds", "_labels"):
            old = getattr(self, name)
            new = torch.empty(new_cap, dtype=old.dtype, device=dev)
            new[:self._count].copy_(old[:self._count])
            setattr(self, name, new)

    @torch.no_grad()
    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        """Appends one batch: floating-point preds [B] or [B, 1], bool / integer / floating-point target of as many
        elements.  Device tensors only."""
        dev = require_gpu(preds, target)
        if not preds.is_floating_point():
            raise ValueError(f"preds must be floating point, got {preds.dtype}")
        if preds.dim() == 2 and preds.shape[1] == 1:
            preds = preds[:, 0]
        if preds.dim() != 1:
            raise ValueError(f"preds must be [B] or [B, 1], got {tuple(preds.shape)}")
        if target.dim() == 2 and target.shape[1] == 1:
            target = target[:, 0]
        if target.shape != preds.shape:
            raise ValueError(f"preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
        label_dtype = torch.float32 if target.is_floating_point() else torch.int64  # what the C ABI takes
        b = preds.numel()
        self._reserve(dev, label_dtype, self._count + b)
        if b:
            self._preds[self._count:self._count + b].copy_(preds)
            self._labels[self._count:self._count + b].copy_(target)
        self._count += b

    def forward(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self.update(preds, target)

    def _group(self):
        """The process group compute() is collective over, or None for a local compute()."""
        if not (dist.is_available() and dist.is_initialized()):
            return None
        pg = self.process_group if self.process_group is not None else dist.group.WORLD
        return pg if dist.get_world_size(pg) > 1 else None

    def _gathered(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(preds, labels) of all ranks, concatenated in rank order; the local ones without a group."""
        preds, labels = self._preds[:self._count], self._labels[:self._count]
        pg = self._group()
        if pg is None:
            return preds, labels
        if not preds.is_cuda:
            raise RuntimeError("compute() over a process group before any update: move the metric to its device first "
                               "(.to(device)), so that a rank without samples can take part in the gather")
        dev = preds.device
        W = dist.get_world_size(pg)
        # 1. the per-rank sample counts (host tensors where the backend has no device collectives: gloo groups whose
        #    ranks share a GPU; device tensors on RCCL)
        on_host = dist.get_backend(pg) != "nccl"
        mine = torch.tensor([self._count], dtype=torch.int64, device="cpu" if on_host else dev)
        sizes = [torch.empty_like(mine) for _ in range(W)]
        dist.all_gather(sizes, mine, group=pg)
        sizes = [int(s.item()) for s in sizes]
        if sum(sizes) >= MAX_SAMPLES:
            raise ValueError(f"{sum(sizes)} samples over all ranks; the device-side AUROC takes fewer than 2^29 = {MAX_SAMPLES}")
        # labels travel as float32 whatever was accumulated (a rank without samples has no dtype of its own to offer):
        # 0 and 1 convert exactly and no other integer becomes 0.0 or 1.0, so the classes {0, 1, neither} survive
        labels = labels.to(torch.float32)
        # 2. all-gather padded to the maximum, 3. drop the padding
        m = max(sizes)
        out = []
        for t in (preds, labels):
            pad = torch.zeros(m, dtype=t.dtype, device=dev)
            pad[:self._count].copy_(t)
            if on_host:
                host = pad.cpu()
                pieces = [torch.empty_like(host) for _ in range(W)]
                dist.all_gather(pieces, host, group=pg)
                out.append(torch.cat([p[:s] for p, s in zip(pieces, sizes)]).to(dev))
            else:
                pieces = [torch.empty_like(pad) for _ in range(W)]
                dist.all_gather(pieces, pad, group=pg)
                out.append(torch.cat([p[:s] for p, s in zip(pieces, sizes)]))
        return out[0], out[1]

    def _compute_counts(self, threshold: float) -> List[int]:
        if self._count >= MAX_SAMPLES:  # before anything is launched or exchanged
            raise ValueError(f"{self._count} samples accumulated; the device-side AUROC takes fewer than 2^29 = {MAX_SAMPLES}")
        preds, labels = self._gathered()
        if not preds.is_cuda:
            require_gpu(preds)  # raises: compute() before any update, metric never moved to a device
        c = _counts(preds.contiguous(), labels.contiguous(), threshold)
        names = ("two_u", "positives", "negatives", "n_correct", "n_nan", "n_bad_label")
        if c[4] or c[5]:
            raise ValueError("predictions contain NaN or labels outside {0, 1}: "
                             + ", ".join(f"{k}={v}" for k, v in zip(names[4:], c[4:])) + f" of {preds.numel()} samples")
        return c


class AUROC(_BinaryMetric):
    """Exact area under the ROC curve of everything passed to update() since the last reset(): ties between a positive
    and a negative count one half (the trapezoidal rule torchmetrics and sklearn apply to the exact curve)."""

    def compute(self) -> torch.Tensor:
        """0-dim float64 tensor (on the host, where the integer division happens).  Collective when a process group of
        more than one rank is initialised: every rank must call it and every rank gets the value of the concatenated
        data."""
        two_u, p, n = self._compute_counts(0.5)[:3]
        if p == 0 or n == 0:
            raise ValueError(f"AUROC needs both classes: positives={p}, negatives={n}")
        return torch.tensor(two_u / (2 * p * n), dtype=torch.float64)  # int / int: correctly rounded


class Accuracy(_BinaryMetric):
    """Fraction of samples with (pred >= threshold) == (target == 1)."""

    def __init__(self, threshold: float = 0.5, compute_on_step: bool = False, process_group: Optional[Any] = None) -> None:
        super().__init__(compute_on_step, process_group)
        self.threshold = float(threshold)

    def compute(self) -> torch.Tensor:
        c = self._compute_counts(self.threshold)
        total = c[1] + c[2]
        if total == 0:
            raise ValueError("Accuracy of zero samples: positives=0, negatives=0")
        return torch.tensor(c[3] / total, dtype=torch.float64)


def evaluate(train_pipeline, iterator: Iterator, next_iterator: Optional[Iterator] = None,
             limit_batches: Optional[int] = None, stage: str = "val") -> Tuple[float, float]:
    """The reference's `_evaluate` (examples/dlrm/dlrm_main.py:209-269): switches the pipelined model to eval(), steps
    the pipeline until it raises StopIteration, feeds sigmoid(logits) and the labels of every step to AUROC and Accuracy,
    and returns (auroc, accuracy) as floats.  Nothing is printed (`stage` only names the stage in error messages); the
    model's training mode is restored on exit.  With a process group both metrics are collective (see compute()).

    next_iterator / limit_batches: the reference chains `islice(iterator, limit_batches - 2)` with the first
    TRAIN_PIPELINE_STAGES - 1 = 2 batches of `next_iterator`, because ITS pipeline stops with two batches still queued:
    the chained ones are left in the queue for the next phase, and the two left over from the phase before are the first
    ones evaluated.  The chaining is kept, but this package's `progress` keeps stepping until its queue is empty
    (DESIGN.md §6), so here every batch of the chain is evaluated in this call: with `next_iterator` given, `limit_batches`
    batches are evaluated in all, the last two of them TAKEN FROM `next_iterator` (they are consumed and do not come back
    in the next phase).  With `next_iterator=None` (the default) nothing is chained or subtracted: exactly the first
    `limit_batches` batches of `iterator` (all of them for None) are evaluated — what a caller of this pipeline wants."""
    model = train_pipeline._model
    device = train_pipeline._device
    was_training = model.training
    model.eval()
    try:
        if next_iterator is None:
            combined = iterator if limit_batches is None else itertools.islice(iterator, limit_batches)
        else:
            if limit_batches is not None:
                limit_batches = max(limit_batches - (TRAIN_PIPELINE_STAGES - 1), 0)
            combined = itertools.chain(
                iterator if limit_batches is None else itertools.islice(iterator, limit_batches),
                itertools.islice(next_iterator, TRAIN_PIPELINE_STAGES - 1))
        if train_pipeline._connected and train_pipeline._batch_i is None:
            train_pipeline._connected = False  # drained by the phase before: fill the queue from this phase's iterator
        auroc = AUROC(compute_on_step=False).to(device)
        accuracy = Accuracy(compute_on_step=False).to(device)
        while True:
            try:
                _loss, logits, labels = train_pipeline.progress(combined)
            except StopIteration:
                break
            preds = torch.sigmoid(logits)
            auroc(preds, labels)
            accuracy(preds, labels)
        try:
            return auroc.compute().item(), accuracy.compute().item()
        except ValueError as e:
            raise ValueError(f"evaluate({stage}): {e}") from e
    finally:
        model.train(was_training)
