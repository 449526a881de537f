"""Recall@k and NDCG@k of the BERT4Rec evaluation: `recalls_and_ndcgs_for_ks` of the reference
(examples/bert4rec/bert4rec_metrics.py:13-61), same call, same keys ("Recall@%d", "NDCG@%d"), same Python floats.

    metrics = recalls_and_ndcgs_for_ks(scores, labels, ks)                                   # the reference's call
    metrics = recalls_and_ndcgs_for_ks(scores[:, -1, :], labels, ks, candidates=candidates)  # bert4rec_main.py:244-245 inside

`scores` is [B, C], or [B, V] with `candidates` [B, C] int64 (the list of row b is scores[b, candidates[b]]); `labels` is
[B, C] with values in {0, 1}.  On a HIP device, for float32 scores with inner stride 1 (any row stride: the `[:, -1, :]`
view goes in as it is), int64 / bool / float32 labels and C <= 8192, a call is one kernel (`tbe_rank_metrics_f32`,
csrc/rank_metrics.hip: no sort, every positive's place counted from the row in LDS), one fixed-order finishing launch and
ONE device-to-host copy.  CPU tensors, other dtypes and C > 8192 take `_recalls_and_ndcgs_torch`: the reference's formula
with a stable sort and a vectorised ideal DCG (no per-sample `.item()`).

Rules, on both paths.  Ties: the reference's `torch.sort` is not stable and leaves ties to chance; here ties go to the lower
index, -0.0 ties with +0.0 and a NaN score ranks after every number, NaNs in index order — `np.argsort(-s, kind="stable")`.
A row without a positive yields NaN, and so does the mean, as in the reference.  `ValueError` before any launch: k < 1,
k > C (the reference fails there with a broadcasting RuntimeError), empty `ks`, more than 8 distinct `ks`.  A candidate
outside [0, V) or a label outside {0, 1} is never used as an address or a hit; it is counted and raises `ValueError` with
the counts.  Out of scope: graded relevance, accumulation across batches (the reference averages batch means on the host)."""
import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from fbgemm_gpu import _lib
from fbgemm_gpu._lib import check, ptr, stream_ptr

__all__ = ["recalls_and_ndcgs_for_ks", "MAX_CANDIDATES", "MAX_KS"]

MAX_CANDIDATES = 8192  # csrc/rank_metrics.hip kRankMaxC
MAX_KS = 8             # csrc/rank_metrics.hip kRankMaxKs

_weights_cache: Dict[Tuple[int, torch.device], torch.Tensor] = {}


def dcg_weights(kmax: int) -> torch.Tensor:
    """w[p] = 1 / log2(p + 2), p < kmax, by the reference's own expression (bert4rec_metrics.py:50-51), on the host."""
    return 1 / torch.log2(torch.arange(2, 2 + kmax).float())


def _device_weights(kmax: int, dev: torch.device) -> torch.Tensor:
    key = (kmax, dev)
    if key not in _weights_cache:
        _weights_cache[key] = dcg_weights(kmax).to(dev)
    return _weights_cache[key]


def _check_ks(ks: Sequence[int], C: int) -> List[int]:
    """The distinct ks, ascending."""
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError("recalls_and_ndcgs_for_ks: ks is empty")
    for k in ks:
        if k < 1 or k > C:
            raise ValueError(f"recalls_and_ndcgs_for_ks: k={k} outside 1 .. C={C}")
    distinct = sorted(set(ks))
    if len(distinct) > MAX_KS:
        raise ValueError(f"recalls_and_ndcgs_for_ks: {len(distinct)} distinct ks, at most {MAX_KS}")
    return distinct


def _bad_data(n_bad_candidate: int, n_bad_label: int, labels: torch.Tensor) -> None:
    if n_bad_candidate or n_bad_label:
        raise ValueError("recalls_and_ndcgs_for_ks: candidates outside [0, V) or labels outside {0, 1}: "
                         f"n_bad_candidate={n_bad_candidate}, n_bad_label={n_bad_label} of {labels.numel()} entries")


def _as_dict(ks: List[int], values: List[float]) -> Dict[str, float]:
    """values = [Recall@k_0 .., NDCG@k_0 ..] for ascending ks -> the reference's dict, in its order (k descending)."""
    out: Dict[str, float] = {}
    for q in range(len(ks) - 1, -1, -1):
        out["Recall@%d" % ks[q]] = values[q]
        out["NDCG@%d" % ks[q]] = values[len(ks) + q]
    return out


def _recalls_and_ndcgs_torch(scores: torch.Tensor, labels: torch.Tensor, ks: List[int],
                             candidates: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """The reference's formula (bert4rec_metrics.py:28-61) with a stable sort, the ideal DCG looked up in a table of the
    reference's own prefix sums instead of one `.item()` per sample, and one host read at the end.  ks: distinct, ascending."""
    n_bad_c = 0
    if candidates is not None:
        V = scores.shape[1]
        bad = (candidates < 0) | (candidates >= V)
        n_bad_c = int(bad.sum())
        if n_bad_c == 0:
            scores = scores.gather(1, candidates)
    _bad_data(n_bad_c, int(((labels != 0) & (labels != 1)).sum()), labels)
    dev = scores.device
    labels_float = labels.float()
    answer_count = labels_float.sum(1)
    _, cut = torch.sort(-scores, dim=1, stable=True)
    recalls, ndcgs = [], []
    for k in ks[::-1]:
        cut = cut[:, :k]
        hits = labels_float.gather(1, cut)
        recalls.append((hits.sum(1) / torch.min(torch.Tensor([k]).to(dev), answer_count)).mean())
        weights = dcg_weights(k)
        dcg = (hits * weights.to(dev)).sum(1)
        table = torch.stack([weights[:n].sum() for n in range(k + 1)]).to(dev)  # host sums: the reference's idcg values
        idcg = table[answer_count.clamp(max=k).long()]
        ndcgs.append((dcg / idcg).mean())
    return _as_dict(ks, torch.stack(recalls[::-1] + ndcgs[::-1]).tolist())


def _kernel_path(scores: torch.Tensor, labels: torch.Tensor, candidates: Optional[torch.Tensor]) -> bool:
    B, C = labels.shape
    return (scores.is_cuda and scores.dtype == torch.float32 and scores.stride(1) == 1
            and (B <= 1 or scores.stride(0) >= scores.shape[1]) and labels.device == scores.device
            and labels.dtype in (torch.int64, torch.bool, torch.float32) and C <= MAX_CANDIDATES
            and (candidates is None or (candidates.dtype == torch.int64 and candidates.device == scores.device)))


def recalls_and_ndcgs_for_ks(scores: torch.Tensor, labels: torch.Tensor, ks: Sequence[int],
                             candidates: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """Recall@k and NDCG@k, averaged over the batch, for every k of `ks` (module docstring)."""
    if scores.dim() != 2 or labels.dim() != 2 or labels.shape[0] != scores.shape[0]:
        raise ValueError(f"recalls_and_ndcgs_for_ks: need scores [B, .] and labels [B, C], got {tuple(scores.shape)} and "
                         f"{tuple(labels.shape)}")
    if candidates is None:
        if labels.shape != scores.shape:
            raise ValueError(f"recalls_and_ndcgs_for_ks: scores {tuple(scores.shape)} and labels {tuple(labels.shape)} differ "
                             "in shape")
    elif candidates.shape != labels.shape:
        raise ValueError(f"recalls_and_ndcgs_for_ks: candidates {tuple(candidates.shape)} and labels {tuple(labels.shape)} "
                         "differ in shape")
    B, C = labels.shape
    if C < 1 or (candidates is not None and scores.shape[1] < 1):
        raise ValueError("recalls_and_ndcgs_for_ks: empty candidate lists")
    kk = _check_ks(ks, C)
    if not _kernel_path(scores, labels, candidates):
        return _recalls_and_ndcgs_torch(scores, labels, kk, candidates)
    dev = scores.device
    lib = _lib.load()
    nk = len(kk)
    labels = labels.contiguous()
    if candidates is not None:
        candidates = candidates.contiguous()
    weights = _device_weights(kk[-1], dev)
    out = torch.empty(2 + nk, dtype=torch.int64, device=dev)  # counts int64 [2], then metrics float32 [2 nk]
    ks_host = (ctypes.c_int32 * nk)(*kk)
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.tbe_rank_metrics_workspace_bytes(B, nk), dev)
        check(lib.tbe_rank_metrics_f32(
            ptr(scores), scores.stride(0) if B > 1 else scores.shape[1], ptr(candidates), scores.shape[1], ptr(labels),
            labels.element_size(), B, C, ks_host, nk, ptr(weights), out.data_ptr() + 16, out.data_ptr(), ptr(ws), ws.numel(),
            stream_ptr(dev)), "tbe_rank_metrics_f32")
    host = out.cpu()  # the one D2H copy (waits for the stream)
    _bad_data(int(host[0]), int(host[1]), labels)
    return _as_dict(kk, host[2:].view(torch.float32).tolist())
