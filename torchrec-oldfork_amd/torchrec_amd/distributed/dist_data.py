"""Module-level distribution primitives with the reference's names
(torchrec/distributed/dist_data.py): `_get_recat` (:40-118), `KJTAllToAll` (:137-524, two-phase
lengths / values exchange + recat permute), `PooledEmbeddingsAllToAll` (:602-697),
`PooledEmbeddingsReduceScatter` (:745-795).  The recat runs on
torch.ops.fbgemm.permute_2D_sparse_data; with a different batch size per rank (`variable_batch_size=True`,
dist_data.py:83-116, :249-255, :321-347) on expand_into_jagged_permute + permute_1D_sparse_data (this repo's HIP kernels)."""
import itertools
from typing import List, Optional

import torch
import torch.distributed as dist
from torch import nn

from ..sparse.jagged_tensor import KeyedJaggedTensor
from ..profiling import label
from .types import Awaitable, LazyAwaitable, NoWait


def _get_recat(local_split: int, num_splits: int, stagger: int = 1,
               device: Optional[torch.device] = None, batch_size_per_rank: Optional[List[int]] = None) -> torch.Tensor:
    """Permutation taking [src rank][local feature] row order to [local feature][src rank]
    (examples at dist_data.py:62-65: (2,4,1) -> [0,2,4,6,1,3,5,7], (2,4,2) -> [0,4,2,6,1,5,3,7]).
    With `batch_size_per_rank` (source rank r sent batch_size_per_rank[r] samples of every feature) the rows have
    different lengths and the result is the same permutation per ELEMENT: entry e is the position, in
    [src rank][local feature][sample] order, of element e of [local feature][src rank][sample] order
    (dist_data.py:83-116)."""
    feature_order = [x + num_splits // stagger * y for x in range(num_splits // stagger) for y in range(stagger)]
    recat = [i + j * local_split for i in range(local_split) for j in feature_order]
    if batch_size_per_rank is None or local_split == 0:
        return torch.tensor(recat, dtype=torch.int32, device=device)
    batch_size_per_feature = [b for b in batch_size_per_rank for _ in range(local_split)]
    input_offset = [0] + list(itertools.accumulate(batch_size_per_feature))
    output_offset = [0] + list(itertools.accumulate(batch_size_per_feature[r] for r in recat))
    as_tensor = lambda x: torch.tensor(x, dtype=torch.int32, device=device)  # noqa: E731
    return torch.ops.fbgemm.expand_into_jagged_permute(as_tensor(recat), as_tensor(input_offset), as_tensor(output_offset),
                                                       output_offset[-1])


def ids_per_destination(length_per_key: List[int], feats_per_rank: List[int]) -> List[int]:
    """Ids this rank sends to each destination: `length_per_key` is in send order, feats_per_rank[r] keys for rank r."""
    val_in, k = [], 0
    for n in feats_per_rank:
        val_in.append(sum(length_per_key[k:k + n]))
        k += n
    return val_in


def exchange_ids(pg: dist.ProcessGroup, values: torch.Tensor, weights: Optional[torch.Tensor], val_out: List[int],
                 val_in: List[int]):
    """The second phase of every id exchange (dist_data.py:190, :213): starts the all-to-all of the 1-D ids, and of the
    per-sample weights if given, with the split sizes the caller has worked out.  Returns (recv_values, recv_weights,
    wait); wait() waits for both."""
    recv_v = torch.empty(sum(val_out), dtype=values.dtype, device=values.device)
    with label("## all2all_data:indices ##"):  # dist_data.py:190
        work = [dist.all_to_all_single(recv_v, values, val_out, val_in, group=pg, async_op=True)]
    recv_w = None
    if weights is not None:
        recv_w = torch.empty(sum(val_out), dtype=weights.dtype, device=weights.device)
        with label("## all2all_data:weights ##"):  # dist_data.py:213
            work.append(dist.all_to_all_single(recv_w, weights, val_out, val_in, group=pg, async_op=True))

    def wait() -> None:
        for w in work:
            w.wait()

    return recv_v, recv_w, wait


def variable_batch_exchange(pg: dist.ProcessGroup, n_per_rank: List[int], val_in: List[int], lengths: torch.Tensor,
                            values: torch.Tensor, weights: Optional[torch.Tensor], B: int, stagger: int = 1):
    """The input exchange when every rank brings its own batch size (KJTAllToAll(variable_batch_size=True),
    dist_data.py:321-347, :387-394, :249-255).  `lengths` / `values` / `weights` are in send order: n_per_rank[r] features
    of B samples for destination r, val_in[r] ids of them.  Exchanges the batch sizes (one int per rank, read to the
    host), then the lengths with output splits F_local * B_r, reads the per-source id counts back in ONE D2H, starts the
    id (and weight) all-to-all and returns (batch_size_per_rank, finish); finish() waits and recats to
    [local feature][src rank][sample]: (lengths, values, weights)."""
    W, me = dist.get_world_size(pg), dist.get_rank(pg)
    F_local, dev = n_per_rank[me], lengths.device
    recv_b = torch.empty(W, dtype=torch.int32, device=dev)
    with label("## all2all_data: B ##"):  # dist_data.py:330
        dist.all_to_all_single(recv_b, torch.full((W,), B, dtype=torch.int32, device=dev), [1] * W, [1] * W, group=pg)
    bpr = [int(b) for b in recv_b.cpu().tolist()]
    len_out = [F_local * b for b in bpr]
    recv_l = torch.empty(sum(len_out), dtype=lengths.dtype, device=dev)
    with label("## all2all_data:lengths ##"):  # dist_data.py:366
        dist.all_to_all_single(recv_l, lengths.view(-1), len_out, [n * B for n in n_per_rank], group=pg)
    with label("## all2all_data:split length for a2a ##"):  # dist_data.py:388-394, one read instead of one .item() per rank
        if recv_l.numel():
            bounds = torch.tensor([0] + list(itertools.accumulate(len_out)), dtype=torch.int64, device=dev)
            cum = torch.ops.fbgemm.asynchronous_complete_cumsum(recv_l).index_select(0, bounds).cpu().tolist()
            val_out = [int(cum[r + 1] - cum[r]) for r in range(W)]
        else:
            val_out = [0] * W
    recv_v, recv_w, wait = exchange_ids(pg, values, weights, val_out, list(val_in))
    with label("## all2all_data:recat_permute_gen ##"):  # dist_data.py:67, while the ids are on the links
        recat = _get_recat(F_local, W, stagger, dev, bpr)

    def finish():
        wait()
        if recat.numel() == 0:  # no local feature, or no sample anywhere: nothing to reorder
            return recv_l, recv_v, recv_w
        with label("## all2all_data:recat_values ##"):  # dist_data.py:246
            return torch.ops.fbgemm.permute_1D_sparse_data(recat, recv_l, recv_v, recv_w, recv_v.numel())

    return bpr, finish


class _KJTValuesAwaitable(LazyAwaitable):
    def __init__(self, fn) -> None:
        super().__init__()
        self._fn = fn

    def _wait_impl(self) -> KeyedJaggedTensor:
        return self._fn()


class KJTAllToAll(nn.Module):
    """Redistributes a KJT so that rank r receives, from every rank, the features
    `splits[r]` owns.  `forward(kjt).wait()` has exchanged the lengths (and read the value counts
    back, dist_data.py:396-398); `.wait().wait()` is the KJT with keys = this rank's features and
    stride = sum of the ranks' batch sizes."""

    def __init__(self, pg: dist.ProcessGroup, splits: List[int], device: Optional[torch.device] = None,
                 stagger: int = 1, variable_batch_size: bool = False) -> None:
        super().__init__()
        assert len(splits) == dist.get_world_size(pg)
        self._pg, self._splits, self._stagger = pg, list(splits), stagger
        self._variable_batch_size = variable_batch_size
        self._W, self._me = dist.get_world_size(pg), dist.get_rank(pg)
        self._recat = _get_recat(splits[self._me], self._W, stagger, device)

    def forward(self, kjt: KeyedJaggedTensor) -> Awaitable[Awaitable[KeyedJaggedTensor]]:
        W, me, pg = self._W, self._me, self._pg
        B = kjt.stride()
        F_local = self._splits[me]
        lengths, values, weights = kjt.lengths(), kjt.values(), kjt.weights_or_none()
        keys = kjt.keys()
        start = sum(self._splits[:me])
        local_keys = keys[start:start + F_local]
        val_in = ids_per_destination(kjt.length_per_key(), self._splits)
        if self._variable_batch_size:
            bpr, finish_var = variable_batch_exchange(pg, self._splits, val_in, lengths, values, weights, B, self._stagger)

            def finish_variable() -> KeyedJaggedTensor:
                l2, v2, w2 = finish_var()
                return KeyedJaggedTensor(keys=local_keys, values=v2, weights=w2, lengths=l2, stride=sum(bpr))

            return NoWait(_KJTValuesAwaitable(finish_variable))
        len_in = [s * B for s in self._splits]
        recv_l = torch.empty(W * F_local * B, dtype=lengths.dtype, device=lengths.device)
        dist.all_to_all_single(recv_l, lengths, [F_local * B] * W, len_in, group=pg)
        val_out = recv_l.view(W, -1).sum(dim=1).cpu().tolist()
        recv_v, recv_w, wait = exchange_ids(pg, values, weights, val_out, val_in)

        def finish() -> KeyedJaggedTensor:
            wait()
            if F_local == 0:
                return KeyedJaggedTensor(keys=[], values=recv_v, weights=recv_w, lengths=recv_l, stride=W * B)
            l2, v2, w2 = torch.ops.fbgemm.permute_2D_sparse_data(
                self._recat.to(recv_l.device), recv_l.view(W * F_local, B), recv_v, recv_w, recv_v.numel())
            return KeyedJaggedTensor(keys=local_keys, values=v2, weights=w2, lengths=l2.view(-1), stride=W * B)

        return NoWait(_KJTValuesAwaitable(finish))


class PooledEmbeddingsAllToAll(nn.Module):
    def __init__(self, pg: dist.ProcessGroup, dim_sum_per_rank: List[int], device: Optional[torch.device] = None,
                 callbacks=None) -> None:
        super().__init__()
        self._pg, self._dims = pg, list(dim_sum_per_rank)
        self._callbacks = callbacks or []
        self.register_buffer("_dim_sum_per_rank_tensor", torch.tensor(dim_sum_per_rank, dtype=torch.int32, device=device),
                             persistent=False)

    def forward(self, local_embs: torch.Tensor, batch_size_per_rank: Optional[List[int]] = None) -> Awaitable[torch.Tensor]:
        W = dist.get_world_size(self._pg)
        if batch_size_per_rank is None:
            batch_size_per_rank = [local_embs.shape[0] // W] * W
        from .comm_ops import alltoall_pooled  # (not at module level: comm_ops -> embeddingbag -> this module)

        aw = alltoall_pooled(local_embs, batch_size_per_rank, self._dims, self._dim_sum_per_rank_tensor, None, self._pg)
        if not self._callbacks:
            return aw
        cbs = self._callbacks

        class _CB(LazyAwaitable):
            def _wait_impl(self_inner):
                out = aw.wait()
                for cb in cbs:
                    out = cb(out)
                return out

        return _CB()


class PooledEmbeddingsReduceScatter(nn.Module):
    def __init__(self, pg: dist.ProcessGroup) -> None:
        super().__init__()
        self._pg = pg

    def forward(self, local_embs: torch.Tensor) -> Awaitable[torch.Tensor]:
        W = dist.get_world_size(self._pg)
        B_l = local_embs.shape[0] // W
        from .comm_ops import reduce_scatter_pooled  # (see PooledEmbeddingsAllToAll.forward)

        return reduce_scatter_pooled([local_embs[r * B_l:(r + 1) * B_l] for r in range(W)], self._pg)
