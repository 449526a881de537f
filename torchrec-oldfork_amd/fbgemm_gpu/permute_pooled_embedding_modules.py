"""PermutePooledEmbeddings: the callback the reference's column-wise sharding hands to its pooled all-to-all
(torchrec/distributed/sharding/cw_sharding.py:12, :221-231) to put the column shards of a table, which arrive grouped by
rank, back next to each other.  One HIP launch per call (csrc/permute_pooled.hip) through
``torch.ops.fbgemm.permute_pooled_embs_auto_grad``; the backward is the same kernel with the inverse permutation."""
from itertools import accumulate
from typing import List, Optional

import torch
from torch import nn

from . import _ops


class PermutePooledEmbeddings(nn.Module):
    """``embs_dims[t]`` is the width of column segment t of the input [B, sum(embs_dims)]; segment i of the output is
    segment ``permute[i]`` of the input.  ``permute`` must be a permutation of range(len(embs_dims))."""

    def __init__(self, embs_dims: List[int], permute: List[int], device: Optional[torch.device] = None) -> None:
        super().__init__()
        dims, perm = [int(d) for d in embs_dims], [int(p) for p in permute]
        if any(d < 0 for d in dims):
            raise ValueError(f"PermutePooledEmbeddings: negative dim in {dims}")
        if len(perm) != len(dims) or sorted(perm) != list(range(len(dims))):
            raise ValueError(f"PermutePooledEmbeddings: permute {perm} is not a permutation of range({len(dims)})")
        if not dims:
            raise ValueError("PermutePooledEmbeddings: no segments")
        inv_perm = [0] * len(perm)
        for i, p in enumerate(perm):
            inv_perm[p] = i
        offsets = [0] + list(accumulate(dims))
        inv_offsets = [0] + list(accumulate(dims[p] for p in perm))
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # buffers (not persistent: they are functions of the constructor's arguments), so that .to(device=...) moves them
        for name, vals in (("_offset_dim_list", offsets), ("_permute", perm), ("_inv_offset_dim_list", inv_offsets),
                           ("_inv_permute", inv_perm)):
            self.register_buffer(name, torch.tensor(vals, dtype=torch.int64, device=dev), persistent=False)
        self._vec = all(d % 4 == 0 for d in dims)
        self._seed_vec_hint()

    def _seed_vec_hint(self) -> None:
        # the op would otherwise read the two offset lists back once to learn whether the 16-B path applies
        _ops.note_offsets_multiple_of_4(self._offset_dim_list, self._vec)
        _ops.note_offsets_multiple_of_4(self._inv_offset_dim_list, self._vec)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._seed_vec_hint()  # .to() / .cuda() replaced the buffers
        return out

    def forward(self, pooled_embs: torch.Tensor) -> torch.Tensor:
        return torch.ops.fbgemm.permute_pooled_embs_auto_grad(
            pooled_embs, self._offset_dim_list, self._permute, self._inv_offset_dim_list, self._inv_permute)
