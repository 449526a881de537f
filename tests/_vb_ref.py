"""TEST-ONLY: numpy restatements of the two index ops of the variable-batch input exchange
(``torch.ops.fbgemm.expand_into_jagged_permute`` / ``permute_1D_sparse_data``) and the reference's recat recipe
(torchrec/distributed/dist_data.py:83-116) over them.  `register()` adds CPU implementations of just these two ops for
host-logic tests on CPU tensors (tests/_cpu_ops.py supplies the others); the product registers the HIP key only."""
import numpy as np
import torch

import _paths  # noqa: F401
import fbgemm_gpu  # noqa: F401  (defines the op schemas)

_lib = torch.library.Library("fbgemm", "IMPL", "CPU")
_registered = False


def expand_into_jagged_permute(permute, input_offset, output_offset, output_size):
    """out[output_offset[i] + k] = input_offset[permute[i]] + k for k < output_offset[i + 1] - output_offset[i]."""
    permute, input_offset, output_offset = (np.asarray(a) for a in (permute, input_offset, output_offset))
    out = np.zeros(output_size, dtype=permute.dtype)
    for i in range(permute.size):
        n = int(output_offset[i + 1] - output_offset[i])
        out[int(output_offset[i]):int(output_offset[i]) + n] = int(input_offset[permute[i]]) + np.arange(n)
    return out


def permute_1d(permute, lengths, values, weights=None):
    """out_lengths[i] = lengths[permute[i]]; segment i of the output is segment permute[i] of the input."""
    permute, lengths, values = np.asarray(permute), np.asarray(lengths), np.asarray(values)
    offs = np.concatenate([[0], np.cumsum(lengths.astype(np.int64))])
    out_lengths = lengths[permute] if permute.size else lengths[:0]
    pick = (np.concatenate([np.arange(offs[p], offs[p + 1]) for p in permute]) if permute.size
            else np.zeros(0)).astype(np.int64)
    return out_lengths, values[pick], (np.asarray(weights)[pick] if weights is not None else None)


def recat(local_split, num_splits, batch_size_per_rank, stagger=1):
    """The element-level recat of dist_data.py:83-116 as a numpy int32 array."""
    order = [x + num_splits // stagger * y for x in range(num_splits // stagger) for y in range(stagger)]
    perm = [i + j * local_split for i in range(local_split) for j in order]
    if local_split == 0:
        return np.zeros(0, dtype=np.int32)
    per_feature = [b for b in batch_size_per_rank for _ in range(local_split)]
    in_off = np.concatenate([[0], np.cumsum(per_feature)]).astype(np.int32)
    out_off = np.concatenate([[0], np.cumsum([per_feature[r] for r in perm])]).astype(np.int32)
    return expand_into_jagged_permute(np.asarray(perm, dtype=np.int32), in_off, out_off, int(out_off[-1]))


def _expand_cpu(permute, input_offset, output_offset, output_size):
    return torch.from_numpy(expand_into_jagged_permute(permute.numpy(), input_offset.numpy(), output_offset.numpy(), output_size))


def _permute_1d_cpu(permute, lengths, values, weights=None, permuted_lengths_sum=None):
    l, v, w = permute_1d(permute.numpy(), lengths.numpy(), values.contiguous().numpy(),
                         weights.contiguous().numpy() if weights is not None else None)
    return (torch.from_numpy(np.ascontiguousarray(l)), torch.from_numpy(np.ascontiguousarray(v)),
            torch.from_numpy(np.ascontiguousarray(w)) if w is not None else None)


def register() -> None:
    global _registered
    if _registered:
        return
    _lib.impl("expand_into_jagged_permute", _expand_cpu)
    _lib.impl("permute_1D_sparse_data", _permute_1d_cpu)
    _registered = True
