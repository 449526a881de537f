"""Variable-batch exchange vectors as the REFERENCE's own test generators lay them out
(torchrec/distributed/tests/test_dist_data.py:58-168 `_generate_sparse_features_batch` / `_generate_pooled_embedding_batch`),
recorded by importing the reference here (build container only).  The generators are plain Python + torch: their expected
outputs depend on no op of this repository.  The module's `_to_tensor` puts its tensors on a GPU; it is swapped for a CPU
one.  KeyedJaggedTensor only carries the generators' tensors, and the reference's cannot carry a local batch of 0 (its
length_per_key reshapes to [-1, stride]); it is swapped for a plain carrier, so that lists with a 0 can be recorded.
The KJT generator never draws weights (its `if weights:` tests an empty dict), so the weighted cases run it a second time
on the same seed with the ids replaced by a running count: where the generator puts id n in the expected output is where
the weight of input position n belongs.
Output: tests/golden/vb_dist_data.npz (data only): per case and rank the inputs and the expected outputs of
KJTAllToAll(variable_batch_size=True) and PooledEmbeddingsAllToAll(local_embs, batch_size_per_rank); for the pooled cases also
the expected input gradient of the output gradient the reference's test feeds (`res.backward(res)`: :362-370, input / W)."""
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REFERENCE = "/root/reference"

# (name, features, splits, batch_size_per_rank, weighted)
KJT_CASES = [
    ("w2_unequal", 3, [2, 1], [3, 5], False),
    ("w2_empty_share_zero_batch", 4, [0, 4], [4, 0], True),
    ("w2_equal", 3, [1, 2], [2, 2], True),
    ("w3_empty_share_zero_batch", 5, [2, 0, 3], [5, 0, 2], True),
    ("w3_equal", 4, [1, 2, 1], [3, 3, 3], False),
    ("w3_all_zero", 4, [2, 1, 1], [0, 0, 0], False),
]
# (name, dims per feature, splits, batch_size_per_rank)
POOLED_CASES = [
    ("w2_unequal", [8, 16, 4], [2, 1], [3, 5]),
    ("w2_empty_share_zero_batch", [4, 8, 12], [0, 3], [4, 0]),
    ("w2_equal_odd_dims", [3, 5, 6], [1, 2], [2, 2]),
    ("w3_empty_share_zero_batch", [8, 4, 4, 16, 8], [2, 0, 3], [5, 0, 2]),
    ("w3_equal", [4, 8, 4, 12], [1, 2, 1], [3, 3, 3]),
]


def main():
    import _paths  # noqa: F401
    import _cpu_ops

    pe = types.ModuleType("pyre_extensions")
    pe.none_throws = lambda x, msg=None: x

    class _PS:
        def __init__(self, name):
            self.args = object
            self.kwargs = object

    pe.ParameterSpecification = _PS
    sys.modules["pyre_extensions"] = pe
    _cpu_ops.register()
    sys.path.insert(0, REFERENCE)
    import torch
    from torchrec.distributed.tests import test_dist_data as ref

    class _NoElements:
        """What `_to_tensor` gives for no elements: the pooled generator's `.view(0, -1)` of a rank with a local batch of 0
        is ambiguous for a tensor."""

        def view(self, *shape):
            return torch.empty([0 if n == -1 else n for n in shape], dtype=torch.float32)

    def _to_tensor(iterator, device_id, dtype):
        flat = list(ref._flatten(iterator))
        return torch.tensor(flat, dtype=dtype) if flat or dtype != torch.float else _NoElements()

    ref._to_tensor = _to_tensor

    class _Carrier:
        def __init__(self, keys, lengths, values, weights):
            self._k, self._l, self._v, self._w = list(keys), lengths, values, weights

        @staticmethod
        def from_lengths_sync(keys, values, lengths, weights=None):
            return _Carrier(keys, lengths, values, weights)

        keys = lambda self: self._k  # noqa: E731
        lengths = lambda self: self._l  # noqa: E731
        values = lambda self: self._v  # noqa: E731
        weights = lambda self: self._w  # noqa: E731

    ref.KeyedJaggedTensor = _Carrier

    class _Random:
        """The module's `random`: the same stream, but with `counting` the ids (randint(0, 1000)) become 0, 1, 2, ..."""
        counting, n = False, 0

        def randint(self, a, b):
            x = random.randint(a, b)
            if self.counting and (a, b) == (0, 1000):
                self.n += 1
                return self.n - 1
            return x

        def random(self):
            return random.random()

    ref.random = shim = _Random()
    torch.Tensor.cuda = lambda self, *a, **k: self  # the generator's empty-share branch: torch.empty(B, 0).cuda(i)
    out, meta = {}, {"kjt": [], "pooled": []}
    for n, (name, features, splits, bpr, weighted) in enumerate(KJT_CASES):
        random.seed(1000 + n)
        keys = [f"F{i}" for i in range(features)]
        ins, outs = ref._generate_sparse_features_batch(keys=keys, splits=splits, batch_size_per_rank=bpr, is_weighted=weighted)
        meta["kjt"].append({"name": name, "keys": keys, "splits": splits, "batch_size_per_rank": bpr, "weighted": weighted,
                            "out_keys": [list(o.keys()) for o in outs]})
        for r, (i, o) in enumerate(zip(ins, outs)):
            for tag, k in (("in", i), ("out", o)):
                out[f"kjt/{name}/r{r}/{tag}_lengths"] = k.lengths().numpy().astype(np.int32)
                out[f"kjt/{name}/r{r}/{tag}_values"] = k.values().numpy().astype(np.int32)
        if weighted:
            random.seed(1000 + n)
            shim.counting, shim.n = True, 0
            pos_in, pos_out = ref._generate_sparse_features_batch(keys=keys, splits=splits, batch_size_per_rank=bpr)
            shim.counting = False
            rng = np.random.default_rng(1000 + n)
            w_of = np.zeros(shim.n, dtype=np.float32)  # weight of id-count position
            for r, i in enumerate(pos_in):
                ids = i.values().numpy().astype(np.int64)
                assert np.array_equal(i.lengths().numpy(), out[f"kjt/{name}/r{r}/in_lengths"])
                w_of[ids] = rng.random(ids.size, dtype=np.float32)
                out[f"kjt/{name}/r{r}/in_weights"] = w_of[ids]
            for r, o in enumerate(pos_out):
                out[f"kjt/{name}/r{r}/out_weights"] = w_of[o.values().numpy().astype(np.int64)]
    for n, (name, dims, splits, bpr) in enumerate(POOLED_CASES):
        random.seed(2000 + n)
        keys = [f"F{i}" for i in range(len(dims))]
        ins, outs = ref._generate_pooled_embedding_batch(keys=keys, dims=dims, splits=splits, batch_size_per_rank=bpr)
        W = len(splits)
        off = np.concatenate([[0], np.cumsum(splits)])
        meta["pooled"].append({"name": name, "dims": dims, "splits": splits, "batch_size_per_rank": bpr,
                               "dim_sum_per_rank": [int(sum(dims[off[r]:off[r + 1]])) for r in range(W)]})
        for r, (i, o) in enumerate(zip(ins, outs)):
            i, o = i.float(), o.float().reshape(bpr[r], sum(dims))
            out[f"pooled/{name}/r{r}/in"] = i.numpy()
            out[f"pooled/{name}/r{r}/out"] = o.numpy()
            out[f"pooled/{name}/r{r}/grad_out"] = o.numpy()  # res.backward(res)
            out[f"pooled/{name}/r{r}/grad_in"] = i.clone().div_(W).numpy()  # test_dist_data.py:367-370
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(sys.argv[1] if len(sys.argv) > 1 else HERE, "vb_dist_data.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(KJT_CASES), "KJT cases,", len(POOLED_CASES), "pooled cases")


if __name__ == "__main__":
    main()
