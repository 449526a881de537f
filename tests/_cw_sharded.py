"""Shared by the column-wise sharding tests (CPU over gloo with the oracle lookup, GPU with the real kernels): one
collection that mixes column-wise, row-wise, table-wise and replicated tables, its inputs, and the unsharded oracle run
it must equal.  Follows tests/test_sharded_gloo.py / tests/test_multirank_gpu.py (sharded-vs-unsharded equivalence after
one train step, torchrec/distributed/test_utils/test_model_parallel_base.py:148-294)."""
import numpy as np
import torch

import _paths  # noqa: F401

LR = 0.25


def tables_and_plan(W, rows, dims, sharding, device_type="cuda", mean_tables=(), min_partition=None):
    """sharding: table number -> sharding type (tables not named are table-wise); min_partition: table -> shard width."""
    from torchrec_amd.distributed.planner import EmbeddingShardingPlanner, ParameterConstraints, Topology
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig, PoolingType

    min_partition = min_partition or {}
    tables = [EmbeddingBagConfig(name=f"t{i}", embedding_dim=dims[i], num_embeddings=rows[i], feature_names=[f"f{i}"],
                                 pooling=PoolingType.MEAN if i in mean_tables else PoolingType.SUM) for i in range(len(rows))]
    cons = {f"t{i}": ParameterConstraints(sharding_types=[sharding.get(i, "table_wise")], min_partition=min_partition.get(i))
            for i in range(len(rows))}
    plan = EmbeddingShardingPlanner(Topology(W, device_type), constraints=cons, dp_max_rows=0).plan_tables(tables)
    return tables, plan


def data(W, B_local, rows, dims, fixed_len, weighted, seed=11, max_len=3):
    rng = np.random.default_rng(seed)
    F = len(rows)
    per_rank = []
    for _ in range(W):
        lengths = (np.full(F * B_local, fixed_len) if fixed_len else rng.integers(0, max_len + 1, size=F * B_local)).astype(np.int32)
        vals = np.concatenate([rng.integers(0, rows[f], size=int(lengths[f * B_local:(f + 1) * B_local].sum()))
                               for f in range(F)]).astype(np.int64)
        wts = (rng.random(vals.size).astype(np.float32) + 0.5) if weighted else None
        grad = rng.standard_normal((B_local, sum(dims))).astype(np.float32)
        per_rank.append((lengths, vals, wts, grad))
    init = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, dims)]
    return per_rank, init


def load_init(sebc, init):
    """The global initial tables into the local pieces / replicas."""
    with torch.no_grad():
        for name, w, row0, col0 in sebc.local_shard_pieces():
            w.copy_(torch.from_numpy(init[int(name[1:])][row0:row0 + w.shape[0], col0:col0 + w.shape[1]]))
        for name, w in sebc.dp_tables().items():
            w.copy_(torch.from_numpy(init[int(name[1:])]))


def pieces_of(sebc):
    return [(n, w.detach().cpu().numpy().copy(), r0, c0) for n, w, r0, c0 in sebc.local_shard_pieces()]


def train_step(sebc, per_rank, rank, W, fixed_len, weighted, device, all_reduce):
    """One forward + backward (+ the dense SGD step of the replicated tables); returns (output, pieces, replicas)."""
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    lengths, vals, wts, grad = per_rank[rank]
    keys = [f"f{i}" for i in range(len(sebc.embedding_bag_configs))]
    wt = torch.from_numpy(wts).to(device) if weighted else None
    if fixed_len:
        kjt = KeyedJaggedTensor.from_fixed_lengths(keys, torch.from_numpy(vals).to(device), [fixed_len] * len(keys), weights=wt)
    else:
        kjt = KeyedJaggedTensor.from_lengths_sync(keys, torch.from_numpy(vals).to(device), torch.from_numpy(lengths).to(device),
                                                  weights=wt)
    out = sebc(kjt).wait()
    assert out.keys() == keys
    assert out.length_per_key() == [c.embedding_dim for c in sebc.embedding_bag_configs]  # per FEATURE, at full D
    vals_out = out.values()
    vals_out.backward(torch.from_numpy(grad).to(device))
    if device.type == "cuda":
        torch.cuda.synchronize()
    replicas = {}
    if sebc._dp_module is not None:
        g = all_reduce(sebc._dp_module.weights.grad.detach().clone()) / W
        with torch.no_grad():
            sebc._dp_module.weights -= LR * g
        replicas = {n: w.detach().cpu().numpy().copy() for n, w in sebc.dp_tables().items()}
    return vals_out.detach().cpu().numpy().copy(), pieces_of(sebc), replicas


def global_batch(per_rank, W, B, F, weighted):
    """The ranks' batches as ONE batch: rank-major concatenation per feature; gradients / W (comm_ops.py:527-528)."""
    g_len = np.concatenate([np.concatenate([per_rank[r][0][f * B:(f + 1) * B] for r in range(W)]) for f in range(F)])
    pos = [np.concatenate([[0], np.cumsum(per_rank[r][0])]) for r in range(W)]
    cat = lambda i: np.concatenate([np.concatenate([per_rank[r][i][pos[r][f * B]:pos[r][(f + 1) * B]]  # noqa: E731
                                                    for r in range(W)]) for f in range(F)])
    g_vals, g_w = cat(1), (cat(2) if weighted else None)
    g_grad = np.ascontiguousarray(np.concatenate([per_rank[r][3] for r in range(W)], axis=0) / W, dtype=np.float32)
    g_offs = np.concatenate([[0], np.cumsum(g_len)]).astype(np.int64)
    return g_vals, g_offs, g_w, g_grad


def check_against_unsharded(ret, W, B, rows, dims, per_rank, init, fixed_len, weighted, plan_kinds, mean_tables=()):
    """ret[r] = (output, pieces, replicas).  Forward of every rank and the SGD-updated tables against the unsharded
    oracle; every element of every sharded table lives in exactly one piece, replicated tables on every rank."""
    from _util import oracle_backward_mixed, oracle_forward_mixed
    from oracle import oracle

    F = len(rows)
    feat_mean = [i in mean_tables for i in range(F)]
    tabs = oracle.Tables(rows, dims)
    for t in range(F):
        tabs.weights[t][...] = init[t]
    for r in range(W):
        lengths, vals, wts, _ = per_rank[r]
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        ref = oracle_forward_mixed(tabs, vals, offs, wts, feat_mean)
        if fixed_len == 1 and not weighted:
            np.testing.assert_array_equal(ret[r][0], ref)  # pure gather: bit-exact through the whole exchange
        else:
            np.testing.assert_allclose(ret[r][0], ref, rtol=1e-5, atol=1e-5)
    g_vals, g_offs, g_w, g_grad = global_batch(per_rank, W, B, F, weighted)
    oracle_backward_mixed(tabs, g_vals, g_offs, g_grad, oracle.OPT_EXACT_SGD, LR, g_w, feat_mean)
    seen = {t: np.zeros((rows[t], dims[t]), dtype=np.int32) for t in range(F)}
    for r in range(W):
        for name, w, row0, col0 in ret[r][1]:
            t = int(name[1:])
            np.testing.assert_allclose(w, tabs.weights[t][row0:row0 + w.shape[0], col0:col0 + w.shape[1]], rtol=3e-5, atol=3e-5)
            seen[t][row0:row0 + w.shape[0], col0:col0 + w.shape[1]] += 1
        for name, w in ret[r][2].items():
            np.testing.assert_allclose(w, tabs.weights[int(name[1:])], rtol=3e-5, atol=3e-5)
    for t in range(F):
        if plan_kinds[f"t{t}"] == "data_parallel":
            assert all(f"t{t}" in ret[r][2] for r in range(W)) and not seen[t].any()
        else:
            assert (seen[t] == 1).all(), f"t{t}: every element of a sharded table lives in exactly one piece"
