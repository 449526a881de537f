"""CPU: a different batch size per rank through the KJT and the pooled-embedding exchange — the host logic of
KJTAllToAll(variable_batch_size=True), PooledEmbeddingsAllToAll(local_embs, batch_size_per_rank) and
ShardedEmbeddingBagCollection(variable_batch_size=True) over gloo, against the vectors the reference's own test generators
lay out (tests/golden/vb_dist_data.npz, tests/golden/make_vb_golden.py) and the unsharded oracle.  The two index ops of the
recat run as their numpy restatements here (tests/_vb_ref.py); tests/test_variable_batch_gpu.py pins the HIP kernels on them."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _paths  # noqa: F401
import _vb_ref
import _vb_sharded
from test_sharded_gloo import DIMS, ROWS, _free_port


def _received(z, case, rank):
    """What rank `rank` holds after the lengths / ids exchange: [src rank][local feature][sample], from the golden inputs."""
    W, splits, bpr = len(case["splits"]), case["splits"], case["batch_size_per_rank"]
    f0, F_local = sum(splits[:rank]), splits[rank]
    lengths, values, weights = [], [], []
    for s in range(W):
        l, v, w = (t.numpy() if t is not None else None for t in _vb_sharded.golden_kjt(z, case, s, "in"))
        offs = np.concatenate([[0], np.cumsum(l)])
        a, b = f0 * bpr[s], (f0 + F_local) * bpr[s]
        lengths.append(l[a:b])
        values.append(v[offs[a]:offs[b]])
        if w is not None:
            weights.append(w[offs[a]:offs[b]])
    return np.concatenate(lengths), np.concatenate(values), (np.concatenate(weights) if case["weighted"] else None)


def test_restatement_and_recat_recipe_turn_golden_inputs_into_golden_outputs():
    z, meta = _vb_sharded.golden()
    assert {len(c["splits"]) for c in meta["kjt"]} == {2, 3}
    assert any(0 in c["batch_size_per_rank"] for c in meta["kjt"]) and any(0 in c["splits"] for c in meta["kjt"])
    assert any(len(set(c["batch_size_per_rank"])) == 1 for c in meta["kjt"])
    for case in meta["kjt"]:
        W, bpr = len(case["splits"]), case["batch_size_per_rank"]
        for r in range(W):
            lengths, values, weights = _received(z, case, r)
            recat = _vb_ref.recat(case["splits"][r], W, bpr)
            assert recat.size == case["splits"][r] * sum(bpr)
            l2, v2, w2 = _vb_ref.permute_1d(recat, lengths, values, weights)
            want = [t.numpy() if t is not None else None for t in _vb_sharded.golden_kjt(z, case, r, "out")]
            np.testing.assert_array_equal(l2, want[0])
            np.testing.assert_array_equal(v2, want[1])
            if case["weighted"]:
                np.testing.assert_array_equal(w2, want[2])


@pytest.mark.parametrize("local_split,W,stagger,bpr", [(2, 4, 1, [3, 0, 2, 5]), (2, 4, 2, [1, 2, 3, 4]), (3, 2, 1, [4, 4]),
                                                       (1, 3, 1, [0, 0, 0]), (0, 3, 1, [2, 1, 0]), (5, 3, 1, [70, 1, 64])])
def test_get_recat_with_batch_sizes_equals_the_restatement(local_split, W, stagger, bpr):
    from torchrec_amd.distributed.dist_data import _get_recat

    _vb_ref.register()
    got = _get_recat(local_split, W, stagger, torch.device("cpu"), bpr)
    assert got.dtype == torch.int32
    want = _vb_ref.recat(local_split, W, bpr, stagger)
    np.testing.assert_array_equal(got.numpy(), want)
    assert sorted(want.tolist()) == list(range(local_split * sum(bpr)))  # a permutation of the received elements


def test_get_recat_without_batch_sizes_is_unchanged():
    from torchrec_amd.distributed.dist_data import _get_recat

    assert _get_recat(2, 4, 1).tolist() == [0, 2, 4, 6, 1, 3, 5, 7]  # dist_data.py:62-65
    assert _get_recat(2, 4, 2).tolist() == [0, 4, 2, 6, 1, 5, 3, 7]
    assert _get_recat(2, 4, 1).dtype == torch.int32


def _init(rank, W, port):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    import _cpu_ops

    _cpu_ops.register()
    _vb_ref.register()


def _golden_worker(rank, W, port, ret):
    _init(rank, W, port)
    try:
        z, meta = _vb_sharded.golden()
        ret[rank] = _vb_sharded.run_golden_exchanges(z, meta, W, rank, dist.group.WORLD, torch.device("cpu"))
        from torchrec_amd.distributed.dist_data import PooledEmbeddingsAllToAll

        with pytest.raises(ValueError, match=r"7 rows.*sums to 8"):
            PooledEmbeddingsAllToAll(dist.group.WORLD, [4] * W, torch.device("cpu"))(torch.zeros(7, 4), [8] + [0] * (W - 1))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("W", [2, 3])
def test_kjt_and_pooled_all_to_all_give_the_golden_results_over_gloo(W):
    """Keys, lengths, values, weights and stride of KJTAllToAll(variable_batch_size=True) on every rank; output and input
    gradient of PooledEmbeddingsAllToAll with batch_size_per_rank; the row-count check raises ValueError with both numbers."""
    from _results import ResultStore

    ret = ResultStore()
    mp.spawn(_golden_worker, args=(W, _free_port(), ret), nprocs=W, join=True)
    z, meta = _vb_sharded.golden()
    assert _vb_sharded.check_golden_exchanges(z, meta, W, ret) >= 4 * W


BATCHES = [5, 0, 2]
# t0 column-wise in two 4-wide shards, t1 replicated, t3 table-column-wise, the others table-wise
SHARDING = {0: "column_wise", 1: "data_parallel", 3: "table_column_wise"}


def _build(W, rank, weighted, mean_tables, variable=True, sharding=SHARDING, env=None):
    from _cw_sharded import LR, tables_and_plan
    from _oracle_tbe import oracle_dp_tbe_factory, oracle_tbe_factory
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    tables, plan = tables_and_plan(W, ROWS, DIMS, sharding, "cpu", mean_tables, {0: 4, 3: 4})
    ebc = EmbeddingBagCollection(tables, is_weighted=weighted, device=torch.device("meta"))
    env = env if env is not None else ShardingEnv.from_local(W, rank)
    return plan, ShardedEmbeddingBagCollection(ebc, plan, env, {"learning_rate": LR}, torch.device("cpu"),
                                               tbe_factory=oracle_tbe_factory, dp_tbe_factory=oracle_dp_tbe_factory,
                                               variable_batch_size=variable)


def _sharded_worker(rank, W, port, fixed_len, weighted, mean_tables, ret):
    _init(rank, W, port)
    try:
        from _cw_sharded import load_init, train_step
        from torchrec_amd.distributed.types import ShardingEnv

        plan, sebc = _build(W, rank, weighted, mean_tables, env=ShardingEnv.from_process_group(dist.group.WORLD))
        assert sebc._variable_batch and not sebc.explicit_step_supported(BATCHES[rank])
        per_rank, init = _vb_sharded.data(BATCHES, ROWS, DIMS, fixed_len, weighted)
        load_init(sebc, init)

        def all_reduce(g):
            dist.all_reduce(g)
            return g

        ret[rank] = train_step(sebc, per_rank, rank, W, fixed_len, weighted, torch.device("cpu"), all_reduce)
        if rank == 0:
            ret["kinds"] = {n: p.sharding_type for n, p in plan.items()}
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("fixed_len,weighted,mean_tables", [(0, True, (2, 3)), (1, False, ())])
def test_variable_batch_sharded_collection_equals_unsharded_world3(fixed_len, weighted, mean_tables):
    """Batches [5, 0, 2] at W = 3, column-wise + table-wise + replicated tables, SUM and mixed SUM / MEAN: forward of every
    rank and the tables after one SGD step equal the unsharded oracle on the concatenated batch."""
    from _results import ResultStore

    W = len(BATCHES)
    ret = ResultStore()
    mp.spawn(_sharded_worker, args=(W, _free_port(), fixed_len, weighted, mean_tables, ret), nprocs=W, join=True)
    kinds = ret["kinds"]
    assert kinds["t0"] == "column_wise" and kinds["t1"] == "data_parallel" and kinds["t2"] == "table_wise"
    per_rank, init = _vb_sharded.data(BATCHES, ROWS, DIMS, fixed_len, weighted)
    _vb_sharded.check_against_unsharded(ret, BATCHES, ROWS, DIMS, per_rank, init, fixed_len, weighted, kinds, mean_tables,
                                        bit_exact=False)


def test_variable_batch_refusals_raise_by_name():
    _, sebc = _build(2, 0, False, ())
    assert sebc._variable_batch
    with pytest.raises(NotImplementedError, match="set_graph_exchange"):
        sebc.set_graph_exchange(4)
    with pytest.raises(NotImplementedError, match="set_half_batch_exchange"):
        sebc.set_half_batch_exchange(True)
    sebc.set_half_batch_exchange(False)
    assert sebc.set_graph_exchange(None) is None
    assert sebc.explicit_step_supported(4) is False
    with pytest.raises(NotImplementedError, match="t3.*row_wise"):
        _build(2, 0, False, (), sharding={3: "row_wise"})
    # a module that exchanges nothing: the flag changes nothing
    _, one = _build(1, 0, False, (), sharding={})
    assert one._variable_batch is False and one._emb_module._W == 0
    _, fixed = _build(2, 0, False, (), variable=False)
    assert fixed._variable_batch is False and fixed._emb_module._W == 2 and sebc._emb_module._W == 0
    assert len(fixed._emb_module.tables.ftm) == 2 * len(sebc._emb_module.tables.ftm)


def test_sharder_passes_the_flag_through():
    from _cw_sharded import tables_and_plan
    from _oracle_tbe import oracle_dp_tbe_factory, oracle_tbe_factory
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    tables, plan = tables_and_plan(2, ROWS, DIMS, SHARDING, "cpu", (), {0: 4, 3: 4})
    ebc = EmbeddingBagCollection(tables, device=torch.device("meta"))
    for flag in (False, True):
        sharder = EmbeddingBagCollectionSharder({"learning_rate": 0.1}, oracle_tbe_factory, oracle_dp_tbe_factory,
                                                variable_batch_size=flag)
        assert sharder.shard(ebc, plan, ShardingEnv.from_local(2, 1), torch.device("cpu"))._variable_batch is flag
    assert EmbeddingBagCollectionSharder().variable_batch_size is False
