"""CPU, world_size 2 (gloo): column-wise tables in ShardedEmbeddingBagCollection — the bookkeeping in units of pieces
(feature, column shard) — against the unsharded oracle, with the oracle lookup standing in for the kernels
(tests/_oracle_tbe.py).  One collection mixes a column-wise table with two pieces on each rank (D = 128, 4 shards), a
3-shard one (D = 100), a row-wise, a table-wise and a replicated table.  Plus the state surface: state_dict round trips,
the sharding-invariant reset, the fused optimizer's state keys, and the combinations that must raise."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _paths  # noqa: F401
from test_sharded_gloo import _free_port

ROWS = [40, 7, 23, 90, 5]
DIMS = [128, 100, 8, 16, 8]
SHARDING = {0: "column_wise", 1: "table_column_wise", 2: "table_wise", 3: "row_wise", 4: "data_parallel"}
B_LOCAL = 6
W = 2


def _build(env, weighted, sharding=SHARDING, mean_tables=(), fused=None):
    import _cpu_ops
    _cpu_ops.register()
    from _cw_sharded import LR, tables_and_plan
    from _oracle_tbe import oracle_dp_tbe_factory, oracle_tbe_factory
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    tables, plan = tables_and_plan(env.world_size, ROWS, DIMS, sharding, "cpu", mean_tables)
    ebc = EmbeddingBagCollection(tables, is_weighted=weighted, device=torch.device("meta"))
    sebc = ShardedEmbeddingBagCollection(ebc, plan, env, dict({"learning_rate": LR}, **(fused or {})), torch.device("cpu"),
                                         tbe_factory=oracle_tbe_factory, dp_tbe_factory=oracle_dp_tbe_factory)
    return plan, sebc


def _worker(rank, port, fixed_len, weighted, mean_tables, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    try:
        from _cw_sharded import data, load_init, train_step
        from torchrec_amd.distributed.types import ShardingEnv

        plan, sebc = _build(ShardingEnv.from_process_group(dist.group.WORLD), weighted, mean_tables=mean_tables)
        per_rank, init = data(W, B_LOCAL, ROWS, DIMS, fixed_len, weighted)
        load_init(sebc, init)

        def all_reduce(g):
            dist.all_reduce(g)
            return g

        out, pieces, replicas = train_step(sebc, per_rank, rank, W, fixed_len, weighted, torch.device("cpu"), all_reduce)
        ret[rank] = (out, pieces, replicas)
        ret["kinds"] = {n: p.sharding_type for n, p in plan.items()}
        ret["ranks"] = {n: list(p.ranks) for n, p in plan.items()}
        ret[f"fast{rank}"] = (sebc.explicit_step_supported(B_LOCAL), sebc._vec_ok, len(sebc._local_feats[rank]), sebc._F_local,
                              sebc._rw_mode_active)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("fixed_len,weighted,mean_tables", [(1, False, ()), (1, True, ()), (0, False, ()), (0, True, ()),
                                                            (0, False, (0, 1))])
def test_column_wise_sharded_equals_unsharded_world2(fixed_len, weighted, mean_tables):
    from _cw_sharded import check_against_unsharded, data

    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(_free_port(), fixed_len, weighted, mean_tables, ret), nprocs=W, join=True)
    assert ret["ranks"]["t0"] == [0, 1, 0, 1] and len(ret["ranks"]["t1"]) == 3  # two pieces of t0 on each rank
    per_rank, init = data(W, B_LOCAL, ROWS, DIMS, fixed_len, weighted)
    check_against_unsharded(ret, W, B_LOCAL, ROWS, DIMS, per_rank, init, fixed_len, weighted, ret["kinds"], mean_tables)
    for r in range(W):
        explicit, vec_ok, n_local, f_local, rw_mode = ret[f"fast{r}"]
        assert rw_mode == "windows"  # also for ragged bags, where "auto" would otherwise bucketize the row-wise table
        assert explicit is False  # the explicit step refuses column-wise collections
        assert vec_ok is True     # 32 / 36 / 16 / 8 wide pieces: all multiples of 4
        assert n_local == f_local
    # rank 0 holds the row-wise piece, t0's shards 0 and 2, and its share of t1's shards and the table-wise table
    assert sorted(n for n, *_ in ret[0][1]).count("t0") == 2 and sorted(n for n, *_ in ret[1][1]).count("t0") == 2


def _state_worker(rank, port, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    try:
        from _cw_sharded import data, load_init, pieces_of
        from torchrec_amd.distributed.types import ShardingEnv

        env = ShardingEnv.from_process_group(dist.group.WORLD)
        _, init = data(W, B_LOCAL, ROWS, DIMS, 1, False)
        plan, src = _build(env, False)
        load_init(src, init)
        sd = src.state_dict()
        # ---- one ShardedTensor [rows, D] per column-wise table, its local shards = this rank's pieces ------------------
        for t, n_local in ((0, 2), (1, 2 if rank == 0 else 1)):
            st = sd[f"embedding_bags.t{t}.weight"]
            assert list(st.size()) == [ROWS[t], DIMS[t]] and len(st.local_shards()) == n_local
            assert len(st.metadata().shards_metadata) == len(plan[f"t{t}"].ranks)
            for sh in st.local_shards():
                c0, w = sh.metadata.shard_offsets[1], sh.metadata.shard_sizes[1]
                assert sh.metadata.shard_offsets[0] == 0 and sh.metadata.shard_sizes[0] == ROWS[t]
                np.testing.assert_array_equal(sh.tensor.numpy(), init[t][:, c0:c0 + w])
        assert "t0" not in src.local_shards() and "t1" not in src.local_shards()  # full-width shards only
        assert {"t2", "t3"} & set(src.local_shards()) and [n for n, *_ in src.local_shard_pieces()].count("t0") == 2
        # ---- round trip from the ShardedTensors into a fresh module ------------------------------------------------------
        _, dst = _build(env, False)
        missing, unexpected = dst.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
        for (n, a, r0, c0), (n2, b, r02, c02) in zip(pieces_of(src), pieces_of(dst)):
            assert (n, r0, c0) == (n2, r02, c02)
            np.testing.assert_array_equal(a, b)
        # ---- from whole [rows, D] tensors: cut at every piece's first column (and row) -----------------------------------
        _, dst2 = _build(env, False)
        whole = {f"embedding_bags.t{t}.weight": torch.from_numpy(init[t] * 2.0) for t in range(len(ROWS))}
        dst2.load_state_dict(whole, strict=True)
        for n, w, r0, c0 in pieces_of(dst2):
            np.testing.assert_array_equal(w, (init[int(n[1:])] * 2.0)[r0:r0 + w.shape[0], c0:c0 + w.shape[1]])
        # a tensor of another shape is an error that names the key
        with pytest.raises(RuntimeError, match="embedding_bags.t0.weight"):
            dst2.load_state_dict(dict(whole, **{"embedding_bags.t0.weight": torch.zeros(ROWS[0], 64)}), strict=True)
        # ---- without ShardedTensors: a [rows, D] COPY assembled from the local pieces ------------------------------------
        src.sharded_tensor_state = False
        plain = src.state_dict()["embedding_bags.t0.weight"]
        assert tuple(plain.shape) == (ROWS[0], DIMS[0])
        for n, w, r0, c0 in pieces_of(src):
            if n == "t0":
                np.testing.assert_array_equal(plain[:, c0:c0 + w.shape[1]].numpy(), w)
        src.sharded_tensor_state = True
        # ---- sharding-invariant reset: column-wise plan == table-wise plan ----------------------------------------------
        _, tw = _build(env, False, sharding={4: "data_parallel"})
        src.reset_parameters_sharding_invariant(seed=5, chunk_rows=16)
        tw.reset_parameters_sharding_invariant(seed=5, chunk_rows=16)
        ret[f"reset{rank}"] = (pieces_of(src), pieces_of(tw))
        # ---- fused row-wise Adagrad: `<t>.momentum1`, 1-D, rows x shards, shard i at i x rows ----------------------------
        from fbgemm_gpu.split_embedding_configs import EmbOptimType
        _, ada = _build(env, False, fused={"optimizer": EmbOptimType.EXACT_ROWWISE_ADAGRAD})
        for i, st in enumerate(ada._emb_module.split_optimizer_states()):
            st[0].fill_(float(i + 1 + 100 * rank))
        osd = ada.fused_optimizer.state_dict()["state"]
        m1 = osd["embedding_bags.t0.weight"]["t0.momentum1"]
        assert list(m1.size()) == [ROWS[0] * 4]
        assert sorted(sh.metadata.shard_offsets[0] for sh in m1.local_shards()) == [(rank + 0) * ROWS[0], (rank + 2) * ROWS[0]]
        assert all(sh.metadata.shard_sizes == [ROWS[0]] for sh in m1.local_shards())
        m1b = osd["embedding_bags.t1.weight"]["t1.momentum1"]
        assert list(m1b.size()) == [ROWS[1] * 3]
        assert list(osd["embedding_bags.t3.weight"]["t3.momentum1"].size()) == [ROWS[3]]  # row-wise: as before
        _, ada2 = _build(env, False, fused={"optimizer": EmbOptimType.EXACT_ROWWISE_ADAGRAD})
        ada2.fused_optimizer.load_state_dict({"state": osd})
        for a, b in zip(ada._emb_module.split_optimizer_states(), ada2._emb_module.split_optimizer_states()):
            np.testing.assert_array_equal(a[0].numpy(), b[0].numpy())
        ada.sharded_tensor_state = False
        flat = ada.fused_optimizer.state_dict()["state"]["embedding_bags.t0.weight"]["t0.momentum1"]
        assert tuple(flat.shape) == (ROWS[0] * 4,) and set(flat.view(4, ROWS[0])[rank].tolist()) != {0.0}
        ret[f"ok{rank}"] = True
    finally:
        dist.destroy_process_group()


def test_column_wise_state_world2():
    ret = mp.Manager().dict()
    mp.spawn(_state_worker, args=(_free_port(), ret), nprocs=W, join=True)
    assert ret["ok0"] and ret["ok1"]
    # the reset gives every table the same values under both plans: assemble each plan's tables from both ranks' pieces
    full = {}
    for which in (0, 1):
        tabs = {t: np.full((ROWS[t], DIMS[t]), np.nan, dtype=np.float32) for t in range(4)}
        for r in range(W):
            for n, w, r0, c0 in ret[f"reset{r}"][which]:
                tabs[int(n[1:])][r0:r0 + w.shape[0], c0:c0 + w.shape[1]] = w
        full[which] = tabs
    for t in range(4):
        assert not np.isnan(full[0][t]).any()
        np.testing.assert_array_equal(full[0][t], full[1][t])


def _sebc(plan_edit=None, sharding=SHARDING, compute_kernel=None, min_partition=None, rw_input_dist=None):
    import _cpu_ops
    _cpu_ops.register()
    from _cw_sharded import tables_and_plan
    from _oracle_tbe import oracle_dp_tbe_factory, oracle_tbe_factory
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    tables, plan = tables_and_plan(W, ROWS, DIMS, sharding, "cpu", min_partition=min_partition)
    if compute_kernel:
        plan["t1"].compute_kernel = compute_kernel
    if plan_edit:
        plan_edit(plan)
    ebc = EmbeddingBagCollection(tables, device=torch.device("meta"))
    return ShardedEmbeddingBagCollection(ebc, plan, ShardingEnv.from_local(W, 0), {}, torch.device("cpu"),
                                         tbe_factory=oracle_tbe_factory, dp_tbe_factory=oracle_dp_tbe_factory,
                                         rw_input_dist=rw_input_dist)


def test_bad_column_wise_plans_raise_value_errors_naming_the_table():
    def gap(plan):
        plan["t0"].sharding_spec[2].shard_offsets = [0, 68]  # 64..68 uncovered, 96..100 twice

    def short_rows(plan):
        plan["t1"].sharding_spec[1].shard_sizes = [ROWS[1] - 1, 32]

    def bad_rank(plan):
        plan["t0"].ranks = [0, 1, 2, 1]

    def missing_rank(plan):
        plan["t0"].ranks = [0, 1]

    for edit, name, what in ((gap, "t0", "tile"), (short_rows, "t1", "rows"), (bad_rank, "t0", "rank 2"),
                             (missing_rank, "t0", "one rank per shard")):
        with pytest.raises(ValueError, match=f"table {name}.*{what}"):
            _sebc(edit)
    _sebc()  # the unedited plan builds


def test_unsupported_column_wise_combinations_raise_not_implemented():
    # pieces of different widths (32, 32, 36) behind the HBM row cache
    with pytest.raises(NotImplementedError, match="table t1.*widths"):
        _sebc(compute_kernel="batched_fused_uvm_caching")
    # the bucketized row-wise input dist refuses; "auto" keeps such collections on row windows
    with pytest.raises(NotImplementedError, match="bucketize"):
        _sebc(rw_input_dist="bucketize")
    # column-wise sequence embeddings stay out of scope
    from _oracle_tbe import oracle_seq_tbe_factory
    from torchrec_amd.distributed.embedding import ShardedEmbeddingCollection
    from torchrec_amd.distributed.types import ParameterSharding, ShardingEnv, ShardMetadata
    from torchrec_amd.modules.embedding_configs import EmbeddingConfig

    ec = [EmbeddingConfig(name="s0", embedding_dim=64, num_embeddings=30, feature_names=["q"])]
    ps = ParameterSharding("column_wise", "batched_fused", [0, 1],
                           [ShardMetadata([0, 0], [30, 32], "rank:0/cpu"), ShardMetadata([0, 32], [30, 32], "rank:1/cpu")])
    with pytest.raises(NotImplementedError, match="table s0.*column_wise"):
        ShardedEmbeddingCollection(ec, {"s0": ps}, ShardingEnv.from_local(W, 0), {}, torch.device("cpu"),
                                   tbe_factory=oracle_seq_tbe_factory)
