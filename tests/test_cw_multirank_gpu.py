"""GPU: column-wise tables through the real kernels.  world_size 2 with both ranks on cuda:0 over gloo (the all-to-all
staged through the host, exactly as tests/test_multirank_gpu.py does): real TBE with one table per column shard, real
pooled-exchange pack / unpack driven by per-piece descriptors, against the unsharded oracle; and one world-size-1 RCCL run
with the exchange forced on.  Row-wise Adagrad is compared with the oracle on the SPLIT model (one table per column shard,
the feature duplicated): every column shard keeps its own per-row state, which is fbgemm's semantics."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _paths  # noqa: F401
from _results import ResultStore
from test_sharded_gloo import _free_port

pytestmark = pytest.mark.gpu

ROWS = [5000, 7, 230, 90000, 5, 1201]
DIMS = [128, 100, 16, 128, 50, 64]
B_LOCAL = 48
# t0 and t1 column-wise, t3 row-wise, t5 table-wise, t2 replicated (t4: table-wise, or column-wise in 20 / 30 wide shards)
SHARDING = {0: "column_wise", 1: "table_column_wise", 2: "data_parallel", 3: "row_wise", 5: "table_wise"}
EPS = 1e-3


def _sharding(t4_cw):
    return ({**SHARDING, 4: "column_wise"}, {4: 20}) if t4_cw else (SHARDING, None)


def _build(env, weighted, t4_cw, mean_tables, adagrad):
    from _cw_sharded import LR, tables_and_plan
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    sharding, min_partition = _sharding(t4_cw)
    tables, plan = tables_and_plan(env.world_size, ROWS, DIMS, sharding, "cuda", mean_tables, min_partition)
    ebc = EmbeddingBagCollection(tables, is_weighted=weighted, device=torch.device("meta"))
    fused = {"learning_rate": LR}
    if adagrad:
        from fbgemm_gpu.split_embedding_configs import EmbOptimType
        fused.update({"optimizer": EmbOptimType.EXACT_ROWWISE_ADAGRAD, "eps": EPS})
    return plan, ShardedEmbeddingBagCollection(ebc, plan, env, fused, torch.device("cuda", 0))


def _run(rank, W, fixed_len, weighted, t4_cw, mean_tables, adagrad, ret):
    from _cw_sharded import data, load_init, train_step
    from torchrec_amd.distributed.types import ShardingEnv

    dev = torch.device("cuda", 0)
    plan, sebc = _build(ShardingEnv.from_process_group(dist.group.WORLD), weighted, t4_cw, mean_tables, adagrad)
    per_rank, init = data(W, B_LOCAL, ROWS, DIMS, fixed_len, weighted)
    load_init(sebc, init)

    def all_reduce(g):
        if W == 1:
            return g
        gc = g.cpu()
        dist.all_reduce(gc)
        return gc.to(dev)

    out, pieces, replicas = train_step(sebc, per_rank, rank, W, fixed_len, weighted, dev, all_reduce)
    ret[rank] = (out, pieces, replicas)
    if rank == 0:  # one writer per key: the store's files are replaced, not locked
        ret["kinds"] = {n: p.sharding_type for n, p in plan.items()}
    ret[f"errors{rank}"] = sebc._emb_module.bounds_check_errors()
    ret[f"vec{rank}"] = sebc._vec_ok
    ret[f"exchange{rank}"] = sebc._exchange
    if adagrad:
        ret[f"m1_{rank}"] = [(lt.cfg.name, lt.col_offset, st[0].detach().cpu().numpy().copy())
                             for lt, st in zip(sebc._local_tables, sebc._emb_module.split_optimizer_states())]
        osd = sebc.fused_optimizer.state_dict()["state"]["embedding_bags.t0.weight"]["t0.momentum1"]
        ret[f"m1_size{rank}"] = (list(osd.size()), sorted(sh.metadata.shard_offsets[0] for sh in osd.local_shards()))


def _worker(rank, W, port, fixed_len, weighted, t4_cw, mean_tables, adagrad, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    try:
        from torchrec_amd.distributed._rehearsal import stage_all_to_all_through_host

        stage_all_to_all_through_host()  # gloo has no device all-to-all
        _run(rank, W, fixed_len, weighted, t4_cw, mean_tables, adagrad, ret)
    finally:
        dist.destroy_process_group()


def _check(ret, W, fixed_len, weighted, t4_cw, mean_tables):
    from _cw_sharded import check_against_unsharded, data

    per_rank, init = data(W, B_LOCAL, ROWS, DIMS, fixed_len, weighted)
    check_against_unsharded(ret, W, B_LOCAL, ROWS, DIMS, per_rank, init, fixed_len, weighted, ret["kinds"], mean_tables)
    for r in range(W):
        assert ret[f"errors{r}"] == 0  # every id is valid on every rank that sees it
        assert ret[f"vec{r}"] is False  # a 50-wide feature (or its 20 / 30 wide shards) turns the 16-B exchange path off
    kinds = ret["kinds"]
    assert kinds["t0"] == "column_wise" and kinds["t1"] == "table_column_wise" and kinds["t3"] == "row_wise"
    assert kinds["t4"] == ("column_wise" if t4_cw else "table_wise")
    pieces = [(n, c0, w.shape[1]) for r in range(W) for n, w, _, c0 in ret[r][1]]
    assert sorted(p[1:] for p in pieces if p[0] == "t1") == [(0, 32), (32, 32), (64, 36)]
    if t4_cw:
        assert sorted(p[1:] for p in pieces if p[0] == "t4") == [(0, 20), (20, 30)]


@pytest.mark.parametrize("t4_cw", [False, True])
@pytest.mark.parametrize("fixed_len,weighted,mean_tables", [(1, False, ()), (0, True, ()), (0, False, (0, 1))])
def test_column_wise_world2_on_one_gpu(fixed_len, weighted, mean_tables, t4_cw):
    """(length 1, unweighted): bit-exact forward; (ragged <= 3, weighted); MEAN pooling on the column-wise tables — every
    column shard divides by the full bag length, so the shards still concatenate to the unsharded row."""
    W = 2
    ret = ResultStore()
    mp.spawn(_worker, args=(W, _free_port(), fixed_len, weighted, t4_cw, mean_tables, False, ret), nprocs=W, join=True)
    _check(ret, W, fixed_len, weighted, t4_cw, mean_tables)


def test_column_wise_world2_rowwise_adagrad_is_per_column_shard():
    """EXACT_ROWWISE_ADAGRAD: weights and `momentum1` of every piece equal the oracle on the split model — one oracle
    table [rows, w_i] per piece, the feature duplicated (the pieces of a feature are consecutive in the output, so the
    split model's output and gradient layout is the collection's)."""
    from _cw_sharded import LR, data, global_batch
    from oracle import oracle

    W, fixed_len, weighted = 2, 2, False
    ret = ResultStore()
    mp.spawn(_worker, args=(W, _free_port(), fixed_len, weighted, True, (), True, ret), nprocs=W, join=True)
    per_rank, init = data(W, B_LOCAL, ROWS, DIMS, fixed_len, weighted)
    F, B = len(ROWS), B_LOCAL * W
    g_vals, g_offs, g_w, g_grad = global_batch(per_rank, W, B_LOCAL, F, weighted)
    # the split model, from the pieces the ranks report (replicated tables: whole, stepped by plain SGD as dense parameters)
    held = sorted({(int(n[1:]), c0, w.shape[1]) for r in range(W) for n, w, _, c0 in ret[r][1]}
                  | {(int(n[1:]), 0, DIMS[int(n[1:])]) for n in ret[0][2]})
    assert [sum(w for t, _, w in held if t == tt) for tt in range(F)] == DIMS
    tabs = oracle.Tables([ROWS[t] for t, _, _ in held], [w for _, _, w in held])
    for i, (t, c0, w) in enumerate(held):
        tabs.weights[i][...] = init[t][:, c0:c0 + w]
    ids = np.concatenate([g_vals[g_offs[t * B]:g_offs[(t + 1) * B]] for t, _, _ in held])
    lens = np.concatenate([np.diff(g_offs[t * B:(t + 1) * B + 1]) for t, _, _ in held])
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    sgd = oracle.Tables(tabs.rows, tabs.dims)
    for i in range(len(held)):
        sgd.weights[i][...] = tabs.weights[i]
    s0 = [np.zeros(ROWS[t], dtype=np.float32) for t, _, _ in held]
    oracle.tbe_backward(sgd, ids, offs, g_grad, oracle.OPT_EXACT_SGD, LR, None)
    oracle.tbe_backward(tabs, ids, offs, g_grad, oracle.OPT_EXACT_ROWWISE_ADAGRAD, LR, None, eps=EPS, state0=s0)
    index = {(t, c0): i for i, (t, c0, _) in enumerate(held)}
    for r in range(W):
        assert ret[f"errors{r}"] == 0
        for n, w, row0, c0 in ret[r][1]:
            i = index[(int(n[1:]), c0)]
            np.testing.assert_allclose(w, tabs.weights[i][row0:row0 + w.shape[0]], rtol=3e-5, atol=3e-5)
        for n, w in ret[r][2].items():
            np.testing.assert_allclose(w, sgd.weights[index[(int(n[1:]), 0)]], rtol=3e-5, atol=3e-5)
        row0_of = {(n, c0): r0 for n, _, r0, c0 in ret[r][1]}
        for n, c0, m1 in ret[f"m1_{r}"]:
            r0 = row0_of[(n, c0)]
            np.testing.assert_allclose(m1, s0[index[(int(n[1:]), c0)]][r0:r0 + m1.shape[0]], rtol=3e-5, atol=3e-5)
        # exposed as the reference does: rows x shards, shard i (column order) at i x rows; t0's shards alternate ranks
        size, local_offsets = ret[f"m1_size{r}"]
        assert size == [ROWS[0] * 4] and local_offsets == [r * ROWS[0], (r + 2) * ROWS[0]]
    # not invariant against the unsharded table: the shards of a row that was touched hold DIFFERENT sums of squares
    m = {(n, c0): m1 for r in range(W) for n, c0, m1 in ret[f"m1_{r}"]}
    assert not np.allclose(m[("t0", 0)], m[("t0", 32)])


def _rccl_worker(rank, port, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    from torchrec_amd.distributed.comm import init_rccl_process_group

    init_rccl_process_group(torch.device("cuda", 0), rank=0, world_size=1)
    try:
        import torchrec_amd.distributed.embeddingbag as eb

        eb.FORCE_EXCHANGE = True
        _run(0, 1, 1, False, True, (), False, ret)
        assert ret["exchange0"]
    finally:
        dist.destroy_process_group()


def test_column_wise_exchange_through_rccl_world1():
    """The id + pooled all-to-all over a real RCCL group with a column-wise collection: every piece is local, the ids of a
    column-wise feature are sent once per shard, unpack reassembles the features from the shards' slab columns."""
    ret = ResultStore()
    mp.spawn(_rccl_worker, args=(_free_port(), ret), nprocs=1, join=True)
    _check(ret, 1, 1, False, True, ())
