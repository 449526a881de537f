"""GPU: a small DLRM whose plan contains a column-wise table trains through DistributedModelParallel +
TrainPipelineSparseDist (world 2 on one GPU over gloo, all-to-all staged through the host) and gives the losses of the same
model under an all-table-wise plan; both start from reset_parameters_sharding_invariant.  rtol 1e-5: the backward's
summation chunks differ with the sort-key layout.  The fast paths that refuse column-wise collections (the
gather-interaction fusion, the explicit step) report themselves off and the model falls back."""
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

ROWS = [3000, 170]
D = 64
B = 32  # per rank
STEPS = 3
LR = 0.05


def _batches(W):
    rng = np.random.default_rng(5)
    out = []
    for _ in range(STEPS + 2):
        dense = rng.standard_normal((W * B, 13)).astype(np.float32)
        ids = np.stack([rng.integers(0, r, size=W * B) for r in ROWS]).astype(np.int64)  # [F, W*B]
        labels = rng.integers(0, 2, size=W * B).astype(np.int64)
        out.append((dense, ids, labels))
    return out


def _model(env, dev, column_wise):
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.planner import EmbeddingShardingPlanner, ParameterConstraints, Topology
    from torchrec_amd.models.dlrm import DLRMTrain
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.optim.keyed import CombinedOptimizer, KeyedOptimizerWrapper

    torch.manual_seed(0)
    keys = [f"c{i}" for i in range(len(ROWS))]
    tables = [EmbeddingBagConfig(name=f"t{i}", embedding_dim=D, num_embeddings=ROWS[i], feature_names=[keys[i]])
              for i in range(len(ROWS))]
    ebc = EmbeddingBagCollection(tables, device=torch.device("meta"))
    tm = DLRMTrain(ebc, 13, [32, D], [48, 1], dense_device=dev)
    cons = {"t0": (ParameterConstraints(["column_wise"], min_partition=32) if column_wise else ParameterConstraints(["table_wise"])),
            "t1": ParameterConstraints(["table_wise"])}
    model = DistributedModelParallel(tm, env=env, device=dev, sharders=[EmbeddingBagCollectionSharder({"learning_rate": LR})],
                                     planner=EmbeddingShardingPlanner(Topology(env.world_size), constraints=cons, dp_max_rows=0))
    opt = CombinedOptimizer([model.fused_optimizer,
                             KeyedOptimizerWrapper(dict(model.named_parameters()), lambda p: torch.optim.SGD(p, lr=LR))])
    sebc = model.sharded_modules()[0]
    assert model.plan.plan["model.sparse_arch.embedding_bag_collection"]["t0"].sharding_type == \
        ("column_wise" if column_wise else "table_wise")
    sebc.reset_parameters_sharding_invariant(seed=3)
    return keys, model, opt


def _train(model, opt, keys, rank, W, dev):
    from torchrec_amd.datasets.random import Batch
    from torchrec_amd.distributed.train_pipeline import TrainPipelineSparseDist
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    sl = slice(rank * B, (rank + 1) * B) if W > 1 else slice(None)
    bl = [Batch(torch.from_numpy(d[sl]).to(dev),
                KeyedJaggedTensor.from_fixed_lengths(keys, torch.from_numpy(np.ascontiguousarray(i[:, sl]).reshape(-1)).to(dev),
                                                     [1] * len(keys)),
                torch.from_numpy(lab[sl]).to(dev)) for d, i, lab in _batches(W)]
    pipe = TrainPipelineSparseDist(model, opt, dev)
    model.train()
    it = iter(bl)
    losses = [float(pipe.progress(it)[0].detach()) for _ in range(STEPS)]
    torch.cuda.synchronize()
    sebc = model.sharded_modules()[0]
    return {"losses": losses, "fused_lookup_steps": model.module.model.fused_lookup_steps,
            "explicit_steps": getattr(model.module, "explicit_steps", 0),
            "explicit_ok": sebc.explicit_step_supported(B), "deferred_ok": sebc.deferred_lookup_supported(bl[0].sparse_features),
            "pieces": [(n, tuple(w.shape), c0) for n, w, _, c0 in sebc.local_shard_pieces()],
            "errors": sebc._emb_module.bounds_check_errors() if sebc._emb_module is not None else 0}


def _worker(rank, W, port, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    try:
        from torchrec_amd.distributed._rehearsal import stage_all_to_all_through_host
        from torchrec_amd.distributed.types import ShardingEnv

        stage_all_to_all_through_host()
        for column_wise in (True, False):
            keys, model, opt = _model(ShardingEnv.from_process_group(dist.group.WORLD), dev, column_wise)
            ret[f"{'cw' if column_wise else 'tw'}{rank}"] = _train(model, opt, keys, rank, W, dev)
    finally:
        dist.destroy_process_group()


def test_dlrm_with_a_column_wise_table_trains_like_the_table_wise_plan_world2():
    W = 2
    ret = ResultStore()
    mp.spawn(_worker, args=(W, _free_port(), ret), nprocs=W, join=True)
    for r in range(W):
        cw, tw = ret[f"cw{r}"], ret[f"tw{r}"]
        print(f"rank {r}: column-wise losses {cw['losses']}  table-wise losses {tw['losses']}")
        np.testing.assert_allclose(cw["losses"], tw["losses"], rtol=1e-5)
        assert cw["errors"] == 0 and cw["fused_lookup_steps"] == 0 and cw["explicit_steps"] == 0
        assert cw["explicit_ok"] is False and cw["deferred_ok"] is False
    # t0's two 32-wide shards sit on different ranks, each a [3000, 32] table of that rank's lookup
    held = sorted((n, shape, c0, r) for r in range(W) for n, shape, c0 in ret[f"cw{r}"]["pieces"])
    assert [h[:3] for h in held if h[0] == "t0"] == [("t0", (ROWS[0], 32), 0), ("t0", (ROWS[0], 32), 32)]
    assert len({h[3] for h in held if h[0] == "t0"}) == 2


def test_gather_interaction_fusion_is_off_for_a_column_wise_collection_world1():
    """One rank, no exchange: the all-table-wise model takes the gather-interaction fusion on every step; the same model
    with a column-wise table reports the fusion off, materialises the pooled embeddings, and gives the same losses."""
    from torchrec_amd.distributed.types import ShardingEnv

    dev = torch.device("cuda", 0)
    runs = {}
    for column_wise in (True, False):
        keys, model, opt = _model(ShardingEnv.from_local(1, 0), dev, column_wise)
        runs[column_wise] = _train(model, opt, keys, 0, 1, dev)
    assert runs[False]["fused_lookup_steps"] > 0 and runs[False]["deferred_ok"] is True
    assert runs[True]["fused_lookup_steps"] == 0 and runs[True]["deferred_ok"] is False and runs[True]["explicit_ok"] is False
    print(f"column-wise losses {runs[True]['losses']}  table-wise losses {runs[False]['losses']}")
    np.testing.assert_allclose(runs[True]["losses"], runs[False]["losses"], rtol=1e-5)
