"""distributed/sharding_geometry.py on the CPU, without a process group: the lists ShardedEmbeddingBagCollection builds its
exchange from, for ALL ranks at once.  A hand-sized world of 2 against literals printed by the constructor before the
arithmetic moved out of it; the 8-rank Criteo plan the benchmark's layout comes from (tests/golden/planner_criteo_w8.json)
for the cross-rank invariants — what rank s packs for rank r is what r unpacks; and every refusal of a plan."""
import json
import os

import pytest

import _paths  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner_criteo_w8.json")


def _tables(rows, dims, mean=()):
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig, PoolingType

    return [EmbeddingBagConfig(name=f"t{i}", embedding_dim=d, num_embeddings=r, feature_names=[f"f{i}"],
                               pooling=PoolingType.MEAN if i in mean else PoolingType.SUM)
            for i, (r, d) in enumerate(zip(rows, dims))]


def _column_wise(rows, widths, ranks, kernel="batched_fused", kind="column_wise"):
    from torchrec_amd.distributed.types import ParameterSharding, ShardMetadata

    offs = [sum(widths[:i]) for i in range(len(widths))]
    return ParameterSharding(kind, kernel, list(ranks), [ShardMetadata([0, o], [rows, w], "") for o, w in zip(offs, widths)])


def _hand_plan():
    """W = 2: t0 table-wise on rank 1, t1 row-wise, t2 column-wise (4 + 4 columns on ranks 0 and 1), t3 replicated."""
    from torchrec_amd.distributed.types import ParameterSharding

    tables = _tables([10, 7, 6, 5], [8, 4, 8, 4])
    plan = {"t0": ParameterSharding("table_wise", "batched_fused", [1]),
            "t1": ParameterSharding("row_wise", "batched_fused", [0, 1]),
            "t2": _column_wise(6, [4, 4], [0, 1]),
            "t3": ParameterSharding("data_parallel", "batched_dense", [0, 1])}
    return tables, plan


def test_hand_sized_world_of_two_equals_the_constructor_literals():
    """The expected lists are what ShardedEmbeddingBagCollection.__init__ stored for this plan (both ranks, over gloo) at
    the commit before the geometry became a function.  Pieces: 0 = f0, 1 = f1, 2 and 3 = the halves of f2, 4 = f3."""
    from torchrec_amd.distributed.sharding_geometry import sharding_geometry

    g = sharding_geometry(*_hand_plan(), 2)
    assert g.table_kind == [1, -1, -3, -2]
    assert g.local_pieces == [[1, 2], [1, 0, 3]]
    assert g.D_local_per_rank == [8, 16]
    assert g.send_feature_order == [1, 2, 1, 0, 2] and g.send_feats_per_rank == [2, 3]
    assert g.feat_src == [1, -1, 0, 1, -2]
    assert g.feat_slab_col == [4, 0, 4, 12, 0]
    assert g.piece_out_col == [0, 8, 12, 16, 20] and g.out_col == [0, 8, 12, 20, 24] and g.D_total == 24
    assert g.piece_feat == [0, 1, 2, 2, 3] and g.piece_dim == [8, 4, 4, 4, 4]
    assert g.rw_feats == [1] and g.rw_block_sizes == [4] and g.rw_mean is False
    assert g.tw_send_order == [2, 0, 2] and g.tw_per_rank == [1, 2] and g.tw_first == [0, 1, 3]
    assert g.dp_feats == [3] and g.sharded_feats == [0, 1, 2] and g.vec_ok is True
    assert g.cw_shards == {2: [(0, 4, 0), (4, 4, 1)]}
    assert g.feature_names == ["f0", "f1", "f2", "f3"] and g.feature_dim == [8, 4, 8, 4]

    def spec(rank):
        tables, ftm = g.local_tables(rank)
        return [(t.cfg.name, t.local_rows, t.row_offset, t.row_wise, t.col_offset, t.cols, t.column_shard) for t in tables], ftm

    assert spec(0) == ([("t1", 4, 0, True, 0, 4, None), ("t2", 6, 0, False, 0, 4, (0, 2))], [0, 1])
    assert spec(1) == ([("t1", 3, 4, True, 0, 4, None), ("t0", 10, 0, False, 0, 8, None), ("t2", 6, 0, False, 4, 4, (1, 2))],
                       [0, 1, 2])


def test_eight_ranks_pack_what_the_others_unpack():
    """The reference planner's 8-rank Criteo plan with one table each made row-wise, column-wise and replicated, so that
    every kind occurs: the invariants between the ranks' lists, for all eight ranks in one process."""
    from torchrec_amd.distributed.sharding_geometry import sharding_geometry
    from torchrec_amd.distributed.types import ParameterSharding, ShardMetadata

    ref = json.load(open(GOLD))
    W, D, rows = 8, ref["dim"], ref["rows"]
    tables = _tables(rows, [D] * len(rows))
    theirs = {f"t{i}": ref["mi355x_estimator"][f"t_cat_{i}"] for i in range(len(rows))}
    plan = {n: ParameterSharding(p["sharding_type"], p["compute_kernel"], p["ranks"],
                                 [ShardMetadata(list(s["offsets"]), list(s["sizes"]), "") for s in p["shards"] or []])
            for n, p in theirs.items()}
    tw = [n for n in plan if plan[n].sharding_type == "table_wise"]
    assert len(tw) == 18 and sum(1 for p in plan.values() if p.sharding_type == "data_parallel") == 8
    plan[tw[0]] = ParameterSharding("row_wise", "batched_fused", list(range(W)))
    plan[tw[1]] = _column_wise(rows[int(tw[1][1:])], [D // 2, D // 2], [2, 5])
    plan[tw[2]] = ParameterSharding("data_parallel", "batched_dense", list(range(W)))
    g = sharding_geometry(tables, plan, W)
    assert sorted(set(g.table_kind)) == [-3, -2, -1] + list(range(W))  # every kind, and every rank owns a table
    P = len(g.piece_feat)
    assert P == len(rows) + 1  # one piece per feature, two for the column-wise one
    for p in range(P):
        holders = [r for r in range(W) if p in g.local_pieces[r]]
        if g.piece_kind[p] == -2:
            assert holders == [] and g.feat_src[p] == -2
        elif g.piece_kind[p] == -1:
            assert holders == list(range(W)) and g.feat_src[p] == -1
        else:
            assert holders == [g.piece_kind[p]] == [g.feat_src[p]]
        assert all(g.local_pieces[r].count(p) == 1 for r in holders)
    for s in range(W):
        col = 0
        for p in g.local_pieces[s]:  # the slab rank s sends to everyone: its local pieces side by side
            assert g.feat_slab_col[p] == col, (s, p)
            col += g.piece_dim[p]
        assert col == g.D_local_per_rank[s]
        local, ftm = g.local_tables(s)
        assert len(ftm) == len(g.local_pieces[s]) == g.send_feats_per_rank[s]
        assert [local[i].cols for i in ftm] == [g.piece_dim[p] for p in g.local_pieces[s]]
    spans = sorted((g.piece_out_col[p], g.piece_out_col[p] + g.piece_dim[p]) for p in range(P))
    assert spans[0][0] == 0 and spans[-1][1] == g.D_total == D * len(rows)
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))  # no gap, no overlap
    assert len(g.send_feature_order) == sum(g.send_feats_per_rank)
    assert g.send_feature_order == [g.piece_feat[p] for r in range(W) for p in g.local_pieces[r]]
    assert g.tw_first[-1] == len(g.tw_send_order) == sum(g.tw_per_rank)


def test_refused_plans_raise_from_the_pure_function():
    """Every refusal the constructor had, with the patterns tests/test_variable_batch.py, test_cw_sharded_gloo.py,
    test_fused_optimizers_gpu.py and test_sharded_gloo.py match."""
    from torchrec_amd.distributed.sharding_geometry import sharding_geometry
    from torchrec_amd.distributed.types import ParameterSharding

    tables, plan = _hand_plan()
    sharding_geometry(tables, plan, 2, False, "windows", "EXACT_ROWWISE_ADAGRAD")  # the plan itself is fine
    with pytest.raises(NotImplementedError, match="t1.*row_wise"):
        sharding_geometry(tables, plan, 2, variable_batch=True)
    with pytest.raises(NotImplementedError, match=r"t2.*LAMB"):
        sharding_geometry(tables, plan, 2, optimizer_name="LAMB")
    with pytest.raises(NotImplementedError, match="bucketize"):
        sharding_geometry(tables, plan, 2, rw_input_dist="bucketize")
    uneven = dict(plan, t2=_column_wise(6, [4, 2, 2], [0, 1, 0], kernel="batched_fused_uvm_caching"))
    with pytest.raises(NotImplementedError, match="table t2.*widths"):
        sharding_geometry(tables, uneven, 2)
    no_cw = dict(plan, t2=ParameterSharding("table_wise", "batched_fused", [0]))
    with pytest.raises(NotImplementedError, match="MEAN"):
        sharding_geometry(_tables([10, 7, 6, 5], [8, 4, 8, 4], mean=(1,)), no_cw, 2, rw_input_dist="bucketize")
    sharding_geometry(_tables([10, 7, 6, 5], [8, 4, 8, 4], mean=(1,)), no_cw, 2, rw_input_dist="auto")
    with pytest.raises(NotImplementedError, match="sharding type table_row_wise is outside the MI355X hot path"):
        sharding_geometry(tables, dict(plan, t0=ParameterSharding("table_row_wise", "batched_fused", [0, 1])), 2)
    with pytest.raises(ValueError, match="table t2.*tile"):
        sharding_geometry(tables, dict(plan, t2=_column_wise(6, [4, 2], [0, 1])), 2)
