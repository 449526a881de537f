"""CPU: column-wise plans on request.  The shard geometry is the reference's (tests/golden/cw_shard_geometry.json, recorded
by tests/golden/make_cw_golden.py from planner/enumerators.py:314-330); the placement is this planner's greedy fill; a plan
without column-wise constraints is what it was before the planner knew the sharding type
(tests/golden/planner_criteo_plans_pre_cw.json: plan_tables() of the 26 Criteo tables, recorded from the parent commit)."""
import dataclasses
import json
import os

import pytest

import _paths  # noqa: F401
from torchrec_amd.distributed.planner import (EmbeddingShardingPlanner, ParameterConstraints, Topology, cw_shard_widths)
from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GEOMETRY = json.load(open(os.path.join(GOLD, "cw_shard_geometry.json")))
# (D, min_partition) -> widths, worked out by hand from the reference formula
BY_HAND = {(128, None): [32, 32, 32, 32], (100, None): [32, 32, 36], (16, None): [16], (128, 64): [64, 64],
           (96, 40): [40, 56], (50, 20): [20, 30]}


def test_fixture_holds_the_hand_computed_cases():
    seen = {(c["dim"], c["min_partition"]): [s[1] for s in c["sizes"]] for c in GEOMETRY["cases"]}
    assert seen == BY_HAND
    assert GEOMETRY["min_cw_dim"] == 32
    for c in GEOMETRY["cases"]:
        assert cw_shard_widths(c["dim"], c["min_partition"]) == [s[1] for s in c["sizes"]]


def _plan(case, W, extra_tables=()):
    rows, D = case["rows"], case["dim"]
    tables = [EmbeddingBagConfig(name="cw", embedding_dim=D, num_embeddings=rows, feature_names=["f_a", "f_b"])]
    tables += list(extra_tables)
    cons = {"cw": ParameterConstraints(sharding_types=[case["sharding_type"]], min_partition=case["min_partition"])}
    return EmbeddingShardingPlanner(Topology(W), cons).plan_tables(tables)


@pytest.mark.parametrize("W", [2, 3, 4, 8])
@pytest.mark.parametrize("case", GEOMETRY["cases"], ids=lambda c: f"{c['sharding_type']}-D{c['dim']}-p{c['min_partition']}")
def test_column_wise_plan_follows_the_reference_geometry(case, W):
    p = _plan(case, W)["cw"]
    assert p.sharding_type == case["sharding_type"] and p.compute_kernel == "batched_fused"
    assert [s.shard_sizes for s in p.sharding_spec] == case["sizes"]
    assert [s.shard_offsets for s in p.sharding_spec] == case["offsets"]
    # the shards tile [0, D)
    col = 0
    for s in p.sharding_spec:
        assert s.shard_offsets == [0, col] and s.shard_sizes[0] == case["rows"]
        col += s.shard_sizes[1]
    assert col == case["dim"]
    assert len(p.ranks) == len(case["sizes"]) and all(0 <= r <= W - 1 for r in p.ranks)
    assert [s.placement for s in p.sharding_spec] == [f"rank:{r}/cuda:{r}" for r in p.ranks]
    # equal-cost shards go round the ranks (ties by rank): no rank gets a second shard before every rank has one
    n = len(p.ranks)
    if len({s[1] for s in case["sizes"]}) == 1:
        assert p.ranks == [i % W for i in range(n)]
    # deterministic
    assert dataclasses.asdict(_plan(case, W)["cw"]) == dataclasses.asdict(p)


def test_column_shards_share_the_greedy_fill_with_table_wise_tables():
    """LPT over (feature count x width): the big table-wise table is placed first (largest first), the four 32-wide shards
    (two features: cost 64 each) then fill the other rank until it carries as much."""
    case = {"rows": 5000, "dim": 128, "min_partition": None, "sharding_type": "column_wise"}
    big = EmbeddingBagConfig(name="big", embedding_dim=128, num_embeddings=10_000_000, feature_names=["g"])
    plan = _plan(case, 2, [big])
    assert plan["big"].sharding_type == "table_wise" and plan["big"].ranks == [0]
    # units after each shard: (128, 64), (128, 128); the tie goes to the rank holding fewer bytes, rank 1 (the table-wise
    # rule's order: units, then memory, then rank): (128, 192); the last shard then goes to rank 0
    assert plan["cw"].ranks == [1, 1, 1, 0]


def test_small_column_wise_table_is_not_replicated():
    case = {"rows": 100, "dim": 128, "min_partition": None, "sharding_type": "column_wise"}
    assert _plan(case, 4)["cw"].sharding_type == "column_wise"


def test_plans_without_column_wise_constraints_are_unchanged():
    from torchrec_amd.datasets.random import CRITEO_1TB_ROWS

    before = json.load(open(os.path.join(GOLD, "planner_criteo_plans_pre_cw.json")))
    tables = [EmbeddingBagConfig(name=f"t{i}", embedding_dim=128, num_embeddings=r, feature_names=[f"c{i}"])
              for i, r in enumerate(CRITEO_1TB_ROWS)]
    for W in (1, 2, 4, 8):
        plan = EmbeddingShardingPlanner(Topology(W)).plan_tables(tables)
        now = {n: dataclasses.asdict(p) for n, p in plan.items()}
        assert list(now) == list(f"t{i}" for i in range(26))
        assert json.dumps(now, sort_keys=True) == json.dumps(before[str(W)], sort_keys=True)
        assert not any("column" in p.sharding_type for p in plan.values())
