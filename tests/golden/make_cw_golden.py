"""Column-wise shard geometry as the REFERENCE computes it (planner/enumerators.py:245-274, :314-330
`calculate_shard_sizes_and_offsets(..., COLUMN_WISE, col_wise_shard_dim)`), recorded by importing the reference here (build
container only).  Output: tests/golden/cw_shard_geometry.json (data only): one entry per (D, min_partition) case."""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REFERENCE = "/root/reference"
ROWS = 1000
CASES = [(128, None), (100, None), (16, None), (128, 64), (96, 40), (50, 20)]  # (embedding dim, min_partition)


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
    from torchrec.distributed.planner.constants import MIN_CW_DIM
    from torchrec.distributed.planner.enumerators import calculate_shard_sizes_and_offsets
    from torchrec.distributed.types import ShardingType

    cases = []
    for D, min_partition in CASES:
        t = torch.empty((ROWS, D), device="meta")
        for st in (ShardingType.COLUMN_WISE.value, ShardingType.TABLE_COLUMN_WISE.value):
            sizes, offsets = calculate_shard_sizes_and_offsets(t, 8, 8, st, min_partition)
            cases.append({"rows": ROWS, "dim": D, "min_partition": min_partition, "sharding_type": st,
                          "sizes": [list(s) for s in sizes], "offsets": [list(o) for o in offsets]})
    result = {"min_cw_dim": MIN_CW_DIM, "cases": cases}
    with open(os.path.join(sys.argv[1] if len(sys.argv) > 1 else HERE, "cw_shard_geometry.json"), "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    for c in cases:
        print(c["dim"], c["min_partition"], c["sharding_type"], [s[1] for s in c["sizes"]])


if __name__ == "__main__":
    main()
