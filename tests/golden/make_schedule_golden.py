"""The explicit train step's host call schedule (graph replays, collectives, lookup stages, optimizer steps), recorded on
an MI355X from the two-rank rehearsal of tests/test_multirank_gpu.py, rank 0, for the three flat-gradient modes.
Output: tests/golden/explicit_step_schedule.json (data only).  Run it at a commit whose schedule is known to be right —
the test then holds every later commit to it.  `--check`: record again and compare with the file instead of writing."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import torch.multiprocessing as mp

    import test_multirank_gpu as t
    from _results import ResultStore
    from test_sharded_gloo import _free_port

    path = os.path.join(HERE, "explicit_step_schedule.json")
    out = {}
    for mode in t.SCHEDULE_MODES:
        ret = ResultStore()
        mp.spawn(t._e2e_worker, args=(2, _free_port(), ret, mode), nprocs=2, join=True)
        out[mode] = ret["schedule"]
        print(mode, len(out[mode]), "events")
    if "--check" in sys.argv[1:]:
        with open(path) as fh:
            have = json.load(fh)
        bad = [m for m in out if out[m] != have.get(m)]
        print(f"differs from {path}: {bad}" if bad else f"identical to {path}")
        sys.exit(1 if bad else 0)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")


if __name__ == "__main__":
    main()
