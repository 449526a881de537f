"""Measurement tool for the variable-batch recat of KJTAllToAll (csrc/sparse_ops.hip expand_into_jagged_permute +
permute_1D_sparse_data) next to its yardstick, the fixed-batch recat (permute_2D_sparse_data) of the SAME received ids read
as equal batches.  F_local features from W source ranks; `--batches` are the ranks' batch sizes (unequal, same sum as W equal
ones) — once with pooling factor 1 and once with ragged bags of 0..6.  Times are device-event times of `--iters` calls in
one window, the two recats alternating over `--rounds` windows each; prints one JSON line per case with the per-call median
and the spread (min .. max) of the rounds.  The recat generation is timed on its own: it includes three small host-to-device
copies and is not kernel time.
Usage: python tools/vb_recat_bench.py [--features 4 --batches 8000,8400,8192,7900,8500,8192,8100,8252]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=4)
    ap.add_argument("--batches", default="8000,8400,8192,7900,8500,8192,8100,8252")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import fbgemm_gpu  # noqa: F401
    from torchrec_amd.distributed.dist_data import _get_recat

    if not torch.cuda.is_available():
        raise SystemExit("vb_recat_bench: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    bpr = [int(b) for b in args.batches.split(",")]
    W, F = len(bpr), args.features
    if sum(bpr) % W:
        raise SystemExit("the batch sizes must sum to a multiple of their count (the yardstick reads them as equal batches)")
    B_eq = sum(bpr) // W
    recat_2d = _get_recat(F, W, 1, dev)
    ops = torch.ops.fbgemm

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters  # us per call

    results = []
    for name, lo, hi in (("pooling_factor_1", 1, 1), ("ragged_0_6", 0, 6)):
        rng = np.random.default_rng(0)
        lengths = torch.from_numpy(rng.integers(lo, hi + 1, size=F * sum(bpr)).astype(np.int32)).to(dev)
        N = int(lengths.sum().item())
        values = torch.from_numpy(rng.integers(0, 1 << 40, size=N)).to(dev)
        recat_1d = _get_recat(F, W, 1, dev, bpr)
        calls = {
            "recat_generation": lambda: _get_recat(F, W, 1, dev, bpr),
            "permute_1D": lambda: ops.permute_1D_sparse_data(recat_1d, lengths, values, None, N),
            "permute_2D": lambda: ops.permute_2D_sparse_data(recat_2d, lengths.view(W * F, B_eq), values, None, N),
        }
        # the two layouts agree wherever the batches are equal: same multiset of ids either way
        l1, v1, _ = calls["permute_1D"]()
        l2, v2, _ = calls["permute_2D"]()
        assert int(l1.sum()) == int(l2.sum()) == N and torch.equal(v1.sort().values, v2.sort().values)
        for fn in calls.values():  # warm-up: code objects, allocator
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                rounds[k].append(timed(fn))
        row = {"case": name, "features": F, "batch_size_per_rank": bpr, "ids": N, "segments": F * sum(bpr),
               "iters": args.iters, "rounds": args.rounds}
        for k, ts in rounds.items():
            row[k + "_us"] = {"median": round(float(np.median(ts)), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}
        print(json.dumps(row))
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
