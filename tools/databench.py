"""Measurement tool for the Criteo datapipe (torchrec_amd/datasets/criteo.py + csrc/criteo_batch.hip): what one batch costs
the training thread and the device on three paths that produce identical batches (checked before anything is timed), in one
process, alternating round by round.

  (a) host     the reference's pipeline restated: the host datapipe's next(), then pin_memory() and .to(device,
               non_blocking=True) — numpy on the training thread, three pinned copies
  (b) torch    the raw rows staged on the device exactly as path (c, resident="host") stages them, then a torch
               composition: index_select when shuffling, t().contiguous().view(-1).long(), remainder
  (c) kernel   the device datapipe, resident="host" and resident="device": copies (or none) and one launch

Synthetic day files of 2^21 rows in two files, B = 65 536 and 8 192, shuffle on and off.  Per batch: the wall time of the
path's next() on the host (no synchronisation inside) and the GPU time between two HIP events recorded round it.  A round is
`--batches` consecutive batches of each path; rows carry the median over the rounds of the per-batch mean.  `spread_us` is the
larger of the two compared paths' (max - min) over the rounds; `kernel_not_slower` says whether the kernel path's median is
within that spread of the other's or below it (the rule of DESIGN.md 3k).  For (c) also the kernel alone next to a device
copy that moves the same number of bytes.  A record: nothing is asserted.

Usage: python tools/databench.py [--rounds 10] [--batches 8] [--rows 2097152] [--out profiles/criteo_databench.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))

BATCHES = [65536, 8192]
HASHES = [40_000_000, 36746, 17245, 7413, 20243, 3, 7114, 1441, 62, 29275261, 1572176, 345138, 10, 2209, 11267, 128, 4,
          974, 14, 40_000_000, 11316796, 40_000_000, 452104, 12606, 104, 35]  # the 1 TB cardinalities, capped at 40 M
SEED = 11
README_STEP_MS = {65536: 8.5, 8192: None, 4096: 0.93}  # the measured train step the README states, where it states one


def write_files(directory, rows):
    import numpy as np

    rng = np.random.default_rng(0)
    paths = ([], [], [])
    for i, n in enumerate((rows // 2, rows - rows // 2)):
        parts = (rng.standard_normal((n, 13), dtype=np.float32),
                 rng.integers(-2 ** 31, 2 ** 31, size=(n, 26), dtype=np.int64).astype(np.int32),
                 rng.integers(0, 2, size=(n, 1), dtype=np.int64).astype(np.int32))
        for kind, lst, a in zip(("dense", "sparse", "labels"), paths, parts):
            p = os.path.join(directory, f"day_{i}_{kind}.npy")
            np.save(p, a)
            lst.append(p)
    return paths


class Cycle:
    """next() over epoch after epoch of an iterable."""

    def __init__(self, source):
        self.source, self.it = source, iter(source)

    def __call__(self):
        try:
            return next(self.it)
        except StopIteration:
            self.it = iter(self.source)
            return next(self.it)


class TorchComposition:
    """Path (b): the staging of the device datapipe (resident="host"), then torch ops instead of the kernel."""

    def __init__(self, pipe):
        import torch

        from torchrec_amd.datasets.criteo import CAT_FEATURE_COUNT, INT_FEATURE_COUNT

        self.pipe, dev, B = pipe, pipe.device, pipe.batch_size
        self.stage = (torch.empty((B, INT_FEATURE_COUNT), dtype=torch.float32, device=dev),
                      torch.empty((B, CAT_FEATURE_COUNT), dtype=torch.int32, device=dev),
                      torch.empty((B, 1), dtype=torch.int32, device=dev))
        self.hashes = torch.tensor(pipe.hashes, dtype=torch.int64, device=dev).view(-1, 1)
        self.perm_dev = torch.empty(B, dtype=torch.int64, device=dev)
        self.perm_pinned = torch.empty(B, dtype=torch.int64, pin_memory=True)
        self.perm_free = torch.cuda.Event()

    def __iter__(self):
        import numpy as np
        import torch

        from torchrec_amd.datasets.utils import Batch
        from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

        p, B = self.pipe, self.pipe.batch_size
        for segs in p._segments():
            off = 0
            for f, r, n in segs:
                for stage, arrs in zip(self.stage, (p.dense_arrs, p.sparse_arrs, p.labels_arrs)):
                    stage[off:off + n].copy_(arrs[f][r:r + n], non_blocking=True)
                off += n
            dense, sparse, labels = self.stage
            if p.shuffle_batches:
                self.perm_free.synchronize()
                self.perm_pinned.numpy()[:] = np.random.permutation(B)
                self.perm_dev.copy_(self.perm_pinned, non_blocking=True)
                self.perm_free.record()
                dense = dense.index_select(0, self.perm_dev)
                sparse = sparse.index_select(0, self.perm_dev)
                labels = labels.index_select(0, self.perm_dev)
            else:
                dense, labels = dense.clone(), labels.clone()
            values = sparse.t().contiguous().view(-1).long()
            values = values.view(-1, B).remainder_(self.hashes).view(-1)
            yield Batch(dense, KeyedJaggedTensor.from_fixed_lengths(p.keys, values, [1] * 26), labels.view(-1))


def _host_path(pipe, dev):
    def step(nxt):
        return nxt().pin_memory().to(dev, non_blocking=True)
    return step


def _measure(step, nxt, n):
    """(host us per batch, GPU us per batch) over n batches: host clock without a synchronisation inside, HIP events round
    the whole run."""
    import torch

    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    keep = []
    a.record()
    t0 = time.perf_counter()
    for _ in range(n):
        keep.append(step(nxt))
    host = (time.perf_counter() - t0) * 1e6 / n
    b.record()
    b.synchronize()
    return host, a.elapsed_time(b) * 1e3 / n


def _compare(t_k, t_o):
    med_k, med_o = statistics.median(t_k), statistics.median(t_o)
    spread = max(max(t_k) - min(t_k), max(t_o) - min(t_o))
    return {"spread_us": round(spread, 1), "other_over_kernel": round(med_o / med_k, 3),
            "kernel_not_slower": bool(med_k <= med_o + spread)}


def _summary(ts):
    return {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}


def _kernel_alone(pipe, rounds):
    """The launch alone on rows that are resident on the device (the permutation too), next to a device copy that moves the
    same number of bytes."""
    import torch

    from fbgemm_gpu import _lib

    B, dev = pipe.batch_size, pipe.device
    lib = _lib.load()
    seg = (_lib.CriteoSegment * 1)()
    seg[0].dense, seg[0].sparse = pipe.dense_arrs[0].data_ptr(), pipe.sparse_arrs[0].data_ptr()
    seg[0].labels, seg[0].rows = pipe.labels_arrs[0].data_ptr(), B
    assert pipe.dense_arrs[0].shape[0] >= B
    perm = torch.randperm(B, device=dev) if pipe.shuffle_batches else None
    dense = torch.empty((B, 13), dtype=torch.float32, device=dev)
    values = torch.empty(26 * B, dtype=torch.int64, device=dev)
    labels = torch.empty(B, dtype=torch.int32, device=dev)

    def launch():
        _lib.check(lib.tbe_criteo_batch_i64(seg, 1, B, _lib.ptr(pipe._hashes_dev), _lib.ptr(perm), dense.data_ptr(),
                                            values.data_ptr(), labels.data_ptr(), None, _lib.stream_ptr(dev)),
                   "tbe_criteo_batch_i64")

    nbytes = B * (13 * 4 + 26 * 4 + 4) + B * (13 * 4 + 26 * 8 + 4) + (8 * B if perm is not None else 0)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    res = {"bytes": nbytes, "with_perm": perm is not None}

    def event_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for name, fn in (("kernel", launch), ("device_copy", lambda: dst.copy_(src))):
        fn()
        us = statistics.median(event_us(fn) for _ in range(max(rounds, 5)))
        res[name] = {"us_median": round(us, 1), "GB_per_s": round(nbytes / us / 1e3, 1)}
    return res


def bench(args, dev, paths):
    import numpy as np
    import torch

    from torchrec_amd.datasets.criteo import InMemoryBinaryCriteoIterDataPipe as Pipe

    rows = []
    for B in BATCHES:
        for shuffle in (False, True):
            common = dict(batch_size=B, rank=0, world_size=1, shuffle_batches=shuffle, hashes=HASHES)
            host = Pipe(*paths, **common)
            c_host = Pipe(*paths, **common, device=dev, resident="host")
            c_dev = Pipe(*paths, **common, device=dev, resident="device")
            b_torch = TorchComposition(Pipe(*paths, **common, device=dev, resident="host"))
            ident = lambda nxt: nxt()  # noqa: E731
            runs = {"a_host": (host, _host_path(host, dev)), "b_torch": (b_torch, ident),
                    "c_kernel_host": (c_host, ident), "c_kernel_device": (c_dev, ident)}
            # identical batches first
            first = {}
            for name, (src, step) in runs.items():
                np.random.seed(SEED)
                nxt = Cycle(src)
                got = [step(nxt) for _ in range(2)]
                torch.cuda.synchronize()
                first[name] = [(b.dense_features.cpu(), b.sparse_features.values().cpu().long(), b.labels.cpu()) for b in got]
            for name, got in first.items():
                for x, y in zip(got, first["a_host"]):
                    if not all(torch.equal(p.view(torch.int32) if p.is_floating_point() else p,
                                           q.view(torch.int32) if q.is_floating_point() else q) for p, q in zip(x, y)):
                        raise SystemExit(f"databench: B={B} shuffle={shuffle}: path {name} and the host path differ")
            del first
            nexts = {name: Cycle(src) for name, (src, _) in runs.items()}
            for name, (_, step) in runs.items():  # warm-up
                _measure(step, nexts[name], 2)
            host_us = {n: [] for n in runs}
            gpu_us = {n: [] for n in runs}
            for _ in range(args.rounds):  # alternating, one process, one device
                for name, (_, step) in runs.items():
                    h, g = _measure(step, nexts[name], args.batches)
                    host_us[name].append(h)
                    gpu_us[name].append(g)
            row = {"B": B, "shuffle": shuffle, "rounds": args.rounds, "batches_per_round": args.batches,
                   "readme_train_step_ms": README_STEP_MS.get(B),
                   "host_us_per_batch": {n: _summary(t) for n, t in host_us.items()},
                   "gpu_us_per_batch": {n: _summary(t) for n, t in gpu_us.items()},
                   "host_time_c_host_vs_a": _compare(host_us["c_kernel_host"], host_us["a_host"]),
                   "host_time_c_device_vs_a": _compare(host_us["c_kernel_device"], host_us["a_host"]),
                   "gpu_time_c_host_vs_b": _compare(gpu_us["c_kernel_host"], gpu_us["b_torch"]),
                   "host_time_c_host_vs_b": _compare(host_us["c_kernel_host"], host_us["b_torch"]),
                   "kernel_alone": _kernel_alone(c_dev, args.rounds)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del host, c_host, c_dev, b_torch, runs, nexts
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("databench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        paths = write_files(tmp, args.rows)
        doc = {"tool": "tools/databench.py", "device": torch.cuda.get_device_name(0), "rows": args.rows,
               "timer": "host: perf_counter round the path's next() calls of a round, no synchronisation inside; gpu: HIP events "
                        "round the same calls; per-batch means, median over alternating rounds",
               "results": bench(args, dev, paths)}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
