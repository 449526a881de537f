"""Kernel-level timing of the TBE hot path at the Criteo-1TB shape (development tool;
bench.py is the judged harness).
Usage: python tools/kbench.py [--batch 65536[,4096]] [--cap ROWS] [--precision fp32|fp16] [--rounding stochastic|nearest] [--repeats N] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import _paths  # noqa: E402,F401
from fbgemm_gpu.split_embedding_configs import EmbOptimType, SparseType  # noqa: E402
from fbgemm_gpu.split_table_batched_embeddings_ops import (  # noqa: E402
    ComputeDevice, EmbeddingLocation, SplitTableBatchedEmbeddingBagsCodegen)

CRITEO_ROWS = [45833188, 36746, 17245, 7413, 20243, 3, 7114, 1441, 62, 29275261, 1572176, 345138, 10, 2209,
               11267, 128, 4, 974, 14, 48937457, 11316796, 40094537, 452104, 12606, 104, 35]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="65536", help="batch size, or a comma-separated list measured on one set of tables")
    ap.add_argument("--cap", type=int, default=0, help="cap rows per table (0 = full 85 GiB in fp32)")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--opt", default="EXACT_SGD")
    ap.add_argument("--nbatches", type=int, default=8)
    ap.add_argument("--pooling", type=int, default=1, help="ids per bag (fixed pooling factor)")
    ap.add_argument("--precision", choices=["fp32", "fp16"], default="fp32", help="storage type of the tables")
    ap.add_argument("--rounding", choices=["stochastic", "nearest"], default="stochastic",
                    help="fp16 tables: rounding of the updated rows (stochastic is the module's default)")
    ap.add_argument("--repeats", type=int, default=1, help="repeat every measurement this often (run-to-run spread)")
    ap.add_argument("--json", default="", help="append one JSON record per (batch, repeat) to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = [min(r, args.cap) if args.cap else r for r in CRITEO_ROWS]
    D = args.dim
    esz = 2 if args.precision == "fp16" else 4  # bytes per table element
    t0 = time.time()
    mod = SplitTableBatchedEmbeddingBagsCodegen(
        [(r, D, EmbeddingLocation.DEVICE, ComputeDevice.CUDA) for r in rows], device=dev,
        weights_precision=SparseType.FP16 if args.precision == "fp16" else SparseType.FP32,
        stochastic_rounding=args.rounding == "stochastic", optimizer=getattr(EmbOptimType, args.opt), learning_rate=0.01)
    for w, r in zip(mod.split_embedding_weights(), rows):
        w.uniform_(-(1.0 / r) ** 0.5, (1.0 / r) ** 0.5)
    torch.cuda.synchronize()
    print(f"tables ({args.precision}): {sum(rows)} rows, {sum(rows) * D * esz / 2**30:.1f} GiB, built in {time.time() - t0:.1f}s",
          flush=True)
    for B in [int(b) for b in str(args.batch).split(",")]:
        for rep in range(args.repeats):
            rec = measure(mod, rows, B, D, esz, args)
            rec.update(batch=B, dim=D, pooling=args.pooling, opt=args.opt, precision=args.precision,
                       rounding=args.rounding if args.precision == "fp16" else None, repeat=rep)
            if args.json:
                with open(args.json, "a") as f:
                    f.write(json.dumps(rec) + "\n")


def measure(mod, rows, B, D, esz, args):
    dev = torch.device("cuda", 0)
    F = len(rows)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    batches = []
    for _ in range(args.nbatches):
        idx = torch.cat([torch.randint(0, r, (B * args.pooling,), generator=g, device=dev, dtype=torch.int64) for r in rows])
        batches.append(idx)
    L = args.pooling
    offsets = torch.arange(F * B + 1, dtype=torch.int64, device=dev) * L
    grad = torch.randn(B, F * D, device=dev)

    def timeit(fn, n):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(n):
            fn(i)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n  # ms

    outs = {}

    def fwd(i):
        with torch.no_grad():  # forward only: do not start the backward's side-stream sort
            outs["o"] = mod(batches[i % len(batches)], offsets)

    ms_f = timeit(fwd, args.iters)
    fwd_bytes = B * (F * L * (D * esz + 8) + F * 8 + F * D * 4)
    print(f"[B={B}] fwd: {ms_f * 1e3:.1f} us  {fwd_bytes / ms_f / 1e6:.1f} GB/s (algorithmic {fwd_bytes / 1e6:.1f} MB)", flush=True)

    def fwdbwd(i):
        o = mod(batches[i % len(batches)], offsets)
        o.backward(grad)

    import ctypes

    from fbgemm_gpu import _lib
    lib = _lib.load()
    for i in range(3):
        fwdbwd(i)
    torch.cuda.synchronize()
    lib.tbe_profile_enable(1)
    tot, n, nrows = ctypes.c_double(0.0), ctypes.c_int64(0), ctypes.c_int64(0)
    for slot in range(4):
        lib.tbe_profile_read(slot, ctypes.byref(tot), ctypes.byref(n))
    lib.tbe_profile_read_rows(ctypes.byref(nrows))
    names = ["fwd kernel", "bwd_update kernel", "bwd apply (update+fixup)", "bwd prepare (linearize+sort)"]
    per_iter = [[] for _ in names]  # one event reading per iteration: the median is robust against a disturbed iteration
    for i in range(args.iters):
        fwdbwd(i)
        for slot in range(4):
            lib.tbe_profile_read(slot, ctypes.byref(tot), ctypes.byref(n))
            if n.value:
                per_iter[slot].append(tot.value / n.value * 1e3)
    lib.tbe_profile_read_rows(ctypes.byref(nrows))
    lib.tbe_profile_enable(0)
    med = [float(np.median(v)) if v else None for v in per_iter]
    for slot in range(4):
        if med[slot] is not None:
            print(f"  [events] {names[slot]}: median {med[slot]:.1f} us, mean {np.mean(per_iter[slot]):.1f} us over "
                  f"{len(per_iter[slot])}", flush=True)
    # algorithmic bytes of the kernels themselves (pooling factor L): the forward reads an id and a row per id and writes
    # the pooled row; the update reads (key, bag) and a gradient row per id and reads + writes each DISTINCT row once
    N = F * B * L
    U = nrows.value / max(1, args.iters)
    fwd_kernel_bytes = N * (D * esz + 8) + F * B * (D * 4 + 8)
    upd_kernel_bytes = N * (D * 4 + 8) + U * 2 * D * esz
    rec = {"fwd_kernel_us": med[0], "bwd_update_kernel_us": med[1], "bwd_apply_us": med[2], "bwd_prepare_us": med[3],
           "distinct_rows_per_step": U, "fwd_kernel_bytes": fwd_kernel_bytes, "bwd_update_kernel_bytes": upd_kernel_bytes}
    if med[0]:
        rec["fwd_kernel_TBps"] = fwd_kernel_bytes / med[0] / 1e6
        print(f"  fwd kernel: {fwd_kernel_bytes / 1e6:.1f} MB algorithmic -> {rec['fwd_kernel_TBps']:.2f} TB/s", flush=True)
    if med[1]:
        rec["bwd_update_kernel_TBps"] = upd_kernel_bytes / med[1] / 1e6
        print(f"  bwd_update kernel: {U:.0f} distinct rows, {upd_kernel_bytes / 1e6:.1f} MB algorithmic -> "
              f"{rec['bwd_update_kernel_TBps']:.2f} TB/s", flush=True)
    ms_fb = timeit(fwdbwd, args.iters)
    bwd_bytes = B * (F * D * 4 + F * 16 + 2 * F * D * esz)
    ms_b = ms_fb - ms_f
    print(f"fwd+bwd: {ms_fb * 1e3:.1f} us ; bwd ~ {ms_b * 1e3:.1f} us  {bwd_bytes / ms_b / 1e6:.1f} GB/s "
          f"(algorithmic {bwd_bytes / 1e6:.1f} MB)", flush=True)
    print(f"train-step TBE samples/s: {B / ms_fb * 1e3:.3e}", flush=True)
    rec.update(fwd_call_us=ms_f * 1e3, fwd_bwd_call_us=ms_fb * 1e3)
    return rec


if __name__ == "__main__":
    main()
