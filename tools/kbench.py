"""Kernel-level timing of the TBE hot path at the Criteo-1TB shape (development tool;
bench.py is the judged harness).
Usage: python tools/kbench.py [--batch 65536[,4096]] [--cap ROWS] [--precision fp32|fp16] [--rounding stochastic|nearest] [--repeats N] [--json FILE]
       python tools/kbench.py --opt LAMB|PARTIAL_ROWWISE_ADAM|PARTIAL_ROWWISE_LAMB|LARS_SGD|ADAM|... [--clip MAX_GRADIENT] ...
       python tools/kbench.py --indice-weights-grad [--pooling L] ...   the per-sample-weight gradient next to the weighted forward"""
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
    ap.add_argument("--opt", default="EXACT_SGD", help="an EmbOptimType name, e.g. ADAM, LAMB, PARTIAL_ROWWISE_ADAM, LARS_SGD")
    ap.add_argument("--clip", type=float, default=None, metavar="MAX_GRADIENT",
                    help="gradient clipping with this bound (such a launch takes the generic update kernel)")
    ap.add_argument("--nbatches", type=int, default=8)
    ap.add_argument("--pooling", type=int, default=1, help="ids per bag (fixed pooling factor)")
    ap.add_argument("--precision", choices=["fp32", "fp16"], default="fp32", help="storage type of the tables")
    ap.add_argument("--rounding", choices=["stochastic", "nearest"], default="stochastic",
                    help="fp16 tables: rounding of the updated rows (stochastic is the module's default)")
    ap.add_argument("--repeats", type=int, default=1, help="repeat every measurement this often (run-to-run spread)")
    ap.add_argument("--json", default="", help="append one JSON record per (batch, repeat) to this file")
    ap.add_argument("--indice-weights-grad", action="store_true",
                    help="time tbe_backward_indice_weights_* (HIP events) next to the WEIGHTED forward on the same tables and "
                         "batches, instead of the forward / backward measurement")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = [min(r, args.cap) if args.cap else r for r in CRITEO_ROWS]
    D = args.dim
    esz = 2 if args.precision == "fp16" else 4  # bytes per table element
    t0 = time.time()
    mod = SplitTableBatchedEmbeddingBagsCodegen(
        [(r, D, EmbeddingLocation.DEVICE, ComputeDevice.CUDA) for r in rows], device=dev,
        weights_precision=SparseType.FP16 if args.precision == "fp16" else SparseType.FP32,
        stochastic_rounding=args.rounding == "stochastic", optimizer=getattr(EmbOptimType, args.opt), learning_rate=0.01,
        gradient_clipping=args.clip is not None, max_gradient=args.clip if args.clip is not None else 1.0)
    for w, r in zip(mod.split_embedding_weights(), rows):
        w.uniform_(-(1.0 / r) ** 0.5, (1.0 / r) ** 0.5)
    torch.cuda.synchronize()
    print(f"tables ({args.precision}): {sum(rows)} rows, {sum(rows) * D * esz / 2**30:.1f} GiB, built in {time.time() - t0:.1f}s",
          flush=True)
    for B in [int(b) for b in str(args.batch).split(",")]:
        for rep in range(args.repeats):
            rec = (measure_indice_weights_grad if args.indice_weights_grad else measure)(mod, rows, B, D, esz, args)
            rec.update(batch=B, dim=D, pooling=args.pooling, opt=args.opt, clip=args.clip, cap=args.cap, precision=args.precision,
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
    # + the optimizer state of each distinct row, read and written once: float[D] per element-wise state, 4 B per row-wise
    elem_states = {"ADAM": 2, "LAMB": 2, "EXACT_ADAGRAD": 1, "LARS_SGD": 1, "PARTIAL_ROWWISE_ADAM": 1, "PARTIAL_ROWWISE_LAMB": 1}
    row_states = {"EXACT_ROWWISE_ADAGRAD": 1, "ROWWISE_ADAGRAD": 1, "PARTIAL_ROWWISE_ADAM": 1, "PARTIAL_ROWWISE_LAMB": 1}
    state_bytes = U * 2 * 4 * (elem_states.get(args.opt, 0) * D + row_states.get(args.opt, 0))
    upd_kernel_bytes = N * (D * 4 + 8) + U * 2 * D * esz + state_bytes
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


def measure_indice_weights_grad(mod, rows, B, D, esz, args):
    """HIP-event time per call of the weighted forward and of the per-sample-weight gradient (memset + gather kernel):
    blocks of --iters back-to-back calls between one event pair (the queue stays full, so the host's launch path is not
    part of the reading), the two alternating block by block over the same batches; the value is the median of 5 block
    means.  The two read the same rows, ids and [B, F*D] block; the forward writes that block, the gradient 4 B per id."""
    dev = torch.device("cuda", 0)
    F, L = len(rows), args.pooling
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    batches = [torch.cat([torch.randint(0, r, (B * L,), generator=g, device=dev, dtype=torch.int64) for r in rows])
               for _ in range(args.nbatches)]
    offsets = torch.arange(F * B + 1, dtype=torch.int64, device=dev) * L
    N = F * B * L
    psw = torch.rand(N, device=dev) + 0.5
    grad = torch.randn(B, F * D, device=dev)
    keep = {}

    def fwd(i):
        keep["out"] = mod._forward_impl(batches[i % len(batches)], offsets, psw, B)

    def giw(i):
        keep["giw"] = mod._indice_weights_grad(grad, batches[i % len(batches)], offsets, B)

    times = {"fwd": [], "giw": []}
    for i in range(3):
        fwd(i)
        giw(i)
    torch.cuda.synchronize()
    for block in range(5):
        for name, fn in (("fwd", fwd), ("giw", giw)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(args.iters):
                fn(i)
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.iters)
    f_us, g_us = float(np.median(times["fwd"])), float(np.median(times["giw"]))
    common = N * (D * esz + 8) + F * B * (D * 4 + 8)  # rows + ids, the [B, F*D] block + offsets
    fwd_bytes, giw_bytes = common + N * 4, common + 2 * N * 4  # + weights read ; + giw zeroed and written
    print(f"[B={B} L={L} {args.precision}] weighted fwd: {f_us:.1f} us ({fwd_bytes / f_us / 1e6:.2f} TB/s)   "
          f"indice_weights_grad: {g_us:.1f} us ({giw_bytes / g_us / 1e6:.2f} TB/s)   ratio {g_us / f_us:.3f}", flush=True)
    return {"weighted_fwd_us": f_us, "indice_weights_grad_us": g_us, "ratio": g_us / f_us,
            "weighted_fwd_us_min_max": [min(times["fwd"]), max(times["fwd"])],
            "indice_weights_grad_us_min_max": [min(times["giw"]), max(times["giw"])],
            "weighted_fwd_bytes": fwd_bytes, "indice_weights_grad_bytes": giw_bytes}


if __name__ == "__main__":
    main()
