"""Kernel timing of the quantized lookup (csrc/tbe_nbit.hip) next to tbe_forward_pooled_f32 on the same ids, and of the
quantizer next to a device copy of its input bytes, at the Criteo-1TB shape (development tool; bench.py never takes these
paths).  Every variant is timed once per round, the rounds alternate the variants, and the record keeps each variant's
median, minimum and maximum over the rounds (HIP events around back-to-back C-ABI calls: `iters` of them, or as many as
fill a window of 30 ms).

--gather times the dot interaction over the quantized tables instead: `fused` (tbe_dlrm_interaction_gather_forward_nbit, one
launch) against the `pair` it replaces (tbe_forward_nbit_i64 with float32 output, then tbe_dlrm_interaction_forward_f32), one
id per bag, rows of D + P floats, with the FP32 tbe_dlrm_interaction_gather_forward_f32 as a yardstick; same rounds and
windows.  The two outputs must be equal bit for bit before anything is timed.  `spread_us` is the larger of the two paths'
(max - min) over the rounds; `kernel_not_slower` says whether fused's median is within that spread of the pair's or below it.
Bytes are counted from the shapes: ids, the rows' header + data bytes, the dense row and the output row; the pair also
writes and reads the pooled float32 buffer.

--gather-f16 times the gather interaction over FP16 training tables, forward and backward: `fused`
(tbe_dlrm_interaction_gather_forward_f16w / _backward_f16w) against the `pair` an FP16 model runs without it
(tbe_forward_pooled_f16w + tbe_dlrm_interaction_forward_f32; tbe_dlrm_interaction_backward_f32 on the pooled buffer) and
against the FP32 gather kernels on FP32 tables of the same shape.  Same rounds, windows, equality check and verdict, per
direction.
Usage: python tools/nbitbench.py [--gather | --gather-f16] [--batch 65536,4096] [--pooling 1,20] [--cap ROWS] [--rounds 7] [--iters 20]
       [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import _paths  # noqa: E402,F401
from fbgemm_gpu import _lib  # noqa: E402
from fbgemm_gpu.split_embedding_configs import SparseType  # noqa: E402
from fbgemm_gpu.split_table_batched_embeddings_ops import (  # noqa: E402
    ComputeDevice, EmbeddingLocation, IntNBitTableBatchedEmbeddingBagsCodegen, SplitTableBatchedEmbeddingBagsCodegen)

CRITEO_ROWS = [45833188, 36746, 17245, 7413, 20243, 3, 7114, 1441, 62, 29275261, 1572176, 345138, 10, 2209,
               11267, 128, 4, 974, 14, 48937457, 11316796, 40094537, 452104, 12606, 104, 35]
TYPES = {"int8": SparseType.INT8, "int4": SparseType.INT4, "int2": SparseType.INT2}


def timed(fn, iters):
    """milliseconds per call of `iters` back-to-back calls (the queue stays full: device time, not launch time)"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


WINDOW_MS = 30.0  # every timed window lasts at least this long: a shorter one measures the clock and the scheduler


def rounds_of(variants, rounds, iters):
    """per variant: median / min / max over the rounds, and the calls per window (`iters`, or more to fill WINDOW_MS)"""
    times, calls = {name: [] for name in variants}, {}
    for name, fn in variants.items():  # warm-up (code objects, the ids' first trip through the caches) sizes the window
        timed(fn, 2)
        calls[name] = max(iters, int(WINDOW_MS / timed(fn, 5)) + 1)
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, calls[name]))
    return {name: {"median_us": 1e3 * statistics.median(t), "min_us": 1e3 * min(t), "max_us": 1e3 * max(t),
                   "calls_per_window": calls[name]} for name, t in times.items()}


def gather_interaction(lib, st, fp32, nbit, rows, D, batches, rounds, iters, gen):
    """The --gather records: per batch, fused / pair / fp32 times of every bit rate."""
    F, dev = len(rows), torch.device("cuda", 0)
    P = F * (F + 1) // 2
    lay, records = fp32._get_layout(), []
    for B in batches:
        ids = torch.cat([torch.randint(0, r, (B,), generator=gen, device=dev, dtype=torch.int64) for r in rows])
        offsets = torch.arange(F * B + 1, dtype=torch.int64, device=dev)
        dense = torch.randn(B, D, device=dev)
        pooled = torch.empty((B, F * D), dtype=torch.float32, device=dev)
        out = {k: torch.empty((B, D + P), dtype=torch.float32, device=dev) for k in ("fused", "pair", "fp32")}
        io_bytes = F * B * 8 + B * D * 4 + B * (D + P) * 4  # ids, the dense row, the output row

        def run_fp32():
            lib.tbe_dlrm_interaction_gather_forward_f32(dense.data_ptr(), lay.feat_weights.data_ptr(), lay.feat_rows.data_ptr(),
                                                        None, ids.data_ptr(), B, F, D, out["fp32"].data_ptr(), D + P, None, st)

        for name, m in nbit.items():
            meta = [x.data_ptr() for x in m._feature_meta()]
            fw, frb, fr, bits, _, _ = m.gather_interaction_args()

            def fused(fw=fw, frb=frb, fr=fr, bits=bits):
                rc = lib.tbe_dlrm_interaction_gather_forward_nbit(dense.data_ptr(), fw.data_ptr(), frb.data_ptr(), fr.data_ptr(),
                                                                  bits, ids.data_ptr(), B, F, D, out["fused"].data_ptr(), D + P,
                                                                  None, st)
                assert rc == 0, lib.tbe_last_error()

            def pair(meta=meta):
                lib.tbe_forward_nbit_i64(*meta, None, F, B, ids.data_ptr(), F * B, offsets.data_ptr(), None, 0,
                                         pooled.data_ptr(), 0, F * D, None, st)
                lib.tbe_dlrm_interaction_forward_f32(dense.data_ptr(), pooled.data_ptr(), B, F, D, out["pair"].data_ptr(),
                                                     D + P, st)

            fused(), pair()
            torch.cuda.synchronize()
            assert torch.equal(out["fused"].view(torch.int32), out["pair"].view(torch.int32)), f"{name} B={B}: fused != pair"
            res = rounds_of({"fused": fused, "pair": pair, "fp32": run_fp32}, rounds, iters)
            row_bytes = F * B * (D * bits // 8 + 4)
            bytes_of = {"fused": io_bytes + row_bytes, "pair": io_bytes + row_bytes + 2 * B * F * D * 4,
                        "fp32": io_bytes + F * B * D * 4}
            for key, r in res.items():
                r["algorithmic_bytes"] = bytes_of[key]
                r["TBps"] = bytes_of[key] / (r["median_us"] * 1e-6) / 1e12
            spread = max(res[k]["max_us"] - res[k]["min_us"] for k in ("fused", "pair"))
            rec = {"batch": B, "type": name, "outputs_bit_equal": True, "variants": res, "spread_us": spread,
                   "pair_over_fused": res["pair"]["median_us"] / res["fused"]["median_us"],
                   "kernel_not_slower": bool(res["fused"]["median_us"] <= res["pair"]["median_us"] + spread)}
            records.append(rec)
            print(json.dumps(rec), flush=True)
    return records


def half_gather_interaction(lib, st, fp32, half, rows, D, batches, rounds, iters, gen):
    """The --gather-f16 records: per batch and direction, fused / pair / fp32 times."""
    F, dev = len(rows), torch.device("cuda", 0)
    P = F * (F + 1) // 2
    lay32, lay16, records = fp32._get_layout(), half._get_layout(), []
    for B in batches:
        ids = torch.cat([torch.randint(0, r, (B,), generator=gen, device=dev, dtype=torch.int64) for r in rows])
        offsets = torch.arange(F * B + 1, dtype=torch.int64, device=dev)
        dense, grad = torch.randn(B, D, device=dev), torch.randn(B, D + P, device=dev)
        pooled = torch.empty((B, F * D), dtype=torch.float32, device=dev)
        keys = ("fused", "pair", "fp32")
        out = {k: torch.empty((B, D + P), dtype=torch.float32, device=dev) for k in keys}
        gd = {k: torch.empty((B, D), dtype=torch.float32, device=dev) for k in keys}
        gs = {k: torch.empty((B, F * D), dtype=torch.float32, device=dev) for k in keys}

        def gather_fwd(entry, lay, k):
            rc = entry(dense.data_ptr(), lay.feat_weights.data_ptr(), lay.feat_rows.data_ptr(), None, ids.data_ptr(), B, F, D,
                       out[k].data_ptr(), D + P, None, st)
            assert rc == 0, lib.tbe_last_error()

        def gather_bwd(entry, lay, k):
            rc = entry(dense.data_ptr(), lay.feat_weights.data_ptr(), lay.feat_rows.data_ptr(), None, ids.data_ptr(),
                       grad.data_ptr(), D + P, B, F, D, gd[k].data_ptr(), gs[k].data_ptr(), None, st)
            assert rc == 0, lib.tbe_last_error()

        def pair_fwd():
            lib.tbe_forward_pooled_f16w(lay16.feat_weights.data_ptr(), lay16.feat_D.data_ptr(), lay16.feat_out_offset.data_ptr(),
                                        lay16.feat_rows.data_ptr(), F, B, D, ids.data_ptr(), F * B, offsets.data_ptr(), None, 0,
                                        None, pooled.data_ptr(), F * D, None, None, st)
            lib.tbe_dlrm_interaction_forward_f32(dense.data_ptr(), pooled.data_ptr(), B, F, D, out["pair"].data_ptr(), D + P, st)

        def pair_bwd():  # reads the pooled buffer the pair's forward left
            lib.tbe_dlrm_interaction_backward_f32(dense.data_ptr(), pooled.data_ptr(), grad.data_ptr(), D + P, B, F, D,
                                                  gd["pair"].data_ptr(), gs["pair"].data_ptr(), st)

        forward = {"fused": lambda: gather_fwd(lib.tbe_dlrm_interaction_gather_forward_f16w, lay16, "fused"), "pair": pair_fwd,
                   "fp32": lambda: gather_fwd(lib.tbe_dlrm_interaction_gather_forward_f32, lay32, "fp32")}
        backward = {"fused": lambda: gather_bwd(lib.tbe_dlrm_interaction_gather_backward_f16w, lay16, "fused"), "pair": pair_bwd,
                    "fp32": lambda: gather_bwd(lib.tbe_dlrm_interaction_gather_backward_f32, lay32, "fp32")}
        for fn in (*forward.values(), *backward.values()):
            fn()
        torch.cuda.synchronize()
        for t in (out, gd, gs):
            assert torch.equal(t["fused"].view(torch.int32), t["pair"].view(torch.int32)), f"B={B}: fused != pair"
        io_fwd = F * B * 8 + B * D * 4 + B * (D + P) * 4                       # ids, the dense row, the output row
        io_bwd = F * B * 8 + B * D * 4 + B * (D + P) * 4 + B * (F + 1) * D * 4  # ids, dense, grad_out, the two gradients
        for direction, variants, io in (("forward", forward, io_fwd), ("backward", backward, io_bwd)):
            res = rounds_of(variants, rounds, iters)
            # per row element the pair moves: forward the half, then the pooled float written and read; backward the pooled float
            pair_row = 2 + 4 + 4 if direction == "forward" else 4
            bytes_of = {"fused": io + F * B * D * 2, "pair": io + F * B * D * pair_row, "fp32": io + F * B * D * 4}
            for key, r in res.items():
                r["algorithmic_bytes"] = bytes_of[key]
                r["TBps"] = bytes_of[key] / (r["median_us"] * 1e-6) / 1e12
            spread = max(res[k]["max_us"] - res[k]["min_us"] for k in ("fused", "pair"))
            rec = {"batch": B, "direction": direction, "outputs_bit_equal": True, "variants": res, "spread_us": spread,
                   "pair_over_fused": res["pair"]["median_us"] / res["fused"]["median_us"],
                   "fp32_over_fused": res["fp32"]["median_us"] / res["fused"]["median_us"],
                   "kernel_not_slower": bool(res["fused"]["median_us"] <= res["pair"]["median_us"] + spread)}
            records.append(rec)
            print(json.dumps(rec), flush=True)
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="65536,4096")
    ap.add_argument("--pooling", default="1,20")
    ap.add_argument("--cap", type=int, default=0, help="cap rows per table (0 = full size: 85 GiB of float32 tables)")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="least calls per timed window")
    ap.add_argument("--json", default="")
    ap.add_argument("--gather", action="store_true", help="time the fused gather interaction against the lookup + interaction pair")
    ap.add_argument("--gather-f16", action="store_true",
                    help="time the gather interaction over FP16 tables, forward and backward, against its pair and the FP32 kernels")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib, st = _lib.load(), None
    rows = [min(r, args.cap) if args.cap else r for r in CRITEO_ROWS]
    F, D = len(rows), args.dim
    fp32 = SplitTableBatchedEmbeddingBagsCodegen([(r, D, EmbeddingLocation.DEVICE, ComputeDevice.CUDA) for r in rows], device=dev)
    for w, r in zip(fp32.split_embedding_weights(), rows):
        w.uniform_(-(1.0 / r) ** 0.5, (1.0 / r) ** 0.5)
    record = {"rows": rows, "dim": D, "rounds": args.rounds, "iters": args.iters, "window_ms": WINDOW_MS, "lookup": [], "quantizer": []}

    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    if args.gather_f16:
        half = SplitTableBatchedEmbeddingBagsCodegen([(r, D, EmbeddingLocation.DEVICE, ComputeDevice.CUDA) for r in rows],
                                                     device=dev, weights_precision=SparseType.FP16)
        for w16, w32 in zip(half.split_embedding_weights(), fp32.split_embedding_weights()):
            w16.copy_(w32)
        record = {"rows": rows, "dim": D, "rounds": args.rounds, "iters": args.iters, "window_ms": WINDOW_MS,
                  "fp16_gather_interaction": half_gather_interaction(lib, st, fp32, half, rows, D,
                                                                     [int(b) for b in args.batch.split(",")], args.rounds,
                                                                     args.iters, g)}
        if args.json:
            with open(args.json, "w") as f:
                json.dump(record, f, indent=1)
        return
    if args.gather:
        nbit = {}
        for name, ty in TYPES.items():
            m = nbit[name] = IntNBitTableBatchedEmbeddingBagsCodegen(
                [(f"t{t}", r, D, ty, EmbeddingLocation.DEVICE) for t, r in enumerate(rows)], device=dev, row_alignment=16)
            for t, w in enumerate(fp32.split_embedding_weights()):
                m.quantize_table_(t, w)
        record = {"rows": rows, "dim": D, "rounds": args.rounds, "iters": args.iters, "window_ms": WINDOW_MS,
                  "gather_interaction": gather_interaction(lib, st, fp32, nbit, rows, D, [int(b) for b in args.batch.split(",")],
                                                           args.rounds, args.iters, g)}
        if args.json:
            with open(args.json, "w") as f:
                json.dump(record, f, indent=1)
        return

    # the quantizer on the largest table, next to a device copy of the same input bytes
    big = max(range(F), key=lambda t: rows[t])
    src = fp32.split_embedding_weights()[big]
    dst = torch.empty_like(src)
    nbit = {}
    for name, ty in TYPES.items():
        m = nbit[name] = IntNBitTableBatchedEmbeddingBagsCodegen(
            [(f"t{t}", r, D, ty, EmbeddingLocation.DEVICE) for t, r in enumerate(rows)], device=dev, row_alignment=16)
        for t, w in enumerate(fp32.split_embedding_weights()):
            m.quantize_table_(t, w)
        res = rounds_of({"copy": lambda: dst.copy_(src), "quantize": lambda m=m: m.quantize_table_(big, src)}, args.rounds, args.iters)
        in_bytes, out_bytes = src.numel() * 4, rows[big] * m.row_bytes[big]
        rec = {"type": name, "rows": rows[big], "in_bytes": in_bytes, "out_bytes": out_bytes, **res}
        rec["quantize_TBps"] = (in_bytes + out_bytes) / (res["quantize"]["median_us"] * 1e-6) / 1e12
        rec["copy_TBps"] = 2 * in_bytes / (res["copy"]["median_us"] * 1e-6) / 1e12
        record["quantizer"].append(rec)
        print(json.dumps(rec), flush=True)
    del dst

    for B in [int(b) for b in args.batch.split(",")]:
        for L in [int(p) for p in args.pooling.split(",")]:
            ids = torch.cat([torch.randint(0, r, (B * L,), generator=g, device=dev, dtype=torch.int64) for r in rows])
            offsets = torch.arange(F * B + 1, dtype=torch.int64, device=dev) * L
            N = ids.numel()
            lay = fp32._get_layout()
            out32 = torch.empty((B, F * D), dtype=torch.float32, device=dev)
            out16 = torch.empty((B, F * D), dtype=torch.float16, device=dev)

            def run_fp32():
                lib.tbe_forward_pooled_f32(lay.feat_weights.data_ptr(), lay.feat_D.data_ptr(), lay.feat_out_offset.data_ptr(),
                                           lay.feat_rows.data_ptr(), F, B, D, ids.data_ptr(), N, offsets.data_ptr(), None, 0,
                                           None, out32.data_ptr(), F * D, None, None, st)

            variants, bytes_of = {"fp32": run_fp32}, {"fp32": N * (D * 4 + 8) + F * B * (8 + D * 4)}
            for name in TYPES:
                for f16 in (False, True):  # the output type is the entry's flag: one set of tables serves both
                    m = nbit[name]
                    meta = [x.data_ptr() for x in m._feature_meta()]
                    out = out16 if f16 else out32

                    def run(meta=meta, out=out, f16=f16):
                        lib.tbe_forward_nbit_i64(*meta, None, F, B, ids.data_ptr(), N, offsets.data_ptr(), None, 0,
                                                 out.data_ptr(), int(f16), F * D, None, st)

                    key = f"{name}_out_{'f16' if f16 else 'f32'}"
                    variants[key] = run
                    bytes_of[key] = N * (m.row_bytes[0] + 8) + F * B * (8 + D * (2 if f16 else 4))
            res = rounds_of(variants, args.rounds, args.iters)
            for key, r in res.items():
                r["algorithmic_bytes"] = bytes_of[key]
                r["TBps"] = bytes_of[key] / (r["median_us"] * 1e-6) / 1e12
            rec = {"batch": B, "pooling": L, "variants": res}
            record["lookup"].append(rec)
            print(json.dumps(rec), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
