"""Measurement tool for the BERT4Rec loss and metrics (torchrec_amd/modules/loss.py + csrc/cross_entropy.hip,
torchrec_amd/metrics/ranking.py + csrc/rank_metrics.hip): HIP-event time on the kernel path next to torch on the same
tensors, timed in the same process, the two alternating round by round.  Both must agree before anything is timed.

Cross-entropy: one forward + backward of `cross_entropy(logits, labels, ignore_index=0)` against `F.cross_entropy`, at
(R, V) = (12 800, 3 708) and (12 800, 26 746) — B * T of the reference's defaults times the ml-1m / ml-20m vocabularies — with
15 % and 100 % of the rows valid.  Each row also carries the peak of `torch.cuda.max_memory_allocated` over one forward +
backward of either path above the level before it, and the two kernels alone: time, the algorithmic byte count computed here
from the shapes and the valid share (forward: the valid rows once, the labels, three floats per row; backward: the valid
rows once more, the whole gradient written), and bytes/s, next to a device-to-device copy of [R, V] floats.

Metrics: `recalls_and_ndcgs_for_ks(scores, labels, [1, 5, 10])` against the reference's formula restated WITH its per-sample
host loop for the ideal DCG and one `.item()` per metric (examples/bert4rec/bert4rec_metrics.py:28-61), at (B, C) = (128, 101)
and (1024, 101), on [B, C] scores and on the `[:, -1, :]` view of [B, 2, V = 3 708] scores with candidates (torch side: the
gather of bert4rec_main.py:244-245 first).  Timed with a host clock round a call that ends in its device-to-host copy.

`spread_us` is the larger of the two paths' (max - min) over the rounds; `kernel_not_slower` says whether the kernel path's
median is within that spread of torch's or below it (the rule of DESIGN.md 3k).  A record: nothing is asserted.

Usage: python tools/lossbench.py [--rounds 10] [--warmup 3] [--out profiles/bert4rec_lossbench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))

CE_SHAPES = [(12800, 3708), (12800, 26746)]
CE_SHARES = [0.15, 1.0]
RANK_SHAPES = [(128, 101), (1024, 101)]
RANK_V = 3708
KS = [1, 5, 10]


def _event_us(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _host_us(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def _peak_bytes(fn):
    """Peak of allocated memory over fn(), above the level before it."""
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def _alternate(kernel, torch_fn, rounds, timer):
    t_k, t_t = [], []
    for _ in range(rounds):  # alternating, one process, one device
        t_k.append(timer(kernel))
        t_t.append(timer(torch_fn))
    med_k, med_t = statistics.median(t_k), statistics.median(t_t)
    spread = max(max(t_k) - min(t_k), max(t_t) - min(t_t))
    return {"rounds": rounds, "kernel_us_median": round(med_k, 1), "kernel_us_min": round(min(t_k), 1),
            "kernel_us_max": round(max(t_k), 1), "torch_us_median": round(med_t, 1), "torch_us_min": round(min(t_t), 1),
            "torch_us_max": round(max(t_t), 1), "spread_us": round(spread, 1), "torch_over_kernel": round(med_t / med_k, 3),
            "kernel_not_slower": bool(med_k <= med_t + spread)}


def ce_bytes(R, V, n_valid):
    """The bytes the two kernels have to move, from the shapes and the number of valid rows."""
    row = 4 * V
    forward = n_valid * row + 8 * R + 3 * 4 * R + 4 * n_valid  # valid rows, labels, stats + row losses, x[label]
    backward = n_valid * row + 8 * R + 2 * 4 * R + R * row      # valid rows, labels, stats, the whole gradient
    return forward, backward


def _ce_kernels_alone(x, labels, rounds):
    import torch

    from fbgemm_gpu import _lib
    from fbgemm_gpu._lib import check, ptr, stream_ptr
    from torchrec_amd.modules import loss as L

    R, V = x.shape
    lib = _lib.load()
    _, state = L._forward(x, labels, 0, "mean")
    g = torch.ones((), device=x.device)
    grad = torch.empty_like(x)
    dst = torch.empty_like(x)

    def backward():
        check(lib.tbe_cross_entropy_backward_f32(ptr(g), ptr(x), V, ptr(labels), state.data_ptr() + 8, state.data_ptr(), R, V, 0, 0,
                                                 ptr(grad), V, stream_ptr(x.device)), "tbe_cross_entropy_backward_f32")

    n_valid = int((labels != 0).sum())
    fb, bb = ce_bytes(R, V, n_valid)
    runs = {"forward": (lambda: L._forward(x, labels, 0, "mean"), fb), "backward": (backward, bb),
            "device_copy": (lambda: dst.copy_(x), 2 * 4 * R * V)}
    res = {"n_valid": n_valid}
    for name, (fn, nbytes) in runs.items():
        fn()
        us = statistics.median(_event_us(fn) for _ in range(max(rounds, 5)))
        res[name] = {"us_median": round(us, 1), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
    return res


def bench_cross_entropy(args, dev):
    import torch
    from torch.nn import functional as F

    from torchrec_amd.modules.loss import cross_entropy

    rows = []
    for R, V in CE_SHAPES:
        for share in CE_SHARES:
            torch.manual_seed(R + V)
            x = (2.0 * torch.randn(R, V, device=dev)).requires_grad_()
            labels = torch.randint(1, V, (R,), device=dev)
            if share < 1.0:
                labels[torch.rand(R, device=dev) >= share] = 0

            def step(fn):
                x.grad = None
                loss = fn(x, labels)
                loss.backward()
                return loss.detach(), x.grad

            kernel = lambda a, t: cross_entropy(a, t, ignore_index=0)  # noqa: E731
            torch_fn = lambda a, t: F.cross_entropy(a, t, ignore_index=0)  # noqa: E731
            (lk, gk), (lt, gt) = step(kernel), step(torch_fn)
            loss_err = float((lk - lt).abs() / lt.abs())
            grad_err = float((gk - gt).abs().max() / gt.abs().max())
            if not (loss_err < 1e-4 and grad_err < 1e-4):
                raise SystemExit(f"lossbench: at {(R, V, share)}: kernel path and torch differ: {loss_err} {grad_err}")
            del lk, gk, lt, gt
            for _ in range(args.warmup):
                step(kernel)
                step(torch_fn)
            x.grad = None
            peak_k = _peak_bytes(lambda: step(kernel))
            x.grad = None
            peak_t = _peak_bytes(lambda: step(torch_fn))
            x.grad = None
            row = {"what": "cross_entropy forward + backward", "R": R, "V": V, "valid_share": share}
            row.update(_alternate(lambda: step(kernel), lambda: step(torch_fn), args.rounds, _event_us))
            row.update({"kernel_peak_MiB": round(peak_k / 2**20, 1), "torch_peak_MiB": round(peak_t / 2**20, 1),
                        "one_matrix_MiB": round(R * V * 4 / 2**20, 1), "loss_rel_diff": loss_err, "grad_rel_diff_max": grad_err})
            x.grad = None
            row["kernels_alone"] = _ce_kernels_alone(x.detach(), labels, args.rounds)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, labels
            torch.cuda.empty_cache()
    return rows


def reference_formula_with_its_loop(scores, labels, ks):
    """The reference's recalls_and_ndcgs_for_ks restated, per-sample host loop and per-metric reads included: what a user of
    the reference pays today."""
    import torch

    out = {}
    n_pos = labels.sum(1)
    hits_of = labels.float()
    order = torch.sort(-scores, dim=1).indices
    for k in sorted(ks, reverse=True):
        order = order[:, :k]
        hits = hits_of.gather(1, order)
        limit = torch.min(torch.tensor([float(k)], device=labels.device), n_pos.float())
        out["Recall@%d" % k] = (hits.sum(1) / limit).mean().cpu().item()
        w = 1 / torch.log2(torch.arange(2, 2 + k).float())
        dcg = (hits * w.to(hits.device)).sum(1)
        ideal = torch.tensor([float(w[:min(int(n), k)].sum()) for n in n_pos], device=dcg.device)  # one read per sample
        out["NDCG@%d" % k] = (dcg / ideal).mean().cpu().item()
    return out


def bench_metrics(args, dev):
    import torch

    from torchrec_amd.metrics import recalls_and_ndcgs_for_ks

    rows = []
    for B, C in RANK_SHAPES:
        for with_candidates in (False, True):
            torch.manual_seed(B + C)
            labels = torch.zeros(B, C, dtype=torch.int64, device=dev)
            labels[:, 0] = 1  # the reference's evaluation: one positive in front of 100 sampled negatives
            if with_candidates:
                full = torch.randn(B, 2, RANK_V, device=dev)
                scores = full[:, -1, :]
                cand = torch.stack([torch.randperm(RANK_V, device=dev)[:C] for _ in range(B)])
                kernel = lambda: recalls_and_ndcgs_for_ks(scores, labels, KS, candidates=cand)  # noqa: E731
                torch_fn = lambda: reference_formula_with_its_loop(scores.gather(1, cand), labels, KS)  # noqa: E731
            else:
                scores = torch.randn(B, C, device=dev)
                kernel = lambda: recalls_and_ndcgs_for_ks(scores, labels, KS)  # noqa: E731
                torch_fn = lambda: reference_formula_with_its_loop(scores, labels, KS)  # noqa: E731
            got, want = kernel(), torch_fn()
            diff = max(abs(got[n] - want[n]) for n in want)
            if not diff < 1e-5:
                raise SystemExit(f"lossbench: at {(B, C, with_candidates)}: kernel path and reference formula differ: {diff}")
            for _ in range(args.warmup):
                kernel()
                torch_fn()
            row = {"what": "recalls_and_ndcgs_for_ks", "B": B, "C": C, "ks": KS, "candidates_from_V": RANK_V if with_candidates else None}
            row.update(_alternate(kernel, torch_fn, args.rounds, _host_us))
            row["max_abs_diff"] = diff
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("lossbench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    doc = {"tool": "tools/lossbench.py", "device": torch.cuda.get_device_name(0),
           "timer": "cross-entropy: HIP events round one forward + backward; metrics: host clock round one call that ends in its "
                    "device-to-host copy; kernel path and torch alternating",
           "cross_entropy": bench_cross_entropy(args, dev), "metrics": bench_metrics(args, dev)}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
