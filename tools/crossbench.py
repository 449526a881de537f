"""Measurement tool for the cross networks (torchrec_amd/modules/crossnet.py, csrc/crossnet.hip): HIP-event time of one
forward + backward of each module on its kernel path, next to the plain torch composition of the same formula (the
module's own fall-back function) on the same tensors and parameters, timed in the same process, the two alternating
round by round.  Both must agree (max |a - b| / max |b| of output and every gradient) before anything is timed.

Shapes: B = 65 536 with (N, r, L) = (3456, 512, 3) — the MLPerf DLRM-v2 interaction — and (512, 128, 3); VectorCrossNet
runs at both N.  `spread_us` is the larger of the two paths' (max - min) over the rounds; `kernel_not_slower` says whether
the kernel path's median is within that spread of the composition's or below it — the rule by which a net ships on its
kernel path.  A record: nothing is asserted.

Usage: python tools/crossbench.py [--rounds 10] [--warmup 3] [--out profiles/crossnet_crossbench.json]
Under a profiler (per-kernel split): rocprofv3 --kernel-trace --stats -d OUT -- python tools/crossbench.py --rounds 3"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))

SHAPES = [(65536, 3456, 512, 3), (65536, 512, 128, 3)]  # (B, N, r, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from torchrec_amd.modules import crossnet

    if not torch.cuda.is_available():
        raise SystemExit("crossbench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    results = []
    for B, N, r, L in SHAPES:
        for kind in ("CrossNet", "LowRankCrossNet", "VectorCrossNet"):
            torch.manual_seed(N + len(kind))
            if kind == "LowRankCrossNet":
                m = crossnet.LowRankCrossNet(N, L, low_rank=r).to(dev)
                compose = lambda t: crossnet._low_rank_cross_torch(t, list(m.W_kernels), list(m.V_kernels), list(m.bias))  # noqa: E731
            elif kind == "CrossNet":
                m = crossnet.CrossNet(N, L).to(dev)
                compose = lambda t: crossnet._cross_torch(t, list(m.kernels), list(m.bias))  # noqa: E731
            else:
                m = crossnet.VectorCrossNet(N, L).to(dev)
                compose = lambda t: crossnet._vector_cross_torch(t, list(m.kernels), list(m.bias))  # noqa: E731
            with torch.no_grad():
                for b in m.bias:
                    b.normal_(0.0, 0.1)
            x = torch.randn(B, N, device=dev).requires_grad_()
            g = torch.randn(B, N, device=dev)
            params = list(m.parameters())

            def step(fn):
                x.grad = None
                for p in params:
                    p.grad = None
                fn(x).backward(g)
                return [x.grad] + [p.grad for p in params]

            got, want = step(m), step(compose)
            with torch.no_grad():
                out_err = float((m(x) - compose(x)).abs().max() / compose(x).abs().max())
            grad_err = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want))
            if not (out_err < 1e-3 and grad_err < 1e-3):
                raise SystemExit(f"crossbench: {kind} at N={N}: kernel path and composition differ: {out_err} {grad_err}")
            del got, want
            for _ in range(args.warmup):
                step(m)
                step(compose)
            torch.cuda.synchronize()
            t_hip, t_torch = [], []
            for _ in range(args.rounds):  # alternating, one process, one device
                for fn, sink in ((m, t_hip), (compose, t_torch)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    step(fn)
                    b.record()
                    b.synchronize()
                    sink.append(a.elapsed_time(b) * 1e3)  # us
            med_h, med_t = statistics.median(t_hip), statistics.median(t_torch)
            spread = max(max(t_hip) - min(t_hip), max(t_torch) - min(t_torch))
            row = {"net": kind, "B": B, "N": N, "r": r if kind == "LowRankCrossNet" else None, "L": L, "rounds": args.rounds,
                   "kernel_us_median": round(med_h, 1), "kernel_us_min": round(min(t_hip), 1), "kernel_us_max": round(max(t_hip), 1),
                   "torch_us_median": round(med_t, 1), "torch_us_min": round(min(t_torch), 1), "torch_us_max": round(max(t_torch), 1),
                   "spread_us": round(spread, 1), "torch_over_kernel": round(med_t / med_h, 3),
                   "kernel_not_slower": bool(med_h <= med_t + spread),
                   "out_rel_diff": out_err, "grad_rel_diff_max": grad_err}
            results.append(row)
            print(json.dumps(row), flush=True)
            del m, x, g, params
            torch.cuda.empty_cache()
    doc = {"tool": "tools/crossbench.py", "device": torch.cuda.get_device_name(0),
           "timer": "HIP events round one forward + backward, kernel path and torch composition alternating",
           "results": results}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
