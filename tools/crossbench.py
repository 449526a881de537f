"""Measurement tool for the cross networks (torchrec_amd/modules/crossnet.py, csrc/crossnet.hip): HIP-event time of one
forward + backward of each module on its kernel path, next to the plain torch composition of the same formula (the
module's own fall-back function) on the same tensors and parameters, timed in the same process, the two alternating
round by round.  Both must agree (max |a - b| / max |b| of output and every gradient) before anything is timed.

Shapes: B = 65 536 with (N, r, L) = (3456, 512, 3) — the MLPerf DLRM-v2 interaction — and (512, 128, 3); VectorCrossNet
runs at both N.  `spread_us` is the larger of the two paths' (max - min) over the rounds; `kernel_not_slower` says whether
the kernel path's median is within that spread of the composition's or below it — the rule by which a net ships on its
kernel path.  A record: nothing is asserted.

`--mixture` measures the fourth net instead, LowRankMixtureCrossNet with its K experts folded, against
`_low_rank_mixture_cross_torch` (the reference's expert stack): B = 8192 and 65 536 at (N, r, L) = (3456, 512, 3) with
K = 1 and 4, and (512, 32, 3) with K = 4.  Its agreement gate is the gradients' 2-norm (a ReLU at 0 may take either side
in either path; both measures are recorded).  Each row also carries the peak of `torch.cuda.max_memory_allocated` over one
forward + backward of either path, above the level before it, and — for K > 1 — the gate kernels alone at the row's
(B, K, r): time, bytes moved and bytes/s, next to a device-to-device copy of the same [B, K r] floats on the same device.

Usage: python tools/crossbench.py [--mixture] [--rounds 10] [--warmup 3] [--out profiles/crossnet_crossbench.json]
Under a profiler (per-kernel split): rocprofv3 --kernel-trace --stats -d OUT -- python tools/crossbench.py --rounds 3"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))

SHAPES = [(65536, 3456, 512, 3), (65536, 512, 128, 3)]  # (B, N, r, L)
MIXTURE_SHAPES = [(B, 3456, 512, 3, K) for B in (8192, 65536) for K in (1, 4)] + \
    [(B, 512, 32, 3, 4) for B in (8192, 65536)]  # (B, N, r, L, K)


def _event_us(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _peak_bytes(fn):
    """Peak of allocated memory over fn(), above the level before it."""
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def _gate_kernels(B, K, r, rounds, dev):
    """The two gate kernels alone and a device copy of [B, K r] floats: median us, bytes moved, GB/s."""
    import torch

    a2 = torch.randn(K, B, r, device=dev)
    logits = torch.randn(B, K, device=dev)
    gm = torch.randn(B, K * r, device=dev)
    dst = torch.empty_like(gm)
    m, p = torch.ops.tbe_hip.mixture_gate_forward(a2, logits)
    wide, narrow = 4 * B * K * r, 4 * B * K
    runs = {"gate_forward": (lambda: torch.ops.tbe_hip.mixture_gate_forward(a2, logits), 2 * wide + 2 * narrow),
            "gate_backward": (lambda: torch.ops.tbe_hip.mixture_gate_backward(gm, a2, p), 3 * wide + 2 * narrow),
            "device_copy": (lambda: dst.copy_(gm), 2 * wide)}
    out = {}
    for name, (fn, nbytes) in runs.items():
        fn()
        us = statistics.median(_event_us(fn) for _ in range(max(rounds, 5)))
        out[name] = {"us_median": round(us, 1), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
    return out


def mixture(args, dev):
    import torch

    from torchrec_amd.modules import crossnet

    results = []
    for B, N, r, L, K in MIXTURE_SHAPES:
        torch.manual_seed(N + K)
        m = crossnet.LowRankMixtureCrossNet(N, L, num_experts=K, low_rank=r).to(dev)
        gate_w = [g.weight for g in m.gates] if m.gates is not None else []
        compose = lambda t: crossnet._low_rank_mixture_cross_torch(  # noqa: E731
            t, list(m.U_kernels), list(m.V_kernels), list(m.bias), gate_w, list(m.C_kernels))
        with torch.no_grad():
            for b in m.bias:
                b.normal_(0.0, 0.1)
            for n, q in m.named_parameters():  # the 3-D xavier fans shrink the kernels with K r: matrix-sized instead
                if n.split("_")[0] in ("U", "V", "C"):
                    q.normal_(0.0, (2.0 / (q.shape[1] + q.shape[2])) ** 0.5)
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
            ref_out = compose(x)
            out_err = float((m(x) - ref_out).abs().max() / ref_out.abs().max())
            del ref_out
        grad_err = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want))
        # The gate is the 2-norm: a ReLU whose argument is within rounding of 0 takes either side in either path, and ONE
        # such element moves a row of a [K, r, r] gradient by 1 / sqrt(B) of its scale (float32 against float64 shows the
        # same for both paths); a wrong formula moves everything.
        grad_l2 = max(float((a - b).norm() / b.norm()) for a, b in zip(got, want))
        if not (out_err < 1e-3 and grad_l2 < 1e-2):
            raise SystemExit(f"crossbench: mixture at {(B, N, r, L, K)}: kernel path and composition differ: {out_err} "
                             f"{grad_l2} {grad_err}")
        del got, want
        for _ in range(args.warmup):
            step(m)
            step(compose)
        x.grad = None
        for p in params:
            p.grad = None
        peak_h = _peak_bytes(lambda: step(m))
        x.grad = None
        for p in params:
            p.grad = None
        peak_t = _peak_bytes(lambda: step(compose))
        t_hip, t_torch = [], []
        for _ in range(args.rounds):  # alternating, one process, one device
            t_hip.append(_event_us(lambda: step(m)))
            t_torch.append(_event_us(lambda: step(compose)))
        med_h, med_t = statistics.median(t_hip), statistics.median(t_torch)
        spread = max(max(t_hip) - min(t_hip), max(t_torch) - min(t_torch))
        row = {"net": "LowRankMixtureCrossNet", "B": B, "N": N, "r": r, "L": L, "K": K, "rounds": args.rounds,
               "kernel_us_median": round(med_h, 1), "kernel_us_min": round(min(t_hip), 1), "kernel_us_max": round(max(t_hip), 1),
               "torch_us_median": round(med_t, 1), "torch_us_min": round(min(t_torch), 1), "torch_us_max": round(max(t_torch), 1),
               "spread_us": round(spread, 1), "torch_over_kernel": round(med_t / med_h, 3),
               "kernel_not_slower": bool(med_h <= med_t + spread),
               "kernel_peak_MiB": round(peak_h / 2**20, 1), "torch_peak_MiB": round(peak_t / 2**20, 1),
               "one_layer_stack_MiB": round(B * N * K * 4 / 2**20, 1),
               "out_rel_diff": out_err, "grad_rel_diff_max": grad_err, "grad_rel_l2_diff_max": grad_l2}
        del m, x, g, params, gate_w
        torch.cuda.empty_cache()
        if K > 1:
            row["gate_kernels"] = _gate_kernels(B, K, r, args.rounds, dev)
        results.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--mixture", action="store_true", help="LowRankMixtureCrossNet instead of the three other nets")
    args = ap.parse_args()
    import torch

    from torchrec_amd.modules import crossnet

    if not torch.cuda.is_available():
        raise SystemExit("crossbench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    results = mixture(args, dev) if args.mixture else []
    for B, N, r, L in ([] if args.mixture else SHAPES):
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
