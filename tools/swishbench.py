"""Measurement tool for SwishLayerNorm (torchrec_amd/modules/activation.py, csrc/swish_layernorm.hip): HIP-event time of one
forward + backward of the module on its kernel path, next to the plain torch composition of the same formula (the module's
own fall-back function `_swish_layernorm_torch`) on the same tensors and parameters, timed in the same process, the two
alternating round by round.  Both must agree (max |a - b| / max |b| of output and every gradient) before anything is timed.

Shapes: B = 65 536 and 8192 at N = 256, 512, 1024, 4096.  `spread_us` is the larger of the two paths' (max - min) over the
rounds; `kernel_not_slower` says whether the kernel path's median is within that spread of the composition's or below it
(the rule of DESIGN.md 3k).  Each row also carries the peak of `torch.cuda.max_memory_allocated` over one forward + backward
of either path, above the level before it, and the two kernels alone: time, bytes moved and bytes/s, next to a
device-to-device copy of the same [B, N] floats on the same device.  A record: nothing is asserted.

Usage: python tools/swishbench.py [--rounds 10] [--warmup 3] [--out profiles/swish_layernorm_swishbench.json]
Under a profiler (per-kernel split): rocprofv3 --kernel-trace --stats -d OUT -- python tools/swishbench.py --rounds 3"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))

SHAPES = [(B, N) for B in (65536, 8192) for N in (256, 512, 1024, 4096)]


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


def _kernels_alone(x, g, gamma, beta, eps, rounds):
    """The two kernels alone (the backward with its finishing launch) and a device copy of [B, N] floats: median us, bytes
    moved, GB/s."""
    import torch

    B, N = x.shape
    dst = torch.empty_like(x)
    out, stats = torch.ops.tbe_hip.swish_layernorm_forward(x, gamma, beta, eps)
    wide, narrow = 4 * B * N, 4 * 2 * B
    runs = {"forward": (lambda: torch.ops.tbe_hip.swish_layernorm_forward(x, gamma, beta, eps), 2 * wide + narrow),
            "backward": (lambda: torch.ops.tbe_hip.swish_layernorm_backward(g, x, stats, gamma, beta), 3 * wide + narrow),
            "device_copy": (lambda: dst.copy_(x), 2 * wide)}
    res = {}
    for name, (fn, nbytes) in runs.items():
        fn()
        us = statistics.median(_event_us(fn) for _ in range(max(rounds, 5)))
        res[name] = {"us_median": round(us, 1), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from torchrec_amd.modules import activation

    if not torch.cuda.is_available():
        raise SystemExit("swishbench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    results = []
    for B, N in SHAPES:
        torch.manual_seed(B + N)
        m = activation.SwishLayerNorm(N, device=dev)
        with torch.no_grad():
            m.norm[0].weight.add_(0.5 * torch.randn(N, device=dev))
            m.norm[0].bias.add_(0.5 * torch.randn(N, device=dev))
        compose = lambda t: activation._swish_layernorm_torch(t, m.norm)  # noqa: E731
        x = (0.5 + 2.0 * torch.randn(B, N, device=dev)).requires_grad_()
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
        if not (out_err < 1e-4 and grad_err < 1e-4):
            raise SystemExit(f"swishbench: at {(B, N)}: kernel path and composition differ: {out_err} {grad_err}")
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
        row = {"B": B, "N": N, "rounds": args.rounds,
               "kernel_us_median": round(med_h, 1), "kernel_us_min": round(min(t_hip), 1), "kernel_us_max": round(max(t_hip), 1),
               "torch_us_median": round(med_t, 1), "torch_us_min": round(min(t_torch), 1), "torch_us_max": round(max(t_torch), 1),
               "spread_us": round(spread, 1), "torch_over_kernel": round(med_t / med_h, 3),
               "kernel_not_slower": bool(med_h <= med_t + spread),
               "kernel_peak_MiB": round(peak_h / 2**20, 1), "torch_peak_MiB": round(peak_t / 2**20, 1),
               "one_matrix_MiB": round(B * N * 4 / 2**20, 1), "out_rel_diff": out_err, "grad_rel_diff_max": grad_err}
        x.grad = None
        row["kernels_alone"] = _kernels_alone(x.detach(), g, m.norm[0].weight.detach(), m.norm[0].bias.detach(),
                                              m.norm[0].eps, args.rounds)
        results.append(row)
        print(json.dumps(row), flush=True)
        del m, x, g, params
        torch.cuda.empty_cache()
    doc = {"tool": "tools/swishbench.py", "device": torch.cuda.get_device_name(0),
           "timer": "HIP events round one forward + backward, kernel path and torch composition alternating",
           "results": results}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
