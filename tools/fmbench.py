"""Measurement tool for the DeepFM interaction (torchrec_amd/modules/deepfm.py, csrc/deepfm.hip): HIP-event time of one
forward + backward of `cat + FM` — the concatenated row of the deep branch and the factorization-machine term, with both
output gradients flowing back into `dense [B, D]` and the KeyedTensor values `[B, F D]` — for three things that alternate
round by round in one process:

  kernel  the fused two-input path FMInteractionArch takes (fm_forward(want_cat) + fm_backward: two launches)
  torch   the reference's expression on the same tensors: dense and the F per-feature views concatenated once per branch
          (torchrec/modules/deepfm.py:28-32), x * x, two row sums, a square (:209-215), autograd's backward
  copy    one device-to-device copy_ of the bytes the kernels must move: forward 4 B N read + 4 B N written, backward
          8 B N read + 4 B N written = 20 B N bytes, i.e. a copy of 2.5 B N floats

Shapes: B = 65 536 and B = 4096 at D = 128, F = 26 (N = 3456).  Every shape is warmed up first; each figure is the median of
--rounds (at least 50) device-event timings.  A record: nothing is asserted but that the two paths agree.

Usage: python tools/fmbench.py [--rounds 50] [--warmup 5] [--out profiles/deepfm_fmbench.json]
Per-kernel split, in a run of its own: rocprofv3 --kernel-trace --stats -d OUT -- python tools/fmbench.py --rounds 50"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))

SHAPES = [(65536, 128, 26), (4096, 128, 26)]  # (B, D, F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepfm_fmbench.json"))
    args = ap.parse_args()
    if args.rounds < 50:
        raise SystemExit("fmbench: at least 50 rounds (the figure is a median)")
    import torch

    from torchrec_amd.modules import deepfm

    if not torch.cuda.is_available():
        raise SystemExit("fmbench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    results = []
    for B, D, F in SHAPES:
        torch.manual_seed(B)
        N = (F + 1) * D
        dense = torch.randn(B, D, device=dev).requires_grad_()
        values = torch.randn(B, F * D, device=dev).requires_grad_()
        gcat, gfm = torch.randn(B, N, device=dev), torch.randn(B, 1, device=dev)
        src = torch.empty(B * N * 5 // 2, device=dev).normal_()
        dst = torch.empty_like(src)

        def kernel():
            fm, cat = deepfm.fm_and_cat([dense, values], True)
            return cat, fm

        def reference():
            views = [dense] + [values[:, f * D:(f + 1) * D] for f in range(F)]
            return deepfm._get_flatten_input(views), deepfm._fm_torch(deepfm._get_flatten_input(views))

        def step(fn):
            dense.grad = values.grad = None
            cat, fm = fn()
            torch.autograd.backward([cat, fm], [gcat, gfm])
            return cat.detach(), fm.detach(), dense.grad, values.grad

        got, want = step(kernel), step(reference)
        diffs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want)]
        if not max(diffs) < 1e-4:
            raise SystemExit(f"fmbench: B={B}: kernel path and torch expression differ: {diffs}")
        del got, want
        for _ in range(args.warmup):
            step(kernel)
            step(reference)
            dst.copy_(src)
        torch.cuda.synchronize()
        times = {"kernel": [], "torch": [], "copy": []}
        for _ in range(args.rounds):  # alternating, one process, one device
            for name, fn in (("kernel", lambda: step(kernel)), ("torch", lambda: step(reference)), ("copy", lambda: dst.copy_(src))):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3)  # us
        med = {k: statistics.median(v) for k, v in times.items()}
        row = {"B": B, "D": D, "F": F, "N": N, "rounds": args.rounds, "bytes_must_move": 20 * B * N}
        for k, v in times.items():
            row.update({f"{k}_us_median": round(med[k], 1), f"{k}_us_min": round(min(v), 1), f"{k}_us_max": round(max(v), 1)})
        row.update({"copy_GBps": round(20 * B * N / med["copy"] / 1e3, 1), "kernel_GBps": round(20 * B * N / med["kernel"] / 1e3, 1),
                    "kernel_share_of_copy_rate": round(med["copy"] / med["kernel"], 3),
                    "torch_over_kernel": round(med["torch"] / med["kernel"], 3), "rel_diff_max": max(diffs)})
        results.append(row)
        print(json.dumps(row), flush=True)
        del dense, values, gcat, gfm, src, dst
        torch.cuda.empty_cache()
    doc = {"tool": "tools/fmbench.py", "device": torch.cuda.get_device_name(0),
           "timer": "HIP events round one forward + backward of cat + FM; kernel path, torch expression and a copy_ of the "
                    "20 B N bytes alternating; median of the rounds; host launch time is inside every figure",
           "results": results}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
