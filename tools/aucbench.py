"""Measurement tool for tbe_auroc_counts_f32 (csrc/auroc.hip): HIP-event time of one call (prepare + pair sort + two reduce
launches) at several sizes, on uniform random predictions and on predictions quantised to 256 levels, next to a torch
restatement of the same integers (torch.sort + cumsum + unique_consecutive) timed in the same process, the two
alternating round by round.  Both must produce the same 2U, P and N before anything is timed.  A record, not a pass
condition: nothing is asserted about speed.

Algorithmic bytes per sample (float32 labels), the traffic the chosen algorithm cannot avoid: prepare reads 4 + 4 and writes
8; the sort's first histogram reads 4 and each of its 4 passes reads 8 and writes 8; each of the two reduce launches reads
8: 8 + 8 + 4 + 64 + 16 = 100 B.  `frac_hbm_peak` prices those bytes against the 8 TB/s spec peak (and `frac_hbm_copy`
against the 6.29 TB/s a float4 copy reaches); at 2^20 samples every array fits the 256 MiB Infinity Cache, so the figure
there is no HBM figure.

Usage: python tools/aucbench.py [--log2 20 24 26] [--rounds 10] [--out profiles/auroc_aucbench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))

BYTES_PER_SAMPLE = 100
HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12


def torch_counts(preds, labels):
    """(2U, P, N) with torch ops on the device: the restatement a user without this library would write."""
    import torch

    xs, idx = torch.sort(preds)  # float compare: -0.0 ties with +0.0
    ys = labels[idx].to(torch.int64)
    pc, nc = torch.cumsum(ys, 0), torch.cumsum(1 - ys, 0)  # inclusive counts
    _, cnt = torch.unique_consecutive(xs, return_counts=True)
    ends = torch.cumsum(cnt, 0) - 1  # last sample of every tie group
    pe, ne = pc[ends], nc[ends]
    zero = torch.zeros(1, dtype=torch.int64, device=preds.device)
    ps, ns = torch.cat([zero, pe[:-1]]), torch.cat([zero, ne[:-1]])
    return ((pe - ps) * (ns + ne)).sum(), pc[-1], nc[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[20, 24, 26])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from fbgemm_gpu import _lib
    from fbgemm_gpu._lib import check, ptr, stream_ptr

    if not torch.cuda.is_available():
        raise SystemExit("aucbench: no GPU (a timing taken anywhere else says nothing)")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    results = []
    for lg in args.log2:
        n = 1 << lg
        for dist_name in ("uniform", "q256"):
            g = torch.Generator(device=dev)
            g.manual_seed(lg * 10 + (dist_name == "q256"))
            preds = torch.rand(n, device=dev, generator=g)
            if dist_name == "q256":
                preds = torch.floor(preds * 256) / 256
            labels = (torch.rand(n, device=dev, generator=g) < 0.1 + 0.5 * preds).float()
            ws = _lib.workspace(lib.tbe_auroc_workspace_bytes(n), dev)
            counts = torch.empty(6, dtype=torch.int64, device=dev)

            def hip_call():
                check(lib.tbe_auroc_counts_f32(ptr(preds), ptr(labels), 4, n, 0.5, ptr(counts), ptr(ws), ws.numel(),
                                               stream_ptr(dev)), "tbe_auroc_counts_f32")

            hip_call()
            got = counts.tolist()
            want = [int(v) for v in torch_counts(preds, labels)]
            if got[:3] != want or got[4] or got[5]:
                raise SystemExit(f"aucbench: results differ at n=2^{lg} {dist_name}: hip {got} torch {want}")
            for _ in range(args.warmup):
                hip_call()
                torch_counts(preds, labels)
            torch.cuda.synchronize()
            t_hip, t_torch = [], []
            for _ in range(args.rounds):  # alternating, one process, one device
                for fn, sink in ((hip_call, t_hip), (lambda: torch_counts(preds, labels), t_torch)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    sink.append(a.elapsed_time(b) * 1e3)  # us
            _lib.raise_on_faults("aucbench")
            med = statistics.median(t_hip)
            row = {
                "n": n, "preds": dist_name, "rounds": args.rounds,
                "hip_us_median": round(med, 1), "hip_us_min": round(min(t_hip), 1),
                "torch_us_median": round(statistics.median(t_torch), 1), "torch_us_min": round(min(t_torch), 1),
                "torch_over_hip": round(statistics.median(t_torch) / med, 2),
                "algorithmic_bytes": BYTES_PER_SAMPLE * n,
                "algorithmic_GBs": round(BYTES_PER_SAMPLE * n / (med * 1e-6) / 1e9, 1),
                "frac_hbm_peak": round(BYTES_PER_SAMPLE * n / (med * 1e-6) / HBM_PEAK, 4),
                "frac_hbm_copy": round(BYTES_PER_SAMPLE * n / (med * 1e-6) / HBM_COPY, 4),
                "two_u": got[0], "positives": got[1], "negatives": got[2],
            }
            results.append(row)
            print(json.dumps(row), flush=True)
            del preds, labels, ws
            torch.cuda.empty_cache()
    doc = {"tool": "tools/aucbench.py", "device": torch.cuda.get_device_name(0), "timer": "HIP events round one call",
           "bytes_per_sample": BYTES_PER_SAMPLE, "hbm_peak_Bps": HBM_PEAK, "hbm_copy_Bps": HBM_COPY,
           "torch_restatement": "torch.sort + cumsum + unique_consecutive", "results": results}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
