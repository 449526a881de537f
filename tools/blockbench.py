"""Measurement tool for BERT4Rec's TransformerBlock (torchrec_amd/models/bert4rec.py, csrc/residual_layernorm.hip): HIP-event
time of one forward + backward of the block with its residual / dropout / LayerNorm passes fused (`kernel_path = True`), next
to the same block on the torch expression (`kernel_path = False`) on the same tensors and parameters, in the same process,
the two alternating round by round.  The attention stays on its own kernel in both: only the block's switch moves.  With
dropout 0 both must agree (max |a - b| / max |b|: the output to 1e-5, every gradient to 5e-2 — see bench_block) before
anything is timed; with dropout 0.1 (training mode) the two draw different masks and only the times are compared.

Shapes (B, L, emb_dim, nhead): (128, 100, 256, 2) — the reference's defaults —, (1024, 100, 256, 2), (128, 200, 128, 2).
Each timed sample is `--steps` forward + backward pairs between two events (one pair of a small shape is mostly launch
overhead and event noise), reported per pair.  `spread_us` is the larger of the two paths' (max - min) over the rounds;
`kernel_not_slower` says whether the fused path's median is within that spread of the torch path's or below it.  Each row
also carries the peak of `torch.cuda.max_memory_allocated` over one forward + backward of either path above the level before
it.  A record: nothing about speed is asserted.

Usage: python tools/blockbench.py [--rounds 20] [--warmup 5] [--steps 10] [--out profiles/bert4rec_blockbench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from attnbench import _alternate, _peak_bytes, _stats  # noqa: E402

SHAPES = [(128, 100, 256, 2), (1024, 100, 256, 2), (128, 200, 128, 2)]


def bench_block(B, L, dim, H, dropout, rounds, warmup, steps, dev):
    import torch

    from torchrec_amd.models import bert4rec

    torch.manual_seed(B + L + dim)
    m = bert4rec.TransformerBlock(dim, H, 4 * dim, dropout, device=dev).train(dropout > 0)
    x = torch.randn(B, L, dim, device=dev).requires_grad_()
    g = torch.randn(B, L, dim, device=dev)
    lengths = torch.randint(L // 4, L + 1, (B,), device=dev)
    mask = (torch.arange(L, device=dev)[None, :] < lengths[:, None])[:, None, None, :].expand(B, 1, L, L)
    params = list(m.parameters())

    def step(kernel):
        m.kernel_path = kernel
        x.grad = None
        for p in params:
            p.grad = None
        out = m(x, mask)
        out.backward(g)
        assert m.last_path == ("kernel" if kernel else "torch") and m.attention.last_path == "kernel"
        return [out.detach(), x.grad] + [p.grad for p in params]

    def many(kernel):
        for _ in range(steps):
            step(kernel)

    row = {"B": B, "L": L, "emb_dim": dim, "nhead": H, "dropout": dropout, "rounds": rounds, "steps_per_sample": steps}
    if dropout == 0:
        got, want = step(True), step(False)
        # the key projection's bias has an exactly zero gradient: every tensor is measured against its own scale or a
        # thousandth of the largest, whichever is larger.  The output agrees to rounding.  The gradients agree less closely
        # at these sizes on ANY two float32 paths (the torch path against its own float64 copy shows the same): among the
        # 10^7 outputs of w_1 a few lie within rounding of 0, pass the ReLU on one path and not on the other, and each moves
        # gradient elements by O(1).
        floor = 1e-3 * max(float(b.abs().max()) for b in want)
        diffs = [float((a - b).abs().max()) / max(float(b.abs().max()), floor) for a, b in zip(got, want)]
        row["out_rel_diff"], row["grad_rel_diff_max"] = diffs[0], max(diffs[1:])
        if not (row["out_rel_diff"] < 1e-5 and row["grad_rel_diff_max"] < 5e-2):
            raise SystemExit(f"blockbench: at {(B, L, dim, H)} fused path and torch path differ: out {row['out_rel_diff']}, "
                             f"gradients {row['grad_rel_diff_max']}")
        del got, want
    ts = _alternate({"kernel": lambda: many(True), "torch": lambda: many(False)}, rounds, warmup)
    ts = {n: [t / steps for t in v] for n, v in ts.items()}
    spread = max(max(t) - min(t) for t in ts.values())
    med_k, med_t = statistics.median(ts["kernel"]), statistics.median(ts["torch"])
    row.update(_stats("kernel", ts["kernel"]))
    row.update(_stats("torch", ts["torch"]))
    row.update({"spread_us": round(spread, 1), "torch_over_kernel": round(med_t / med_k, 3),
                "kernel_not_slower": bool(med_k <= med_t + spread)})
    x.grad = None
    row["kernel_peak_MiB"] = round(_peak_bytes(lambda: step(True)) / 2**20, 1)
    x.grad = None
    row["torch_peak_MiB"] = round(_peak_bytes(lambda: step(False)) / 2**20, 1)
    row["one_residual_stream_MiB"] = round(B * L * dim * 4 / 2**20, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("blockbench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    results = []
    for B, L, dim, H in SHAPES:
        for dropout in (0.0, 0.1):
            results.append(bench_block(B, L, dim, H, dropout, args.rounds, args.warmup, args.steps, dev))
            print(json.dumps(results[-1]), flush=True)
            torch.cuda.empty_cache()
    doc = {"tool": "tools/blockbench.py", "device": torch.cuda.get_device_name(0),
           "timer": "HIP events round `steps_per_sample` forward + backward pairs, fused path and torch path alternating",
           "results": results}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
