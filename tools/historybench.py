"""Measurement tool for BERT4Rec's HistoryArch (torchrec_amd/models/bert4rec.py, csrc/history_arch.hip): HIP-event time of one
forward + backward of the module on its kernel path (`kernel_path = True`: one launch each way, then the item table's own
backward) next to the same module on the torch expression (`kernel_path = False`: lookup, jagged_2d_to_dense, positional
add, nn.LayerNorm, nn.Dropout) on the same batch and parameters, in the same process, the two alternating round by round.
The item table (26 746 rows, ml-20m's vocabulary) sits behind the fused class with ADAM, as in the reference's main; both
paths apply its update in every backward.  History lengths are uniform in [L / 4, L].  With dropout 0 a row records
max |a - b| / max |b| of the output and of the three parameter gradients between the two paths; the table moves by one ADAM
step of 1e-3 between the two calls, which is what bounds that agreement (tests/test_history_arch_gpu.py compares the paths
on equal tables).  With dropout 0.1 (training mode) the two draw different masks and only the times are compared.

Shapes (B, L, emb_dim): (128, 100, 256) — the reference's defaults —, (1024, 100, 256), (128, 200, 128).  Timing, `spread_us`,
`kernel_not_slower` and the peak-memory columns are tools/blockbench.py's.  A record: nothing about speed is asserted.

Usage: python tools/historybench.py [--rounds 20] [--warmup 5] [--steps 10] [--out profiles/bert4rec_historybench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from attnbench import _alternate, _peak_bytes, _stats  # noqa: E402

SHAPES = [(128, 100, 256), (1024, 100, 256), (128, 200, 128)]
VOCAB = 26746


def bench_history(B, L, dim, dropout, rounds, warmup, steps, dev):
    import torch

    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from torchrec_amd.models import bert4rec
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    torch.manual_seed(B + L + dim)
    fused = {"optimizer": EmbOptimType.ADAM, "learning_rate": 1e-3, "eps": 1e-8, "beta1": 0.9, "beta2": 0.999,
             "weight_decay": 0.0}
    m = bert4rec.HistoryArch(VOCAB, L, dim, dropout=dropout, device=dev, fused_params=fused).train(dropout > 0)
    lengths = torch.randint(L // 4, L + 1, (B,), device=dev, dtype=torch.int32)
    ids = torch.randint(1, VOCAB, (int(lengths.sum()),), device=dev, dtype=torch.int64)
    kjt = KeyedJaggedTensor.from_lengths_sync(["item"], ids, lengths)
    g = torch.randn(B, L, dim, device=dev)
    params = [m.positional, m.layernorm.weight, m.layernorm.bias]

    def step(kernel):
        m.kernel_path = kernel
        for p in params:
            p.grad = None
        out = m(kjt)
        out.backward(g)
        assert m.last_path == ("kernel" if kernel else "torch")
        return [out.detach()] + [p.grad for p in params]

    def many(kernel):
        for _ in range(steps):
            step(kernel)

    row = {"B": B, "L": L, "emb_dim": dim, "dropout": dropout, "rounds": rounds, "steps_per_sample": steps}
    if dropout == 0:
        got, want = step(True), step(False)  # (the table has moved by one ADAM step of 1e-3 in between)
        diffs = [float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(got, want)]
        row["out_rel_diff"], row["grad_rel_diff_max"] = diffs[0], max(diffs[1:])
        del got, want
    ts = _alternate({"kernel": lambda: many(True), "torch": lambda: many(False)}, rounds, warmup)
    ts = {n: [t / steps for t in v] for n, v in ts.items()}
    spread = max(max(t) - min(t) for t in ts.values())
    med_k, med_t = statistics.median(ts["kernel"]), statistics.median(ts["torch"])
    row.update(_stats("kernel", ts["kernel"]))
    row.update(_stats("torch", ts["torch"]))
    row.update({"spread_us": round(spread, 1), "torch_over_kernel": round(med_t / med_k, 3),
                "kernel_not_slower": bool(med_k <= med_t + spread)})
    row["kernel_peak_MiB"] = round(_peak_bytes(lambda: step(True)) / 2**20, 1)
    row["torch_peak_MiB"] = round(_peak_bytes(lambda: step(False)) / 2**20, 1)
    row["one_stream_MiB"] = round(B * L * dim * 4 / 2**20, 1)
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
        raise SystemExit("historybench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    results = []
    for B, L, dim in SHAPES:
        for dropout in (0.0, 0.1):
            results.append(bench_history(B, L, dim, dropout, args.rounds, args.warmup, args.steps, dev))
            print(json.dumps(results[-1]), flush=True)
            torch.cuda.empty_cache()
    doc = {"tool": "tools/historybench.py", "device": torch.cuda.get_device_name(0),
           "timer": "HIP events round `steps_per_sample` forward + backward pairs, kernel path and torch path alternating",
           "results": results}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
