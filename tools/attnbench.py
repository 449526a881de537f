"""Measurement tool for BERT4Rec's attention (torchrec_amd/models/bert4rec.py, csrc/attention.hip): HIP-event time of one
forward + backward of MultiHeadedAttention on its kernel path, next to the same module forced onto `_attention_torch` (the
reference's formula) on the same tensors and parameters, timed in the same process, the two alternating round by round.  With
dropout 0 both must agree (max |a - b| / max |b| of output and every gradient) before anything is timed; with dropout 0.1
(training mode) the two draw different masks and only the times are compared.

Shapes (B, L, emb_dim, nhead): (128, 100, 256, 2) — the reference's defaults —, (128, 200, 128, 2), (1024, 100, 256, 2).
`spread_us` is the larger of the two paths' (max - min) over the rounds; `kernel_not_slower` says whether the kernel path's
median is within that spread of the torch path's or below it (the rule of DESIGN.md 3k).  Each row also carries the peak of
`torch.cuda.max_memory_allocated` over one forward + backward of either path above the level before it, and the attention
alone, without the four projections: the two kernels, and `_attention_torch` forward + backward on the same projections.

JaggedTensor.to_padded_dense is timed at B = 128 and 1024 (histories of 0 .. 150 ids, desired_length 100) against the
reference's loop (torchrec/sparse/jagged_tensor.py:344-363), restated here.  A record: nothing is asserted.

Usage: python tools/attnbench.py [--rounds 20] [--warmup 5] [--out profiles/bert4rec_attnbench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))

SHAPES = [(128, 100, 256, 2), (128, 200, 128, 2), (1024, 100, 256, 2)]


def _event_us(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _peak_bytes(fn):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def _stats(name, ts):
    return {f"{name}_us_median": round(statistics.median(ts), 1), f"{name}_us_min": round(min(ts), 1),
            f"{name}_us_max": round(max(ts), 1)}


def _alternate(fns, rounds, warmup):
    """{name: [us per round]}: the functions alternating round by round."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ts = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            ts[n].append(_event_us(fn))
    return ts


def reference_to_padded_dense(values, lengths, desired_length, padding_value=0.0, pad_from_beginning=True,
                              chop_from_beginning=True):
    """torchrec/sparse/jagged_tensor.py:344-363, restated."""
    import torch

    lengths_list = lengths.tolist()
    N = max(lengths_list) if desired_length is None else desired_length
    offset, rows = 0, []
    for length in lengths_list:
        value = values[offset:offset + length]
        if length <= N:
            pad = torch.full([N - length], padding_value, device=values.device)
            value = torch.cat((pad, value), 0) if pad_from_beginning else torch.cat((value, pad), 0)
        else:
            value = value[-N:] if chop_from_beginning else value[:N]
        rows.append(value)
        offset += length
    return torch.stack(rows)


def bench_attention(B, L, dim, H, dropout, rounds, warmup, dev):
    import torch

    from torchrec_amd.distributed._device_ops import attention_backward, attention_forward
    from torchrec_amd.models import bert4rec

    torch.manual_seed(B + L + dim)
    m = bert4rec.MultiHeadedAttention(num_heads=H, dim_model=dim, dropout=dropout, device=dev).train(dropout > 0)
    x = torch.randn(B, L, dim, device=dev).requires_grad_()
    g = torch.randn(B, L, dim, device=dev)
    lengths = torch.randint(L // 4, L + 1, (B,), device=dev)
    valid = torch.arange(L, device=dev)[None, :] < lengths[:, None]
    mask = valid[:, None, None, :].expand(B, 1, L, L)
    params = list(m.parameters())

    def step(kernel):
        m.kernel_path = kernel
        x.grad = None
        for p in params:
            p.grad = None
        m(x, x, x, mask=mask).backward(g)
        assert m.last_path == ("kernel" if kernel else "torch")
        return [x.grad] + [p.grad for p in params]

    row = {"B": B, "L": L, "emb_dim": dim, "nhead": H, "dropout": dropout, "rounds": rounds}
    if dropout == 0:
        got, want = step(True), step(False)
        # the key projection's bias has an exactly zero gradient (both paths leave rounding residue there): every tensor
        # is measured against its own scale or a thousandth of the largest, whichever is larger
        floor = 1e-3 * max(float(b.abs().max()) for b in want)
        row["grad_rel_diff_max"] = max(float((a - b).abs().max()) / max(float(b.abs().max()), floor) for a, b in zip(got, want))
        if not row["grad_rel_diff_max"] < 1e-3:
            raise SystemExit(f"attnbench: at {(B, L, dim, H)} kernel path and torch path differ: {row['grad_rel_diff_max']}")
        del got, want
    ts = _alternate({"kernel": lambda: step(True), "torch": lambda: step(False)}, rounds, warmup)
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
    row["one_score_tensor_MiB"] = round(B * H * L * L * 4 / 2**20, 1)
    # the attention alone, on the projections
    with torch.no_grad():
        q, k, v = (layer(x) for layer in m.linear_layers)
    kv = valid.to(torch.uint8).contiguous()
    _, lse = attention_forward(q, k, v, kv, H, dropout, 1, 1)
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    drop = m.dropout if dropout > 0 else None

    def torch_alone():
        for t in leaves:
            t.grad = None
        bert4rec._attention_torch(*leaves, mask, H, drop).backward(g)

    alone = _alternate({"fwd_kernel": lambda: attention_forward(q, k, v, kv, H, dropout, 1, 1),
                        "bwd_kernel": lambda: attention_backward(g, q, k, v, kv, lse, H, dropout, 1, 1),
                        "torch_fwd_bwd": torch_alone}, rounds, warmup)
    row["attention_alone"] = {n: _stats(n, t) for n, t in alone.items()}
    flops = 4.0 * B * H * L * L * (dim // H)  # forward: S and P V
    row["attention_alone"]["fwd_kernel_TFLOPs"] = round(flops / statistics.median(alone["fwd_kernel"]) / 1e6, 2)
    row["attention_alone"]["bwd_kernel_TFLOPs"] = round(3.5 * flops / statistics.median(alone["bwd_kernel"]) / 1e6, 2)
    return row


def bench_to_padded_dense(B, rounds, warmup, dev):
    import torch

    from torchrec_amd.sparse.jagged_tensor import JaggedTensor

    torch.manual_seed(B)
    lengths = torch.randint(0, 151, (B,), device=dev)
    values = torch.randint(1, 50000, (int(lengths.sum()),), device=dev)
    jt = JaggedTensor(values=values, lengths=lengths)
    jt.offsets()
    ours = lambda: jt.to_padded_dense(desired_length=100, pad_from_beginning=False)  # noqa: E731
    loop = lambda: reference_to_padded_dense(values, lengths, 100, pad_from_beginning=False)  # noqa: E731
    assert torch.equal(ours(), loop().float())
    batch = 10  # launches per timed sample: one 20 us launch between two events would be mostly event and launch overhead

    def ours_batch():
        for _ in range(batch):
            ours()

    ts = _alternate({"kernel": ours_batch, "reference_loop": loop}, rounds, warmup)
    ts["kernel"] = [t / batch for t in ts["kernel"]]
    row = {"B": B, "desired_length": 100, "rounds": rounds, "kernel_launches_per_sample": batch}
    for n, t in ts.items():
        row.update(_stats(n, t))
    row["loop_over_kernel"] = round(statistics.median(ts["reference_loop"]) / statistics.median(ts["kernel"]), 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("attnbench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    results, padded = [], []
    for B, L, dim, H in SHAPES:
        for dropout in (0.0, 0.1):
            results.append(bench_attention(B, L, dim, H, dropout, args.rounds, args.warmup, dev))
            print(json.dumps(results[-1]), flush=True)
            torch.cuda.empty_cache()
    for B in (128, 1024):
        padded.append(bench_to_padded_dense(B, args.rounds, args.warmup, dev))
        print(json.dumps(padded[-1]), flush=True)
    doc = {"tool": "tools/attnbench.py", "device": torch.cuda.get_device_name(0),
           "timer": "HIP events round one forward + backward, kernel path and torch path alternating",
           "results": results, "to_padded_dense": padded}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
