"""Measurement tool for torch.ops.fbgemm.permute_pooled_embs (csrc/permute_pooled.hip): runs, back to back, the op, the
same permutation as torch.index_select over columns, and a same-size device copy, `--iters` times each on a
[B, F x D] float32 matrix with the segments rotated by `--shift` — to be run under `rocprofv3 --kernel-trace --stats`,
whose per-kernel averages are the result (tools/prof_summary.py prints them).  Prints the bytes moved per call.
Usage: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/permute_pooled_bench.py [--batch 8192 --features 26 --dim 128]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchrec-oldfork_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--features", type=int, default=26)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--shift", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import torch

    import fbgemm_gpu  # noqa: F401
    from fbgemm_gpu.permute_pooled_embedding_modules import PermutePooledEmbeddings

    dev = torch.device("cuda", 0)
    T, D = args.features, args.dim
    permute = [(i * args.shift + 3) % T for i in range(T)]  # a non-trivial permutation when gcd(shift, T) == 1
    assert sorted(permute) == list(range(T))
    mod = PermutePooledEmbeddings([D] * T, permute, device=dev)
    x = torch.randn(args.batch, T * D, device=dev)
    cols = torch.cat([torch.arange(p * D, (p + 1) * D) for p in permute]).to(dev)
    want = x.index_select(1, cols)
    assert torch.equal(mod(x), want)
    dst = torch.empty_like(x)
    for _ in range(args.iters):
        mod(x)
    torch.cuda.synchronize()
    for _ in range(args.iters):
        x.index_select(1, cols)
    torch.cuda.synchronize()
    for _ in range(args.iters):
        dst.copy_(x)
    torch.cuda.synchronize()
    print(f"shape [{args.batch}, {T} x {D}] float32: {2 * x.numel() * 4 / 1e6:.1f} MB read + written per call, "
          f"{args.iters} calls each of permute_pooled_embs, index_select, copy_")


if __name__ == "__main__":
    main()
