"""Timing of the KJT index ops at the BASELINE shape (26 features x batch 65 536, pooling factor 1), of the jagged <-> dense
pair at the BERT4Rec shape and of the plain pooled all-to-all layout copies: development tool, numbers quoted in DESIGN.md."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import _paths  # noqa: E402,F401
import fbgemm_gpu  # noqa: E402,F401


def timeit(fn, n=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def main():
    F, B, W = 26, 65536, 8
    dev = "cuda"
    lengths = torch.ones(F * B, dtype=torch.int32, device=dev)
    values = torch.randint(0, 1 << 25, (F * B,), device=dev, dtype=torch.int64)
    perm = torch.randperm(F, device=dev).to(torch.int32)
    blocks = torch.full((F,), (1 << 25) // W, dtype=torch.int64, device=dev)
    us = timeit(lambda: torch.ops.fbgemm.asynchronous_complete_cumsum(lengths))
    print(f"asynchronous_complete_cumsum  n={F * B}: {us:.1f} us  ({F * B * 8 / us / 1e3:.1f} GB/s r+w)")
    us = timeit(lambda: torch.ops.fbgemm.permute_2D_sparse_data(perm, lengths.view(F, B), values, None, F * B))
    print(f"permute_2D_sparse_data        {F}x{B}: {us:.1f} us  ({F * B * 24 / us / 1e3:.1f} GB/s r+w incl. lengths)")
    us = timeit(lambda: torch.ops.fbgemm.block_bucketize_sparse_features(lengths, values, False, False, blocks, W, None))
    print(f"block_bucketize_sparse_features W={W}: {us:.1f} us")
    W_wide = 64  # above 32 buckets the per-bag counters live in global memory
    blocks_wide = torch.full((F,), (1 << 25) // W_wide, dtype=torch.int64, device=dev)
    us = timeit(lambda: torch.ops.fbgemm.block_bucketize_sparse_features(lengths, values, False, False, blocks_wide, W_wide, None))
    print(f"block_bucketize_sparse_features W={W_wide}: {us:.1f} us")
    starts = torch.arange(F * B, dtype=torch.int64, device=dev)
    us = timeit(lambda: torch.ops.fbgemm.offsets_range(starts, F * B))
    print(f"offsets_range                 n={F * B}: {us:.1f} us")
    # BERT4Rec (tools/attnbench.py): 1024 sequences of up to 100 items, embedding width 256
    Bs, L, D = 1024, 100, 256
    seq_offsets = torch.ops.fbgemm.asynchronous_complete_cumsum(torch.randint(1, L + 1, (Bs,), device=dev))
    items = torch.randn(int(seq_offsets[-1]), D, device=dev, requires_grad=True)
    grad = torch.randn(Bs, L, D, device=dev)
    us = timeit(lambda: torch.ops.fbgemm.jagged_2d_to_dense(items.detach(), seq_offsets, L))
    print(f"jagged_2d_to_dense            {Bs}x{L}x{D}: {us:.1f} us")
    us = timeit(lambda: torch.autograd.grad(torch.ops.fbgemm.jagged_2d_to_dense(items, seq_offsets, L), items, grad))
    print(f"jagged_2d_to_dense + backward {Bs}x{L}x{D}: {us:.1f} us")
    # the plain pooled all-to-all layout at the 8-rank shape of tools/xbench.py: 26 features of 128 columns from 8 ranks
    from torchrec_amd.distributed._device_ops import _simple_pack, _simple_unpack

    Bl, dims = 8192, torch.tensor([3 * 128] * 6 + [4 * 128] * 2, dtype=torch.int32, device=dev)
    D_total = int(dims.sum())
    pooled = torch.randn(Bl, D_total, device=dev)
    us = timeit(lambda: _simple_pack(pooled, dims, True, 0.125))
    print(f"a2a_pooled_pack   W=8 B_local={Bl}: {us:.1f} us  ({Bl * D_total * 8 / us / 1e3:.0f} GB/s r+w)")
    slabs = _simple_pack(pooled, dims, True, 1.0)
    us = timeit(lambda: _simple_unpack(slabs, dims, Bl, D_total, True, 1.0))
    print(f"a2a_pooled_unpack W=8 B_local={Bl}: {us:.1f} us  ({Bl * D_total * 8 / us / 1e3:.0f} GB/s r+w)")


if __name__ == "__main__":
    main()
