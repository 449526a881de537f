"""GPU: the order of the one finishing launch (include/tbe_hip.h tbe_multi_chunk_sum_host_table_f32).  A segment whose chunk
count carries TBE_CHUNKS_WAVE_ORDER is added in the order of the column sums' second stage at EVERY count — bit for bit the
host model tests/_colsum_order.second_stage and what tbe_relu_backward_bias_grad_f32 makes of the same row blocks — a
segment of at most 16 chunks without it keeps the plain sequence, and the wave order is compared with torch.sum(dim=0) at the
split-K weight gradients' shapes of the DLRM step (reported per pair: DESIGN.md records the outcome)."""
import ctypes

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _colsum_order as co
from _guarded import Buf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

# Chunk counts: one block; fewer blocks than waves; a tail; the sequential form's limit; past it; 38: past the 8-deep unroll of
# the general kernel's wave form (4 * 7 < 38), still inside the tail loop of multi_colsum_partials_kernel, whose 32-deep main
# loop a wave enters from 125 chunks on (4 * 31 < chunks).
CHUNKS = (1, 3, 5, 16, 17, 38)
# Past that unroll (the all-flagged table, i.e. the kernel that finishes an eager backward): 125 = wave 0 alone runs the main
# loop, once, no tail; 130 = every wave runs it once, then waves 0 and 1 one tail block each; 300 = twice and a tail of 11;
# 256 and 1024 = the row blocks of the benchmark's step (B = 65 536 in 256-row and in 64-row blocks: 2 and 8 trips, no tail).
DEEP_CHUNKS = {8: (125, 130, 256, 300, 1024), 516: (130,)}
WIDTHS = (8, 516)  # 64-row and 256-row blocks; 516: a column tile with a tail
# (chunks, out, in) of the step's seven split-K weight gradients (modules/mlp.py _wgrad_chunks at batch 65 536)
SPLITK = [(32, 512, 13), (32, 256, 512), (32, 256, 512), (32, 128, 256), (8, 1024, 479), (8, 512, 1024), (4, 1024, 1024)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _done(lib, rc):
    assert rc == 0, lib.tbe_last_error()
    torch.cuda.synchronize()


def _table(segs):
    """int64 [n][4] = {src address, chunks (| flag), numel, dst element offset} in host memory."""
    t = (ctypes.c_int64 * (4 * len(segs)))()
    for k, s in enumerate(segs):
        t[4 * k:4 * k + 4] = list(s)
    return t


def _sequential(part):
    acc = part[0].copy()
    for c in range(1, part.shape[0]):
        acc = acc + part[c]
    return acc


def test_flagged_segments_end_as_the_second_stage_at_every_count():
    lib = _lib.load()
    rng = np.random.default_rng(77)
    parts, own, segs, off = [], [], [], 0
    for N in WIDTHS:
        for chunks in CHUNKS + DEEP_CHUNKS[N]:
            B = (chunks - 1) * co.rows_per_block(N) + 1  # the last row block holds one row
            assert lib.tbe_colsum_row_blocks(B, N) == chunks
            gy, act = (rng.standard_normal((B, N)).astype(np.float32) for _ in range(2))
            bgy, bact, bgx = Buf(B * N, gy), Buf(B * N, act), Buf(B * N)
            bpart, bgb = Buf(chunks * N), Buf(N)
            _done(lib, lib.tbe_relu_backward_bias_partials_f32(bgy.ptr, bact.ptr, B, N, bgx.ptr, bpart.ptr, 4 * chunks * N, _stream()))
            wb = lib.tbe_relu_backward_bias_grad_workspace_bytes(B, N)
            bws = Buf(wb // 4)
            _done(lib, lib.tbe_relu_backward_bias_grad_f32(bgy.ptr, bact.ptr, B, N, bgx.ptr, bgb.ptr, bws.ptr, wb, _stream()))
            parts.append(bpart)
            own.append(bgb.get())
            segs.append((bpart.ptr, chunks | _lib.CHUNKS_WAVE_ORDER, N, off))
            off += (N + 63) // 64 * 64
    assert len(segs) <= _lib.CHUNK_SEGS_BY_VALUE
    bdst = Buf(off)
    _done(lib, lib.tbe_multi_chunk_sum_host_table_f32(_table(segs), len(segs), max(WIDTHS), bdst.ptr, 1.0, _stream()))
    dst = bdst.get()
    differ = 0
    for (ptr, chunks, N, o), bpart, gb in zip(segs, parts, own):
        chunks &= ~_lib.CHUNKS_WAVE_ORDER
        part = bpart.get((chunks, N))
        got = dst[o:o + N]
        np.testing.assert_array_equal(got, co.second_stage(part), err_msg=f"{chunks} chunks of {N}")
        np.testing.assert_array_equal(got, gb, err_msg=f"{chunks} chunks of {N}: the one-pass entry's own second stage")
        differ += int((got != _sequential(part)).any())
        pad = dst[o + N:o + (N + 63) // 64 * 64]
        assert (pad == bdst.all()[0]).all(), "the padding between two slices was written"
    assert differ >= 4  # the order matters for these inputs: from 5 chunks on, at both widths, the plain sequence gives other bits


def test_unflagged_short_segments_keep_the_plain_sequence():
    lib = _lib.load()
    rng = np.random.default_rng(78)
    segs, parts, off = [], [], 0
    for N in WIDTHS:
        for chunks in (3, 5, 16):
            part = rng.standard_normal((chunks, N)).astype(np.float32)
            b = Buf(chunks * N, part)
            parts.append((b, part))
            segs.append((b.ptr, chunks, N, off))
            off += (N + 63) // 64 * 64
    # in the same table a flagged segment (a mixed table goes through the general kernel, which honours the flag too)
    mixed = [(c, n, rng.standard_normal((c, n)).astype(np.float32)) for c, n in ((1, 8), (5, 516), (17, 8), (38, 516))]
    mixed_bufs = []
    for c, n, part in mixed:
        mixed_bufs.append((Buf(c * n, part), off))
        segs.append((mixed_bufs[-1][0].ptr, c | _lib.CHUNKS_WAVE_ORDER, n, off))
        off += (n + 63) // 64 * 64
    bdst = Buf(off)
    _done(lib, lib.tbe_multi_chunk_sum_host_table_f32(_table(segs), len(segs), max(WIDTHS), bdst.ptr, 1.0, _stream()))
    dst = bdst.get()
    for (c, n, part), (_, o) in zip(mixed, mixed_bufs):
        np.testing.assert_array_equal(dst[o:o + n], co.second_stage(part), err_msg=f"flagged, {c} chunks of {n}")
    differ = 0
    for (ptr, chunks, N, o), (b, part) in zip(segs, parts):
        np.testing.assert_array_equal(dst[o:o + N], _sequential(part), err_msg=f"{chunks} chunks of {N}")
        differ += int((dst[o:o + N] != co.second_stage(part)).any())
        np.testing.assert_array_equal(b.get((chunks, N)), part)
    assert differ >= 4  # (and it is another order than the flagged one)


@pytest.mark.parametrize("chunks,out_f,in_f", SPLITK)
def test_wave_order_against_torch_sum_at_the_split_k_shapes(chunks, out_f, in_f):
    """Reported, not required: a pair whose bits agree may send its batched-GEMM slices to the finishing launch instead of a
    torch.sum kernel (dense side, records which do).  Required: both are sums of the same numbers."""
    lib = _lib.load()
    numel = out_f * in_f
    g = torch.Generator(device="cuda").manual_seed(1000 * chunks + out_f + in_f)
    x = torch.randn((chunks, numel), generator=g, device="cuda", dtype=torch.float32)
    ref = x.sum(dim=0)
    dst = torch.empty(numel, dtype=torch.float32, device="cuda")
    seg = _table([(x.data_ptr(), chunks | _lib.CHUNKS_WAVE_ORDER, numel, 0)])
    _done(lib, lib.tbe_multi_chunk_sum_host_table_f32(seg, 1, numel, dst.data_ptr(), 1.0, _stream()))
    same = torch.equal(dst, ref)
    n_diff = int((dst != ref).sum().item())
    print(f"split-K sum c={chunks} {out_f}x{in_f}: wave order {'==' if same else '!='} torch.sum(dim=0) "
          f"({n_diff} of {numel} elements differ)")
    exact = x.double().sum(dim=0)
    bound = 2.0 ** -23 * chunks * x.double().abs().sum(dim=0)
    assert ((dst.double() - exact).abs() <= bound).all() and ((ref.double() - exact).abs() <= bound).all()
