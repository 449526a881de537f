"""Device ops of the distributed layer that are not part of the fbgemm surface, exposed as
dispatcher ops (`torch.ops.tbe_hip.*`) over the C ABI (include/tbe_hip.h
tbe_pooled_exchange_*).  Only the HIP key is registered here; CPU tensors raise."""
import torch

from fbgemm_gpu import _lib
from fbgemm_gpu._lib import check, ptr, require_gpu, stream_ptr, workspace

_def = torch.library.Library("tbe_hip", "DEF")
_def.define("pooled_exchange_unpack(Tensor recv, Tensor feat_out_col, Tensor feat_src, Tensor feat_slab_col, "
            "Tensor slab_offset, Tensor slab_stride, int B_local, int D_total, bool vec, float scale) -> Tensor")
_def.define("pooled_exchange_unpack_into(Tensor recv, Tensor feat_out_col, Tensor feat_src, Tensor feat_slab_col, "
            "Tensor slab_offset, Tensor slab_stride, int B_local, int D_total, bool vec, float scale, Tensor(a!) out) -> Tensor(a!)")
_def.define("pooled_exchange_pack(Tensor grad, Tensor feat_out_col, Tensor feat_src, Tensor feat_slab_col, "
            "Tensor slab_offset, Tensor slab_stride, int numel, bool vec, float scale) -> Tensor")
_def.define("pooled_exchange_pack_into(Tensor grad, Tensor feat_out_col, Tensor feat_src, Tensor feat_slab_col, "
            "Tensor slab_offset, Tensor slab_stride, bool vec, float scale, Tensor(a!) send) -> Tensor(a!)")
_def.define("a2a_pooled_unpack(Tensor recv, Tensor dim_sum_per_rank, int B_local, int D_total, bool vec, float scale) -> Tensor")
_def.define("a2a_pooled_pack(Tensor grad, Tensor dim_sum_per_rank, bool vec, float scale) -> Tensor")
_def.define("relu_backward_bias_grad(Tensor grad_out, Tensor act) -> (Tensor, Tensor)")
_def.define("weighted_colsum(Tensor x, Tensor w) -> Tensor")
_def.define("copy_rows(Tensor src, Tensor rows) -> Tensor")
_def.define("relu_backward_bias_partials(Tensor grad_out, Tensor act) -> (Tensor, Tensor)")
_def.define("weighted_colsum_partials(Tensor x, Tensor w) -> Tensor")
_def.define("relu_linear1_backward(Tensor act, Tensor dy, Tensor w) -> (Tensor, Tensor)")
_def.define("relu_linear1_backward_partials(Tensor act, Tensor dy, Tensor w) -> (Tensor, Tensor)")
_def.define("multi_chunk_sum(Tensor seg_table, int nseg, int max_numel, Tensor(a!) dst, float scale) -> Tensor(a!)")
_def.define("bce_with_logits(Tensor logits, Tensor labels) -> (Tensor, Tensor)")
_def.define("cross_backward(Tensor grad_out, Tensor x0, Tensor t, Tensor(a!) acc, bool first) -> (Tensor, Tensor)")
_def.define("vector_cross_forward(Tensor x0, Tensor weights, Tensor bias) -> (Tensor, Tensor)")
_def.define("vector_cross_backward(Tensor grad_out, Tensor x0, Tensor s, Tensor weights, Tensor bias) -> (Tensor, Tensor)")
_def.define("swish_layernorm_forward(Tensor y, Tensor gamma, Tensor beta, float eps) -> (Tensor, Tensor)")
_def.define("swish_layernorm_backward(Tensor grad_out, Tensor y, Tensor stats, Tensor gamma, Tensor beta) -> (Tensor, Tensor)")
_def.define("mixture_gate_forward(Tensor a2, Tensor logits) -> (Tensor, Tensor)")
_def.define("mixture_gate_backward(Tensor grad_m, Tensor a2, Tensor p) -> (Tensor, Tensor)")
_def.define("fm_forward(Tensor[] xs, bool want_cat) -> (Tensor, Tensor, Tensor)")
_def.define("fm_backward(Tensor[] xs, Tensor grad_fm, Tensor row_sum, Tensor? grad_cat, bool[] wanted) -> Tensor[]")
_impl = torch.library.Library("tbe_hip", "IMPL", "CUDA")


def _copy_rows(src, rows):
    """src[rows] for a contiguous 2-D `src` whose rows are multiples of 16 bytes and a device int32 `rows`
    (csrc/sparse_ops.hip copy_rows_kernel)."""
    dev = require_gpu(src, rows)
    if src.dim() != 2 or not src.is_contiguous() or rows.dtype != torch.int32 or rows.dim() != 1:
        raise RuntimeError(f"copy_rows: need a contiguous 2-D src and int32 rows, got {tuple(src.shape)} / {rows.dtype}")
    out = src.new_empty((rows.numel(), src.shape[1]))
    lib = _lib.load()
    with torch.cuda.device(dev):
        check(lib.tbe_copy_rows(ptr(src), src.shape[0], ptr(rows), rows.numel(), src.shape[1] * src.element_size(), ptr(out),
                                stream_ptr(dev)), "tbe_copy_rows")
    return out


def _weighted_colsum_args(name, x, w):
    """(device, contiguous float32 x [B, N], w [B]) of weighted_colsum / weighted_colsum_partials."""
    dev = require_gpu(x, w)
    if x.dim() != 2 or w.numel() != x.shape[0] or x.dtype != torch.float32 or w.dtype != torch.float32:
        raise RuntimeError(f"{name}: need float32 x [B, N] and w [B], got {tuple(x.shape)} and {tuple(w.shape)}")
    return dev, x.contiguous(), w.contiguous().view(-1)


def _relu_backward_args(name, grad_out, act):
    """(device, contiguous float32 grad_out, act [B, N]) of relu_backward_bias_grad / relu_backward_bias_partials."""
    dev = require_gpu(grad_out, act)
    if grad_out.dim() != 2 or grad_out.shape != act.shape or grad_out.dtype != torch.float32 or act.dtype != torch.float32:
        raise RuntimeError(f"{name}: need two float32 [B, N] tensors of one shape, got "
                           f"{tuple(grad_out.shape)} and {tuple(act.shape)}")
    return dev, grad_out.contiguous(), act.contiguous()


def _weighted_colsum(x, w):
    """out[c] = sum_b w[b] * x[b, c] (csrc/mlp_epilogue.hip)."""
    dev, x, w = _weighted_colsum_args("weighted_colsum", x, w)
    B, N = x.shape
    out = torch.empty(N, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = workspace(lib.tbe_weighted_colsum_workspace_bytes(B, N), dev)
        check(lib.tbe_weighted_colsum_f32(ptr(x), ptr(w), B, N, ptr(out), ptr(ws), ws.numel(), stream_ptr(dev)),
              "tbe_weighted_colsum_f32")
    return out


def _relu_backward_bias_grad(grad_out, act):
    """(grad_out * (act > 0), its column sums) in one pass (csrc/mlp_epilogue.hip)."""
    dev, grad_out, act = _relu_backward_args("relu_backward_bias_grad", grad_out, act)
    B, N = grad_out.shape
    gx = torch.empty_like(grad_out)
    gb = torch.empty(N, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = workspace(lib.tbe_relu_backward_bias_grad_workspace_bytes(B, N), dev)
        check(lib.tbe_relu_backward_bias_grad_f32(ptr(grad_out), ptr(act), B, N, ptr(gx), ptr(gb), ptr(ws), ws.numel(),
                                                  stream_ptr(dev)), "tbe_relu_backward_bias_grad_f32")
    return gx, gb


def _relu_backward_bias_partials(grad_out, act):
    """(grad_out * (act > 0), column sums of its row blocks [row blocks, N]) — the first stage of relu_backward_bias_grad
    alone; `multi_chunk_sum` finishes every layer's bias gradient in one launch (csrc/mlp_epilogue.hip)."""
    dev, grad_out, act = _relu_backward_args("relu_backward_bias_partials", grad_out, act)
    B, N = grad_out.shape
    lib = _lib.load()
    gx = torch.empty_like(grad_out)
    partial = torch.empty((lib.tbe_colsum_row_blocks(B, N), N), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.tbe_relu_backward_bias_partials_f32(ptr(grad_out), ptr(act), B, N, ptr(gx), ptr(partial),
                                                      partial.numel() * 4, stream_ptr(dev)), "tbe_relu_backward_bias_partials_f32")
    return gx, partial


def _weighted_colsum_partials(x, w):
    """Row-block partials [row blocks, N] of out[c] = sum_b w[b] * x[b, c] (first stage of weighted_colsum)."""
    dev, x, w = _weighted_colsum_args("weighted_colsum_partials", x, w)
    B, N = x.shape
    lib = _lib.load()
    partial = torch.empty((lib.tbe_colsum_row_blocks(B, N), N), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.tbe_weighted_colsum_partials_f32(ptr(x), ptr(w), B, N, ptr(partial), partial.numel() * 4, stream_ptr(dev)),
              "tbe_weighted_colsum_partials_f32")
    return partial


def _relu_linear1_args(name, act, dy, w):
    """(device, contiguous float32 act [B, N], dy [B], w [N]) of relu_linear1_backward / relu_linear1_backward_partials."""
    dev = require_gpu(act, dy, w)
    if (act.dim() != 2 or dy.numel() != act.shape[0] or w.numel() != act.shape[1]
            or any(t.dtype != torch.float32 for t in (act, dy, w))):
        raise RuntimeError(f"{name}: need float32 act [B, N], dy [B] and w [N], got {tuple(act.shape)}, {tuple(dy.shape)} "
                           f"and {tuple(w.shape)}")
    return dev, act.contiguous(), dy.contiguous().view(-1), w.contiguous().view(-1)


def _relu_linear1_backward(act, dy, w):
    """(gx = (act > 0) * dy[:, None] * w[None, :], sums [2 N]: the column sums of gx, then of dy[:, None] * act) in one pass
    over act (csrc/mlp_epilogue.hip): the backward of a one-output Linear behind a hidden layer with ReLU."""
    dev, act, dy, w = _relu_linear1_args("relu_linear1_backward", act, dy, w)
    B, N = act.shape
    gx = torch.empty_like(act)
    sums = torch.empty(2 * N, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = workspace(lib.tbe_relu_linear1_backward_workspace_bytes(B, N), dev)
        check(lib.tbe_relu_linear1_backward_f32(ptr(act), ptr(dy), ptr(w), B, N, ptr(gx), ptr(sums), ptr(ws), ws.numel(),
                                                stream_ptr(dev)), "tbe_relu_linear1_backward_f32")
    return gx, sums


def _relu_linear1_backward_partials(act, dy, w):
    """(gx, the row blocks' sums [row blocks, 2 N]) — the first stage of relu_linear1_backward alone; `finish_row_block_sums`
    finishes it together with every other gradient of the backward."""
    dev, act, dy, w = _relu_linear1_args("relu_linear1_backward_partials", act, dy, w)
    B, N = act.shape
    lib = _lib.load()
    gx = torch.empty_like(act)
    partial = torch.empty((lib.tbe_colsum_row_blocks(B, N), 2 * N), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.tbe_relu_linear1_backward_partials_f32(ptr(act), ptr(dy), ptr(w), B, N, ptr(gx), ptr(partial),
                                                         partial.numel() * 4, stream_ptr(dev)),
              "tbe_relu_linear1_backward_partials_f32")
    return gx, partial


def finish_row_block_sums(segments, dst):
    """dst[off : off + n] = the column sums of `partial` [row blocks, n], in the order of the column sums' second stage
    (csrc/colsum.hpp), for every (partial, off) of `segments`: one launch per 32 segments, the table travelling in the
    kernel arguments (csrc/mlp_epilogue.hip multi_chunk_sum_args_kernel).  The caller keeps the partials alive until then."""
    dev = require_gpu(dst, *[p for p, _ in segments])
    if dst.dtype != torch.float32 or not dst.is_contiguous():
        raise RuntimeError("finish_row_block_sums: dst must be a contiguous float32 tensor")
    lib = _lib.load()
    with torch.cuda.device(dev):
        for lo in range(0, len(segments), _lib.CHUNK_SEGS_BY_VALUE):
            group = segments[lo:lo + _lib.CHUNK_SEGS_BY_VALUE]
            table = (_lib.c_i64 * (4 * len(group)))()
            for k, (part, off) in enumerate(group):
                if part.dim() != 2 or part.dtype != torch.float32 or not part.is_contiguous() or off + part.shape[1] > dst.numel():
                    raise RuntimeError(f"finish_row_block_sums: segment {lo + k} is not a contiguous float32 [row blocks, n] "
                                       f"that fits dst ({tuple(part.shape)} at {off} of {dst.numel()})")
                table[4 * k:4 * k + 4] = [part.data_ptr(), part.shape[0] | _lib.CHUNKS_WAVE_ORDER, part.shape[1], off]
            check(lib.tbe_multi_chunk_sum_host_table_f32(table, len(group), max(p.shape[1] for p, _ in group), ptr(dst), 1.0,
                                                         stream_ptr(dev)), "tbe_multi_chunk_sum_host_table_f32")
    return dst


def _cross_backward(grad_out, x0, t, acc, first):
    """One layer's backward epilogue of CrossNet / LowRankCrossNet (csrc/crossnet.hip): returns (grad_out * x0, its column
    sums) and writes acc = grad_out * t (`first`) or acc += grad_out * t in place."""
    dev = require_gpu(grad_out, x0, t, acc)
    if (grad_out.dim() != 2 or any(a.shape != grad_out.shape or a.dtype != torch.float32 or not a.is_contiguous()
                                   for a in (grad_out, x0, t, acc))):
        raise RuntimeError(f"cross_backward: need four contiguous float32 [B, N] tensors of one shape, got "
                           f"{[tuple(a.shape) for a in (grad_out, x0, t, acc)]}")
    B, N = grad_out.shape
    gy = torch.empty_like(grad_out)
    gb = torch.empty(N, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = workspace(lib.tbe_cross_backward_workspace_bytes(B, N), dev)
        check(lib.tbe_cross_backward_f32(ptr(grad_out), ptr(x0), ptr(t), B, N, int(bool(first)), ptr(gy), ptr(acc), ptr(gb),
                                         ptr(ws), ws.numel(), stream_ptr(dev)), "tbe_cross_backward_f32")
    return gy, gb


def _vector_cross_check(name, x0, weights, bias, *more):
    dev = require_gpu(x0, weights, bias, *more)
    if (x0.dim() != 2 or weights.dim() != 2 or weights.shape[1] != x0.shape[1] or bias.shape != weights.shape
            or any(a.dtype != torch.float32 or not a.is_contiguous() for a in (x0, weights, bias) + more)):
        raise RuntimeError(f"{name}: need contiguous float32 x0 [B, N], weights [L, N], bias [L, N], got "
                           f"{tuple(x0.shape)}, {tuple(weights.shape)}, {tuple(bias.shape)}")
    return dev


def _vector_cross_forward(x0, weights, bias):
    """(x_L [B, N], s [L, B]) of VectorCrossNet, all layers in one kernel (csrc/crossnet.hip)."""
    dev = _vector_cross_check("vector_cross_forward", x0, weights, bias)
    (B, N), L = x0.shape, weights.shape[0]
    out = torch.empty_like(x0)
    s = torch.empty((L, B), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_vector_cross_forward_f32(ptr(x0), ptr(weights), ptr(bias), B, N, L, ptr(out), ptr(s),
                                                       stream_ptr(dev)), "tbe_vector_cross_forward_f32")
    return out, s


def _vector_cross_backward(grad_out, x0, s, weights, bias):
    """(input gradient [B, N], parameter gradients [2 L, N]: bias rows first, then weight rows) (csrc/crossnet.hip)."""
    dev = _vector_cross_check("vector_cross_backward", x0, weights, bias, grad_out, s)
    (B, N), L = x0.shape, weights.shape[0]
    if grad_out.shape != x0.shape or s.shape != (L, B):
        raise RuntimeError(f"vector_cross_backward: grad_out {tuple(grad_out.shape)} / s {tuple(s.shape)} do not fit "
                           f"x0 {tuple(x0.shape)}, L = {L}")
    gin = torch.empty_like(x0)
    gp = torch.empty((2 * L, N), dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = workspace(lib.tbe_vector_cross_backward_workspace_bytes(B, N, L), dev)
        check(lib.tbe_vector_cross_backward_f32(ptr(grad_out), ptr(x0), ptr(s), ptr(weights), ptr(bias), B, N, L, ptr(gin),
                                                ptr(gp), ptr(ws), ws.numel(), stream_ptr(dev)), "tbe_vector_cross_backward_f32")
    return gin, gp


def _swish_layernorm_check(name, y, gamma, beta, *more):
    dev = require_gpu(y, gamma, beta, *more)
    if (y.dim() != 2 or gamma.shape != (y.shape[1],) or beta.shape != gamma.shape
            or any(a.dtype != torch.float32 or not a.is_contiguous() for a in (y, gamma, beta) + more)):
        raise RuntimeError(f"{name}: need contiguous float32 y [B, N], gamma [N], beta [N], got "
                           f"{tuple(y.shape)}, {tuple(gamma.shape)}, {tuple(beta.shape)}")
    return dev


def _swish_layernorm_forward(y, gamma, beta, eps):
    """(y * sigmoid(layer_norm(y)) [B, N], stats [2, B]: mean, rstd) in one kernel (csrc/swish_layernorm.hip)."""
    dev = _swish_layernorm_check("swish_layernorm_forward", y, gamma, beta)
    B, N = y.shape
    out = torch.empty_like(y)
    stats = torch.empty((2, B), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_swish_layernorm_forward_f32(ptr(y), ptr(gamma), ptr(beta), eps, B, N, ptr(out), ptr(stats),
                                                          stream_ptr(dev)), "tbe_swish_layernorm_forward_f32")
    return out, stats


def _swish_layernorm_backward(grad_out, y, stats, gamma, beta):
    """(input gradient [B, N], parameter gradients [2, N]: gamma row, beta row) (csrc/swish_layernorm.hip)."""
    dev = _swish_layernorm_check("swish_layernorm_backward", y, gamma, beta, grad_out, stats)
    B, N = y.shape
    if grad_out.shape != y.shape or stats.shape != (2, B):
        raise RuntimeError(f"swish_layernorm_backward: grad_out {tuple(grad_out.shape)} / stats {tuple(stats.shape)} do not "
                           f"fit y {tuple(y.shape)}")
    gy = torch.empty_like(y)
    gp = torch.empty((2, N), dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = workspace(lib.tbe_swish_layernorm_backward_workspace_bytes(B, N), dev)
        check(lib.tbe_swish_layernorm_backward_f32(ptr(grad_out), ptr(y), ptr(stats), ptr(gamma), ptr(beta), B, N, ptr(gy),
                                                   ptr(gp), ptr(ws), ws.numel(), stream_ptr(dev)),
              "tbe_swish_layernorm_backward_f32")
    return gy, gp


def _mixture_gate_check(name, a2, bk, bk_name, *more):
    """(device, K, B, r) of a gate op: contiguous float32 a2 [K, B, r] and a [B, K] tensor (logits or p)."""
    dev = require_gpu(a2, bk, *more)
    if (a2.dim() != 3 or bk.shape != (a2.shape[1], a2.shape[0])
            or any(a.dtype != torch.float32 or not a.is_contiguous() for a in (a2, bk) + more)):
        raise RuntimeError(f"{name}: need contiguous float32 a2 [K, B, r] and {bk_name} [B, K], got "
                           f"{tuple(a2.shape)} and {tuple(bk.shape)}")
    return (dev,) + tuple(a2.shape)


def _mixture_gate_forward(a2, logits):
    """(m [B, K r], p [B, K]) of LowRankMixtureCrossNet's folded layer: p = softmax(logits), m[b, k r + j] =
    p[b, k] * relu(a2[k, b, j]) (csrc/crossnet.hip)."""
    dev, K, B, r = _mixture_gate_check("mixture_gate_forward", a2, logits, "logits")
    m = torch.empty((B, K * r), dtype=torch.float32, device=dev)
    p = torch.empty_like(logits)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_mixture_gate_forward_f32(ptr(a2), ptr(logits), B, K, r, ptr(m), ptr(p), stream_ptr(dev)),
              "tbe_mixture_gate_forward_f32")
    return m, p


def _mixture_gate_backward(grad_m, a2, p):
    """(grad_a2 [K, B, r], grad_logits [B, K]): the mirror of mixture_gate_forward (csrc/crossnet.hip)."""
    dev, K, B, r = _mixture_gate_check("mixture_gate_backward", a2, p, "p", grad_m)
    if grad_m.shape != (B, K * r):
        raise RuntimeError(f"mixture_gate_backward: grad_m {tuple(grad_m.shape)} does not fit a2 {tuple(a2.shape)}")
    ga2 = torch.empty_like(a2)
    gl = torch.empty_like(p)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_mixture_gate_backward_f32(ptr(grad_m), ptr(a2), ptr(p), B, K, r, ptr(ga2), ptr(gl),
                                                        stream_ptr(dev)), "tbe_mixture_gate_backward_f32")
    return ga2, gl


def fm_segments(xs, wanted=None):
    """The segment list of csrc/deepfm.hip for the column blocks `xs` (each float32 [B, w], inner stride 1): list
    neighbours that are adjacent column slices of one buffer (same row stride, the next one's address = the previous one's
    + its width — the per-feature views of a KeyedTensor) and, with `wanted`, share their flag are merged into one segment.
    Returns [(first index, count, address, row stride, width)]."""
    groups = []
    for i, x in enumerate(xs):
        w = x.shape[1]
        stride = x.stride(0) if x.shape[0] > 1 else max(x.stride(0), w)
        if groups:
            j, n, addr, st, gw = groups[-1]
            if st == stride and addr + 4 * gw == x.data_ptr() and gw + w <= st and (wanted is None or wanted[j] == wanted[i]):
                groups[-1] = (j, n + 1, addr, st, gw + w)
                continue
        groups.append((i, 1, x.data_ptr(), stride, w))
    return groups


def _fm_check(name, xs):
    if len(xs) == 0:
        raise RuntimeError(f"{name}: empty input list")
    dev = require_gpu(*xs)
    B = xs[0].shape[0]
    for i, x in enumerate(xs):
        if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] != B or x.shape[1] < 1 or (x.shape[1] > 1 and x.stride(1) != 1):
            raise RuntimeError(f"{name}: xs[{i}] must be float32 [B={B}, w >= 1] with a contiguous inner dimension, got "
                               f"{x.dtype} {tuple(x.shape)} strides {tuple(x.stride())}")
        if B > 1 and x.stride(0) < x.shape[1]:
            raise RuntimeError(f"{name}: xs[{i}] has overlapping rows (strides {tuple(x.stride())})")
    return dev, B


def _fm_seg_array(name, groups):
    if len(groups) > _lib.FM_MAX_SEGMENTS:
        raise RuntimeError(f"{name}: {len(groups)} segments are left after merging neighbours, more than "
                           f"{_lib.FM_MAX_SEGMENTS}; concatenate the inputs first (FactorizationMachine does)")
    segs = (_lib.FmSegment * len(groups))()
    for k, (_, _, addr, stride, w) in enumerate(groups):
        segs[k].x, segs[k].row_stride, segs[k].width = addr, stride, w
    return segs


def _fm_forward(xs, want_cat):
    """(fm [B, 1], row_sum [B], cat [B, N] or an empty tensor) of the column blocks `xs` in one pass (csrc/deepfm.hip)."""
    dev, B = _fm_check("fm_forward", xs)
    groups = fm_segments(xs)
    segs = _fm_seg_array("fm_forward", groups)
    N = sum(g[4] for g in groups)
    fm = torch.empty((B, 1), dtype=torch.float32, device=dev)
    row_sum = torch.empty(B, dtype=torch.float32, device=dev)
    cat = torch.empty((B, N) if want_cat else (0,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_fm_forward_f32(segs, len(groups), B, ptr(fm), 1, ptr(row_sum), ptr(cat) if want_cat else None,
                                             stream_ptr(dev)), "tbe_fm_forward_f32")
    return fm, row_sum, cat


def _fm_backward(xs, grad_fm, row_sum, grad_cat, wanted):
    """One gradient per entry of `xs` (an empty tensor where `wanted` is False) in one pass (csrc/deepfm.hip):
    grad_cat[:, its columns] + grad_fm * (row_sum - x).  grad_fm may be a strided [B, 1] view."""
    dev, B = _fm_check("fm_backward", xs)
    require_gpu(grad_fm, row_sum, grad_cat)
    wanted = [bool(w) for w in wanted]
    if len(wanted) != len(xs):
        raise RuntimeError(f"fm_backward: {len(wanted)} flags for {len(xs)} inputs")
    groups = fm_segments(xs, wanted)
    segs = _fm_seg_array("fm_backward", groups)
    N = sum(g[4] for g in groups)
    if grad_fm.dtype != torch.float32 or grad_fm.numel() != B or grad_fm.dim() not in (1, 2):
        raise RuntimeError(f"fm_backward: grad_fm must be float32 [B] or [B, 1] with B = {B}, got {grad_fm.dtype} "
                           f"{tuple(grad_fm.shape)}")
    if B > 1 and grad_fm.stride(0) < 1:  # an expanded scalar (out.sum().backward())
        grad_fm = grad_fm.contiguous()
    if row_sum.dtype != torch.float32 or row_sum.shape != (B,) or not row_sum.is_contiguous():
        raise RuntimeError(f"fm_backward: row_sum must be a contiguous float32 [{B}], got {row_sum.dtype} {tuple(row_sum.shape)}")
    if grad_cat is not None:
        if grad_cat.dtype != torch.float32 or grad_cat.shape != (B, N):
            raise RuntimeError(f"fm_backward: grad_cat must be float32 [{B}, {N}], got {grad_cat.dtype} {tuple(grad_cat.shape)}")
        grad_cat = grad_cat.contiguous()
    gsegs = (_lib.FmGradSegment * len(groups))()
    out = [None] * len(xs)
    for k, (first, count, _, _, w) in enumerate(groups):
        if wanted[first]:
            g = torch.empty((B, w), dtype=torch.float32, device=dev)
            gsegs[k].g, gsegs[k].row_stride = g.data_ptr(), w
            col = 0
            for i in range(first, first + count):
                out[i] = g if count == 1 else g[:, col:col + xs[i].shape[1]]
                col += xs[i].shape[1]
        else:
            gsegs[k].g, gsegs[k].row_stride = None, 0
            for i in range(first, first + count):
                out[i] = torch.empty(0, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_fm_backward_f32(segs, gsegs, len(groups), B, ptr(grad_fm), grad_fm.stride(0) if B > 1 else 1,
                                              ptr(row_sum), ptr(grad_cat), stream_ptr(dev)), "tbe_fm_backward_f32")
    return out


def _multi_chunk_sum(seg_table, nseg, max_numel, dst, scale):
    """dst[off_s + i] = scale * sum_c src_s[c, i] for every segment of `seg_table` (device int64 [nseg, 4]: src address,
    chunks, numel, dst element offset) in one launch; the caller keeps the sources alive."""
    dev = require_gpu(seg_table, dst)
    if seg_table.dtype != torch.int64 or not seg_table.is_contiguous() or seg_table.numel() != 4 * nseg:
        raise RuntimeError("multi_chunk_sum: seg_table must be a contiguous int64 [nseg, 4] device tensor")
    if dst.dtype != torch.float32 or not dst.is_contiguous():
        raise RuntimeError("multi_chunk_sum: dst must be a contiguous float32 tensor")
    with torch.cuda.device(dev):
        check(_lib.load().tbe_multi_chunk_sum_f32(ptr(seg_table), nseg, max_numel, ptr(dst), scale, stream_ptr(dev)),
              "tbe_multi_chunk_sum_f32")
    return dst


_bce_ws = {}


def _bce_with_logits(logits, labels):
    """(mean BCE-with-logits loss [scalar], d loss / d logits [B]) in one launch; labels float32 or int64."""
    dev = require_gpu(logits, labels)
    if logits.dim() != 1 or labels.shape != logits.shape or logits.dtype != torch.float32:
        raise RuntimeError(f"bce_with_logits: need float32 logits [B] and labels [B], got {tuple(logits.shape)} / {tuple(labels.shape)}")
    if labels.dtype not in (torch.float32, torch.int64):
        labels = labels.float()
    logits, labels = logits.contiguous(), labels.contiguous()
    lib = _lib.load()
    key = (dev, stream_ptr(dev))  # one workspace per stream: two streams must not share block partials / the ticket
    ws = _bce_ws.get(key)
    if ws is None:  # [block partials | ticket]: zeroed once, the kernel resets its ticket
        if torch.cuda.is_current_stream_capturing():
            # a persistent buffer must not come from a graph's memory pool (an earlier graph of the pool may use its
            # address for transient tensors and clobber it at every replay): run the op once on this stream before capturing
            raise RuntimeError("bce_with_logits: first use on this stream happens inside a graph capture; warm the op up "
                               "on the capture stream first (GraphedSegment does)")
        ws = _bce_ws[key] = torch.zeros(lib.tbe_bce_with_logits_workspace_bytes(), dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dlogits = torch.empty_like(logits)
    with torch.cuda.device(dev):
        check(lib.tbe_bce_with_logits_f32(ptr(logits), ptr(labels), labels.element_size(), logits.numel(), ptr(loss),
                                          ptr(dlogits), ptr(ws), ws.numel(), stream_ptr(dev)), "tbe_bce_with_logits_f32")
    return loss, dlogits


def _simple_unpack(recv, dims, B_local, D_total, vec, scale):
    dev = require_gpu(recv, dims)
    recv = recv.contiguous()
    out = torch.empty((B_local, D_total), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_a2a_pooled_unpack(ptr(recv), ptr(out), ptr(dims), dims.numel(), B_local, D_total,
                                                int(vec), scale, stream_ptr(dev)), "tbe_a2a_pooled_unpack")
    return out


def _simple_pack(grad, dims, vec, scale):
    dev = require_gpu(grad, dims)
    grad = grad.contiguous()
    B_local, D_total = grad.shape
    send = torch.empty(B_local * D_total, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_a2a_pooled_pack(ptr(grad), ptr(send), ptr(dims), dims.numel(), B_local, D_total,
                                              int(vec), scale, stream_ptr(dev)), "tbe_a2a_pooled_pack")
    return send



def _unpack(recv, feat_out_col, feat_src, feat_slab_col, slab_offset, slab_stride, B_local, D_total, vec, scale):
    out = torch.empty((B_local, D_total), dtype=torch.float32, device=recv.device)
    return _unpack_into(recv, feat_out_col, feat_src, feat_slab_col, slab_offset, slab_stride, B_local, D_total, vec,
                        scale, out)


def _unpack_into(recv, feat_out_col, feat_src, feat_slab_col, slab_offset, slab_stride, B_local, D_total, vec, scale, out):
    """Same, into a caller-provided [B_local, D_total] buffer (e.g. the static input of a HIP-graph segment)."""
    dev = require_gpu(recv, feat_out_col, feat_src, feat_slab_col, slab_offset, slab_stride, out)
    recv = recv.contiguous()
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B_local * D_total:
        raise RuntimeError("pooled_exchange_unpack_into: out must be a contiguous float32 [B_local, D_total] buffer")
    with torch.cuda.device(dev):
        check(_lib.load().tbe_pooled_exchange_unpack(
            ptr(recv), ptr(out), ptr(feat_out_col), ptr(feat_src), ptr(feat_slab_col), ptr(slab_offset),
            ptr(slab_stride), feat_src.numel(), slab_offset.numel(), B_local, D_total, int(vec), scale,
            stream_ptr(dev)), "tbe_pooled_exchange_unpack")
    return out


def _pack(grad, feat_out_col, feat_src, feat_slab_col, slab_offset, slab_stride, numel, vec, scale):
    dev = require_gpu(grad, feat_out_col, feat_src, feat_slab_col, slab_offset, slab_stride)
    grad = grad.contiguous()
    B_local, D_total = grad.shape
    send = torch.empty(numel, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_pooled_exchange_pack(
            ptr(grad), ptr(send), ptr(feat_out_col), ptr(feat_src), ptr(feat_slab_col), ptr(slab_offset),
            ptr(slab_stride), feat_src.numel(), slab_offset.numel(), B_local, D_total, int(vec), scale,
            stream_ptr(dev)), "tbe_pooled_exchange_pack")
    return send


def _pack_into(grad, feat_out_col, feat_src, feat_slab_col, slab_offset, slab_stride, vec, scale, send):
    """pooled_exchange_pack into the caller's (persistent) send buffer — what a captured backward graph needs."""
    dev = require_gpu(grad, feat_out_col, feat_src, feat_slab_col, slab_offset, slab_stride, send)
    if grad.dim() != 2 or not grad.is_contiguous() or grad.dtype != torch.float32:
        raise RuntimeError("pooled_exchange_pack_into: grad must be a contiguous float32 [B_local, D_total] matrix")
    if send.dtype != torch.float32 or not send.is_contiguous():
        raise RuntimeError("pooled_exchange_pack_into: send must be a contiguous float32 buffer")
    B_local, D_total = grad.shape
    with torch.cuda.device(dev):
        check(_lib.load().tbe_pooled_exchange_pack(
            ptr(grad), ptr(send), ptr(feat_out_col), ptr(feat_src), ptr(feat_slab_col), ptr(slab_offset),
            ptr(slab_stride), feat_src.numel(), slab_offset.numel(), B_local, D_total, int(vec), scale,
            stream_ptr(dev)), "tbe_pooled_exchange_pack")
    return send


_impl.impl("relu_backward_bias_grad", _relu_backward_bias_grad)
_impl.impl("weighted_colsum", _weighted_colsum)
_impl.impl("copy_rows", _copy_rows)
_impl.impl("relu_backward_bias_partials", _relu_backward_bias_partials)
_impl.impl("weighted_colsum_partials", _weighted_colsum_partials)
_impl.impl("relu_linear1_backward", _relu_linear1_backward)
_impl.impl("relu_linear1_backward_partials", _relu_linear1_backward_partials)
_impl.impl("cross_backward", _cross_backward)
_impl.impl("vector_cross_forward", _vector_cross_forward)
_impl.impl("vector_cross_backward", _vector_cross_backward)
_impl.impl("swish_layernorm_forward", _swish_layernorm_forward)
_impl.impl("swish_layernorm_backward", _swish_layernorm_backward)
_impl.impl("mixture_gate_forward", _mixture_gate_forward)
_impl.impl("mixture_gate_backward", _mixture_gate_backward)
_impl.impl("fm_forward", _fm_forward)
_impl.impl("fm_backward", _fm_backward)
_impl.impl("multi_chunk_sum", _multi_chunk_sum)
_impl.impl("bce_with_logits", _bce_with_logits)
_impl.impl("pooled_exchange_unpack", _unpack)
_impl.impl("pooled_exchange_unpack_into", _unpack_into)
_impl.impl("pooled_exchange_pack", _pack)
_impl.impl("pooled_exchange_pack_into", _pack_into)
_impl.impl("a2a_pooled_unpack", _simple_unpack)
_impl.impl("a2a_pooled_pack", _simple_pack)


# ---- fused masked attention (csrc/attention.hip): plain functions, not dispatcher ops — the tensors are read where the
# projections left them (per-tensor strides) and the wanted gradients are chosen per call, which no op schema expresses.

def attention_supported(L: int, d: int) -> bool:
    """The kernel's (L, d_k) range: include/tbe_hip.h tbe_attention_supported."""
    return bool(_lib.load().tbe_attention_supported(L, d))


def _attention_strides(name, t, H):
    """(batch stride, row stride) in floats of a float32 [B, L, H * d] tensor whose last dimension is dense."""
    if t.dim() != 3 or t.dtype != torch.float32 or t.stride(2) != 1 or t.shape[2] % H:
        raise RuntimeError(f"{name}: want float32 [B, L, H * d] with a dense last dimension, got {tuple(t.shape)} "
                           f"{t.dtype} strides {t.stride()}")
    return t.stride(0), t.stride(1)


def attention_forward(q, k, v, key_valid, H, p=0.0, seed=0, call=0):
    """(out [B, L, H * d], lse [B, H, L]) of tbe_attention_forward_f32; q, k, v [B, L, H * d] float32 views with any batch /
    row strides, key_valid None or uint8 [B, L]."""
    dev = require_gpu(q, k, v, key_valid)
    B, L, HD = q.shape
    if k.shape != q.shape or v.shape != q.shape:
        raise RuntimeError(f"attention_forward: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} differ")
    strides = [s for t in (q, k, v) for s in _attention_strides("attention_forward", t, H)]
    if key_valid is not None and (key_valid.dtype != torch.uint8 or key_valid.shape != (B, L) or not key_valid.is_contiguous()):
        raise RuntimeError("attention_forward: key_valid must be a contiguous uint8 [B, L]")
    out = torch.empty((B, L, HD), dtype=torch.float32, device=dev)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().tbe_attention_forward_f32(
            ptr(q), strides[0], strides[1], ptr(k), strides[2], strides[3], ptr(v), strides[4], strides[5], ptr(key_valid),
            B, H, L, HD // H, p, seed, call, ptr(out), ptr(lse), stream_ptr(dev)), "tbe_attention_forward_f32")
    return out, lse


def attention_backward(grad_out, q, k, v, key_valid, lse, H, p=0.0, seed=0, call=0, need=(True, True, True)):
    """(dq, dk, dv), each contiguous [B, L, H * d] or None where `need` says so (tbe_attention_backward_f32)."""
    dev = require_gpu(grad_out, q, k, v, lse, key_valid)
    B, L, HD = q.shape
    strides = [s for t in (q, k, v) for s in _attention_strides("attention_backward", t, H)]
    if grad_out.shape != q.shape or grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
        raise RuntimeError("attention_backward: grad_out must be a contiguous float32 [B, L, H * d]")
    if lse.shape != (B, H, L) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise RuntimeError("attention_backward: lse must be the forward's [B, H, L]")
    grads = [torch.empty((B, L, HD), dtype=torch.float32, device=dev) if w else None for w in need]
    with torch.cuda.device(dev):
        check(_lib.load().tbe_attention_backward_f32(
            ptr(grad_out), ptr(q), strides[0], strides[1], ptr(k), strides[2], strides[3], ptr(v), strides[4], strides[5],
            ptr(key_valid), ptr(lse), B, H, L, HD // H, p, seed, call, ptr(grads[0]), ptr(grads[1]), ptr(grads[2]),
            stream_ptr(dev)), "tbe_attention_backward_f32")
    return tuple(grads)
