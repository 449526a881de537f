"""numpy float32 host model of the summation ORDERS of the row-in-registers kernels (csrc/rowreg.hpp): the two VectorCrossNet
kernels (csrc/crossnet.hip) and the two SwishLayerNorm kernels (csrc/swish_layernorm.hip).

Geometry: TPR threads share a row; thread `lane` holds the float4 columns lane, lane + TPR, ... (at most 4 slots); a workgroup
of 256 threads has RP = 256 / TPR rows in flight and owns `rows per block` rows.
  VectorCrossNet   TPR = 64 for N <= 1024, else 256; 128 rows per block at both
  SwishLayerNorm   TPR = 16, 64, 256 for N <= 64, <= 1024, <= 4096; 128, 32, 16 rows per block
Row sum (`row_sum`): a thread starts from 0.0f and adds its own elements in slot order, x, y, z, w inside a float4 (a dot adds
the rounded products); then the xor butterfly v += shfl_xor(v, o) for o = min(TPR, 64) / 2 ... 1; for TPR = 256 then
((w0 + w1) + w2) + w3 over the four waves.
Column sum (`first_stage`): thread group `sub` starts from 0.0f and adds the rows sub, sub + RP, ... of its row block; the
block's sum is fin[0] + fin[1] + ... + fin[RP - 1], left to right (TPR = 256: the one group's own value); it goes to
partial[row block][sums][N], which the second stage of tests/_colsum_order.py finishes over sums * N columns.

Every add and multiply below is one float32 operation on numpy float32 arrays, so the model reproduces the kernels bit for
bit (tests/test_rowreg_order_gpu.py); tests/test_rowreg_order.py checks that the order matters for the inputs used."""
import functools

import numpy as np

import _crossnet_ref as cr
import _swish_layernorm_ref as sr
from _colsum_order import second_stage

SLOTS = 4  # float4 slots per thread
F32 = np.float32

# (B, N, L): tests/_crossnet_ref.py VECTOR_GPU_SHAPES, and three row blocks with a ragged last one on the block-per-row kernel
VECTOR_SHAPES = cr.VECTOR_GPU_SHAPES + [(257, 1028, 2)]
# the class edges (16 threads per row | a wave | the block), a width with several slots of which the last is partial, the limit
SLN_WIDTHS = (60, 64, 68, 772, 1024, 1028, 4096)
# (B, N): at each width one row, and three row blocks with a ragged last one (the batch sizes of sr.abi_shapes())
SLN_SHAPES = [s for s in sr.abi_shapes() if s[1] in SLN_WIDTHS]
# seeds other than 2025: with 2025 the one row of (1, 60) happens to sum to the same bits left to right, and the test would
# pin nothing there (tests/test_rowreg_order.py)
SLN_SEEDS = {(1, 60): 2026}


def vector_tpr(N):
    return 64 if N <= 1024 else 256


def row_sum(terms, tpr):
    """[B] float32: the sum of every row of terms [B, N] over the tpr threads that share it."""
    terms = np.asarray(terms, dtype=F32)
    B, N = terms.shape
    assert N % 4 == 0 and N <= tpr * SLOTS * 4
    t = np.zeros((B, SLOTS * tpr * 4), dtype=F32)  # columns beyond N hold zeros
    t[:, :N] = terms
    t = t.reshape(B, SLOTS, tpr, 4)
    v = np.zeros((B, tpr), dtype=F32)
    for k in range(SLOTS):
        for c in range(4):
            v = v + t[:, k, :, c]
    wave = min(tpr, 64)
    lanes = np.arange(tpr)
    o = wave // 2
    while o > 0:
        v = v + v[:, lanes ^ o]
        o //= 2
    if tpr == 256:
        return ((v[:, 0] + v[:, 64]) + v[:, 128]) + v[:, 192]
    return v[:, 0].copy()


def left_to_right_row_sum(terms):
    """The same sum in plain column order — what the kernels do NOT compute."""
    terms = np.asarray(terms, dtype=F32)
    acc = np.zeros(terms.shape[0], dtype=F32)
    for c in range(terms.shape[1]):
        acc = acc + terms[:, c]
    return acc


def first_stage(terms, tpr, rows_per_block):
    """[row blocks, N] float32: the column sums of the row blocks of terms [B, N]."""
    terms = np.asarray(terms, dtype=F32)
    B, N = terms.shape
    RP = 256 // tpr
    out = np.empty((-(-B // rows_per_block), N), dtype=F32)
    for rb in range(out.shape[0]):
        row1 = min(B, (rb + 1) * rows_per_block)
        fin = np.zeros((RP, N), dtype=F32)
        for r0 in range(rb * rows_per_block, row1, RP):  # thread groups 0 .. n-1 take one row each
            n = min(RP, row1 - r0)
            fin[:n] = fin[:n] + terms[r0:r0 + n]
        s = fin[0]
        for j in range(1, RP):
            s = s + fin[j]
        out[rb] = s
    return out


def col_sums(term_list, tpr, rows_per_block):
    """(partial [row blocks, sums, N], result [sums, N]) of the `sums` column sums a kernel keeps."""
    partial = np.stack([first_stage(t, tpr, rows_per_block) for t in term_list], axis=1)
    nrb, S, N = partial.shape
    return partial, second_stage(partial.reshape(nrb, S * N)).reshape(S, N)


# ---- VectorCrossNet ------------------------------------------------------------------------------------------------------------
def vector_cross(w, b, x0, g):
    """Forward and backward of tbe_vector_cross_{forward,backward}_f32.  w, b [L, N]; x0, g [B, N].  Returns out, s [L, B],
    grad_in, grad_params [2 L, N] (bias rows, then weight rows), and the addends of every pinned sum:
    "row_terms" {name: ([B, N], pinned [B])}, "col_terms" {name: ([B, N], pinned [N])}."""
    w, b, x0, g = (np.asarray(a, dtype=F32) for a in (w, b, x0, g))
    (B, N), L = x0.shape, w.shape[0]
    tpr = vector_tpr(N)
    rows, cols = {}, {}
    xs, s = [x0], np.empty((L, B), dtype=F32)
    for l in range(L):
        t = xs[l] * w[l]
        s[l] = row_sum(t, tpr)
        rows[f"s.{l}"] = (t, s[l])
        xs.append((x0 * s[l][:, None] + b[l]) + xs[l])  # the forward's order; the backward recomputes x_l the same way
    G = g
    acc = np.zeros_like(x0)
    bias_terms, weight_terms = [None] * L, [None] * L
    for l in reversed(range(L)):
        t = G * x0
        d = row_sum(t, tpr)
        rows[f"d.{l}"] = (t, d)
        acc = acc + G * s[l][:, None]
        bias_terms[l] = G
        weight_terms[l] = d[:, None] * xs[l]
        G = G + d[:, None] * w[l]
    partial, gp = col_sums(bias_terms + weight_terms, tpr, cr.VECTOR_ROWS_PER_BLOCK)
    for l in range(L):
        cols[f"bias.{l}"] = (bias_terms[l], gp[l])
        cols[f"weight.{l}"] = (weight_terms[l], gp[L + l])
    return {"out": xs[L], "s": s, "grad_in": G + acc, "grad_params": gp, "partial": partial, "row_terms": rows,
            "col_terms": cols}


@functools.lru_cache(maxsize=None)
def vector_case(B, N, L):
    """Inputs (w, b [L, N]; x, g [B, N]: tests/_crossnet_ref.py gpu_case) and the model's results of one shape (computed once,
    shared; treat as read-only)."""
    p, x, g = cr.gpu_case("VectorCrossNet", B, N, L)
    w = np.stack([p[f"kernels.{l}"].reshape(N) for l in range(L)])
    b = np.stack([p[f"bias.{l}"].reshape(N) for l in range(L)])
    return dict(w=w, b=b, x=x, g=g, model=vector_cross(w, b, x, g))


# ---- SwishLayerNorm ------------------------------------------------------------------------------------------------------------
def swish_layernorm_zero_affine(y, g, eps=sr.EPS):
    """tbe_swish_layernorm_{forward,backward}_f32 with gamma = 0 and beta = 0: z = n * 0 + 0 = +0, so the sigmoid is
    1 / (1 + expf(-0)) = 0.5 where expf(-0) is exactly 1 (the GPU test asserts out == y * 0.5 first) and no result depends on
    expf beyond that.  Every other operation is the kernels', in their order.  Returns mean, rstd, out, grad_y, grad_params
    [2, N] (gamma row, beta row) and the addends of the pinned sums as `vector_cross` does."""
    y, g = np.asarray(y, dtype=F32), np.asarray(g, dtype=F32)
    B, N = y.shape
    tpr, rpb = sr.threads_per_row(N), sr.rows_per_block(N)
    fn, one, half = F32(N), F32(1), F32(0.5)
    gamma = np.zeros(N, dtype=F32)
    rows, cols = {}, {}
    total = row_sum(y, tpr)
    mean = total / fn
    d = y - mean[:, None]
    dd = d * d
    sq = row_sum(dd, tpr)
    rows["mean"], rows["var"] = (y, total), (dd, sq)
    rstd = one / np.sqrt(sq / fn + F32(eps))
    n = d * rstd[:, None]
    s = np.full((B, N), half, dtype=F32)
    out = y * s
    dz = ((g * y) * s) * (one - s)
    dn = dz * gamma
    c1 = row_sum(dn, tpr) / fn
    c2 = row_sum(dn * n, tpr) / fn
    grad_y = g * s + rstd[:, None] * ((dn - c1[:, None]) - n * c2[:, None])
    partial, gp = col_sums([dz * n, dz], tpr, rpb)
    cols["gamma"], cols["beta"] = (dz * n, gp[0]), (dz, gp[1])
    return {"mean": mean, "rstd": rstd, "out": out, "grad_y": grad_y, "grad_params": gp, "partial": partial,
            "row_terms": rows, "col_terms": cols}


@functools.lru_cache(maxsize=None)
def sln_case(B, N):
    """Inputs (y of mean 0.5 and deviation 2, standard normal g) and the model's results of one shape (shared, read-only)."""
    rng = np.random.default_rng([SLN_SEEDS.get((B, N), 2025), B, N])
    y = (0.5 + 2.0 * rng.standard_normal((B, N))).astype(F32)
    g = rng.standard_normal((B, N)).astype(F32)
    return dict(y=y, g=g, model=swish_layernorm_zero_affine(y, g))
