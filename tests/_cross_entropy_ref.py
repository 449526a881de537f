"""Float64 numpy restatement of cross-entropy with ignore_index (include/tbe_hip.h, tbe_cross_entropy_*_f32), the inputs the
GPU tests use, and the float32-vs-float64 error of torch's own F.cross_entropy on exactly those inputs, from which the GPU
tolerance is derived (8 x, this project's convention: the factor covers summation order and exp rounding).

    valid row r, label t:  lse = log sum_v exp(x[r, v]);  loss_r = lse - x[r, t];  grad[r, v] = (exp(x[r, v] - lse) - [v == t]) * s
    ignored row:           loss_r = 0, grad row = 0
    mean: loss = sum_r loss_r / n_valid, s = g / n_valid;   sum: s = g;   none: s = g[r]"""
import functools

import numpy as np
import torch
from torch.nn import functional as F

IGNORE = -100
REDUCTIONS = ("mean", "sum", "none")

# Threads per row and rows per workgroup by V (csrc/cross_entropy.hip): 16 x 16 up to 256, 64 x 4 up to 4096, 256 x 1 beyond.
RULE_EDGES = (256, 4096)
# 1023 .. 1025: both sides of one float4 trip of 256 threads; 2049: the second trip plus one; 256 | 257 and 4096 | 4097: the
# edges of the rule; 3708: ml-1m's vocabulary (26 746, ml-20m's, runs once at R = 5).
ABI_WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3708, 4096, 4097)


def rows_per_block(V):
    return 16 if V <= RULE_EDGES[0] else 4 if V <= RULE_EDGES[1] else 1


def ragged_rows(V):
    """Three row blocks, the last one ragged (a single row where a block is one row)."""
    rpb = rows_per_block(V)
    return 2 * rpb + max(1, rpb // 3)


def abi_shapes():
    """(R, V, share of valid rows)."""
    out = []
    for V in ABI_WIDTHS:
        out += [(1, V, 1.0), (ragged_rows(V), V, 1.0)]
    out += [(5, 26746, 1.0)]
    out += [(300, V, 0.15) for V in (65, 1025, 4097)]
    return out


def gpu_case(R, V, share=1.0, seed=0):
    """(x float32 [R, V], target int64 [R] with IGNORE in about 1 - share of the rows, at least one row valid)."""
    rng = np.random.default_rng([seed, R, V])
    x = (2.0 * rng.standard_normal((R, V))).astype(np.float32)
    target = rng.integers(0, V, size=R).astype(np.int64)
    if share < 1.0:
        drop = rng.random(R) >= share
        drop[rng.integers(0, R)] = False
        target[drop] = IGNORE
    return x, target


def label_cases():
    """[(name, x, target)]: the label and value cases of tests/test_cross_entropy_abi_gpu.py, ignore_index = IGNORE, at a
    width of each threads-per-row class with V % 4 != 0."""
    out = []
    for V in (65, 1025, 4099):
        R = 2 * rows_per_block(V) + 1
        x, target = gpu_case(R, V, seed=3)
        out.append((f"label0|{V}", x, np.zeros(R, dtype=np.int64)))
        out.append((f"label_last|{V}", x, np.full(R, V - 1, dtype=np.int64)))
        out.append((f"label_on_max|{V}", x, x.argmax(1).astype(np.int64)))
        rng = np.random.default_rng([7, V])
        big = np.where(rng.random((R, V)) < 0.5, np.float32(1e4), np.float32(-1e4)).astype(np.float32)
        out.append((f"pm1e4|{V}", big, target))
        holes = x.copy()
        holes[rng.random((R, V)) < 0.3] = -np.inf
        holes[np.arange(R), target] = x[np.arange(R), target]  # the label's logit stays finite: so does the loss
        holes[0, :] = -np.inf                                  # one row with a single finite entry
        holes[0, target[0]] = 0.25
        out.append((f"neg_inf|{V}", holes, target))
    return out


def grad_out_for(R, reduction):
    """The upstream gradient the tests use: a scalar for mean / sum, a vector for none."""
    if reduction == "none":
        return (0.5 + np.arange(R, dtype=np.float64) % 7 / 4.0).astype(np.float32)
    return np.float32(0.75)


def run(x, target, ignore_index, reduction, grad_out):
    """{"loss", "grad", "n_valid"} in float64."""
    x = np.asarray(x, dtype=np.float64)
    target = np.asarray(target)
    R, V = x.shape
    valid = target != ignore_index
    t = np.where(valid, target, 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = x.max(1) if R else np.zeros(0)
        lse = m + np.log(np.exp(x - m[:, None]).sum(1))
        rows = np.where(valid, lse - x[np.arange(R), t], 0.0)
        n = int(valid.sum())
        g = np.asarray(grad_out, dtype=np.float64)
        s = {"mean": g / n if n else np.float64("nan"), "sum": g, "none": g}[reduction]
        onehot = np.zeros((R, V))
        onehot[np.arange(R), t] = 1.0
        grad = (np.exp(x - lse[:, None]) - onehot) * (s[:, None] if reduction == "none" else s)
        grad[~valid] = 0.0
        loss = {"mean": rows.sum() / n if n else np.float64("nan"), "sum": rows.sum(), "none": rows}[reduction]
    return {"loss": np.asarray(loss), "grad": grad, "n_valid": n}


def torch_run(x, target, ignore_index, reduction, grad_out, dtype=torch.float32, device="cpu"):
    """The same through F.cross_entropy."""
    xt = torch.from_numpy(np.asarray(x)).to(device=device, dtype=dtype).requires_grad_()
    loss = F.cross_entropy(xt, torch.from_numpy(np.asarray(target)).to(device), ignore_index=ignore_index, reduction=reduction)
    loss.backward(torch.from_numpy(np.asarray(grad_out)).to(device=device, dtype=dtype))
    return {"loss": loss.detach().cpu().numpy(), "grad": xt.grad.cpu().numpy(), "n_valid": int((np.asarray(target) != ignore_index).sum())}


def result_errors(got, want):
    """{"loss", "grad"}: the largest deviation from the float64 result `want`, each relative to the scale of what it is
    compared with (the largest |loss| of the case, the largest |gradient element| of the case)."""
    out = {}
    for k in ("loss", "grad"):
        w = np.asarray(want[k], dtype=np.float64)
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert (np.isfinite(g) == np.isfinite(w)).all(), k
        fin = np.isfinite(w)
        scale = float(np.abs(w[fin]).max()) if fin.any() else 0.0
        out[k] = float(np.abs(g[fin] - w[fin]).max()) / scale if scale > 0.0 else 0.0
    return out


def all_gpu_cases():
    """[(name, x, target)] of every input the GPU tests compare within the tolerance."""
    out = [(f"{R}x{V}@{share}", *gpu_case(R, V, share)) for R, V, share in abi_shapes()]
    return out + label_cases()


@functools.lru_cache(maxsize=None)
def measured_errors():
    """{"loss", "grad"}: the float32-vs-float64 error of F.cross_entropy itself (CPU) on the GPU tests' own inputs, largest
    over the cases and the three reductions."""
    worst = {"loss": 0.0, "grad": 0.0}
    for _, x, target in all_gpu_cases():
        for red in REDUCTIONS:
            g = grad_out_for(x.shape[0], red)
            e = result_errors(torch_run(x, target, IGNORE, red, g), run(x, target, IGNORE, red, g))
            worst = {k: max(worst[k], e[k]) for k in worst}
    return worst


def gpu_tolerance():
    """{"loss", "grad"}: 8 x measured_errors()."""
    return {k: 8.0 * v for k, v in measured_errors().items()}
