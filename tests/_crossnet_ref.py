"""numpy restatement of the three cross networks (torchrec/modules/crossnet.py: CrossNet :19-89, LowRankCrossNet :92-188,
VectorCrossNet :191-268) and of their gradients, in float64 or in float32 with the reference's operation order, laid out
the way csrc/crossnet.hip computes them (running x_0 gradient `acc`, column sums per row block, row dots) so that the
faults a kernel of this kind can have are expressible (`fault=`):

  "dot_last_col"    the last column left out of a row dot (VectorCrossNet: s_l and d_l)
  "colsum_last_row" the last row of the first row block left out of every column sum
  "skip_bias"       the bias of the last layer skipped in the forward
  "acc_overwrite"   acc overwritten instead of accumulated on the non-first layers of the backward

Also: the fixtures' accessors, the inputs of the GPU tests (`gpu_case`), and the tolerance of the GPU tests, which is
MEASURED here (`gpu_tolerance`): 8 x the worst float32-vs-float64 error of the reference's own fixtures and of this
restatement on the GPU tests' shapes."""
import functools
import os

import numpy as np

from _colsum_order import rows_per_block  # rows per workgroup of cross_bwd_kernel (csrc/colsum.hpp)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crossnet.npz")
KINDS = ("CrossNet", "LowRankCrossNet", "VectorCrossNet")
CASES = {"3x10": (3, 10, 2, 3), "37x20": (37, 20, 3, 5), "70x64": (70, 64, 2, 1)}  # (B, N, L, r)
FAULTS = ("dot_last_col", "colsum_last_row", "skip_bias", "acc_overwrite")
VECTOR_ROWS_PER_BLOCK = 128  # csrc/crossnet.hip kVecRowsPerBlock
# the GPU tests' shapes (the issue's): vector kernels (B, N, L); modules (B, N, L, r)
VECTOR_GPU_SHAPES = [(1, 4, 1), (5, 12, 3), (67, 64, 2), (130, 260, 3), (64, 1028, 4), (3, 4096, 8)]
TRAIN_SHAPE = (130, 260, 3, 16)


def param_names(kind, L):
    groups = {"CrossNet": ("kernels", "bias"), "LowRankCrossNet": ("W_kernels", "V_kernels", "bias"),
              "VectorCrossNet": ("kernels", "bias")}[kind]
    return [f"{g}.{i}" for g in groups for i in range(L)]


def param_shapes(kind, N, L, r):
    shp = {"kernels": (N, N) if kind == "CrossNet" else (N, 1), "W_kernels": (N, r), "V_kernels": (r, N), "bias": (N, 1)}
    return {n: shp[n.split(".")[0]] for n in param_names(kind, L)}


# ---- pieces ------------------------------------------------------------------------------------------------------------------
def _rowdot(a, w, fault):
    """[B] = a[b, :] . w"""
    if fault == "dot_last_col":
        return (a[:, :-1] * w[..., :-1]).sum(axis=1, dtype=a.dtype)
    return (a * w).sum(axis=1, dtype=a.dtype)


def _colsum(a, rpb, fault):
    if fault == "colsum_last_row":
        keep = np.ones(a.shape[0], dtype=bool)
        keep[min(rpb, a.shape[0]) - 1] = False
        a = a[keep]
    return a.sum(axis=0, dtype=a.dtype)


def cross_backward_f32(G, x0, t, acc, first):
    """tbe_cross_backward_f32 in float32: (grad_y, acc, bias_grad); each product and add rounded on its own.  The column
    sum is exact, whatever its order, for the integer-valued inputs the ABI test uses."""
    G, x0, t = (np.asarray(a, dtype=np.float32) for a in (G, x0, t))
    gy = G * x0
    gt = G * t
    new_acc = gt if first else np.asarray(acc, dtype=np.float32) + gt
    return gy, new_acc, gy.sum(axis=0, dtype=np.float32)


def layer_from_y(x0, x_l, y, b):
    """x_{l+1} = x_0 * (y + b) + x_l — the element-wise part of a GEMM-based layer given the GEMM's result."""
    return x0 * (y + b) + x_l


def vector_layer_from_s(x0, x_l, s, b):
    """x_{l+1} = (x_0 * s + b) + x_l — the element-wise part of a VectorCrossNet layer given the row dots s [B]."""
    return (x0 * s[:, None] + b) + x_l


def _cast(params, dtype):
    return {k: np.asarray(v, dtype=dtype) for k, v in params.items()}


# ---- the nets ------------------------------------------------------------------------------------------------------------------
def run(kind, params, x, g, dtype="float64", fault=None):
    """Forward and backward of one net.  params: {"kernels.0": ..., "bias.0": ...} with the reference's shapes.
    Returns {"out", "grad_input", "s" (VectorCrossNet: [L, B]), "grad": {parameter name: gradient}}."""
    dt = np.dtype(dtype)
    p = _cast(params, dt)
    x0, g = np.asarray(x, dtype=dt), np.asarray(g, dtype=dt)
    B, N = x0.shape
    L = sum(1 for k in p if k.startswith("bias."))
    bias = [p[f"bias.{l}"].reshape(N) for l in range(L)]
    if fault == "skip_bias":
        bias[L - 1] = np.zeros(N, dtype=dt)
    res = {"grad": {}}
    xs, ts, vs, ss = [x0], [], [], []
    x_l = x0
    for l in range(L):
        if kind == "VectorCrossNet":
            s = _rowdot(x_l, p[f"kernels.{l}"].reshape(N), fault)
            ss.append(s)
            x_l = vector_layer_from_s(x0, x_l, s, bias[l])
        else:
            if kind == "CrossNet":
                y = x_l @ p[f"kernels.{l}"].T
            else:
                v = x_l @ p[f"V_kernels.{l}"].T
                vs.append(v)
                y = v @ p[f"W_kernels.{l}"].T
            t = y + bias[l]
            ts.append(t)
            x_l = x0 * t + x_l
        xs.append(x_l)
    res["out"] = xs[L]
    rpb = VECTOR_ROWS_PER_BLOCK if kind == "VectorCrossNet" else rows_per_block(N)
    G = g
    acc = np.zeros_like(x0)
    for l in reversed(range(L)):
        first = l == L - 1
        if kind == "VectorCrossNet":
            w = p[f"kernels.{l}"].reshape(N)
            d = _rowdot(G, x0, fault)
            gs = G * ss[l][:, None]
            acc = gs if (first or fault == "acc_overwrite") else acc + gs
            res["grad"][f"bias.{l}"] = _colsum(G, rpb, fault).reshape(N, 1)
            res["grad"][f"kernels.{l}"] = _colsum(d[:, None] * xs[l], rpb, fault).reshape(N, 1)
            G = G + d[:, None] * w
        else:
            gy = G * x0
            gt = G * ts[l]
            acc = gt if (first or fault == "acc_overwrite") else acc + gt
            res["grad"][f"bias.{l}"] = _colsum(gy, rpb, fault).reshape(N, 1)
            if kind == "CrossNet":
                K = p[f"kernels.{l}"]
                res["grad"][f"kernels.{l}"] = gy.T @ xs[l]
                G = G + gy @ K
            else:
                W, V = p[f"W_kernels.{l}"], p[f"V_kernels.{l}"]
                gv = gy @ W
                res["grad"][f"W_kernels.{l}"] = gy.T @ vs[l]
                res["grad"][f"V_kernels.{l}"] = gv.T @ xs[l]
                G = G + gv @ V
    res["grad_input"] = G + acc
    if kind == "VectorCrossNet":
        res["s"] = np.stack(ss)
    return res


def sgd_steps(kind, params, x, g, lr, steps, dtype="float64"):
    """`steps` plain SGD steps on the loss sum(out * g); returns the parameters after them (float64 by default)."""
    p = _cast(params, np.dtype(dtype))
    for _ in range(steps):
        grads = run(kind, p, x, g, dtype)["grad"]
        p = {k: v - lr * grads[k] for k, v in p.items()}
    return p


# ---- error measure, inputs of the GPU tests, fixtures ------------------------------------------------------------------------------
def rel_err(a, ref):
    """max |a - ref| / max |ref|: the error of a tensor relative to its own scale (an element-wise quotient would measure
    cancellation in single elements, not the arithmetic)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    scale = np.abs(ref).max()
    return float(np.abs(a - ref).max() / scale) if scale > 0 else float(np.abs(a).max())


def result_errors(got, ref):
    """{name: rel_err} over out, grad_input, s (if both have it) and every parameter gradient."""
    errs = {"out": rel_err(got["out"], ref["out"]), "grad_input": rel_err(got["grad_input"], ref["grad_input"])}
    if "s" in got and "s" in ref:
        errs["s"] = rel_err(got["s"], ref["s"])
    for k in ref["grad"]:
        errs["grad." + k] = rel_err(got["grad"][k], ref["grad"][k])
    return errs


def gpu_case(kind, B, N, L, r=1, seed=0):
    """(params, x, g) float32 for a GPU test: xavier-normal-sized kernels (VectorCrossNet: 0.4 / sqrt(N), so that the row
    dots stay near 0.4 and an 8-layer net stays as well conditioned as a 2-layer one: with xavier's 1.4 / sqrt(N) the
    float32 restatement itself is 2.5e-5 from float64 at L = 8), biases of size 0.1, standard normal x and g."""
    rng = np.random.default_rng([seed, B, N, L, r, KINDS.index(kind)])
    params = {}
    for name, shape in param_shapes(kind, N, L, r).items():
        if name.startswith("bias"):
            std = 0.1
        elif kind == "VectorCrossNet":
            std = 0.4 / np.sqrt(N)
        else:
            std = np.sqrt(2.0 / (shape[0] + shape[1]))
        params[name] = (rng.standard_normal(shape) * std).astype(np.float32)
    x = rng.standard_normal((B, N)).astype(np.float32)
    g = rng.standard_normal((B, N)).astype(np.float32)
    return params, x, g


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture(kind, case):
    """The reference's recorded run: {"params", "x", "g", "y" ([L, ...] the per-layer GEMM / dot results in float32),
    "f32": {"out", "grad_input", "grad": {...}}, "f64": the same from the .double() module}."""
    z = _golden()
    B, N, L, r = CASES[case]
    names = param_names(kind, L)
    pre = f"{kind}|{case}|"
    fx = {"params": {n: z[pre + "param|" + n] for n in names}, "x": z[f"case|{case}|x"], "g": z[f"case|{case}|g"],
          "y": z[pre + "y"]}
    for prec in ("f32", "f64"):
        fx[prec] = {"out": z[pre + prec + "|out"], "grad_input": z[pre + prec + "|grad_input"],
                    "grad": {n: z[pre + prec + "|grad|" + n] for n in names}}
    return fx


@functools.lru_cache(maxsize=None)
def measured_errors():
    """The float32-vs-float64 error of (a) the reference's fixtures and (b) this restatement on the GPU tests' shapes:
    {label: worst rel_err over the run's tensors}."""
    errs = {}
    for kind in KINDS:
        for case in CASES:
            fx = fixture(kind, case)
            errs[f"reference {kind} {case}"] = max(result_errors(fx["f32"], fx["f64"]).values())
    for B, N, L in VECTOR_GPU_SHAPES:
        p, x, g = gpu_case("VectorCrossNet", B, N, L)
        e = result_errors(run("VectorCrossNet", p, x, g, "float32"), run("VectorCrossNet", p, x, g, "float64"))
        errs[f"restatement VectorCrossNet {B}x{N} L={L}"] = max(e.values())
    B, N, L, r = TRAIN_SHAPE
    for kind in KINDS:
        p, x, g = gpu_case(kind, B, N, L, r)
        e = result_errors(run(kind, p, x, g, "float32"), run(kind, p, x, g, "float64"))
        errs[f"restatement {kind} {B}x{N} L={L} r={r}"] = max(e.values())
    return errs


def gpu_tolerance():
    """8 x the worst measured float32-vs-float64 error: the factor covers another summation order and the GEMM library's
    accumulation (as in tests/test_fused_optimizers.py).  Compared with `rel_err`."""
    return 8.0 * max(measured_errors().values())
