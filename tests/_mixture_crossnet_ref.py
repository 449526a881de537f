"""numpy restatement of LowRankMixtureCrossNet (torchrec/modules/crossnet.py:271-446) and of its gradients, in float64 or
float32, in the FOLDED layout torchrec_amd/modules/crossnet.py computes: the K experts side by side as one low-rank layer
of rank K r, a2 [K, B, r] -> m [B, K r] through the gate pass of csrc/crossnet.hip (whose formulas `gate_forward` and
`gate_backward` restate), the running x_0 gradient `acc` and the bias gradient as a row-block column sum.  So the faults
these kernels can have are expressible (`fault=`):

  "softmax_last_expert"  the last expert left out of the softmax's denominator
  "dot_last_col"         j = r - 1 left out of the row dot d_k
  "mask_dropped"         grad_a2 not masked by a2 > 0
  "gates_one_layer"      the gate weights' gradient taken from the last layer only (it is a sum over the layers)
  "p_dropped_backward"   grad_a2 not scaled by p_k
  "colsum_last_row"      the last row of the first row block left out of the bias gradient's column sum

Also: the fixtures' accessors, the inputs of the GPU tests (`gpu_case`, `gate_case`, `exact_gate_case`) and the two
tolerances of the GPU tests, which are MEASURED here (`gpu_tolerance`, `softmax_tolerance`)."""
import functools
import os

import numpy as np

from _colsum_order import rows_per_block  # rows per workgroup of cross_bwd_kernel (csrc/colsum.hpp)
from _crossnet_ref import _colsum, rel_err  # noqa: F401  (rel_err is part of this module's surface)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixture_crossnet.npz")
CASES = {"3x10": (3, 10, 2, 5, 3), "37x20": (37, 20, 3, 1, 4), "70x64": (70, 64, 2, 4, 8)}  # (B, N, L, K, r)
FAULTS = ("softmax_last_expert", "dot_last_col", "mask_dropped", "gates_one_layer", "p_dropped_backward", "colsum_last_row")
GATE_FAULTS = FAULTS[:5]  # need K > 1
TRAIN_SHAPES = [(130, 260, 3, 4, 16), (67, 64, 2, 2, 1)]  # (B, N, L, K, r); the second: default rank, the scalar path
# the gate kernels' shapes through the C ABI (B, K, r): one row / r = 1; odd everything; four rows per workgroup with a ragged
# last one and float4; both limits of K, two workgroups; r beyond one round of a wave (260 = 65 float4); r = 1028: five rounds
GATE_SHAPES = [(1, 2, 1), (5, 3, 3), (67, 5, 4), (130, 16, 16), (64, 2, 260), (3, 4, 1028)]
GATE_SHAPE_OFF_GRID = (9, 16, 7)  # run on a base 4 bytes off the 16-byte grid


def param_names(L, K):
    names = [f"{g}.{i}" for g in ("U_kernels", "V_kernels", "bias") for i in range(L)]
    names += [f"gates.{k}.weight" for k in range(K)] if K > 1 else []
    return names + [f"C_kernels.{i}" for i in range(L)]


def param_shapes(N, L, K, r):
    shp = {"U_kernels": (K, N, r), "V_kernels": (K, r, N), "bias": (N, 1), "gates": (1, N), "C_kernels": (K, r, r)}
    return {n: shp[n.split(".")[0]] for n in param_names(L, K)}


# ---- the gate pass (csrc/crossnet.hip mixture_gate_fwd_kernel / _bwd_kernel) ------------------------------------------------
def relu(a):
    return np.where(a > 0, a, np.zeros((), dtype=a.dtype))


def gate_forward(a2, logits, fault=None):
    """(m [B, K r], p [B, K]) from a2 [K, B, r] and logits [B, K], in the dtype of a2; every operation rounded on its own,
    max and sum in k order."""
    K, B, r = a2.shape
    dt = a2.dtype
    logits = np.asarray(logits, dtype=dt)
    mx = logits[:, 0]
    for k in range(1, K):
        mx = np.maximum(mx, logits[:, k])
    e = np.exp(logits - mx[:, None]).astype(dt)
    s = e[:, 0]
    for k in range(1, K - 1 if fault == "softmax_last_expert" else K):
        s = s + e[:, k]
    p = e / s[:, None]
    m = (p.T[:, :, None] * relu(a2)).transpose(1, 0, 2).reshape(B, K * r)
    return np.ascontiguousarray(m), p


def gate_backward(gm, a2, p, fault=None, reverse=False):
    """(grad_a2 [K, B, r], grad_logits [B, K]); `reverse` sums the row dots from the last column."""
    K, B, r = a2.shape
    dt = a2.dtype
    g = np.asarray(gm, dtype=dt).reshape(B, K, r).transpose(1, 0, 2)  # [K, B, r]
    pk = np.asarray(p, dtype=dt).T  # [K, B]
    prod = g * relu(a2)
    cols = range(r - 1 if fault == "dot_last_col" else r)
    d = np.zeros((K, B), dtype=dt)
    for j in (reversed(cols) if reverse else cols):
        d = d + prod[:, :, j]
    t = pk[0] * d[0]
    for k in range(1, K):
        t = t + pk[k] * d[k]
    gl = (pk * (d - t)).T
    scaled = g if fault == "p_dropped_backward" else pk[:, :, None] * g
    ga2 = scaled if fault == "mask_dropped" else np.where(a2 > 0, scaled, np.zeros((), dtype=dt))
    return np.ascontiguousarray(ga2), np.ascontiguousarray(gl)


# ---- the net ------------------------------------------------------------------------------------------------------------------
def _ucat(u):
    K, N, r = u.shape
    return u.transpose(1, 0, 2).reshape(N, K * r)


def run(params, x, g, dtype="float64", fault=None):
    """Forward and backward.  params: the reference's names and shapes.  Returns {"out", "grad_input", "p" [L, B, K],
    "grad": {parameter name: gradient}}."""
    dt = np.dtype(dtype)
    P = {k: np.asarray(v, dtype=dt) for k, v in params.items()}
    x0, g = np.asarray(x, dtype=dt), np.asarray(g, dtype=dt)
    B, N = x0.shape
    L = sum(1 for k in P if k.startswith("bias."))
    K, _, r = P["U_kernels.0"].shape
    wg = np.concatenate([P[f"gates.{k}.weight"] for k in range(K)]) if K > 1 else None  # [K, N]
    kept = []
    x_l = x0
    for l in range(L):
        U, V, C = P[f"U_kernels.{l}"], P[f"V_kernels.{l}"], P[f"C_kernels.{l}"]
        h1 = relu(x_l @ V.reshape(K * r, N).T)  # [B, K r]
        a2 = h1.reshape(B, K, r).transpose(1, 0, 2) @ C.transpose(0, 2, 1)  # [K, B, r]
        if K > 1:
            m, p = gate_forward(a2, x_l @ wg.T, fault)
        else:
            m, p = relu(a2[0]), np.ones((B, 1), dtype=dt)
        t = m @ _ucat(U).T + P[f"bias.{l}"].reshape(N)
        kept.append((x_l, t, h1, a2, m, p))
        x_l = x0 * t + x_l
    res = {"out": x_l, "p": np.stack([k[5] for k in kept]), "grad": {}}
    G = g
    acc = np.zeros_like(x0)
    g_wg = np.zeros((K, N), dtype=dt)
    for l in reversed(range(L)):
        x_l, t, h1, a2, m, p = kept[l]
        U, V, C = P[f"U_kernels.{l}"], P[f"V_kernels.{l}"], P[f"C_kernels.{l}"]
        gy = G * x0
        acc = G * t if l == L - 1 else acc + G * t
        res["grad"][f"bias.{l}"] = _colsum(gy, rows_per_block(N), fault).reshape(N, 1)
        res["grad"][f"U_kernels.{l}"] = (gy.T @ m).reshape(N, K, r).transpose(1, 0, 2)
        gm = gy @ _ucat(U)
        if K > 1:
            ga2, gl = gate_backward(gm, a2, p, fault)
        else:
            ga2, gl = np.where(a2 > 0, gm[None], np.zeros((), dtype=dt)), None
        h1k = h1.reshape(B, K, r).transpose(1, 0, 2)
        res["grad"][f"C_kernels.{l}"] = ga2.transpose(0, 2, 1) @ h1k
        ga1 = np.where(h1 > 0, (ga2 @ C).transpose(1, 0, 2).reshape(B, K * r), np.zeros((), dtype=dt))
        res["grad"][f"V_kernels.{l}"] = (ga1.T @ x_l).reshape(K, r, N)
        G = G + ga1 @ V.reshape(K * r, N)
        if K > 1:
            if fault != "gates_one_layer" or l == L - 1:
                g_wg = g_wg + gl.T @ x_l
            G = G + gl @ wg
    for k in range(K if K > 1 else 0):
        res["grad"][f"gates.{k}.weight"] = g_wg[k:k + 1]
    res["grad_input"] = G + acc
    return res


def sgd_steps(params, x, g, lr, steps, dtype="float64"):
    """`steps` plain SGD steps on the loss sum(out * g); returns the parameters after them (float64 by default)."""
    p = {k: np.asarray(v, dtype=np.dtype(dtype)) for k, v in params.items()}
    for _ in range(steps):
        grads = run(p, x, g, dtype)["grad"]
        p = {k: v - lr * grads[k] for k, v in p.items()}
    return p


def result_errors(got, ref):
    """{name: rel_err} over out, grad_input, p (if both have it) and every parameter gradient."""
    errs = {"out": rel_err(got["out"], ref["out"]), "grad_input": rel_err(got["grad_input"], ref["grad_input"])}
    if "p" in got and "p" in ref:
        errs["p"] = rel_err(got["p"], ref["p"])
    for k in ref["grad"]:
        errs["grad." + k] = rel_err(got["grad"][k], ref["grad"][k])
    return errs


# ---- inputs of the GPU tests ---------------------------------------------------------------------------------------------------
def gpu_case(B, N, L, K, r, seed=0):
    """(params, x, g) float32: each expert's U_k, V_k, C_k xavier-normal-sized as a matrix of its own (the reference's
    initialiser takes the 3-D fans, which shrinks them with K r: results of size 1e-3 would test little), gate weights of
    size 1 / sqrt(N) (logits of size 1: a softmax that is neither flat nor one-hot), biases of size 0.1, standard normal x
    and g.  For r = 1 see below."""
    rng = np.random.default_rng([seed, B, N, L, K, r])
    params = {}
    for name, shape in param_shapes(N, L, K, r).items():
        kind = name.split(".")[0]
        std = {"bias": 0.1, "gates": 1.0 / np.sqrt(N)}.get(kind) or np.sqrt(2.0 / (shape[-2] + shape[-1]))
        params[name] = (rng.standard_normal(shape) * std).astype(np.float32)
        if kind == "C_kernels" and r == 1:
            # a negative scalar C_k kills expert k outright (relu(C_k relu(.)) = 0), and a layer whose C_k are all negative
            # is dead: the signs alternate from +, so every layer has live and masked experts
            params[name] = np.abs(params[name]) * np.where(np.arange(K) % 2 == 0, 1, -1).astype(np.float32).reshape(K, 1, 1)
    x = rng.standard_normal((B, N)).astype(np.float32)
    g = rng.standard_normal((B, N)).astype(np.float32)
    return params, x, g


def gate_case(B, K, r, seed=0):
    """(a2 [K, B, r], logits [B, K], grad_m [B, K r]) float32 for the gate kernels: logits of size 2; a2 standard normal
    with some +0.0 and -0.0 sprinkled in."""
    rng = np.random.default_rng([seed, B, K, r, 77])
    a2 = rng.standard_normal((K, B, r)).astype(np.float32)
    zero = rng.integers(0, 8, a2.shape)
    a2[zero == 0] = 0.0
    a2[zero == 1] = -0.0
    logits = (2.0 * rng.standard_normal((B, K))).astype(np.float32)
    gm = rng.standard_normal((B, K * r)).astype(np.float32)
    return a2, logits, gm


def exact_gate_case(B, K, r, seed=0):
    """(grad_m, a2, p) for the gate backward whose every product and sum is exact in float32 in any order: grad_m and a2
    small integers times powers of two, p multiples of 1/8 that sum to 1 per row."""
    rng = np.random.default_rng([seed, B, K, r, 78])
    gm = rng.integers(-4, 5, (B, K * r)).astype(np.float32) * np.float32(0.25)
    a2 = rng.integers(-4, 5, (K, B, r)).astype(np.float32) * np.float32(0.5)
    eighths = np.zeros((B, K), dtype=np.int64)
    for b in range(B):
        np.add.at(eighths[b], rng.integers(0, K, 8), 1)
    return gm, a2, (eighths / 8.0).astype(np.float32)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture(case):
    """The reference's recorded run: {"params", "x", "g", "f32": {"out", "grad_input", "grad": {...}, "p" [L, B, K]},
    "f64": the same without p, from the .double() module}."""
    z = _golden()
    B, N, L, K, r = CASES[case]
    names = param_names(L, K)
    pre = case + "|"
    fx = {"params": {n: z[pre + "param|" + n] for n in names}, "x": z[pre + "x"], "g": z[pre + "g"]}
    for prec in ("f32", "f64"):
        fx[prec] = {"out": z[pre + prec + "|out"], "grad_input": z[pre + prec + "|grad_input"],
                    "grad": {n: z[pre + prec + "|grad|" + n] for n in names}}
    fx["f32"]["p"] = z[pre + "p"]
    return fx


# ---- the tolerances ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def measured_errors():
    """The float32-vs-float64 error of (a) the reference's fixtures and (b) this restatement on TRAIN_SHAPES:
    {label: worst rel_err over the run's tensors}."""
    errs = {}
    for case in CASES:
        fx = fixture(case)
        errs[f"reference {case}"] = max(result_errors(fx["f32"], fx["f64"]).values())
    for shape in TRAIN_SHAPES:
        p, x, g = gpu_case(*shape)
        e = result_errors(run(p, x, g, "float32"), run(p, x, g, "float64"))
        errs["restatement " + "x".join(map(str, shape))] = max(e.values())
    return errs


def gpu_tolerance():
    """8 x the worst measured float32-vs-float64 error: the factor covers another summation order and the GEMM library's
    accumulation (the argument of _crossnet_ref.gpu_tolerance).  Compared with `rel_err`."""
    return 8.0 * max(measured_errors().values())


@functools.lru_cache(maxsize=None)
def measured_softmax_errors():
    """{shape: worst |p32 - p64|} of the float32 restatement of the softmax over the gate kernels' test shapes."""
    errs = {}
    for shape in GATE_SHAPES + [GATE_SHAPE_OFF_GRID]:
        a2, logits, _ = gate_case(*shape)
        p32 = gate_forward(a2, logits)[1]
        p64 = gate_forward(a2.astype(np.float64), logits.astype(np.float64))[1]
        errs[shape] = float(np.abs(p32 - p64).max())
    return errs


def softmax_tolerance():
    """8 x the worst absolute float32-vs-float64 error of p: the device's expf may round the last bit otherwise than the
    host's.  p <= 1, so it is absolute."""
    return 8.0 * max(measured_softmax_errors().values())
