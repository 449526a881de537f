"""What the DeepFM tests share: the recorded runs of the reference (tests/golden/deepfm.npz, written by
tests/golden/make_deepfm_golden.py), a float64 restatement of torchrec/modules/deepfm.py and torchrec/models/deepfm.py, the
exact integer model the C-ABI tests compare with bit for bit, and the GPU tolerance, which is measured from the reference's
own float32-vs-float64 error."""
import functools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

MODULE_CASES = {
    "doc3d": (3, [(2, 64), (2, 32)]),
    "d3": (37, [(3,), (3,), (3,)]),
    "d8": (5, [(8,), (8,), (8,), (8,)]),
    "mixed": (33, [(5,), (260,), (12,)]),
    "w1": (64, [(64,), (1,), (67,)]),
    "criteo": (70, [(128,)] * 27),
}
# name -> (B, D, [(table, rows, features)], KeyedJaggedTensor key order, dense features, hidden, deep_fm_dimension)
MODEL_CASES = {
    "doc": (2, 8, [("t1", 100, ["f1", "f3"]), ("t2", 100, ["f2"])], ["f1", "f2", "f3"], 10, 20, 5),
    "ragged": (5, 3, [("t1", 7, ["a"]), ("t2", 11, ["b"]), ("t3", 5, ["c"])], ["a", "b", "c"], 4, 6, 3),
}
DEEP_OUT = 4
GEMM_TOL = dict(rtol=1e-3, atol=2e-5)  # tests/test_dlrm_e2e_gpu.py's tolerance for quantities that pass through GEMMs


@functools.lru_cache(maxsize=None)
def _npz():
    g = np.load(os.path.join(HERE, "golden", "deepfm.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def module_fixture(case):
    """{"xs": inputs in their recorded shapes, "gfm", "gdeep", "params", "rows", "f32": {...}, "f64": {...}}."""
    g, pre = _npz(), f"mod|{case}|"
    B, shapes = MODULE_CASES[case]
    if case == "criteo":  # drawn, not stored (the golden script's docstring says why); the recorded row sums pin the draw
        gen = torch.Generator().manual_seed(int(g[pre + "x_seed"].item()))
        xs = [torch.randn(B, *s, generator=gen).numpy() for s in shapes]
        np.testing.assert_array_equal(np.concatenate(xs, 1).astype(np.float64).sum(1), g[pre + "x_rowsum64"])
    else:
        xs = [g[pre + f"x{i}"] for i in range(len(shapes))]
    fx = {"xs": xs, "gfm": g[pre + "gfm"], "gdeep": g[pre + "gdeep"], "rows": g[pre + "rows"],
          "params": {k[len(pre) + 6:]: v for k, v in g.items() if k.startswith(pre + "param|")}}
    for prec in ("f32", "f64"):
        p = pre + prec + "|"
        fx[prec] = {k[len(p):]: v for k, v in g.items() if k.startswith(p)}
    return fx


@functools.lru_cache(maxsize=None)
def model_fixture(case):
    g, pre = _npz(), f"model|{case}|"
    fx = {k: g[pre + k] for k in ("values", "lengths", "dense", "g")}
    fx["sd"] = {k[len(pre) + 3:]: v for k, v in g.items() if k.startswith(pre + "sd|")}
    for prec in ("f32", "f64"):
        p = pre + prec + "|"
        fx[prec] = {"logits": g[p + "logits"], "grad": {k[len(p) + 5:]: v for k, v in g.items() if k.startswith(p + "grad|")}}
    return fx


def flat_cat(xs, dtype=np.float64):
    return np.concatenate([np.asarray(x, dtype=dtype).reshape(x.shape[0], -1) for x in xs], axis=1)


# ---- float64 restatement of the modules ------------------------------------------------------------------------------
def fm_ref(xs, gfm, dtype=np.float64):
    """(fm [B, 1], d fm / d x [B, N]) of torchrec/modules/deepfm.py:209-215: 0.5 * ((sum x)^2 - sum x^2); gradient g (s - x)."""
    x = flat_cat(xs, dtype)
    s = x.sum(1, keepdims=True)
    fm = (s * s - (x * x).sum(1, keepdims=True)) * dtype(0.5)
    return fm, np.asarray(gfm, dtype=dtype).reshape(-1, 1) * (s - x)


def deep_ref(xs, params, gdeep, dtype=np.float64):
    """DeepFM(Linear + ReLU): (out, d / d x, {parameter gradients})."""
    x = flat_cat(xs, dtype)
    W, b = params["0.weight"].astype(dtype), params["0.bias"].astype(dtype)
    y = x @ W.T + b
    gy = np.asarray(gdeep, dtype=dtype) * (y > 0)
    return np.maximum(y, 0), gy @ W, {"0.weight": gy.T @ x, "0.bias": gy.sum(0)}


# ---- float64 restatement of SimpleDeepFMNN (torchrec/models/deepfm.py), torch autograd over plain tensor operations -----
def model_ref(case, sd, values, lengths, dense, g, dtype=torch.float64):
    """(logits, {parameter gradients by the reference's state-dict key})."""
    B, D, tables, keys, _, _, _ = MODEL_CASES[case]
    p = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_() for k, v in sd.items()}
    x = torch.from_numpy(dense).to(dtype)
    x = torch.relu(x @ p["dense_arch.model.0.weight"].T + p["dense_arch.model.0.bias"])
    x = torch.relu(x @ p["dense_arch.model.2.weight"].T + p["dense_arch.model.2.bias"])
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    pooled = {}
    for i, k in enumerate(keys):
        table = next(t for t, _, fs in tables if k in fs)
        w = p[f"sparse_arch.embedding_bag_collection.embedding_bags.{table}.weight"]
        bags = []
        for b in range(B):
            ids = torch.from_numpy(values[offsets[i * B + b]:offsets[i * B + b + 1]])
            bags.append(w[ids].sum(0))
        pooled[k] = torch.stack(bags)
    row = torch.cat([x] + [pooled[f] for _, _, fs in tables for f in fs], dim=1)  # table order, as the collection's keys
    deep = torch.relu(row @ p["inter_arch.deep_fm.dense_module.0.weight"].T + p["inter_arch.deep_fm.dense_module.0.bias"])
    s = row.sum(1, keepdim=True)
    fm = (s * s - (row * row).sum(1, keepdim=True)) * 0.5
    logits = torch.sigmoid(torch.cat([x, deep, fm], 1) @ p["over_arch.model.0.weight"].T + p["over_arch.model.0.bias"])
    logits.backward(torch.from_numpy(g).to(dtype))
    return logits.detach().numpy(), {k: v.grad.numpy() for k, v in p.items()}


# ---- the two normalised errors of the FM term ------------------------------------------------------------------------
def fm_errors(xs, gfm, fm, gx, rows=None):
    """(worst |fm - fm64| / (0.5 (s^2 + sum x^2)), worst |gx - gx64| / (|g| sum |x|)) per row, against the float64
    restatement; `gx` holds `rows` only."""
    x = flat_cat(xs)
    fm64, gx64 = fm_ref(xs, gfm)
    s = x.sum(1, keepdims=True)
    out = np.abs(fm.astype(np.float64) - fm64) / (0.5 * (s * s + (x * x).sum(1, keepdims=True)))
    rows = np.arange(x.shape[0]) if rows is None else rows
    scale = np.abs(np.asarray(gfm, np.float64).reshape(-1, 1)) * np.abs(x).sum(1, keepdims=True)
    grad = np.abs(gx.astype(np.float64) - gx64[rows]) / scale[rows]
    return float(out.max()), float(grad.max())


@functools.lru_cache(maxsize=None)
def measured_errors():
    """The reference's own float32 results against its float64 results, worst over the module fixtures."""
    worst_out = worst_grad = 0.0
    for case in MODULE_CASES:
        fx = module_fixture(case)
        x = flat_cat(fx["xs"])
        s = x.sum(1, keepdims=True)
        out = np.abs(fx["f32"]["fm"].astype(np.float64) - fx["f64"]["fm"]) / (0.5 * (s * s + (x * x).sum(1, keepdims=True)))
        scale = (np.abs(fx["gfm"].astype(np.float64)).reshape(-1, 1) * np.abs(x).sum(1, keepdims=True))[fx["rows"]]
        grad = np.abs(fx["f32"]["gx_fm"].astype(np.float64) - fx["f64"]["gx_fm"]) / scale
        worst_out, worst_grad = max(worst_out, float(out.max())), max(worst_grad, float(grad.max()))
    return worst_out, worst_grad


def gpu_tolerances():
    """(output, gradient): 8 x the measured figures; the factor covers the kernel's summation order."""
    o, g = measured_errors()
    return 8.0 * o, 8.0 * g


# ---- the exact model of the C-ABI tests --------------------------------------------------------------------------------
def fm_int_model(xs, gfm, gcat=None):
    """int64 arithmetic on integer-valued inputs: (fm, row_sum, cat, [gradient per segment]) as float32.  With x in
    {-1, 0, 1}, |gfm| <= 4, |gcat| <= 8 and N <= 3456 every intermediate of the float32 kernel is an integer or half-integer
    below 2^24, so float32 is exact in any summation order and the comparison is bit for bit."""
    xi = [np.asarray(x).astype(np.int64) for x in xs]
    cat = np.concatenate(xi, axis=1)
    assert all((np.asarray(x) == i).all() for x, i in zip(xs, xi))
    s = cat.sum(1)
    twice = s * s - (cat * cat).sum(1)
    assert np.abs(s * s).max(initial=0) < 2 ** 24
    gf = np.asarray(gfm).astype(np.int64).reshape(-1, 1)
    grads, col = [], 0
    for x in xi:
        g = gf * (s.reshape(-1, 1) - x)
        if gcat is not None:
            g = g + np.asarray(gcat).astype(np.int64)[:, col:col + x.shape[1]]
        assert np.abs(g).max(initial=0) < 2 ** 24
        grads.append(g.astype(np.float32))
        col += x.shape[1]
    return (twice.astype(np.float64) * 0.5).astype(np.float32), s.astype(np.float32), cat.astype(np.float32), grads
