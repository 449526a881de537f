"""numpy restatement of csrc/residual_layernorm.hip (include/tbe_hip.h): the dropout draw beside the attention kernel's, the
formulas in float64, torch's own composition of the same operations, the cases of the GPU test and its tolerance — 8 x the
worst float32-vs-float64 error of torch's composition over those cases; nothing of the kernel enters."""
import functools

import numpy as np

from _attention_ref import dropout_threshold, fmix32
from _crossnet_ref import rel_err  # max |a - ref| / max |ref|

EPS = 1e-5
SEED, CALL = 20240917, (3 << 32) | 5
SITE_IN, SITE_OUT = 1, 2
# one width per threads-per-row class with both sides of its edges (64 | 68, 1024 | 1028), the limits 4 and 4096, and
# widths whose last float4 slot only some threads of the row hold (4, 260, 1028)
WIDTHS = (4, 64, 68, 260, 1024, 1028, 4096)
# name: (s given, p_in, p_out, n wanted, y wanted, g_y given, parameter gradients wanted)
VARIANTS = {"plain": (True, 0.0, 0.0, True, True, True, True), "both_drops": (True, 0.25, 0.25, True, True, True, True),
            "no_s_no_gy": (False, 0.0, 0.25, True, True, False, False), "no_n": (True, 0.25, 0.0, False, True, True, False),
            "norm_only": (False, 0.0, 0.0, True, False, False, True)}


def rows_per_block(N):
    return 128 if N <= 64 else 32 if N <= 1024 else 16


def cases():
    """(R, N, variant): one row, and one row more than a workgroup's (second row block, the column sums' finish)."""
    return [(R, N, v) for N in WIDTHS for R in (1, rows_per_block(N) + 1) for v in VARIANTS]


def draws(seed, call, site, rows, cols):
    """uint32 r of every (row, col) of the given index arrays (broadcast)."""
    with np.errstate(over="ignore"):
        c = fmix32(np.uint32(seed & 0xFFFFFFFF) ^ np.uint32(0x9E3779B9))
        c = fmix32(c ^ np.uint32((seed >> 32) & 0xFFFFFFFF))
        c = fmix32(c ^ np.uint32(call & 0xFFFFFFFF))
        c = fmix32(c ^ np.uint32((call >> 32) & 0xFFFFFFFF))
        c2 = fmix32(c ^ np.uint32(0x52DCE729))
        w1 = fmix32(c2 ^ (np.uint32(site) * np.uint32(0x9E3779B1)))
        w2 = fmix32(w1 ^ (np.asarray(rows, np.uint32) * np.uint32(0x85EBCA6B)))
        return fmix32(w2 ^ (np.asarray(cols, np.uint32) * np.uint32(0xC2B2AE35)))


def keep(p, seed, call, site, R, N):
    """float64 [R, N]: 0 or float32(1 / (1 - p)); all ones for p == 0.  relu_dropout's flat array of n < 2^32 elements is
    the row 0 of (1, n)."""
    if p == 0:
        return np.ones((R, N))
    kept = draws(seed, call, site, np.arange(R)[:, None], np.arange(N)[None, :]) >= np.uint32(dropout_threshold(p))
    return kept * np.float64(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def inputs(R, N, variant):
    """float32 x, s, gamma, beta, g_y, g_n without zeros (|x|, |s| >= 0.25: a dropped s never rounds away in x + s), the
    last row constant where nothing is added or dropped; k_in, k_out the float64 keep multipliers."""
    has_s, p_in, p_out = VARIANTS[variant][:3]
    rng = np.random.default_rng([R, N, sorted(VARIANTS).index(variant)])
    away = lambda a: (np.sign(a) * (0.25 + np.abs(a))).astype(np.float32)  # noqa: E731
    x, s, g_y, g_n = (away(rng.standard_normal((R, N))) for _ in range(4))
    gamma, beta = away(rng.standard_normal(N)), away(rng.standard_normal(N))
    if variant == "norm_only" and R > 1:
        x[-1] = 1.5  # var = 0, rstd = 1 / sqrt(eps)
    k_in, k_out = keep(p_in if has_s else 0.0, SEED, CALL, SITE_IN, R, N), keep(p_out, SEED, CALL, SITE_OUT, R, N)
    return {"x": x, "s": s if has_s else None, "gamma": gamma, "beta": beta, "g_y": g_y, "g_n": g_n, "k_in": k_in, "k_out": k_out}


def run(c, variant):
    """The float64 restatement: {"y", "n", "mean", "rstd", "g_x", "g_s", "grad_gamma", "grad_beta"}, each where wanted."""
    has_s, _, _, want_n, want_y, has_gy, want_pg = VARIANTS[variant]
    x, gamma, beta = (c[k].astype(np.float64) for k in ("x", "gamma", "beta"))
    N = x.shape[1]
    y = (x + (c["s"].astype(np.float64) * c["k_in"] if has_s else 0.0)) * c["k_out"]
    out = {"y": y} if want_y else {}
    g = c["g_y"].astype(np.float64) if has_gy else np.zeros_like(y)
    if want_n:
        mean = y.sum(axis=1) / N
        rstd = 1.0 / np.sqrt(((y - mean[:, None]) ** 2).sum(axis=1) / N + EPS)
        xhat, g_n = (y - mean[:, None]) * rstd[:, None], c["g_n"].astype(np.float64)
        d = g_n * gamma
        g = g + rstd[:, None] * (d - d.mean(axis=1)[:, None] - xhat * (d * xhat).mean(axis=1)[:, None])
        out.update(n=xhat * gamma + beta, mean=mean, rstd=rstd)
        if want_pg:
            out.update(grad_gamma=(g_n * xhat).sum(axis=0), grad_beta=g_n.sum(axis=0))
    out["g_x"] = g * c["k_out"]
    if has_s:
        out["g_s"] = out["g_x"] * c["k_in"]
    return out


def torch_composition(c, variant, dtype):
    """The same outputs from F.layer_norm plus torch's adds and multiplies in `dtype`, given the same keep multipliers."""
    import torch

    has_s, _, _, want_n, want_y, has_gy, want_pg = VARIANTS[variant]
    t = {k: None if v is None else torch.from_numpy(v).to(dtype) for k, v in c.items()}
    leaves = {k: t[k].requires_grad_() for k in ("x", "s", "gamma", "beta") if t[k] is not None}
    y = (t["x"] + t["s"] * t["k_in"] if has_s else t["x"]) * t["k_out"]
    out, loss = ({"y": y} if want_y else {}), (y * t["g_y"]).sum() if has_gy else 0.0
    if want_n:
        n = torch.nn.functional.layer_norm(y, y.shape[-1:], t["gamma"], t["beta"], EPS)
        out.update(n=n, mean=y.mean(dim=1), rstd=1.0 / torch.sqrt(y.var(dim=1, unbiased=False) + EPS))
        loss = loss + (n * t["g_n"]).sum()
    loss.backward()
    out["g_x"] = leaves["x"].grad
    if has_s:
        out["g_s"] = leaves["s"].grad
    if want_pg:
        out.update(grad_gamma=leaves["gamma"].grad, grad_beta=leaves["beta"].grad)
    return {k: v.detach().double().numpy() for k, v in out.items()}


def errors(got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return {k: rel_err(got[k], ref[k]) for k in ref}


@functools.lru_cache(maxsize=None)
def tolerance():
    """8 x the worst float32 error of torch's composition against the float64 restatement over cases(); the factor covers
    another summation order and fused multiply-adds, as for the project's other row kernels."""
    import torch

    worst = 0.0
    for R, N, v in cases():
        c = inputs(R, N, v)
        worst = max(worst, *errors(torch_composition(c, v, torch.float32), run(c, v)).values())
    return 8.0 * worst
