"""Host model of the fused masked attention (csrc/attention.hip, include/tbe_hip.h): forward and backward in numpy, the
numpy restatement of the kernel's dropout draw, and the inputs, mask patterns and tolerance the attention tests share.

Layout: q, k, v, dout, out, dq, dk, dv are [B, L, H, d] here (the kernel's logical layout); key_valid is bool [B, L] or None;
`keep` is None or the [B, H, L, L] array the probabilities are multiplied with (0, or 1 / (1 - p))."""
import functools

import numpy as np

# (B, H, L, d, input scale): the edges of the kernel — one key, fewer keys than a wave, one past a 64-wide tile, two and
# four keys per lane, the LDS limit (appended by the GPU test from the support rule).  `hot` has scores far above 100.
SHAPES = [(1, 1, 1, 4), (2, 3, 3, 4), (3, 2, 7, 8), (2, 2, 33, 32), (2, 1, 64, 64), (2, 2, 65, 64), (1, 2, 100, 128),
          (1, 1, 200, 64)]
HOT = (2, 2, 33, 32)
PATTERNS = ("none", "all", "empty", "first", "last", "hole", "per_sample")
DROPOUT = ((0.1, 20240917, 3), (0.5, 7, 0))  # (p, seed, call) the GPU test uses; the keep rates are checked on the CPU


def max_L(supported, d):
    """The largest L the support rule admits for d."""
    return max(L for L in range(1, 4097) if supported(L, d))


def make_inputs(B, H, L, d, scale=1.0, seed=0):
    """float32 q, k, v, dout [B, L, H, d]."""
    rng = np.random.default_rng(1000 * L + d + seed)
    q, k, v, g = (rng.standard_normal((B, L, H, d)).astype(np.float32) for _ in range(4))
    return q * np.float32(scale), k * np.float32(scale), v, g


def key_valid(pattern, B, L):
    """bool [B, L] or None.  `per_sample`: sample b takes the (b mod 5)-th of empty, all, last, first, hole."""
    if pattern == "none":
        return None
    one = {"all": np.ones(L, bool), "empty": np.zeros(L, bool), "first": np.arange(L) == 0, "last": np.arange(L) == L - 1,
           "hole": ~((np.arange(L) >= L // 3) & (np.arange(L) <= L // 2))}
    if pattern == "per_sample":
        order = ("empty", "all", "last", "first", "hole")
        return np.stack([one[order[b % 5]] for b in range(B)])
    return np.broadcast_to(one[pattern], (B, L)).copy()


# ---- the dropout draw (include/tbe_hip.h), uint32 arithmetic

def fmix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def dropout_draws(seed, call, B, H, L):
    """uint32 [B, H, L, L]: r of every element."""
    with np.errstate(over="ignore"):
        c = fmix32(np.uint32(seed & 0xFFFFFFFF) ^ np.uint32(0x9E3779B9))
        c = fmix32(c ^ np.uint32((seed >> 32) & 0xFFFFFFFF))
        c = fmix32(c ^ np.uint32(call & 0xFFFFFFFF))
        c = fmix32(c ^ np.uint32((call >> 32) & 0xFFFFFFFF))
        bh = np.arange(B * H, dtype=np.uint32).reshape(B, H, 1, 1)
        i = np.arange(L, dtype=np.uint32).reshape(1, 1, L, 1)
        j = np.arange(L, dtype=np.uint32).reshape(1, 1, 1, L)
        w1 = fmix32(c ^ (bh * np.uint32(0x9E3779B1)))
        w2 = fmix32(w1 ^ (i * np.uint32(0x85EBCA6B)))
        return fmix32(w2 ^ (j * np.uint32(0xC2B2AE35)))


def dropout_threshold(p):
    return min(2 ** 32 - 1, int(np.floor(float(np.float32(p)) * 2.0 ** 32)))


def dropout_keep(p, seed, call, B, H, L):
    """The multiplier [B, H, L, L] of the probabilities: 0 or float32(1 / (1 - p)); None for p == 0."""
    if p == 0:
        return None
    kept = dropout_draws(seed, call, B, H, L) >= np.uint32(dropout_threshold(p))
    return kept * np.float64(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ---- the model

def forward(q, k, v, valid=None, keep=None, dtype=np.float64, masked_value=-1e9, subtract_max=True):
    """(out [B, L, H, d], lse [B, H, L], P [B, H, L, L]).  masked_value / subtract_max exist for the fault checks."""
    q, k, v = (np.asarray(a, dtype=dtype) for a in (q, k, v))
    d = q.shape[-1]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = np.einsum("bihc,bjhc->bhij", q, k) / dtype(np.sqrt(dtype(d)))
        if valid is not None:
            s = np.where(valid[:, None, None, :], s, dtype(masked_value))
        m = s.max(axis=-1, keepdims=True) if subtract_max else np.zeros_like(s[..., :1])
        e = np.exp(s - m)
        tot = e.sum(axis=-1, keepdims=True)
        P = e / tot
        lse = (m + np.log(tot))[..., 0]
        Pd = P if keep is None else P * keep.astype(dtype)
        out = np.einsum("bhij,bjhc->bihc", Pd, v)
    return out, lse, P


def backward(dout, q, k, v, valid=None, keep=None, dtype=np.float64, cut_masked=True):
    """(dq, dk, dv) [B, L, H, d].  cut_masked=False lets dS through at masked keys (a fault check)."""
    dout, q, k, v = (np.asarray(a, dtype=dtype) for a in (dout, q, k, v))
    d = q.shape[-1]
    _, _, P = forward(q, k, v, valid, None, dtype)
    keepm = np.ones_like(P) if keep is None else keep.astype(dtype)
    Pd = P * keepm
    dv = np.einsum("bhij,bihc->bjhc", Pd, dout)
    dP = np.einsum("bihc,bjhc->bhij", dout, v) * keepm
    D = (P * dP).sum(axis=-1, keepdims=True)
    dS = P * (dP - D) / dtype(np.sqrt(dtype(d)))
    if valid is not None and cut_masked:
        dS = np.where(valid[:, None, None, :], dS, 0)
    dq = np.einsum("bhij,bjhc->bihc", dS, k)
    dk = np.einsum("bhij,bihc->bjhc", dS, q)
    return dq, dk, dv


# ---- the torch composition and the tolerance measured from it

def torch_composition(dout, q, k, v, valid, keep, dtype):
    """out, dq, dk, dv [B, L, H, d] of the product's `_attention_torch` (the reference's operations in the reference's
    order, the dropout replaced by the given multiplier) in torch `dtype` on the CPU."""
    import torch

    import _paths  # noqa: F401
    from torchrec_amd.models.bert4rec import _attention_torch

    B, L, H, d = q.shape
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dtype).reshape(B, L, H * d).requires_grad_() for a in (q, k, v)]
    mask = None if valid is None else torch.from_numpy(valid)[:, None, None, :].expand(B, 1, L, L)
    mult = None if keep is None else torch.from_numpy(keep).to(dtype)
    out = _attention_torch(*ts, mask, H, None if mult is None else (lambda p: p * mult))
    out.backward(torch.from_numpy(np.ascontiguousarray(dout)).to(dtype).reshape(B, L, H * d))
    return [t.detach().double().numpy().reshape(B, L, H, d) for t in (out, ts[0].grad, ts[1].grad, ts[2].grad)]


def abi_cases(extra_shapes=()):
    """Every (shape, scale, pattern, dropout) the GPU ABI test runs: all shapes with all patterns at p = 0, the hot case,
    and the dropout settings on two shapes."""
    cases = [(s, 1.0, pat, None) for s in list(SHAPES) + list(extra_shapes) for pat in PATTERNS]
    cases += [(HOT, 6.0, pat, None) for pat in ("none", "per_sample")]
    cases += [(s, 1.0, pat, dr) for s in ((3, 2, 7, 8), (2, 2, 65, 64)) for pat in ("none", "per_sample") for dr in DROPOUT]
    return cases


def scale_of(a):
    return max(float(np.abs(a).max()), 1e-30)


@functools.lru_cache(maxsize=None)
def measured_tolerance(extra_shapes=()):
    """8 x the worst |float32 - float64| of the torch composition over abi_cases(), relative to each output's scale
    (max |float64 output|).  The factor covers the kernel's other summation order and its recomputed P.  Nothing of the
    kernel enters."""
    import torch

    worst = 0.0
    for (B, H, L, d), scale, pat, dr in abi_cases(extra_shapes):
        q, k, v, g = make_inputs(B, H, L, d, scale)
        valid = key_valid(pat, B, L)
        keep = None if dr is None else dropout_keep(dr[0], dr[1], dr[2], B, H, L)
        lo = torch_composition(g, q, k, v, valid, keep, torch.float32)
        hi = torch_composition(g, q, k, v, valid, keep, torch.float64)
        for a, b in zip(lo, hi):
            worst = max(worst, float(np.abs(a - b).max()) / scale_of(b))
    return 8.0 * worst


def assert_close(got, want, tol, what, scale=None):
    """|got - want| <= tol * scale everywhere (NaN fails); scale: max|want| unless given."""
    err = float(np.abs(np.asarray(got, np.float64) - want).max()) / (scale_of(want) if scale is None else scale)
    assert err <= tol, f"{what}: error {err:.3e} of the output's scale, tolerance {tol:.3e}"
    return err
