"""Access to tests/golden/bert4rec.npz (written by tests/golden/make_bert4rec_golden.py from the reference's own code)."""
import functools
import os

import numpy as np
import torch

import _paths

DRAW_SEED = 4242  # make_bert4rec_golden.py DRAW_SEED


@functools.lru_cache(maxsize=None)
def load():
    z = np.load(os.path.join(_paths.ROOT, "tests", "golden", "bert4rec.npz"))
    return {k: z[k] for k in z.files}


def cases(kind):
    return sorted({k.split("|")[1] for k in load() if k.startswith(kind + "|")})


def mha_inputs(case):
    """(xq, xk, xv, g float32 arrays [B, L, dim], rows): stored, or for the larger cases drawn as the recorder drew them;
    `rows` are the sequence positions the recorded out / gx* hold."""
    z, pre = load(), f"mha|{case}|"
    if pre + "xq" in z:
        xs = [z[pre + n] for n in ("xq", "xk", "xv", "g")]
        return (*xs, np.arange(xs[0].shape[1]))
    B, L = z[pre + "valid"].shape
    dim = z[pre + "param|output_linear.bias"].shape[0]
    assert int(z[pre + "x_seed"].ravel()[0]) == DRAW_SEED + L
    gen = torch.Generator().manual_seed(DRAW_SEED + L)
    xs = [torch.randn(B, L, dim, generator=gen) for _ in range(4)]
    assert abs(sum(float(t.double().sum()) for t in xs) - float(z[pre + "x_sum64"].ravel()[0])) < 1e-9, "the draw moved"
    return (*[t.numpy() for t in xs], z[pre + "rows"])


def stored_grad(g):
    """The rows of a parameter gradient the archive keeps (make_bert4rec_golden.py stored_grad)."""
    if g.ndim == 2 and g.size >= 1024:
        n = g.shape[0]
        return g[sorted({0, 1, n // 2, n - 1})]
    return g


def params(kind, case):
    z, pre = load(), f"{kind}|{case}|param|"
    return {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}


def mask_of(valid, how, device="cpu"):
    """[B, 1, L, L] key-padding mask from bool [B, L]: "expand" (stride 0 along the queries, as this package's BERT4Rec
    builds it) or "repeat" (materialised, as the reference builds it)."""
    v = torch.from_numpy(valid).to(device)
    B, L = v.shape
    if how == "expand":
        return v[:, None, None, :].expand(B, 1, L, L)
    return v.unsqueeze(1).repeat(1, L, 1).unsqueeze(1)
