"""Records tests/golden/swish_layernorm.npz from the REFERENCE's own SwishLayerNorm (torchrec/modules/activation.py) and its
MLP(activation="swish_layernorm") (torchrec/modules/mlp.py, utils.py), plain torch, loaded by path under stub `torchrec` /
`torchrec.modules` entries of sys.modules — nothing else of the checkout is imported.  Data only: parameters, input, output
gradient, the float32 results and the results of the module's .double() copy.

    python tests/golden/make_swish_layernorm_golden.py --reference /path/to/torchrec-checkout

Keys:  sln|<case>|x, |g, |param|<name>                                   input, output gradient, gamma / beta (non-zero)
       sln|<case>|f32|out, |f32|grad_input, |f32|grad|<name>              and the same with f64
       mlp|x, |g, |param|<name>, |f32|out, |f32|grad_input, |f32|grad|<name>   and the same with f64
"""
import argparse
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

# case -> (leading dims, input_dims); 3x100 is the docstring's width, 9x10 the fall-back width
CASES = {"3x100": ((3,), [100]), "37x20": ((37,), [20]), "70x64": ((70,), [64]), "5x3x4x8": ((5, 3), [4, 8]),
         "9x10": ((9,), [10])}
MLP_ARGS = (40, [16, 8, 4])
MLP_BATCH = 3


def load_reference(root):
    """(activation module, mlp module) of the checkout, loaded by path."""
    for name in ("torchrec", "torchrec.modules"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    mods = {}
    for leaf in ("activation", "utils", "mlp"):
        name = "torchrec.modules." + leaf
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "torchrec", "modules", leaf + ".py"))
        mods[leaf] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[leaf]
        spec.loader.exec_module(mods[leaf])
    return mods["activation"], mods["mlp"]


def randomise_norms(m):
    """gamma about 1, beta about 0, every element non-zero (LayerNorm's own init is ones / zeros)."""
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "norm.0." in name:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.5 * torch.randn_like(p))
            assert bool((p != 0).all()), name


def run(m, x, g):
    m.zero_grad()
    xi = x.clone().requires_grad_()
    out = m(xi)
    out.backward(g)
    return out.detach(), xi.grad.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def record(rec, pre, m, x, g):
    rec[pre + "x"], rec[pre + "g"] = x.numpy(), g.numpy()
    for n, p in m.named_parameters():
        rec[pre + "param|" + n] = p.detach().numpy().copy()
    m64 = copy.deepcopy(m).double()
    for prec, (o, gi, gr) in (("f32", run(m, x, g)), ("f64", run(m64, x.double(), g.double()))):
        rec[pre + prec + "|out"], rec[pre + prec + "|grad_input"] = o.numpy(), gi.numpy()
        for n, t in gr.items():
            rec[pre + prec + "|grad|" + n] = t.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds torchrec/modules/)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "swish_layernorm.npz"))
    args = ap.parse_args()
    act, mlp = load_reference(args.reference)
    torch.manual_seed(20240611)
    torch.set_num_threads(1)
    rec = {}
    for case, (lead, dims) in CASES.items():
        m = act.SwishLayerNorm(dims[0] if len(dims) == 1 else dims)
        randomise_norms(m)
        shape = tuple(lead) + tuple(dims)
        x = 0.5 + 2.0 * torch.randn(shape)  # mean about 0.5, std about 2: the mean subtraction is exercised
        record(rec, f"sln|{case}|", m, x, torch.randn(shape))
    m = mlp.MLP(*MLP_ARGS, activation="swish_layernorm")
    randomise_norms(m)
    record(rec, "mlp|", m, 0.5 + 2.0 * torch.randn(MLP_BATCH, MLP_ARGS[0]), torch.randn(MLP_BATCH, MLP_ARGS[1][-1]))
    np.savez_compressed(args.out, **rec)
    print(f"{args.out}: {len(rec)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
