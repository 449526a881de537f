"""Records tests/golden/crossnet.npz from the REFERENCE's own cross networks (torchrec/modules/crossnet.py, plain torch,
loaded by path — nothing else of the checkout is imported).  Data only: parameters, input, output gradient, the float32
results and the results of the module's .double() copy.

    python tests/golden/make_crossnet_golden.py --reference /path/to/torchrec-checkout

Keys:  case|<case>|x, case|<case>|g                       input and output gradient (shared by the three classes)
       <Class>|<case>|param|<name>                         parameters (biases and kernels non-zero)
       <Class>|<case>|y                                    float32 per-layer GEMM result [L, B, N] / row dots [L, B]
       <Class>|<case>|f32|out, |f32|grad_input, |f32|grad|<name>   and the same with f64
"""
import argparse
import copy
import importlib.util
import os

import numpy as np
import torch

CASES = {"3x10": (3, 10, 2, 3), "37x20": (37, 20, 3, 5), "70x64": (70, 64, 2, 1)}  # (B, N, L, r); 3x10 is the docstring's
KINDS = ("CrossNet", "LowRankCrossNet", "VectorCrossNet")


def load_reference(root):
    path = os.path.join(root, "torchrec", "modules", "crossnet.py")
    spec = importlib.util.spec_from_file_location("reference_crossnet", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(ref, kind, N, L, r):
    if kind == "LowRankCrossNet":
        m = ref.LowRankCrossNet(N, L, low_rank=r)
    else:
        m = getattr(ref, kind)(N, L)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("bias"):
                p.copy_(torch.randn_like(p) * 0.1)
            assert bool((p != 0).all()), name
    return m


def run(m, x, g):
    m.zero_grad()
    xi = x.clone().requires_grad_()
    out = m(xi)
    out.backward(g)
    return out.detach(), xi.grad.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def per_layer_y(m, kind, x):
    """The per-layer GEMM result (row dots for VectorCrossNet) of the float32 forward, with the output it leads to."""
    sd = dict(m.named_parameters())
    L = m._num_layers
    x0 = x.unsqueeze(2)
    x_l, ys = x0, []
    with torch.no_grad():
        for l in range(L):
            b = sd[f"bias.{l}"]
            if kind == "VectorCrossNet":
                y = torch.tensordot(x_l, sd[f"kernels.{l}"], dims=([1], [0]))
                x_l = torch.matmul(x0, y) + b + x_l
                ys.append(y.reshape(-1))
            else:
                if kind == "CrossNet":
                    y = torch.matmul(sd[f"kernels.{l}"], x_l)
                else:
                    y = torch.matmul(sd[f"W_kernels.{l}"], torch.matmul(sd[f"V_kernels.{l}"], x_l))
                x_l = x0 * (y + b) + x_l
                ys.append(y.squeeze(2))
    return torch.stack(ys), x_l.squeeze(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds torchrec/modules/crossnet.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "crossnet.npz"))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.manual_seed(20240607)
    torch.set_num_threads(1)
    rec = {}
    for case, (B, N, L, r) in CASES.items():
        x, g = torch.randn(B, N), torch.randn(B, N)
        rec[f"case|{case}|x"], rec[f"case|{case}|g"] = x.numpy(), g.numpy()
        for kind in KINDS:
            m = build(ref, kind, N, L, r)
            pre = f"{kind}|{case}|"
            for n, p in m.named_parameters():
                rec[pre + "param|" + n] = p.detach().numpy().copy()
            out, gx, grads = run(m, x, g)
            ys, out_again = per_layer_y(m, kind, x)
            assert torch.equal(out, out_again), (kind, case)
            rec[pre + "y"] = ys.numpy()
            m64 = copy.deepcopy(m).double()
            out64, gx64, grads64 = run(m64, x.double(), g.double())
            for prec, (o, gi, gr) in (("f32", (out, gx, grads)), ("f64", (out64, gx64, grads64))):
                rec[pre + prec + "|out"], rec[pre + prec + "|grad_input"] = o.numpy(), gi.numpy()
                for n, t in gr.items():
                    rec[pre + prec + "|grad|" + n] = t.numpy()
    np.savez_compressed(args.out, **rec)
    print(f"{args.out}: {len(rec)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
