"""Records tests/golden/mixture_crossnet.npz from the REFERENCE's own LowRankMixtureCrossNet (torchrec/modules/crossnet.py
:271-446, plain torch, loaded by path — nothing else of the checkout is imported).  Data only: parameters, input, output
gradient, the float32 results, the results of the module's .double() copy and the float32 softmax weights of every layer.

    python tests/golden/make_mixture_crossnet_golden.py --reference /path/to/torchrec-checkout

Keys:  <case>|x, <case>|g                                   input and output gradient
       <case>|param|<name>                                  parameters (biases and kernels non-zero)
       <case>|p                                             float32 per-layer softmax weights [L, B, K] (ones for K = 1)
       <case>|f32|out, |f32|grad_input, |f32|grad|<name>    and the same with f64
"""
import argparse
import copy
import importlib.util
import os

import numpy as np
import torch

# (B, N, L, K, r); 3x10 is the docstring's (N % 4 != 0: the fall-back), 37x20 has no gates
CASES = {"3x10": (3, 10, 2, 5, 3), "37x20": (37, 20, 3, 1, 4), "70x64": (70, 64, 2, 4, 8)}


def load_reference(root):
    path = os.path.join(root, "torchrec", "modules", "crossnet.py")
    spec = importlib.util.spec_from_file_location("reference_crossnet", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(ref, N, L, K, r):
    m = ref.LowRankMixtureCrossNet(N, L, num_experts=K, low_rank=r)
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


def per_layer_softmax(m, x):
    """The softmax weights [L, B, K] of the float32 forward, with the output they lead to (the reference's own operations)."""
    L, K = m._num_layers, m._num_experts
    x0 = x.unsqueeze(2)
    x_l, ps = x0, []
    with torch.no_grad():
        for l in range(L):
            experts = []
            for i in range(K):
                e = torch.matmul(m.V_kernels[l][i], x_l)
                e = torch.matmul(m.C_kernels[l][i], m._activation(e))
                e = torch.matmul(m.U_kernels[l][i], m._activation(e))
                experts.append((x0 * (e + m.bias[l])).squeeze(2))
            experts = torch.stack(experts, 2)
            if K > 1:
                gating = torch.stack([m.gates[i](x_l.squeeze(2)) for i in range(K)], 1)
                p = torch.nn.functional.softmax(gating, 1)
                x_l = torch.matmul(experts, p) + x_l
                ps.append(p.squeeze(2))
            else:
                x_l = experts + x_l
                ps.append(torch.ones(x.shape[0], 1))
    return torch.stack(ps), x_l.squeeze(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds torchrec/modules/crossnet.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "mixture_crossnet.npz"))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.manual_seed(20240611)
    torch.set_num_threads(1)
    rec = {}
    for case, (B, N, L, K, r) in CASES.items():
        x, g = torch.randn(B, N), torch.randn(B, N)
        pre = case + "|"
        rec[pre + "x"], rec[pre + "g"] = x.numpy(), g.numpy()
        m = build(ref, N, L, K, r)
        for n, p in m.named_parameters():
            rec[pre + "param|" + n] = p.detach().numpy().copy()
        out, gx, grads = run(m, x, g)
        ps, out_again = per_layer_softmax(m, x)
        assert torch.equal(out, out_again), case
        rec[pre + "p"] = ps.numpy()
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
