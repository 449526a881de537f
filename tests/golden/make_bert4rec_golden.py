"""Records tests/golden/bert4rec.npz from the REFERENCE's own BERT4Rec code (examples/bert4rec/models/bert4rec.py) and its
JaggedTensor.to_padded_dense (torchrec/sparse/jagged_tensor.py).  Data only.

    python tests/golden/make_bert4rec_golden.py --reference /path/to/torchrec-checkout

The reference package is imported the way make_deepfm_golden.py does (this repository's fbgemm_gpu enums and the CPU op
stand-ins of tests/_cpu_ops.py), then examples.bert4rec.models.bert4rec.

Keys:  tpd|<case>|values, |lengths                                     one jagged tensor per values dtype (i64, f32)
       tpd|<case>|<pad_from_beginning><chop_from_beginning>            the reference's result for the four flag pairs (0 / 1)
       mha|<case>|xq, |xk, |xv, |valid, |g, |param|<name>              inputs, key validity [B, L], output gradient
       mha|<case>|<f32|f64>|out, |gxq, |gxk, |gxv, |grad|<name>
The full record of the two larger mha cases would be 1.5 MB.  Their inputs are therefore drawn from a torch.Generator seeded
with mha|<case>|x_seed and not stored (mha|<case>|x_sum64 pins the draw; tests/_bert4rec_golden.py draws them the same way),
and out / gx* are stored for the sequence positions mha|<case>|rows only.  Everywhere, the gradient of a weight matrix of
1024 or more elements is stored for its rows 0, 1, n // 2, n - 1 only (stored_grad below; every such row depends on every
input row).
       block|<case>|x, |valid, |g, |param|<name>, |<f32|f64>|out, |gx, |grad|<name>       TransformerBlock in .eval()
       model|<case>|values, |lengths, |g, |names, |sd|<name>           ids, d logits, state_dict keys in order, state_dict
       model|<case>|config, |dropout                                   vocab_size, max_len, emb_dim, nhead, num_layers, training
       model|<case>|<f32|f64>|logits, |grad|<name>                      gradients of every parameter above the lookup
The stand-in jagged_2d_to_dense of tests/_cpu_ops.py does not differentiate, so the item table has no recorded gradient;
its training is pinned by tests/test_bert4rec_gpu.py.  Masks are key-padding masks [B, 1, L, L] built from `valid` with
.repeat, as BERT4Rec.forward builds them.  The archive is written with fixed member times (make_deepfm_golden.write_npz)."""
import argparse
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_deepfm_golden import import_reference_package, write_npz  # noqa: E402

TPD_N = 4
TPD_LENGTHS = [0, 2, 4, 7, 1, 5, 4]  # 0, < N, == N, > N
TPD_PADDING = 10.5
# (B, L, dim_model, num_heads); sample b of a case takes the (b mod 5)-th of VALID_ORDER
MHA_CASES = {"3x3x16h4": (3, 3, 16, 4), "5x7x32h2": (5, 7, 32, 2), "4x33x64h2": (4, 33, 64, 2), "2x100x64h1": (2, 100, 64, 1)}
VALID_ORDER = ("empty", "last", "all", "hole", "first")
# (B, L, hidden, heads, feed_forward_hidden)
BLOCK_CASES = {"3x5x16h2": (3, 5, 16, 2, 64), "2x33x32h4": (2, 33, 32, 4, 128)}
# vocab_size, max_len, emb_dim, nhead, num_layers, dropout, training, lengths (ids are drawn; see model_cases)
MODEL_CASES = {
    "doc": (6, 3, 4, 4, 4, 0.1, False, None),  # the docstring's example: ids [2, 4 | 3, 4, 5]; d_k = 1
    "train": (20, 8, 16, 2, 2, 0.0, True, [0, 8, 3, 5, 2]),
    "eval": (20, 8, 16, 4, 2, 0.1, False, [0, 8, 3, 5, 2]),
}


BIG = 4000  # elements of an mha input above which it is drawn, not stored
DRAW_SEED = 4242


def drawn_inputs(B, L, dim):
    """xq, xk, xv, g of a larger mha case; tests/_bert4rec_golden.py draws them the same way."""
    gen = torch.Generator().manual_seed(DRAW_SEED + L)
    return [torch.randn(B, L, dim, generator=gen) for _ in range(4)]


def stored_grad(g):
    """What the archive keeps of a parameter gradient; tests/_bert4rec_golden.py cuts the same rows."""
    if g.ndim == 2 and g.size >= 1024:
        n = g.shape[0]
        return g[sorted({0, 1, n // 2, n - 1})]
    return g


def valid_rows(B, L):
    one = {"all": np.ones(L, bool), "empty": np.zeros(L, bool), "first": np.arange(L) == 0, "last": np.arange(L) == L - 1,
           "hole": ~((np.arange(L) >= L // 3) & (np.arange(L) <= L // 2))}
    return np.stack([one[VALID_ORDER[b % 5]] for b in range(B)])


def reference_mask(valid):
    """[B, 1, L, L] as examples/bert4rec/models/bert4rec.py:488-493 builds it."""
    v = torch.from_numpy(valid)
    return v.unsqueeze(1).repeat(1, v.size(1), 1).unsqueeze(1)


def randomise(m):
    """LayerNorm's own init is ones / zeros, Linear biases are small: make every parameter count."""
    with torch.no_grad():
        for name, p in m.named_parameters():
            if ".norm." in name or "layernorm" in name:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.3 * torch.randn_like(p))
            elif name.endswith("bias"):
                p.copy_(0.3 * torch.randn_like(p))


def tpd_cases(rec):
    from torchrec.sparse.jagged_tensor import JaggedTensor

    rng = np.random.default_rng(5)
    total = sum(TPD_LENGTHS)
    for case, values in (("i64", rng.integers(1, 1000, size=total).astype(np.int64)),
                         ("f32", rng.standard_normal(total).astype(np.float32))):
        pre = f"tpd|{case}|"
        rec[pre + "values"], rec[pre + "lengths"] = values, np.asarray(TPD_LENGTHS, np.int32)
        for pad in (0, 1):
            for chop in (0, 1):
                jt = JaggedTensor(values=torch.from_numpy(values), lengths=torch.tensor(TPD_LENGTHS, dtype=torch.int32))
                out = jt.to_padded_dense(desired_length=TPD_N, padding_value=TPD_PADDING, pad_from_beginning=bool(pad),
                                         chop_from_beginning=bool(chop))
                rec[pre + f"{pad}{chop}"] = out.numpy()


def mha_cases(ref, rec):
    for case, (B, L, dim, H) in MHA_CASES.items():
        m = ref.MultiHeadedAttention(num_heads=H, dim_model=dim, dropout=0.0)
        randomise(m)
        pre = f"mha|{case}|"
        valid = valid_rows(B, L)
        rec[pre + "valid"] = valid
        if B * L * dim > BIG:
            *xs, g = drawn_inputs(B, L, dim)
            rows = np.asarray(sorted({0, 1, L // 2, L - 1}))
            rec[pre + "x_seed"], rec[pre + "rows"] = np.int64(DRAW_SEED + L), rows
            rec[pre + "x_sum64"] = np.float64(sum(float(t.double().sum()) for t in (*xs, g)))
        else:
            xs = [torch.randn(B, L, dim) for _ in range(3)]
            g = torch.randn(B, L, dim)
            rows = np.arange(L)
            for n, x in zip(("xq", "xk", "xv"), xs):
                rec[pre + n] = x.numpy()
            rec[pre + "g"] = g.numpy()
        for n, p in m.named_parameters():
            rec[pre + "param|" + n] = p.detach().numpy().copy()
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            mm = copy.deepcopy(m).to(dtype)
            leaves = [x.detach().clone().to(dtype).requires_grad_() for x in xs]
            out = mm(*leaves, mask=reference_mask(valid))
            out.backward(g.to(dtype))
            rec[pre + prec + "|out"] = out.detach().numpy()[:, rows]
            for n, x in zip(("gxq", "gxk", "gxv"), leaves):
                rec[pre + prec + "|" + n] = x.grad.numpy()[:, rows]
            for n, p in mm.named_parameters():
                rec[pre + prec + "|grad|" + n] = stored_grad(p.grad.numpy())


def block_cases(ref, rec):
    for case, (B, L, hidden, heads, ff) in BLOCK_CASES.items():
        m = ref.TransformerBlock(hidden, heads, ff, 0.1).eval()
        randomise(m)
        x, g = torch.randn(B, L, hidden), torch.randn(B, L, hidden)
        valid = valid_rows(B, L)
        pre = f"block|{case}|"
        rec[pre + "x"], rec[pre + "valid"], rec[pre + "g"] = x.numpy(), valid, g.numpy()
        for n, p in m.named_parameters():
            rec[pre + "param|" + n] = p.detach().numpy().copy()
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            mm = copy.deepcopy(m).to(dtype)
            leaf = x.detach().clone().to(dtype).requires_grad_()
            out = mm(leaf, reference_mask(valid))
            out.backward(g.to(dtype))
            rec[pre + prec + "|out"], rec[pre + prec + "|gx"] = out.detach().numpy(), leaf.grad.numpy()
            for n, p in mm.named_parameters():
                rec[pre + prec + "|grad|" + n] = stored_grad(p.grad.numpy())


def model_cases(ref, rec):
    from torchrec.sparse.jagged_tensor import KeyedJaggedTensor

    for case, (vocab, max_len, emb, nhead, layers, dropout, training, lengths) in MODEL_CASES.items():
        rng = np.random.default_rng(len(case))
        if lengths is None:
            values, lengths = np.asarray([2, 4, 3, 4, 5], np.int64), [2, 3]
        else:
            values = rng.integers(1, vocab, size=sum(lengths)).astype(np.int64)
            values[lengths[0] + lengths[1] + 1] = 0  # an id 0 inside the third history: a masked key between valid ones
        model = ref.BERT4Rec(vocab_size=vocab, max_len=max_len, emb_dim=emb, nhead=nhead, num_layers=layers, dropout=dropout)
        randomise(model)
        model.train(training)
        B = len(lengths)
        g = torch.from_numpy(rng.standard_normal((B, max_len, vocab)).astype(np.float32))
        pre = f"model|{case}|"
        rec[pre + "values"], rec[pre + "lengths"], rec[pre + "g"] = values, np.asarray(lengths, np.int32), g.numpy()
        rec[pre + "config"] = np.asarray([vocab, max_len, emb, nhead, layers, int(training)], np.int64)
        rec[pre + "dropout"] = np.float64(dropout)
        rec[pre + "names"] = np.asarray(list(model.state_dict().keys()))
        for n, v in model.state_dict().items():
            rec[pre + "sd|" + n] = v.numpy().copy()
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            m = copy.deepcopy(model).to(dtype)
            for n, p in m.named_parameters():
                if ".ec." in n:  # the lookup: the stand-in jagged_2d_to_dense has no backward
                    p.requires_grad_(False)
            kjt = KeyedJaggedTensor.from_lengths_sync(keys=["item"], values=torch.from_numpy(values),
                                                      lengths=torch.tensor(lengths, dtype=torch.int32))
            logits = m(kjt)
            logits.backward(g.to(dtype))
            rec[pre + prec + "|logits"] = logits.detach().numpy()
            for n, p in m.named_parameters():
                if p.grad is not None:
                    rec[pre + prec + "|grad|" + n] = stored_grad(p.grad.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds torchrec/ and examples/)")
    ap.add_argument("--out", default=os.path.join(HERE, "bert4rec.npz"))
    args = ap.parse_args()
    torch.manual_seed(20241020)
    torch.set_num_threads(1)
    import_reference_package(args.reference)
    import examples.bert4rec.models.bert4rec as ref

    rec = {}
    tpd_cases(rec)
    mha_cases(ref, rec)
    block_cases(ref, rec)
    model_cases(ref, rec)
    write_npz(args.out, rec)
    print(f"{args.out}: {len(rec)} arrays, {os.path.getsize(args.out)} bytes, largest "
          f"{max(a.nbytes for a in rec.values())} bytes")


if __name__ == "__main__":
    main()
