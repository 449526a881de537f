"""Records tests/golden/deepfm.npz from the REFERENCE's own DeepFM code.  Data only.

    python tests/golden/make_deepfm_golden.py --reference /path/to/torchrec-checkout

Module cases: torchrec/modules/deepfm.py is loaded by path (nothing else of the checkout is imported), as
make_crossnet_golden.py does.  Model cases: the reference package is imported the way make_golden.py does (this
repository's fbgemm_gpu enums and the CPU op stand-ins of tests/_cpu_ops.py), and its SimpleDeepFMNN is run.

Keys:  mod|<case>|x<i>, |gfm, |gdeep, |param|<name>           inputs, the two output gradients, DeepFM's dense_module
       mod|<case>|<f32|f64>|fm, |deep, |gx_fm, |gx_deep, |gparam|<name>   gx_*: [rows, N], the input gradients side by side
       mod|<case>|rows                                         the rows gx_* holds (all of them but for `criteo`)
The full record of the `criteo` case (70 x 3456) would be 6.8 MB.  Its inputs are therefore drawn from a torch.Generator
seeded with mod|criteo|x_seed and not stored (mod|criteo|x_rowsum64 pins the draw), and its input gradients are stored for
GRAD_ROWS only; outputs and parameter gradients, which depend on every row, are stored whole.
       model|<case>|values, |lengths, |dense, |g, |sd|<name>    ids (KeyedJaggedTensor order), input, d logits, state_dict
       model|<case>|<f32|f64>|logits, |grad|<name>              every parameter gradient, embedding tables included
The archive is written with fixed member times, so a second run reproduces the file byte for byte."""
import argparse
import copy
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))

# (B, shapes after the batch dimension); the first is the docstring's example
MODULE_CASES = {
    "doc3d": (3, [(2, 64), (2, 32)]),
    "d3": (37, [(3,), (3,), (3,)]),
    "d8": (5, [(8,), (8,), (8,), (8,)]),
    "mixed": (33, [(5,), (260,), (12,)]),
    "w1": (64, [(64,), (1,), (67,)]),
    "criteo": (70, [(128,)] * 27),
}
DEEP_OUT = 4
CRITEO_SEED = 4242
GRAD_ROWS = (0, 69)  # of the criteo case


def criteo_inputs():
    """The inputs of the `criteo` case; tests/_deepfm_ref.py draws them the same way."""
    B, shapes = MODULE_CASES["criteo"]
    gen = torch.Generator().manual_seed(CRITEO_SEED)
    return [torch.randn(B, *s, generator=gen) for s in shapes]


# name -> (B, D, [(table, rows, features)], KeyedJaggedTensor key order, dense features, hidden, deep_fm_dimension, max bag)
MODEL_CASES = {
    "doc": (2, 8, [("t1", 100, ["f1", "f3"]), ("t2", 100, ["f2"])], ["f1", "f2", "f3"], 10, 20, 5, 2),
    "ragged": (5, 3, [("t1", 7, ["a"]), ("t2", 11, ["b"]), ("t3", 5, ["c"])], ["a", "b", "c"], 4, 6, 3, 3),
}


def load_reference_modules(root):
    path = os.path.join(root, "torchrec", "modules", "deepfm.py")
    spec = importlib.util.spec_from_file_location("reference_deepfm", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def import_reference_package(root):
    sys.path.insert(0, os.path.dirname(HERE))
    import _paths  # noqa: F401
    import _cpu_ops

    pe = types.ModuleType("pyre_extensions")
    pe.none_throws = lambda x, msg=None: x

    class _PS:
        def __init__(self, name):
            self.args = object
            self.kwargs = object

    pe.ParameterSpecification = _PS
    sys.modules["pyre_extensions"] = pe
    _cpu_ops.register()
    sys.path.insert(0, root)
    import torchrec  # noqa: F401


def run_modules(ref, xs, deep, gfm, gdeep, dtype):
    xs = [x.to(dtype) for x in xs]
    deep = copy.deepcopy(deep).to(dtype)
    out = {}
    leaves = [x.clone().requires_grad_() for x in xs]
    fm = ref.FactorizationMachine()(embeddings=leaves)
    fm.backward(gfm.to(dtype))
    out["fm"] = fm.detach()
    out["gx_fm"] = torch.cat([l.grad.flatten(1) for l in leaves], dim=1)
    leaves = [x.clone().requires_grad_() for x in xs]
    d = ref.DeepFM(dense_module=deep)(embeddings=leaves)
    d.backward(gdeep.to(dtype))
    out["deep"] = d.detach()
    out["gx_deep"] = torch.cat([l.grad.flatten(1) for l in leaves], dim=1)
    for n, p in deep.named_parameters():
        out["gparam|" + n] = p.grad
    return {k: v.numpy() for k, v in out.items()}


def module_cases(ref, rec):
    for case, (B, shapes) in MODULE_CASES.items():
        xs = criteo_inputs() if case == "criteo" else [torch.randn(B, *s) for s in shapes]
        rows = np.array(GRAD_ROWS if case == "criteo" else range(B), dtype=np.int64)
        N = sum(int(np.prod(s)) for s in shapes)
        deep = nn.Sequential(nn.Linear(N, DEEP_OUT), nn.ReLU())
        gfm, gdeep = torch.randn(B, 1), torch.randn(B, DEEP_OUT)
        pre = f"mod|{case}|"
        rec[pre + "rows"] = rows
        if case == "criteo":
            rec[pre + "x_seed"] = np.int64(CRITEO_SEED)
            rec[pre + "x_rowsum64"] = torch.cat(xs, dim=1).double().sum(1).numpy()
        else:
            for i, x in enumerate(xs):
                rec[pre + f"x{i}"] = x.numpy()
        rec[pre + "gfm"], rec[pre + "gdeep"] = gfm.numpy(), gdeep.numpy()
        for n, p in deep.named_parameters():
            rec[pre + "param|" + n] = p.detach().numpy().copy()
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            for k, v in run_modules(ref, xs, deep, gfm, gdeep, dtype).items():
                rec[pre + prec + "|" + k] = v[rows] if k.startswith("gx_") else v


def model_cases(rec):
    from torchrec.models.deepfm import SimpleDeepFMNN
    from torchrec.modules.embedding_configs import EmbeddingBagConfig
    from torchrec.modules.embedding_modules import EmbeddingBagCollection
    from torchrec.sparse.jagged_tensor import KeyedJaggedTensor

    for case, (B, D, tables, keys, n_dense, hidden, deep_dim, max_bag) in MODEL_CASES.items():
        rng = np.random.default_rng(len(case))
        ebc = EmbeddingBagCollection(tables=[
            EmbeddingBagConfig(name=t, embedding_dim=D, num_embeddings=r, feature_names=list(f)) for t, r, f in tables])
        model = SimpleDeepFMNN(num_dense_features=n_dense, embedding_bag_collection=ebc, hidden_layer_size=hidden,
                               deep_fm_dimension=deep_dim)
        rows = {f: r for _, r, fs in tables for f in fs}
        lengths = rng.integers(1 if case == "doc" else 0, max_bag + 1, size=len(keys) * B).astype(np.int32)
        if case == "ragged":
            lengths[1] = 0  # an empty bag
        values = np.concatenate([rng.integers(0, rows[k], size=int(lengths[i * B:(i + 1) * B].sum()))
                                 for i, k in enumerate(keys)]).astype(np.int64)
        dense = torch.from_numpy(rng.standard_normal((B, n_dense)).astype(np.float32))
        g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32))
        pre = f"model|{case}|"
        rec[pre + "values"], rec[pre + "lengths"], rec[pre + "dense"], rec[pre + "g"] = values, lengths, dense.numpy(), g.numpy()
        for n, v in model.state_dict().items():
            rec[pre + "sd|" + n] = v.numpy().copy()
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            m = copy.deepcopy(model).to(dtype)
            kjt = KeyedJaggedTensor.from_lengths_sync(keys=keys, values=torch.from_numpy(values),
                                                      lengths=torch.from_numpy(lengths))
            logits = m(dense_features=dense.to(dtype), sparse_features=kjt)
            logits.backward(g.to(dtype))
            rec[pre + prec + "|logits"] = logits.detach().numpy()
            for n, p in m.named_parameters():
                rec[pre + prec + "|grad|" + n] = p.grad.numpy()


def write_npz(path, rec):
    """np.load-compatible archive with fixed member times (np.savez stamps the clock into every member)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in rec.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds torchrec/)")
    ap.add_argument("--out", default=os.path.join(HERE, "deepfm.npz"))
    args = ap.parse_args()
    torch.manual_seed(20240911)
    torch.set_num_threads(1)
    rec = {}
    module_cases(load_reference_modules(args.reference), rec)
    import_reference_package(args.reference)
    model_cases(rec)
    write_npz(args.out, rec)
    print(f"{args.out}: {len(rec)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
