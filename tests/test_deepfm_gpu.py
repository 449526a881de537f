"""GPU: the DeepFM modules and SimpleDeepFMNN (torchrec_amd/modules/deepfm.py, torchrec_amd/models/deepfm.py) over
csrc/deepfm.hip against the reference's float64 runs (tests/golden/deepfm.npz).  The FM term and its input gradients are
held to the tolerance measured in tests/test_deepfm.py (8 x the reference's own float32 error); whatever passes through a
GEMM to the tolerance tests/test_dlrm_e2e_gpu.py uses."""
import numpy as np
import pytest
import torch
from torch import nn

import _paths  # noqa: F401
import _deepfm_ref as dr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _close(got, want, err_msg=""):
    np.testing.assert_allclose(got.detach().cpu().numpy() if torch.is_tensor(got) else got, want, err_msg=err_msg, **dr.GEMM_TOL)


@pytest.mark.parametrize("case", list(dr.MODULE_CASES))
def test_modules_reproduce_the_float64_fixtures(case):
    """doc3d: 3-D inputs; d3 / mixed / w1: scalar-path widths, 3 segments; d8: the 8-lane rows; criteo: 27 segments, more
    than the kernel takes, so the module concatenates first."""
    from torchrec_amd.modules import DeepFM, FactorizationMachine

    fx = dr.module_fixture(case)
    tol_out, tol_grad = dr.gpu_tolerances()
    leaves = [_dev(x).requires_grad_() for x in fx["xs"]]
    fm = FactorizationMachine()(embeddings=leaves)
    assert fm.shape == (leaves[0].shape[0], 1) and fm.grad_fn is not None and "_FM" in type(fm.grad_fn).__name__
    fm.backward(_dev(fx["gfm"]))
    gx = torch.cat([l.grad.flatten(1) for l in leaves], 1).cpu().numpy()
    e_out, e_grad = dr.fm_errors(fx["xs"], fx["gfm"], fm.detach().cpu().numpy(), gx)
    print(f"{case}: output error {e_out:.2e} (tolerance {tol_out:.2e}), gradient error {e_grad:.2e} ({tol_grad:.2e})")
    assert e_out <= tol_out and e_grad <= tol_grad
    assert [l.grad.shape for l in leaves] == [l.shape for l in leaves]
    # DeepFM: torch's cat and Linear
    N = fx["params"]["0.weight"].shape[1]
    deep = DeepFM(dense_module=nn.Sequential(nn.Linear(N, dr.DEEP_OUT), nn.ReLU())).to(DEV)
    deep.load_state_dict({"dense_module." + k: _dev(v) for k, v in fx["params"].items()}, strict=True)
    leaves = [_dev(x).requires_grad_() for x in fx["xs"]]
    out = deep(embeddings=leaves)
    out.backward(_dev(fx["gdeep"]))
    _close(out, fx["f64"]["deep"])
    _close(torch.cat([l.grad.flatten(1) for l in leaves], 1)[_dev(fx["rows"])], fx["f64"]["gx_deep"])
    for n, p in deep.dense_module.named_parameters():
        _close(p.grad, fx["f64"]["gparam|" + n], n)


def _arch_from_fixture(case, names=None):
    """FMInteractionArch on the module fixture `case` (first input = dense, the rest = features of one KeyedTensor)."""
    from torchrec_amd.models.deepfm import FMInteractionArch
    from torchrec_amd.sparse.jagged_tensor import KeyedTensor

    fx = dr.module_fixture(case)
    widths = [x.shape[1] for x in fx["xs"]]
    keys = [f"k{i}" for i in range(len(widths) - 1)]
    arch = FMInteractionArch(fm_in_features=sum(widths), sparse_feature_names=list(names or keys),
                             deep_fm_dimension=dr.DEEP_OUT).to(DEV)
    arch.deep_fm.load_state_dict({"dense_module." + k: _dev(v) for k, v in fx["params"].items()}, strict=True)
    dense = _dev(fx["xs"][0]).requires_grad_()
    values = _dev(np.concatenate(fx["xs"][1:], 1)).requires_grad_()
    return fx, arch, dense, values, KeyedTensor(keys=keys, length_per_key=widths[1:], values=values)


@pytest.mark.parametrize("case", ["d3", "d8", "mixed", "w1"])
def test_interaction_arch_reproduces_the_float64_fixtures(case):
    fx, arch, dense, values, kt = _arch_from_fixture(case)
    tol_out, tol_grad = dr.gpu_tolerances()
    D = dense.shape[1]
    out = arch(dense, kt)
    assert out.shape == (dense.shape[0], D + dr.DEEP_OUT + 1)
    assert torch.equal(out[:, :D], dense)
    _close(out[:, D:D + dr.DEEP_OUT], fx["f64"]["deep"])
    g = torch.zeros_like(out)
    g[:, D:D + dr.DEEP_OUT], g[:, -1:] = _dev(fx["gdeep"]), _dev(fx["gfm"])
    out.backward(g)
    gx = torch.cat([dense.grad, values.grad], 1).cpu().numpy().astype(np.float64)
    fm64, gfm64 = dr.fm_ref(fx["xs"], fx["gfm"])
    e_out, _ = dr.fm_errors(fx["xs"], fx["gfm"], out[:, -1:].detach().cpu().numpy(), gfm64.astype(np.float32))
    assert e_out <= tol_out
    # the input gradient is the sum of the two branches': the deep part carries the GEMM tolerance, the FM part its own
    x = dr.flat_cat(fx["xs"])
    bound = (dr.GEMM_TOL["atol"] + dr.GEMM_TOL["rtol"] * np.abs(fx["f64"]["gx_deep"])
             + tol_grad * np.abs(fx["gfm"].astype(np.float64)) * np.abs(x).sum(1, keepdims=True))
    assert (np.abs(gx - (fx["f64"]["gx_deep"] + fx["f64"]["gx_fm"])) <= bound).all()
    for n, p in arch.deep_fm.dense_module.named_parameters():
        _close(p.grad, fx["f64"]["gparam|" + n], n)


def _dyadic_arch(names):
    """An arch and inputs whose every product and sum is exact in float32 (multiples of 1/4 and 1/8 of small magnitude):
    results cannot depend on the order of a summation, so two paths that compute the same thing agree bit for bit."""
    from torchrec_amd.models.deepfm import FMInteractionArch
    from torchrec_amd.sparse.jagged_tensor import KeyedTensor

    rng = np.random.default_rng(21)
    B, D, keys, DI = 37, 8, ["k0", "k1", "k2"], 4
    dense = _dev(rng.integers(-8, 9, (B, D)).astype(np.float32) / 4).requires_grad_()
    values = _dev(rng.integers(-8, 9, (B, 3 * D)).astype(np.float32) / 4).requires_grad_()
    W = rng.integers(-8, 9, (DI, 4 * D)).astype(np.float32) / 8
    b = rng.integers(-8, 9, DI).astype(np.float32) / 8 + np.float32(1 / 16)  # no pre-activation is exactly 0
    g = _dev(rng.integers(-4, 5, (B, D + DI + 1)).astype(np.float32) / 4)
    arch = FMInteractionArch(fm_in_features=4 * D, sparse_feature_names=list(names), deep_fm_dimension=DI).to(DEV)
    order = [0] + [1 + keys.index(n) for n in names]  # the column blocks of the arch's row, in blocks of the canonical row
    cols = np.concatenate([np.arange(D) + D * blk for blk in order])
    with torch.no_grad():
        arch.deep_fm.dense_module[0].weight.copy_(_dev(W[:, cols]))
        arch.deep_fm.dense_module[0].bias.copy_(_dev(b))
    return arch, dense, values, KeyedTensor(keys=keys, length_per_key=[D] * 3, values=values), g


def test_the_fused_path_and_the_list_path_agree_bit_for_bit():
    """The same features under a permuted sparse_feature_names (the list path: per-feature views) with the deep weight's
    columns permuted to match, against the key order (the fused two-input path)."""
    results = []
    for names in (["k0", "k1", "k2"], ["k2", "k0", "k1"]):
        arch, dense, values, kt, g = _dyadic_arch(names)
        out = arch(dense, kt)
        out.backward(g)
        results.append((out.detach(), dense.grad, values.grad))
    (o1, d1, v1), (o2, d2, v2) = results
    assert torch.equal(o1[:, -1], o2[:, -1])  # the FM column
    assert torch.equal(o1, o2)
    assert torch.equal(d1, d2) and torch.equal(v1, v2)
    # and the FM column is the right number: exact against float64
    x = np.concatenate([dense.detach().cpu().numpy(), values.detach().cpu().numpy()], 1)
    fm64, _ = dr.fm_ref([x], np.zeros((x.shape[0], 1)))
    np.testing.assert_array_equal(o1[:, -1:].cpu().numpy().astype(np.float64), fm64)


@pytest.mark.parametrize("dense_grad,sparse_grad", [(True, False), (False, True), (False, False)])
def test_grad_flags(dense_grad, sparse_grad):
    fx, arch, dense, values, kt = _arch_from_fixture("d8")
    full = arch(dense, kt)
    full.backward(torch.ones_like(full))
    want_d, want_v = dense.grad.clone(), values.grad.clone()
    fx, arch, dense, values, kt = _arch_from_fixture("d8")
    dense.requires_grad_(dense_grad)
    values.requires_grad_(sparse_grad)
    out = arch(dense, kt)
    assert torch.equal(out, full)
    out.backward(torch.ones_like(out))
    assert (dense.grad is not None) == dense_grad and (values.grad is not None) == sparse_grad
    if dense_grad:
        assert torch.equal(dense.grad, want_d)
    if sparse_grad:
        assert torch.equal(values.grad, want_v)
    # the stand-alone module: one gradient per input that asks for one
    from torchrec_amd.modules import FactorizationMachine

    xs = [_dev(x).requires_grad_(f) for x, f in zip(fx["xs"], (dense_grad, sparse_grad, True, False))]
    FactorizationMachine()(xs).sum().backward()
    assert [x.grad is not None for x in xs] == [dense_grad, sparse_grad, True, False]
    _, gx = dr.fm_ref(fx["xs"], np.ones((xs[0].shape[0], 1)))
    np.testing.assert_allclose(xs[2].grad.cpu().numpy(), gx[:, 16:24], rtol=1e-5, atol=1e-5)


def test_no_grad_forward_equals_the_training_forward_bit_for_bit():
    from torchrec_amd.modules import FactorizationMachine

    for case in ("d8", "mixed", "criteo"):
        fx = dr.module_fixture(case)
        leaves = [_dev(x).requires_grad_() for x in fx["xs"]]
        train = FactorizationMachine()(leaves)
        with torch.no_grad():
            plain = FactorizationMachine()(leaves)
        assert plain.grad_fn is None and not plain.requires_grad
        assert torch.equal(train.detach(), plain)
    fx, arch, dense, values, kt = _arch_from_fixture("w1")
    train = arch(dense, kt)
    with torch.no_grad():
        assert torch.equal(arch(dense, kt), train.detach())


def test_3d_and_non_contiguous_inputs():
    from torchrec_amd.modules import FactorizationMachine

    tol_out, _ = dr.gpu_tolerances()
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((6, 2, 8)).astype(np.float32), rng.standard_normal((6, 10, 3)).astype(np.float32)
    fm = FactorizationMachine()
    out = fm([_dev(a), _dev(b)])
    e, _ = dr.fm_errors([a, b], np.ones((6, 1)), out.cpu().numpy(), dr.fm_ref([a, b], np.ones((6, 1)))[1])
    assert e <= tol_out
    # an inner dimension that is not contiguous: the torch expression, and the result of the contiguous copy
    bt = _dev(np.ascontiguousarray(b.transpose(0, 2, 1))).transpose(1, 2)  # [6, 10, 3] again, strides permuted
    assert not bt.is_contiguous() and torch.equal(bt, _dev(b))
    strided = _dev(np.repeat(a.reshape(6, 16), 2, axis=1))[:, ::2]  # a [6, 16] view with inner stride 2
    got = fm([strided, bt])
    e, _ = dr.fm_errors([a, b], np.ones((6, 1)), got.cpu().numpy(), dr.fm_ref([a, b], np.ones((6, 1)))[1])
    assert e <= tol_out
    np.testing.assert_allclose(got.cpu().numpy(), out.cpu().numpy(), rtol=1e-5, atol=1e-5)
    # a row-strided view (a column block of a wider matrix) stays on the kernel path
    wide = _dev(rng.standard_normal((6, 40)).astype(np.float32))
    blk = wide[:, 8:24].requires_grad_()
    o = fm([blk])
    assert "_FM" in type(o.grad_fn).__name__
    assert torch.equal(o, fm([blk.detach().contiguous()]))


def test_forward_and_backward_capture_into_one_hip_graph():
    fx, arch, dense, values, kt = _arch_from_fixture("w1")
    params = list(arch.parameters())
    gout = torch.randn(dense.shape[0], dense.shape[1] + dr.DEEP_OUT + 1, device=DEV)

    def step():
        out = arch(dense, kt)
        return (out,) + torch.autograd.grad(out, [dense, values] + params, gout)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    # new data in the same buffers
    with torch.no_grad():
        dense.copy_(torch.randn_like(dense))
        values.copy_(torch.randn_like(values))
        gout.copy_(torch.randn_like(gout))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in static]
    eager = step()
    for i, (r, e) in enumerate(zip(replayed, eager)):
        if i < 3:  # out and the two input gradients of the kernels: the same launches, the same bits
            assert torch.equal(r, e), i
        else:
            torch.testing.assert_close(r, e, rtol=1e-5, atol=1e-6)


# ---- the model ---------------------------------------------------------------------------------------------------------
def _configs(case):
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig

    _, D, tables, _, _, _, _ = dr.MODEL_CASES[case]
    return [EmbeddingBagConfig(name=t, embedding_dim=D, num_embeddings=r, feature_names=list(f)) for t, r, f in tables]


def _kjt(case, fx):
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    return KeyedJaggedTensor.from_lengths_sync(keys=dr.MODEL_CASES[case][3], values=_dev(fx["values"]),
                                               lengths=_dev(fx["lengths"]))


@pytest.mark.parametrize("case", list(dr.MODEL_CASES))
def test_model_reproduces_the_float64_fixtures(case):
    """Unsharded collection on the device (its tables are ordinary parameters), so every parameter gradient is there to
    compare, embedding tables included."""
    from torchrec_amd.models.deepfm import SimpleDeepFMNN
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    fx = dr.model_fixture(case)
    _, D, tables, _, n_dense, hidden, deep_dim = dr.MODEL_CASES[case]
    ebc = EmbeddingBagCollection(_configs(case), device=DEV)
    model = SimpleDeepFMNN(num_dense_features=n_dense, embedding_bag_collection=ebc, hidden_layer_size=hidden,
                           deep_fm_dimension=deep_dim).to(DEV)
    pre = "sparse_arch.embedding_bag_collection.embedding_bags."
    res = model.load_state_dict({k: _dev(v) for k, v in fx["sd"].items() if not k.startswith(pre)}, strict=False)
    assert not res.unexpected_keys
    views = ebc.table_weights()
    with torch.no_grad():
        for name, w in views.items():
            w.copy_(_dev(fx["sd"][pre + name + ".weight"]))
    logits = model(dense_features=_dev(fx["dense"]), sparse_features=_kjt(case, fx))
    logits.backward(_dev(fx["g"]))
    _close(logits, fx["f64"]["logits"])
    grads = fx["f64"]["grad"]
    seen = 0
    for n, p in model.named_parameters():
        if n in grads:
            _close(p.grad, grads[n], n)
            seen += 1
    assert seen == len(grads) - len(views)
    flat = [p for n, p in model.named_parameters() if n not in grads]
    assert len(flat) == 1  # the collection's one weight buffer
    for name, w in views.items():
        g = flat[0].grad.view(-1)[w.storage_offset():w.storage_offset() + w.numel()].view_as(w)
        _close(g, grads[pre + name + ".weight"], name)


def _sharded_model(case, lr=0.0):
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.models.deepfm import SimpleDeepFMNN
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    _, D, tables, _, n_dense, hidden, deep_dim = dr.MODEL_CASES[case]
    model = SimpleDeepFMNN(num_dense_features=n_dense, embedding_bag_collection=EmbeddingBagCollection(
        _configs(case), device=torch.device("meta")), hidden_layer_size=hidden, deep_fm_dimension=deep_dim).to(DEV)
    return DistributedModelParallel(model, env=ShardingEnv.from_local(1, 0), device=DEV,
                                    sharders=[EmbeddingBagCollectionSharder({"learning_rate": lr})])


@pytest.mark.parametrize("case", list(dr.MODEL_CASES))
def test_a_reference_state_dict_round_trips_on_the_device(case):
    fx = dr.model_fixture(case)
    dmp = _sharded_model(case)
    assert sorted(dmp.state_dict().keys()) == sorted(fx["sd"].keys())
    res = dmp.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in fx["sd"].items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = dmp.state_dict()
    for k, v in fx["sd"].items():
        t = back[k]
        t = t.local_shards()[0].tensor if hasattr(t, "local_shards") else t
        np.testing.assert_array_equal(t.cpu().numpy(), v, err_msg=k)
    dmp.eval()
    with torch.no_grad():
        logits = dmp(dense_features=_dev(fx["dense"]), sparse_features=_kjt(case, fx))
    _close(logits, fx["f64"]["logits"])


class _TorchTwin(nn.Module):
    """SimpleDeepFMNN the reference's way: nn.EmbeddingBag per table, torch.cat, the reference's formula."""

    def __init__(self, rows, D, n_dense, hidden, deep_dim):
        super().__init__()
        F = len(rows)
        self.bags = nn.ModuleList([nn.EmbeddingBag(r, D, mode="sum", include_last_offset=True) for r in rows])
        self.dense = nn.Sequential(nn.Linear(n_dense, hidden), nn.ReLU(), nn.Linear(hidden, D), nn.ReLU())
        self.deep = nn.Sequential(nn.Linear((F + 1) * D, deep_dim), nn.ReLU())
        self.over = nn.Sequential(nn.Linear(D + deep_dim + 1, 1), nn.Sigmoid())

    def forward(self, dense, values, B):
        x = self.dense(dense)
        offs = torch.arange(B + 1, device=dense.device)
        row = torch.cat([x] + [bag(values[f * B:(f + 1) * B], offs) for f, bag in enumerate(self.bags)], dim=1)
        s = torch.sum(row, dim=1, keepdim=True)
        fm = torch.sum(s * s - torch.sum(row * row, dim=1, keepdim=True), dim=1, keepdim=True) * 0.5
        return self.over(torch.cat([x, self.deep(row), fm], dim=1))


class _Train(nn.Module):
    """What a train pipeline drives: batch -> (loss, (loss, logits, labels)); the model ends in a Sigmoid, hence BCELoss."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.loss_fn = nn.BCELoss()

    def forward(self, batch):
        logits = self.model(batch.dense_features, batch.sparse_features).squeeze(-1)
        loss = self.loss_fn(logits, batch.labels.float())
        return loss, (loss.detach(), logits.detach(), batch.labels)


def test_training_follows_a_plain_torch_twin():
    """SimpleDeepFMNN under DistributedModelParallel (world 1), fused SGD in the table update, TrainPipelineSparseDist:
    the construction of tests/test_dlrm_e2e_gpu.py at B = 64, three small tables, D = 8, four steps, its tolerances."""
    from torchrec_amd.datasets.random import RandomRecDataset
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.train_pipeline import TrainPipelineSparseDist
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.models.deepfm import SimpleDeepFMNN
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.optim.keyed import CombinedOptimizer, KeyedOptimizerWrapper

    torch.manual_seed(0)
    rows, D, B, lr, n_dense, hidden, deep_dim, steps = [50, 3, 1000], 8, 64, 0.05, 13, 16, 6, 4
    keys = [f"cat_{i}" for i in range(len(rows))]
    tables = [EmbeddingBagConfig(name=f"t_{k}", embedding_dim=D, num_embeddings=rows[i], feature_names=[k])
              for i, k in enumerate(keys)]
    net = SimpleDeepFMNN(num_dense_features=n_dense, embedding_bag_collection=EmbeddingBagCollection(
        tables, device=torch.device("meta")), hidden_layer_size=hidden, deep_fm_dimension=deep_dim).to(DEV)
    model = DistributedModelParallel(_Train(net), env=ShardingEnv.from_local(1, 0), device=DEV,
                                     sharders=[EmbeddingBagCollectionSharder({"learning_rate": lr})])
    opt = CombinedOptimizer([model.fused_optimizer,
                             KeyedOptimizerWrapper(dict(model.named_parameters()), lambda p: torch.optim.SGD(p, lr=lr))])
    twin = _TorchTwin(rows, D, n_dense, hidden, deep_dim).to(DEV)
    shards = model.sharded_modules()[0].local_shards()
    with torch.no_grad():
        for i, k in enumerate(keys):
            twin.bags[i].weight.copy_(shards[f"t_{k}"][0])
        twin.dense.load_state_dict(net.dense_arch.model.state_dict())
        twin.deep.load_state_dict(net.inter_arch.deep_fm.dense_module.state_dict())
        twin.over.load_state_dict(net.over_arch.model.state_dict())
    twin_opt = torch.optim.SGD(twin.parameters(), lr=lr)
    data = RandomRecDataset(keys, B, rows, manual_seed=5, num_generated_batches=steps, num_batches=steps, device=DEV)
    batches = list(iter(data))
    torch.cuda.synchronize()
    pipe = TrainPipelineSparseDist(model, opt, DEV)
    model.train()
    it = iter(batches)
    bce = nn.BCELoss()
    for step in range(steps):
        loss = pipe.progress(it)[0]
        b = batches[step]
        twin_opt.zero_grad()
        twin_loss = bce(twin(b.dense_features, b.sparse_features.values(), B).squeeze(-1), b.labels.float())
        twin_loss.backward()
        twin_opt.step()
        torch.testing.assert_close(loss, twin_loss, rtol=2e-4, atol=2e-5)
    torch.cuda.synchronize()
    for i, k in enumerate(keys):
        torch.testing.assert_close(shards[f"t_{k}"][0], twin.bags[i].weight, rtol=1e-3, atol=2e-5)
    torch.testing.assert_close(net.over_arch.model[0].weight, twin.over[0].weight, rtol=1e-3, atol=2e-5)
    torch.testing.assert_close(net.dense_arch.model[0].weight, twin.dense[0].weight, rtol=1e-3, atol=2e-5)
    torch.testing.assert_close(net.inter_arch.deep_fm.dense_module[0].weight, twin.deep[0].weight, rtol=1e-3, atol=2e-5)
