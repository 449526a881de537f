"""CPU half of DeepFM (torchrec_amd/modules/deepfm.py, torchrec_amd/models/deepfm.py, csrc/deepfm.hip): the new symbols,
the entries' argument checks, the modules' and the model's fall-back path against the reference's recorded runs
(tests/golden/deepfm.npz, written by tests/golden/make_deepfm_golden.py from the reference itself), the float64
restatement (tests/_deepfm_ref.py) against the same, where the GPU tests' tolerance comes from, and the exact integer
model of the C-ABI tests."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import _paths
import _deepfm_ref as dr
from fbgemm_gpu import _lib
from torchrec_amd.models.deepfm import DenseArch, FMInteractionArch, OverArch, SimpleDeepFMNN, SparseArch
from torchrec_amd.modules import DeepFM, FactorizationMachine
from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor, KeyedTensor

NEW_SYMBOLS = ["tbe_fm_forward_f32", "tbe_fm_backward_f32"]
INVALID = -1


def test_new_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(_paths.ROOT, "include", "tbe_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    for text in ("#define TBE_FM_MAX_SEGMENTS 8", "tbe_fm_segment;", "tbe_fm_grad_segment;",
                 "torchrec/modules/deepfm.py:28-32", "torchrec/models/deepfm.py:175-184"):
        assert text in hdr, text
    assert _lib.FM_MAX_SEGMENTS == 8
    assert ctypes.sizeof(_lib.FmSegment) == 24 and ctypes.sizeof(_lib.FmGradSegment) == 16
    assert lib.tbe_abi_version() == 3


def _segs(*items):
    a = (_lib.FmSegment * len(items))()
    for k, (x, stride, width) in enumerate(items):
        a[k].x, a[k].row_stride, a[k].width = x, stride, width
    return a


def _gsegs(*items):
    a = (_lib.FmGradSegment * len(items))()
    for k, (g, stride) in enumerate(items):
        a[k].g, a[k].row_stride = g, stride
    return a


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every call here must return before a launch: the addresses are not device memory."""
    lib = _lib.load()
    P = 0x10000
    good = (P, 8, 8)

    def fwd(segs, nseg=None, B=4, fm=P, fm_stride=1, row_sum=P, cat=None):
        rc = lib.tbe_fm_forward_f32(segs, len(segs) if nseg is None else nseg, B, fm, fm_stride, row_sum, cat, None)
        return rc, lib.tbe_last_error().decode()

    def bwd(segs, grads, nseg=None, B=4, gfm=P, gfm_stride=1, row_sum=P, gcat=None):
        rc = lib.tbe_fm_backward_f32(segs, grads, len(segs) if nseg is None else nseg, B, gfm, gfm_stride, row_sum, gcat, None)
        return rc, lib.tbe_last_error().decode()

    for call in (lambda **kw: fwd(_segs(good), **kw), lambda **kw: bwd(_segs(good), _gsegs((P, 8)), **kw)):
        rc, msg = call(nseg=0)
        assert rc == INVALID and "nseg=0" in msg
        rc, msg = call(nseg=9)
        assert rc == INVALID and "nseg=9" in msg and "1 .. 8" in msg
        rc, msg = call(B=4 * 2 ** 31)
        assert rc == INVALID and "too large" in msg
        rc, msg = call(row_sum=None)
        assert rc == INVALID and "null" in msg
        rc, msg = call(row_sum=P + 2)
        assert rc == INVALID and "misaligned" in msg
    for bad, word in (((P, 8, 0), "width 0 < 1"), ((P, 7, 8), "row stride 7 smaller than its width 8"),
                      ((None, 8, 8), "null"), ((P + 1, 8, 8), "misaligned")):
        rc, msg = fwd(_segs(good, bad))
        assert rc == INVALID and word in msg and "segment 1" in msg, msg
        rc, msg = bwd(_segs(good, bad), _gsegs((P, 8), (P, 8)))
        assert rc == INVALID and word in msg and "segment 1" in msg, msg
    rc, msg = fwd(_segs(good), fm_stride=0)
    assert rc == INVALID and "fm_stride=0" in msg
    rc, msg = fwd(_segs(good), fm=None)
    assert rc == INVALID and "null" in msg
    rc, msg = fwd(_segs(good), cat=P + 3)
    assert rc == INVALID and "misaligned" in msg
    rc, msg = bwd(_segs(good), _gsegs((P, 8)), gfm_stride=0)
    assert rc == INVALID and "grad_fm_stride=0" in msg
    rc, msg = bwd(_segs(good), _gsegs((P, 7)))
    assert rc == INVALID and "gradient segment 0 has row stride 7" in msg
    rc, msg = bwd(_segs(good), _gsegs((P + 2, 8)))
    assert rc == INVALID and "misaligned" in msg
    rc, msg = bwd(_segs(good), _gsegs((P, 8)), gcat=P + 1)
    assert rc == INVALID and "misaligned" in msg
    # the empty batch launches nothing and succeeds, whatever the pointers
    assert fwd(_segs((None, 8, 8)), B=0, fm=None, row_sum=None)[0] == 0
    assert bwd(_segs((None, 8, 8)), _gsegs((None, 0)), B=0, gfm=None, row_sum=None)[0] == 0


def test_ops_refuse_cpu_tensors_by_name():
    from torchrec_amd.distributed import _device_ops

    x = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _device_ops._fm_forward([x], False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _device_ops._fm_backward([x], torch.zeros(2, 1), torch.zeros(2), None, [True])
    with pytest.raises(RuntimeError, match="empty input list"):
        _device_ops._fm_forward([], False)
    # merging: adjacent column slices of one buffer are one segment; a gap, another stride or another flag splits
    buf = torch.zeros(5, 12)
    views = [buf[:, 0:3], buf[:, 3:8], buf[:, 8:12]]
    assert [(g[0], g[1], g[3], g[4]) for g in _device_ops.fm_segments(views)] == [(0, 3, 12, 12)]
    assert [(g[0], g[1], g[4]) for g in _device_ops.fm_segments(views, [True, False, False])] == [(0, 1, 3), (1, 2, 9)]
    assert len(_device_ops.fm_segments([buf[:, 0:3], buf[:, 4:8]])) == 2
    assert len(_device_ops.fm_segments([buf[:, 0:3], torch.zeros(5, 3)])) == 2


# ---- modules ---------------------------------------------------------------------------------------------------------------
def _deep_module(fx):
    N = fx["params"]["0.weight"].shape[1]
    deep = DeepFM(dense_module=nn.Sequential(nn.Linear(N, dr.DEEP_OUT), nn.ReLU()))
    assert list(deep.state_dict().keys()) == ["dense_module.0.weight", "dense_module.0.bias"]
    deep.load_state_dict({"dense_module." + k: torch.from_numpy(v.copy()) for k, v in fx["params"].items()}, strict=True)
    return deep


@pytest.mark.parametrize("case", list(dr.MODULE_CASES))
def test_modules_on_cpu_reproduce_the_reference_bit_for_bit(case):
    """The fall-back IS the reference's expression: same operations, same order, same bits (one thread, as recorded)."""
    fx = dr.module_fixture(case)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        leaves = [torch.from_numpy(x.copy()).requires_grad_() for x in fx["xs"]]
        fm = FactorizationMachine()(embeddings=leaves)
        assert fm.shape == (leaves[0].shape[0], 1)
        fm.backward(torch.from_numpy(fx["gfm"].copy()))
        np.testing.assert_array_equal(fm.detach().numpy(), fx["f32"]["fm"])
        gx = torch.cat([l.grad.flatten(1) for l in leaves], 1).numpy()
        np.testing.assert_array_equal(gx[fx["rows"]], fx["f32"]["gx_fm"])
        leaves = [torch.from_numpy(x.copy()).requires_grad_() for x in fx["xs"]]
        deep = _deep_module(fx)
        out = deep(embeddings=leaves)
        out.backward(torch.from_numpy(fx["gdeep"].copy()))
        np.testing.assert_array_equal(out.detach().numpy(), fx["f32"]["deep"])
        gx = torch.cat([l.grad.flatten(1) for l in leaves], 1).numpy()
        np.testing.assert_array_equal(gx[fx["rows"]], fx["f32"]["gx_deep"])
        for n, p in deep.dense_module.named_parameters():
            np.testing.assert_array_equal(p.grad.numpy(), fx["f32"]["gparam|" + n], err_msg=n)
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("case", list(dr.MODULE_CASES))
def test_float64_restatement_of_the_modules_equals_the_reference_in_float64(case):
    fx = dr.module_fixture(case)
    fm, gx = dr.fm_ref(fx["xs"], fx["gfm"])
    tol = dict(rtol=1e-12, atol=1e-11)
    np.testing.assert_allclose(fm, fx["f64"]["fm"], **tol)
    np.testing.assert_allclose(gx[fx["rows"]], fx["f64"]["gx_fm"], **tol)
    out, gxd, gp = dr.deep_ref(fx["xs"], fx["params"], fx["gdeep"])
    np.testing.assert_allclose(out, fx["f64"]["deep"], **tol)
    np.testing.assert_allclose(gxd[fx["rows"]], fx["f64"]["gx_deep"], **tol)
    for n, v in gp.items():
        np.testing.assert_allclose(v, fx["f64"]["gparam|" + n], err_msg=n, **tol)


def test_double_backward_and_other_dtypes_take_the_torch_expression():
    xs = [torch.randn(4, 3, dtype=torch.float64, requires_grad=True), torch.randn(4, 2, 2, dtype=torch.float64, requires_grad=True)]
    assert torch.autograd.gradcheck(lambda *a: FactorizationMachine()(list(a)), xs)
    assert torch.autograd.gradgradcheck(lambda *a: FactorizationMachine()(list(a)), xs)
    x16 = [torch.randn(4, 6).bfloat16()]
    assert FactorizationMachine()(x16).dtype == torch.bfloat16


# ---- model ---------------------------------------------------------------------------------------------------------------
class _TorchEBC(nn.Module):
    """The reference's unsharded design on the CPU (torchrec/modules/embedding_modules.py:149-193): nn.EmbeddingBag per
    table under `embedding_bags`, the reference's state-dict keys.  This package's own collection computes on a HIP device
    or sharded only."""

    def __init__(self, tables):
        super().__init__()
        self.embedding_bag_configs = list(tables)
        self.embedding_bags = nn.ModuleDict({c.name: nn.EmbeddingBag(c.num_embeddings, c.embedding_dim, mode="sum",
                                                                     include_last_offset=True) for c in tables})

    def forward(self, features):
        B, keys, offsets = features.stride(), features.keys(), features.offsets()
        pooled, names = [], []
        for c in self.embedding_bag_configs:
            for f in c.feature_names:
                i = keys.index(f)
                o = offsets[i * B:(i + 1) * B + 1]
                pooled.append(self.embedding_bags[c.name](features.values()[int(o[0]):int(o[-1])], o - o[0]))
                names.append(f)
        return KeyedTensor(keys=names, length_per_key=[p.shape[1] for p in pooled], values=torch.cat(pooled, 1))


def _configs(case):
    _, D, tables, _, _, _, _ = dr.MODEL_CASES[case]
    return [EmbeddingBagConfig(name=t, embedding_dim=D, num_embeddings=r, feature_names=list(f)) for t, r, f in tables]


def _kjt(case, fx):
    keys = dr.MODEL_CASES[case][3]
    lengths = torch.from_numpy(fx["lengths"].astype(np.int64))
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0)])
    return KeyedJaggedTensor(keys=keys, values=torch.from_numpy(fx["values"].copy()), lengths=lengths, offsets=offsets)


@pytest.mark.parametrize("case", list(dr.MODEL_CASES))
def test_model_on_cpu_loads_the_reference_state_dict_and_reproduces_it_bit_for_bit(case):
    fx = dr.model_fixture(case)
    _, D, _, _, n_dense, hidden, deep_dim = dr.MODEL_CASES[case]
    model = SimpleDeepFMNN(num_dense_features=n_dense, embedding_bag_collection=_TorchEBC(_configs(case)),
                           hidden_layer_size=hidden, deep_fm_dimension=deep_dim)
    assert list(model.state_dict().keys()) == list(fx["sd"].keys())  # the reference's keys, in its order
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in fx["sd"].items()}, strict=True)
    assert isinstance(model.sparse_arch, SparseArch) and isinstance(model.dense_arch, DenseArch)
    assert isinstance(model.inter_arch, FMInteractionArch) and isinstance(model.over_arch, OverArch)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        logits = model(dense_features=torch.from_numpy(fx["dense"].copy()), sparse_features=_kjt(case, fx))
        logits.backward(torch.from_numpy(fx["g"].copy()))
    finally:
        torch.set_num_threads(threads)
    np.testing.assert_array_equal(logits.detach().numpy(), fx["f32"]["logits"])
    for n, p in model.named_parameters():
        np.testing.assert_array_equal(p.grad.numpy(), fx["f32"]["grad"][n], err_msg=n)


@pytest.mark.parametrize("case", list(dr.MODEL_CASES))
def test_float64_restatement_of_the_model_equals_the_reference_in_float64(case):
    fx = dr.model_fixture(case)
    logits, grads = dr.model_ref(case, fx["sd"], fx["values"], fx["lengths"], fx["dense"], fx["g"])
    np.testing.assert_allclose(logits, fx["f64"]["logits"], rtol=1e-12, atol=1e-13)
    assert set(grads) == set(fx["f64"]["grad"])
    for n, v in grads.items():
        np.testing.assert_allclose(v, fx["f64"]["grad"][n], rtol=1e-11, atol=1e-13, err_msg=n)
    if case == "ragged":
        assert fx["lengths"][1] == 0  # the empty bag


def test_constructor_assertions_and_the_empty_feature_list():
    with pytest.raises(AssertionError, match="At least one embedding bag is required"):
        SimpleDeepFMNN(4, _TorchEBC([]), 8, 3)
    mixed = [EmbeddingBagConfig(name="a", embedding_dim=4, num_embeddings=5, feature_names=["a"]),
             EmbeddingBagConfig(name="b", embedding_dim=8, num_embeddings=5, feature_names=["b"])]
    with pytest.raises(AssertionError, match="All EmbeddingBagConfigs must have the same dimension"):
        SimpleDeepFMNN(4, _TorchEBC(mixed), 8, 3)
    m = SimpleDeepFMNN(num_dense_features=4, embedding_bag_collection=_TorchEBC(_configs("doc")), hidden_layer_size=6,
                       deep_fm_dimension=3)
    assert m.inter_arch.sparse_feature_names == ["f1", "f3", "f2"]
    assert m.inter_arch.deep_fm.dense_module[0].in_features == 8 * 4 and m.over_arch.model[0].in_features == 8 + 3 + 1
    arch = FMInteractionArch(fm_in_features=6, sparse_feature_names=[], deep_fm_dimension=2)
    dense = torch.randn(3, 2)
    assert arch(dense, KeyedTensor(keys=[], length_per_key=[], values=torch.zeros(3, 0))) is dense
    # a permuted name list picks the features by name, as the reference does
    keys, D = ["f1", "f2"], 3
    arch = FMInteractionArch(fm_in_features=3 * D, sparse_feature_names=["f2", "f1"], deep_fm_dimension=2)
    vals = torch.randn(4, 2 * D)
    out = arch(torch.randn(4, D), KeyedTensor(keys=keys, length_per_key=[D, D], values=vals))
    assert out.shape == (4, D + 2 + 1)


# ---- tolerance and the exact model --------------------------------------------------------------------------------------
def test_the_gpu_tolerance_is_measured_not_chosen():
    """The worst error of the reference's own float32 results against its float64 results over the six module fixtures:
    the FM output normalised by 0.5 (s^2 + sum x^2), an input gradient by |g| sum |x| of its row.  Measured when this was
    written: 2.54e-7 (output) and 1.28e-7 (gradient); the GPU tests allow 8 x each (the factor covers the kernel's
    summation order, as in test_fused_optimizers.py).  The bands are one float32 rounding (6e-8) to ten."""
    out, grad = dr.measured_errors()
    print(f"measured: output {out:.3e}, gradient {grad:.3e}")
    assert 6e-8 < out < 6e-7, out
    assert 3e-8 < grad < 6e-7, grad
    assert dr.gpu_tolerances() == (8.0 * out, 8.0 * grad)
    # the restatement in float32 stays inside the tolerance on every fixture: the tolerance can be met
    for case in dr.MODULE_CASES:
        fx = dr.module_fixture(case)
        fm, gx = dr.fm_ref(fx["xs"], fx["gfm"], np.float32)
        e_out, e_grad = dr.fm_errors(fx["xs"], fx["gfm"], fm, gx)
        assert e_out <= 8.0 * out and e_grad <= 8.0 * grad, (case, e_out, e_grad)


def test_the_integer_model_of_the_abi_tests_equals_the_float64_restatement():
    rng = np.random.default_rng(11)
    B, widths = 9, [5, 3456 - 17, 12]
    xs = [rng.integers(-1, 2, (B, w)).astype(np.float32) for w in widths]
    gfm = rng.integers(-4, 5, (B, 1)).astype(np.float32)
    gcat = rng.integers(-8, 9, (B, sum(widths))).astype(np.float32)
    fm, s, cat, grads = dr.fm_int_model(xs, gfm, gcat)
    fm64, gx64 = dr.fm_ref(xs, gfm)
    np.testing.assert_array_equal(fm.astype(np.float64), fm64[:, 0])
    np.testing.assert_array_equal(s.astype(np.float64), dr.flat_cat(xs).sum(1))
    np.testing.assert_array_equal(cat, dr.flat_cat(xs, np.float32))
    np.testing.assert_array_equal(np.concatenate(grads, 1).astype(np.float64), gx64 + gcat)
    _, _, _, plain = dr.fm_int_model(xs, gfm)
    np.testing.assert_array_equal(np.concatenate(plain, 1).astype(np.float64), gx64)
    # and in float32, in two different summation orders, the same bits: the premise of the bit-for-bit comparison
    x32 = dr.flat_cat(xs, np.float32)
    for order in (slice(None), slice(None, None, -1)):
        s32 = np.float32(0) + np.add.reduce(x32[:, order], axis=1, dtype=np.float32)
        q32 = np.add.reduce((x32 * x32)[:, order], axis=1, dtype=np.float32)
        np.testing.assert_array_equal((s32 * s32 - q32) * np.float32(0.5), fm)
