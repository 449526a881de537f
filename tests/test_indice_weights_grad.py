"""CPU: the per-sample-weight gradient's reference and designed inputs (tests/_indice_weights_ref.py), its two C-ABI
entry points' argument checks, the differentiable KeyedJaggedTensor.permute and PositionWeightedModule."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _cpu_ops
import _indice_weights_ref as R
from fbgemm_gpu import _lib

_cpu_ops.register()

F32 = "tbe_backward_indice_weights_f32"
F16 = "tbe_backward_indice_weights_f16w"


# ---- the premise of the bit-for-bit GPU comparisons -------------------------------------------------------------------
@pytest.fixture(scope="module")
def designed():
    case = R.make_case([16, 256], [40, 30], ftm=[0, 1, 0], B=9, bags="short", seed=3)
    return case, R.reference(case)


def test_reference_equals_torch_embedding_bag_autograd(designed):
    """The reference's unsharded collection is nn.EmbeddingBag: its per_sample_weights.grad (mode="sum") is the contract."""
    case, ref = designed
    psw = R.designed_weights(np.random.default_rng(0), case.N)
    opk = case.offsets[::case.B]
    for f in range(case.F):
        lo, hi = int(opk[f]), int(opk[f + 1])
        w = torch.tensor(psw[lo:hi], requires_grad=True)
        out = torch.nn.functional.embedding_bag(
            torch.tensor(case.indices[lo:hi]), torch.tensor(case.tables[case.ftm[f]]),
            torch.tensor(case.offsets[f * case.B:(f + 1) * case.B] - lo), mode="sum", per_sample_weights=w)
        c0 = int(case.out_offset[f])
        out.backward(torch.tensor(case.grad[:, c0:c0 + case.feat_D[f]]))
        np.testing.assert_array_equal(w.grad.numpy().astype(np.float64), ref[lo:hi])


def test_designed_inputs_are_exact_in_fp32_in_any_order(designed):
    case, ref = designed
    checked = 0
    for f in range(case.F):
        W, c0, D = case.tables[case.ftm[f]], int(case.out_offset[f]), case.feat_D[f]
        for b in range(case.B):
            for i in range(int(case.offsets[f * case.B + b]), int(case.offsets[f * case.B + b + 1])):
                prod = case.grad[b, c0:c0 + D] * W[case.indices[i]]  # float32 products
                fwd = rev = np.float32(0)
                for d in range(D):
                    fwd = np.float32(fwd + prod[d])
                    rev = np.float32(rev + prod[D - 1 - d])
                blocked = np.float32(0)
                for part in prod.reshape(-1, 4).sum(axis=1, dtype=np.float32):
                    blocked = np.float32(blocked + part)
                assert float(fwd) == float(rev) == float(blocked) == ref[i]
                checked += 1
    assert checked == case.N > 0


def test_reference_mean_masks_and_malformed_bags():
    tables = [np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32)]
    grad = np.array([[1.0, 1.0], [2.0, 0.0]], dtype=np.float32)
    case = R.Case(tables, [0], 2, [0, 1, 1, R.ID_SKIP, 5], [0, 2, 5], grad)
    np.testing.assert_array_equal(R.reference(case), [3, 7, 6, 0, 0])
    np.testing.assert_array_equal(R.reference(case, pooling=R.MEAN), [1.5, 3.5, 2, 0, 0])
    np.testing.assert_array_equal(R.reference(case, pooling=R.MEAN, feat_pooling=[R.SUM]), [3, 7, 6, 0, 0])
    np.testing.assert_array_equal(R.reference(case, feat_requires_grad=[0]), [0] * 5)
    np.testing.assert_array_equal(R.reference(case, feat_window=[(1, 3)]), [0, 1 * 3, 2, 0, 0])  # row 0 of the shard is id 1
    bad = R.Case(tables, [0], 2, [0, 1, 1, 0, 1], [0, 2, 6], grad)  # the second bag ends past N
    np.testing.assert_array_equal(R.reference(bad), [3, 7, 0, 0, 0])


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name in (F32, F16):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES[F32] == _lib.SIGNATURES[F16]
    assert lib.tbe_abi_version() == 3


def _call(lib, name, F=2, B=4, max_D=128, N=8, pooling=R.SUM, stride=256, ptr=16, grad=16, giw=16):
    return getattr(lib, name)(ptr, ptr, ptr, ptr, F, B, max_D, ptr, N, ptr, pooling, None, grad, stride, None, giw, None, None)


@pytest.mark.parametrize("name", [F32, F16])
def test_entry_points_validate_before_any_launch(name):
    lib = _lib.load()
    assert _call(lib, name, F=0) == -1 and b"bad sizes" in lib.tbe_last_error()
    assert _call(lib, name, B=-1) == -1 and b"bad sizes" in lib.tbe_last_error()
    assert _call(lib, name, N=-1) == -1 and b"bad sizes" in lib.tbe_last_error()
    assert _call(lib, name, max_D=0) == -1 and b"max_D=0" in lib.tbe_last_error()
    assert _call(lib, name, max_D=2049) == -1 and b"max_D=2049" in lib.tbe_last_error()
    assert _call(lib, name, stride=0) == -1 and b"grad_row_stride" in lib.tbe_last_error()
    assert _call(lib, name, grad=None) == -1 and b"null pointer" in lib.tbe_last_error()
    assert _call(lib, name, giw=None) == -1 and b"null grad_indice_weights" in lib.tbe_last_error()
    assert _call(lib, name, ptr=None) == -1 and b"null pointer" in lib.tbe_last_error()
    assert _call(lib, name, pooling=3) == -1 and b"pooling_mode 3" in lib.tbe_last_error()
    assert _call(lib, name, pooling=R.NONE) == -4 and b"NONE" in lib.tbe_last_error()  # TBE_ERR_UNSUPPORTED
    assert _call(lib, name, N=0) == 0 and _call(lib, name, N=0, B=0) == 0  # nothing to write: nothing is launched


# ---- KeyedJaggedTensor.permute ---------------------------------------------------------------------------------------
def _kjt(weights):
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    lengths = torch.tensor([2, 0, 1, 1, 1, 3, 0, 2, 1], dtype=torch.int32)  # 3 keys x 3 samples
    values = torch.arange(100, 111, dtype=torch.int64)
    return KeyedJaggedTensor.from_lengths_sync(["a", "b", "c"], values, lengths, weights=weights)


@pytest.mark.parametrize("order", [[2, 0, 1], [1, 1, 2]], ids=["permutation", "duplicated_key"])
def test_permute_carries_the_gradient_of_trained_weights(order):
    w = torch.arange(1, 12, dtype=torch.float32) / 4
    plain = _kjt(w.clone()).permute(order)
    assert not plain.weights().requires_grad
    trained_w = w.clone().requires_grad_(True)
    trained = _kjt(trained_w).permute(order)
    assert trained.keys() == plain.keys() and trained.length_per_key() == plain.length_per_key()
    for a, b in ((trained.values(), plain.values()), (trained.lengths(), plain.lengths()),
                 (trained.weights().detach(), plain.weights())):
        assert a.dtype == b.dtype and torch.equal(a, b)
    coeff = torch.arange(1, trained.weights().numel() + 1, dtype=torch.float32)
    (trained.weights() * coeff).sum().backward()
    # position p of the input ends up at the places where the permuted VALUES hold its id 100 + p
    expect = torch.zeros(11)
    expect.index_add_(0, plain.values() - 100, coeff)
    assert torch.equal(trained_w.grad, expect)
    if order == [1, 1, 2]:
        assert (trained_w.grad[:3] == 0).all() and (trained_w.grad[3:8] > coeff[:5]).all()  # key "b" is used twice


def test_permute_without_trained_weights_is_unchanged():
    w = torch.arange(1, 12, dtype=torch.float32)
    out = _kjt(w).permute([2, 0, 1])
    assert out.values().tolist() == [108, 109, 110, 100, 101, 102, 103, 104, 105, 106, 107]
    assert out.weights().tolist() == [9, 10, 11, 1, 2, 3, 4, 5, 6, 7, 8] and out.weights().dtype == torch.float32
    assert out.lengths().tolist() == [0, 2, 1, 2, 0, 1, 1, 1, 3]
    with torch.no_grad():  # trained weights outside a recorded region take the plain path too
        again = _kjt(w.clone().requires_grad_(True)).permute([2, 0, 1])
    assert torch.equal(again.weights(), out.weights()) and not again.weights().requires_grad
    assert _kjt(None).permute([1]).weights_or_none() is None


# ---- PositionWeightedModule ------------------------------------------------------------------------------------------
def _reference_vector_features():
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    # the vector of the reference's own test of this module: keys f1 / f2, three samples
    return KeyedJaggedTensor.from_offsets_sync(["f1", "f2"], torch.arange(8, dtype=torch.int64),
                                               torch.tensor([0, 2, 2, 3, 4, 5, 8], dtype=torch.int64)).to_dict()


def test_position_weighted_module_reference_vector():
    from torchrec_amd.modules import BaseFeatureProcessor, PositionWeightedModule

    pw = PositionWeightedModule({"f1": 10, "f2": 10})
    assert isinstance(pw, BaseFeatureProcessor)
    assert sorted(pw.state_dict()) == ["position_weights.f1", "position_weights.f2"]
    assert all(torch.equal(p, torch.ones(10)) for p in pw.state_dict().values())
    with torch.no_grad():
        pw.position_weights["f1"].copy_(torch.arange(10) + 1.0)
        pw.position_weights["f2"].copy_(torch.arange(10) + 11.0)
    features = _reference_vector_features()
    out = pw(features)
    assert list(out) == ["f1", "f2"]
    assert out["f1"].weights().tolist() == [1, 2, 1]  # positions [0, 1, 0]
    assert out["f2"].weights().tolist() == [11, 11, 11, 12, 13]  # positions [0, 0, 0, 1, 2]
    for k in out:
        assert out[k].values() is features[k].values() and torch.equal(out[k].lengths(), features[k].lengths())
    (out["f1"].weights().sum() + 2 * out["f2"].weights().sum()).backward()
    assert pw.position_weights["f1"].grad.tolist() == [2, 1] + [0] * 8
    assert pw.position_weights["f2"].grad.tolist() == [6, 2, 2] + [0] * 7


def test_position_weighted_module_clamps_bags_longer_than_max_length():
    from torchrec_amd.modules import PositionWeightedModule

    pw = PositionWeightedModule({"f2": 2})
    with torch.no_grad():
        pw.position_weights["f2"].copy_(torch.tensor([5.0, 7.0]))
    out = pw(_reference_vector_features())
    assert list(out) == ["f2"]
    assert out["f2"].weights().tolist() == [5, 5, 5, 7, 7]  # position 2 reads the last entry
    out["f2"].weights().sum().backward()
    assert pw.position_weights["f2"].grad.tolist() == [3, 2]
    with pytest.raises(ValueError):
        PositionWeightedModule({"f": 0})
