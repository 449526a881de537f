"""GPU: the per-sample-weight gradient of the pooled TBE lookup (include/tbe_hip.h `tbe_backward_indice_weights_*`),
through the C ABI and up to PositionWeightedModule -> weighted EmbeddingBagCollection.

On the designed inputs of tests/_indice_weights_ref.py every summation order is exact in FP32, so results are compared
with the float64 reference bit for bit.  Shapes are the smallest at which the kernels can go wrong: one dim per
(G, NV) branch (D <= 256 and one dim for each of NV = 2, 4, 8), dims without a 16-B path, B = 67 (no multiple of 16 or 64) and B = 1, bags
of {0, 1, 2, 4} ids (the short-bag kernel) and a batch averaging >= 4 ids per bag with bags of 100 and 1000 ids next to
empty ones (the wave-per-bag kernel)."""
import functools

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _indice_weights_ref as R

pytestmark = pytest.mark.gpu

GUARD_BYTES, GUARD_BYTE = 256, 0xC3


def _cu(a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Abi:
    """The tables of a case and giw[N] in ONE device buffer, the tables 16-B aligned (4 B further for those in `misalign`),
    between GUARD_BYTES bytes of GUARD_BYTE.  `run` checks afterwards that every byte outside giw is what it was: the
    guards are intact and the tables bit-identical."""

    def __init__(self, case, misalign=()):
        self.case = case
        self.f16 = case.tables[0].dtype == np.float16
        off, self.table_off = GUARD_BYTES, []
        for t, w in enumerate(case.tables):
            off = (off + 15) // 16 * 16 + (4 if t in misalign else 0)
            self.table_off.append(off)
            off += w.nbytes + GUARD_BYTES
        self.giw_off = (off + 15) // 16 * 16 + 4 * (case.N % 4)  # giw itself starts 0 .. 12 B off the 16-B grid
        self.nbytes = self.giw_off + 4 * case.N + GUARD_BYTES
        host = np.full(self.nbytes, GUARD_BYTE, dtype=np.uint8)
        for o, w in zip(self.table_off, case.tables):
            host[o:o + w.nbytes] = np.ascontiguousarray(w).view(np.uint8).reshape(-1)
        self.host = host
        self.buf = _cu(host)
        assert self.buf.data_ptr() % 16 == 0
        base = self.buf.data_ptr()
        self.feat_weights = _cu([base + self.table_off[t] for t in case.ftm], torch.int64)
        self.feat_D, self.feat_rows = _cu(case.feat_D, torch.int32), _cu(case.feat_rows, torch.int64)
        self.out_offset, self.indices, self.offsets = _cu(case.out_offset), _cu(case.indices), _cu(case.offsets)
        self.grad = _cu(case.grad)
        assert self.grad.data_ptr() % 16 == 0

    def launch(self, pooling=R.SUM, feat_pooling=None, feat_requires_grad=None, feat_window=None):
        """Enqueues one call on the current stream (device arrays of the optional arguments are kept alive on self)."""
        from fbgemm_gpu import _lib

        lib, c, p = _lib.load(), self.case, _lib.ptr
        self._opt = (None if feat_pooling is None else _cu(feat_pooling, torch.int32),
                     None if feat_requires_grad is None else _cu(feat_requires_grad, torch.int32),
                     None if feat_window is None else _cu(np.asarray(feat_window).reshape(-1), torch.int64))
        fn = lib.tbe_backward_indice_weights_f16w if self.f16 else lib.tbe_backward_indice_weights_f32
        _lib.check(fn(p(self.feat_weights), p(self.feat_D), p(self.out_offset), p(self.feat_rows), c.F, c.B, max(c.feat_D),
                      p(self.indices), c.N, p(self.offsets), int(pooling), p(self._opt[0]), p(self.grad),
                      int(c.grad.shape[1]), p(self._opt[1]), self.buf.data_ptr() + self.giw_off, p(self._opt[2]),
                      _lib.stream_ptr(torch.device("cuda", 0))), "tbe_backward_indice_weights")

    def poison(self):
        self.buf.copy_(_cu(self.host))  # giw holds guard bytes (a NaN pattern) again: every element has to be written

    def read(self):
        torch.cuda.synchronize()
        after = self.buf.cpu().numpy()
        lo, hi = self.giw_off, self.giw_off + 4 * self.case.N
        assert (after[:lo] == self.host[:lo]).all() and (after[hi:] == self.host[hi:]).all(), \
            "a guard byte or a table changed"
        return after[lo:hi].view(np.float32).copy()

    def run(self, **kw):
        self.poison()
        self.launch(**kw)
        return self.read()


def _exact(got, ref64):
    """Bit for bit: the float64 value is a float32 on the designed inputs under SUM, and under MEAN wherever the bag
    length is a power of two; for the bags of 100 and 1000 ids it is the exact dot divided once, whose float32 rounding
    is what one correctly rounded FP32 division gives (tests/_indice_weights_ref.py)."""
    assert got.dtype == np.float32
    np.testing.assert_array_equal((got + np.float32(0)).view(np.uint32), (ref64.astype(np.float32) + np.float32(0)).view(np.uint32))  # + 0: -0 -> +0
    assert np.count_nonzero(ref64) > ref64.size // 4  # the case says something


# ---- dispatch coverage on designed inputs -----------------------------------------------------------------------------
# name -> (dims, rows, ftm, tables whose base is 4 B off the 16-B grid)
SHAPES = {
    "D16": ([16], [50], None, ()), "D64": ([64], [50], None, ()), "D128": ([128], [50], None, ()),
    "D256": ([256], [50], None, ()), "D6_scalar": ([6], [50], None, ()), "D12_misaligned": ([12], [50], None, (0,)),
    "mixed_shared": ([16, 64, 128], [50, 7, 33], [0, 1, 2, 1], ()),
    # beyond D = 256 a lane holds NV = 2 .. 8 column blocks of a row: one dim per branch (sums stay below 2^13: still exact)
    "D320_nv2": ([320], [20], None, ()), "D520_nv4": ([520], [20], None, ()), "D1100_nv8": ([1100], [20], None, ()),
}


@functools.lru_cache(maxsize=None)
def _designed(shape, bags, B=67):
    dims, rows, ftm, misalign = SHAPES[shape]
    case = R.make_case(dims, rows, ftm=ftm, B=B, bags=bags, seed=11, bad_ids=B > 1)  # ids -1, rows and TBE_ID_SKIP included
    if bags == "long":
        assert case.N / (case.F * B) >= 4 and 1000 in np.diff(case.offsets) and 100 in np.diff(case.offsets)
    else:
        assert case.N / (case.F * B) < 3.5
    return case, Abi(case, misalign), R.reference(case)


@pytest.mark.parametrize("bags", ["short", "long"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sum_matches_reference_bit_for_bit(shape, bags):
    case, abi, ref = _designed(shape, bags)
    bad = (case.indices == -1) | (case.indices == R.ID_SKIP) | (case.indices == np.repeat(case.feat_rows, np.diff(case.offsets[::case.B])))
    assert bad.sum() >= 3 * case.F
    got = abi.run()
    _exact(got, ref)
    assert (got[bad] == 0).all()


@pytest.mark.parametrize("bags", ["short", "long"])
def test_mean_and_per_feature_pooling(bags):
    case, abi, ref_sum = _designed("mixed_shared", bags)
    ref_mean = R.reference(case, pooling=R.MEAN)
    assert (ref_mean != ref_sum).any()
    _exact(abi.run(pooling=R.MEAN), ref_mean)
    mix = [R.MEAN, R.SUM, R.SUM, R.MEAN]
    ref_mix = R.reference(case, pooling=R.MEAN, feat_pooling=mix)
    assert (ref_mix != ref_mean).any() and (ref_mix != ref_sum).any()
    _exact(abi.run(pooling=R.MEAN, feat_pooling=mix), ref_mix)
    _exact(abi.run(pooling=R.SUM, feat_pooling=mix), ref_sum)  # feat_pooling counts only under MEAN, as in the forward


@pytest.mark.parametrize("bags", ["short", "long"])
def test_batch_of_one(bags):
    case, abi, ref = _designed("mixed_shared", bags, B=1)
    _exact(abi.run(), ref)
    _exact(abi.run(pooling=R.MEAN), R.reference(case, pooling=R.MEAN))


@pytest.mark.parametrize("bags", ["short", "long"])
def test_feature_requires_grad_masks_one_feature(bags):
    case, abi, ref = _designed("mixed_shared", bags)
    mask = [1, 0, 1, 1]
    got = abi.run(feat_requires_grad=mask)
    _exact(got, R.reference(case, feat_requires_grad=mask))
    lo, hi = case.offsets[case.B], case.offsets[2 * case.B]
    assert hi > lo and (got[lo:hi] == 0).all() and (ref[lo:hi] != 0).any()


@pytest.mark.parametrize("bags", ["short", "long"])
def test_row_window_keeps_the_middle_third(bags):
    full = R.make_case([64, 16], [60, 30], B=67, bags=bags, seed=5)
    windows = [(20, 60), (10, 30)]  # (first global row held, global rows)
    shard = R.Case([full.tables[0][20:40], full.tables[1][10:20]], full.ftm, full.B, full.indices, full.offsets, full.grad)
    ref = R.reference(shard, feat_window=windows)
    outside = np.concatenate([(ids < lo) | (ids >= lo + n) for ids, lo, n in (
        (full.indices[:full.offsets[full.B]], 20, 20), (full.indices[full.offsets[full.B]:], 10, 10))])
    assert outside.sum() > full.N // 2 and (~outside).sum() > full.N // 5
    got = Abi(shard).run(feat_window=windows)
    _exact(got, ref)
    assert (got[outside] == 0).all()


@pytest.mark.parametrize("bags", ["short", "long"])
def test_malformed_bags_give_zero_and_touch_nothing(bags):
    good = R.make_case([64, 64], [40, 40], B=67, bags=bags, seed=9)
    offsets, lengths = good.offsets.copy(), np.diff(good.offsets)

    def two_full_bags(f):  # the offsets entry between two non-empty bags of feature f
        return next(f * 67 + k for k in range(1, 66) if lengths[f * 67 + k - 1] > 0 and lengths[f * 67 + k] > 0)

    offsets[two_full_bags(0)] = -2  # the bag before it: start > end; the bag after it: start < 0
    offsets[two_full_bags(1)] = good.N + 5  # the bag before it: end > N; the bag after it: start > end
    case = R.Case(good.tables, good.ftm, good.B, good.indices, offsets, good.grad)
    ref = R.reference(case)
    lost = (ref == 0) & (R.reference(good) != 0)
    assert lost.sum() >= 4
    _exact(Abi(case).run(), ref)
    _exact(Abi(case).run(pooling=R.MEAN), R.reference(case, pooling=R.MEAN))


# ---- FP16 tables, random values, graphs -------------------------------------------------------------------------------
@pytest.mark.parametrize("bags", ["short", "long"])
@pytest.mark.parametrize("D", [8, 128, 6])
def test_f16w_equals_f32_on_the_upcast_twin(D, bags):
    half = R.make_case([D, D], [50, 20], B=67, bags=bags, seed=D, dtype=np.float16, designed=False, bad_ids=True)
    twin = R.Case([w.astype(np.float32) for w in half.tables], half.ftm, half.B, half.indices, half.offsets, half.grad)
    for kw in ({}, {"pooling": R.MEAN}):
        a, b = Abi(half).run(**kw), Abi(twin).run(**kw)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.count_nonzero(a) > a.size // 2


@pytest.mark.parametrize("bags", ["short", "long"])
def test_random_values_deterministic_and_within_the_dot_product_bound(bags):
    D = 128
    case = R.make_case([D, D], [300, 50], B=67, bags=bags, seed=21, designed=False)
    abi = Abi(case)
    first, second = abi.run(), abi.run()
    np.testing.assert_array_equal(first.view(np.uint32), second.view(np.uint32))
    ref = R.reference(case)
    # |fl(x . y) - x . y| <= gamma_D * sum |x_d y_d| for any order, with or without fma; gamma_D ~ D * 2^-24, doubled
    bound = D * 2.0 ** -23 * R.abs_dot(case)
    err = np.abs(first.astype(np.float64) - ref)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert np.count_nonzero(ref) == case.N


@pytest.mark.parametrize("bags", ["short", "long"])
def test_graph_capture_and_replay(bags):
    case, abi, ref = _designed("mixed_shared", bags)
    eager = abi.run(pooling=R.MEAN)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        abi.launch(pooling=R.MEAN)
    for _ in range(2):
        abi.poison()
        graph.replay()
        np.testing.assert_array_equal(abi.read().view(np.uint32), eager.view(np.uint32))


# ---- modules ----------------------------------------------------------------------------------------------------------
def _fused(case, locations=None, fp16=False, **kw):
    from fbgemm_gpu.split_embedding_configs import EmbOptimType, SparseType
    from fbgemm_gpu.split_table_batched_embeddings_ops import (
        ComputeDevice, EmbeddingLocation, SplitTableBatchedEmbeddingBagsCodegen)

    locations = locations or [EmbeddingLocation.DEVICE] * len(case.tables)
    mod = SplitTableBatchedEmbeddingBagsCodegen(
        [(w.shape[0], w.shape[1], loc, ComputeDevice.CUDA) for w, loc in zip(case.tables, locations)],
        feature_table_map=case.ftm, device=torch.device("cuda", 0), optimizer=EmbOptimType.EXACT_SGD, learning_rate=1.0,
        weights_precision=SparseType.FP16 if fp16 else SparseType.FP32, stochastic_rounding=False, **kw)
    for w, init in zip(mod.split_embedding_weights(), case.tables):
        w.copy_(torch.from_numpy(init))
    return mod


def _tables_of(mod):
    torch.cuda.synchronize()
    return [w.cpu().numpy().copy() for w in mod.split_embedding_weights()]


@functools.lru_cache(maxsize=None)
def _module_case(fp16=False):
    case = R.make_case([16, 64, 128], [50, 7, 33], ftm=[0, 1, 2, 1], B=67, bags="short", seed=2,
                       dtype=np.float16 if fp16 else np.float32)
    psw = R.designed_weights(np.random.default_rng(1), case.N)
    return case, psw, R.reference(case)


def _lookup(mod, case, weights, variant):
    if variant == "forward_into":
        stride = int(case.grad.shape[1]) + 4
        out = torch.zeros(case.B, stride, device="cuda")
        return mod.forward_into(out, _cu(case.out_offset + 4), stride, _cu(case.indices), _cu(case.offsets), weights)
    return mod(_cu(case.indices), _cu(case.offsets), weights)


def _grad_for(case, variant):
    if variant == "forward_into":
        return torch.cat([torch.zeros(case.B, 4), torch.tensor(case.grad)], dim=1).cuda()
    return _cu(case.grad)


@pytest.mark.parametrize("variant", ["forward", "forward_into", "fp16"])
def test_fused_module_weight_gradient_reads_the_tables_before_the_update(variant):
    case, psw, ref = _module_case(variant == "fp16")
    trained, detached = _fused(case, fp16=variant == "fp16"), _fused(case, fp16=variant == "fp16")
    w = _cu(psw).requires_grad_(True)
    _lookup(trained, case, w, variant).backward(_grad_for(case, variant))
    _lookup(detached, case, _cu(psw), variant).backward(_grad_for(case, variant))
    assert w.grad is not None and w.grad.shape == (case.N,)
    _exact(w.grad.cpu().numpy(), ref)
    after = _tables_of(trained)
    for a, b, init in zip(after, _tables_of(detached), case.tables):
        np.testing.assert_array_equal(a, b)  # the extra kernel changes nothing about the step
        assert (a != init).any()
    # had the kernel run after the update it would have read these tables: the step (lr = 1, integer gradients, weights
    # in {0.5, 1, 2}) moves touched rows by multiples of 1/2, so that result differs by >= 1/8 wherever it differs
    late = R.reference(case, tables=after)
    assert np.abs(late - ref).max() >= 0.125


def test_fused_module_feature_requires_grad_and_no_extra_work_without_it():
    case, psw, ref = _module_case()
    mod = _fused(case)
    w = _cu(psw).requires_grad_(True)
    mask = torch.tensor([1, 0, 1, 1])
    mod(_cu(case.indices), _cu(case.offsets), w, feature_requires_grad=mask.cuda()).backward(_cu(case.grad))
    _exact(w.grad.cpu().numpy(), R.reference(case, feat_requires_grad=mask.tolist()))
    calls = []
    mod._indice_weights_grad = lambda *a, **k: calls.append(a)  # weights that do not require grad: no launch, no allocation
    mod(_cu(case.indices), _cu(case.offsets), _cu(psw)).backward(_cu(case.grad))
    assert calls == []


def test_cached_table_matches_the_uncached_module():
    from fbgemm_gpu.split_table_batched_embeddings_ops import EmbeddingLocation as L

    case, psw, ref = _module_case()
    cached = _fused(case, locations=[L.DEVICE, L.MANAGED_CACHING, L.DEVICE], cache_sets=1)
    plain = _fused(case)
    assert cached._cache is not None
    grads = []
    for mod in (cached, plain):
        w = _cu(psw).requires_grad_(True)
        mod(_cu(case.indices), _cu(case.offsets), w).backward(_cu(case.grad))
        grads.append(w.grad.cpu().numpy())
    np.testing.assert_array_equal(grads[0].view(np.uint32), grads[1].view(np.uint32))
    _exact(grads[0], ref)
    for a, b in zip(_tables_of(cached), _tables_of(plain)):
        np.testing.assert_array_equal(a, b)


def test_dense_module_gives_both_gradients_from_one_backward():
    from fbgemm_gpu.split_table_batched_embeddings_ops import DenseTableBatchedEmbeddingBagsCodegen

    case, psw, ref = _module_case()
    mod = DenseTableBatchedEmbeddingBagsCodegen([w.shape for w in case.tables], feature_table_map=case.ftm).cuda()
    for w, init in zip(mod.split_embedding_weights(), case.tables):
        w.copy_(torch.from_numpy(init))
    mod(_cu(case.indices), _cu(case.offsets), _cu(psw)).backward(_cu(case.grad))
    table_grad = mod.weights.grad.clone()
    mod.weights.grad = None
    w = _cu(psw).requires_grad_(True)
    mod(_cu(case.indices), _cu(case.offsets), w).backward(_cu(case.grad))
    _exact(w.grad.cpu().numpy(), ref)
    assert torch.equal(mod.weights.grad, table_grad) and table_grad.abs().sum() > 0
    # forward_into: the same two gradients
    mod.weights.grad = None
    w2 = _cu(psw).requires_grad_(True)
    _lookup(mod, case, w2, "forward_into").backward(_grad_for(case, "forward_into"))
    _exact(w2.grad.cpu().numpy(), ref)
    assert torch.equal(mod.weights.grad, table_grad)


def test_explicit_path_matches_autograd():
    case, psw, ref = _module_case()
    mod, twin = _fused(case), _fused(case)
    out, rec = mod.lookup_no_autograd(_cu(case.indices), _cu(case.offsets), _cu(psw))
    giw = mod.indice_weights_grad(rec, _cu(case.grad))  # before the update of the same record
    mod.backward_no_autograd(rec, _cu(case.grad))
    _exact(giw.cpu().numpy(), ref)
    twin(_cu(case.indices), _cu(case.offsets), _cu(psw)).backward(_cu(case.grad))
    for a, b in zip(_tables_of(mod), _tables_of(twin)):
        np.testing.assert_array_equal(a, b)
    _, unweighted = mod.lookup_no_autograd(_cu(case.indices), _cu(case.offsets))
    with pytest.raises(RuntimeError, match="per_sample_weights"):
        mod.indice_weights_grad(unweighted, _cu(case.grad))
    mod.backward_no_autograd(unweighted, _cu(case.grad))  # the record owes one backward


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_order", ["table_order", "reversed"])
def test_position_weights_train_through_a_weighted_collection(key_order):
    from torchrec_amd.modules import PositionWeightedModule
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    dims, rows, B, max_len = [16, 64], [40, 25], 67, 4
    case = R.make_case(dims, rows, B=B, bags="short", seed=4)
    names = ["fa", "fb"]
    dev = torch.device("cuda", 0)
    ebc = EmbeddingBagCollection(
        [EmbeddingBagConfig(name=f"t_{n}", embedding_dim=d, num_embeddings=r, feature_names=[n])
         for n, d, r in zip(names, dims, rows)], is_weighted=True, device=dev)
    for n, init in zip(names, case.tables):
        ebc.table_weights()[f"t_{n}"].copy_(torch.from_numpy(init))
    pw = PositionWeightedModule({n: max_len for n in names}).to(dev)
    init_pw = {n: R.designed_weights(np.random.default_rng(i), max_len) for i, n in enumerate(names)}
    with torch.no_grad():
        for n in names:
            pw.position_weights[n].copy_(torch.from_numpy(init_pw[n]))
    keys = names if key_order == "table_order" else names[::-1]
    opk = case.offsets[::B]
    per_key = {n: (case.indices[opk[f]:opk[f + 1]], np.diff(case.offsets[f * B:(f + 1) * B + 1])) for f, n in enumerate(names)}
    features = KeyedJaggedTensor.from_lengths_sync(
        keys, _cu(np.concatenate([per_key[k][0] for k in keys])),
        _cu(np.concatenate([per_key[k][1] for k in keys]), torch.int32)).to_dict()
    weighted = pw(features)
    kjt = KeyedJaggedTensor.from_lengths_sync(
        keys, torch.cat([weighted[k].values() for k in keys]), torch.cat([weighted[k].lengths() for k in keys]),
        weights=torch.cat([weighted[k].weights() for k in keys]))
    out = ebc(kjt)
    assert out.keys() == names
    # forward: the weighted pooled sum, exact on these inputs
    pos = np.concatenate([np.arange(n) for n in np.diff(case.offsets)])
    psw = np.concatenate([init_pw[n][pos[opk[f]:opk[f + 1]]] for f, n in enumerate(names)])
    expect = np.zeros((B, sum(dims)))
    for f in range(2):
        for b in range(B):
            for i in range(case.offsets[f * B + b], case.offsets[f * B + b + 1]):
                expect[b, case.out_offset[f]:case.out_offset[f] + dims[f]] += psw[i] * case.tables[f][case.indices[i]].astype(np.float64)
    np.testing.assert_array_equal(out.values().detach().cpu().numpy().astype(np.float64), expect)
    (out.values() * _cu(case.grad)).sum().backward()
    giw = R.reference(case)
    for f, n in enumerate(names):
        grad = pw.position_weights[n].grad
        assert grad is not None, "the position weights received no gradient"
        ref = np.zeros(max_len)
        np.add.at(ref, pos[opk[f]:opk[f + 1]], giw[opk[f]:opk[f + 1]])
        assert np.count_nonzero(ref) == max_len
        np.testing.assert_array_equal(grad.cpu().numpy().astype(np.float64), ref)
