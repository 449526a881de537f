"""Pooling-factor-1 lookup fused into the dot interaction (csrc/dlrm_interaction.hip gather kernels,
models/dlrm.py _FusedGatherInteraction): bit-identical to the lookup + interaction pair and to the oracle, same id
semantics, same training trajectory, and every configuration it does not cover still takes the two-kernel path."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
from oracle import oracle

pytestmark = pytest.mark.gpu

ID_SKIP = -(1 << 63)  # TBE_ID_SKIP
SHAPES = [(1, 26, 128), (3, 1, 64), (17, 7, 128), (257, 26, 128), (4099, 27, 128), (8192, 26, 128), (2600, 5, 64)]
ROW_MIX = [1, 3, 1000, 200000]  # some rows repeat thousands of times within a batch
# The gather kernels share the dense ones' second row tile (on from R = F + 1 = 17) and the forward's counted wait for the
# next sample's copy (T = ceil(P / 64) pair stores; it matters once a wave loops, B > 2048, on unaligned rows).  R = 16 and
# 17 with three trips per wave run on the 16-B store path, which waits for everything: P = 120 and 136 are multiples of 4,
# so the row strides 248 and 200 are those of 16-B rows, padded or not.  The counted wait loops at T = 2
# and 4 (F = 11 and 20 on rows of D + P; the shapes above reach 1 and 6); R = 17 with fewer samples than waves.  The
# counted wait at R = 16 | 17 and the other row layouts: tests/test_gather_interaction_abi_gpu.py.
EDGE_SHAPES = [(4101, 15, 128), (4101, 16, 64), (4101, 11, 128), (4101, 20, 64), (5, 16, 128)]
SHAPES += EDGE_SHAPES
SMALL_ROW_MIX = [1, 3, 1000, 5000]  # for EDGE_SHAPES: the tables, which the oracle test copies to the host, stay small


def _lib():
    from fbgemm_gpu import _lib

    return _lib.load()


def _check(rc, what):
    assert rc == 0, f"{what}: rc={rc} {_lib().tbe_last_error()}"


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """Random tables in one flat device buffer + the feat_* arrays the kernels take + one id per (feature, sample)."""

    def __init__(self, B, F, D, seed=0, rows=None, window=None):
        g = torch.Generator(device="cuda").manual_seed(seed * 7919 + B * 31 + F * 7 + D)
        self.B, self.F, self.D = B, F, D
        self.rows = list(rows) if rows is not None else [ROW_MIX[f % 4] for f in range(F)]
        starts = np.concatenate([[0], np.cumsum([r * D for r in self.rows])])
        self.flat = torch.randn(int(starts[-1]), generator=g, device="cuda")
        self.tables = [self.flat[int(starts[f]):int(starts[f + 1])].view(self.rows[f], D) for f in range(F)]
        self.feat_weights = torch.tensor([t.data_ptr() for t in self.tables], dtype=torch.int64).cuda()
        self.feat_rows = torch.tensor(self.rows, dtype=torch.int64).cuda()
        self.feat_D = torch.full((F,), D, dtype=torch.int32).cuda()
        self.feat_out_offset = (torch.arange(F, dtype=torch.int64) * D).cuda()
        self.feat_window = None
        hi = self.rows
        if window is not None:  # (first global row, global rows) per feature
            self.feat_window = torch.tensor([x for pair in window for x in pair], dtype=torch.int64).cuda()
            hi = [w[1] for w in window]
        cpu = torch.Generator().manual_seed(seed + B + F)
        self.ids = torch.cat([torch.randint(0, hi[f], (B,), generator=cpu) for f in range(F)]).to(torch.int64)
        self.dense = torch.randn(B, D, generator=g, device="cuda")
        self.width = D + (F + 1) * F // 2
        self.grad = torch.randn(B, self.width, generator=g, device="cuda")

    def stride(self, pad):
        return (self.D + ((self.F + 1) * self.F // 2 + 3) // 4 * 4) if pad else self.width

    def unfused(self, pad, ids=None):
        """tbe_forward_pooled_f32 + tbe_dlrm_interaction_{forward,backward}_f32 -> (out, grad_dense, grad_sparse, errors)"""
        lib, B, F, D = _lib(), self.B, self.F, self.D
        ids = (self.ids if ids is None else ids).cuda()
        offsets = torch.arange(F * B + 1, dtype=torch.int64, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        pooled = torch.full((B, F * D), float("nan"), device="cuda")
        win = self.feat_window.data_ptr() if self.feat_window is not None else None
        _check(lib.tbe_forward_pooled_f32(self.feat_weights.data_ptr(), self.feat_D.data_ptr(), self.feat_out_offset.data_ptr(),
                                          self.feat_rows.data_ptr(), F, B, D, ids.data_ptr(), F * B, offsets.data_ptr(), None, 0,
                                          None, pooled.data_ptr(), F * D, err.data_ptr(), win, _stream()), "forward_pooled")
        S = self.stride(pad)
        out = torch.full((B, S), float("nan"), device="cuda")
        _check(lib.tbe_dlrm_interaction_forward_f32(self.dense.data_ptr(), pooled.data_ptr(), B, F, D, out.data_ptr(), S,
                                                    _stream()), "interaction_forward")
        gbuf = torch.full((B, S), float("nan"), device="cuda")
        gbuf[:, :self.width] = self.grad
        gd = torch.full((B, D), float("nan"), device="cuda")
        gs = torch.full((B, F * D), float("nan"), device="cuda")
        _check(lib.tbe_dlrm_interaction_backward_f32(self.dense.data_ptr(), pooled.data_ptr(), gbuf.data_ptr(), S, B, F, D,
                                                     gd.data_ptr(), gs.data_ptr(), _stream()), "interaction_backward")
        torch.cuda.synchronize()
        return out, gd, gs, int(err.item())

    def fused(self, pad, ids=None):
        """tbe_dlrm_interaction_gather_{forward,backward}_f32 -> (out, grad_dense, grad_sparse, errors)"""
        lib, B, F, D = _lib(), self.B, self.F, self.D
        ids = (self.ids if ids is None else ids).cuda()
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        win = self.feat_window.data_ptr() if self.feat_window is not None else None
        S = self.stride(pad)
        out = torch.full((B, S), float("nan"), device="cuda")
        _check(lib.tbe_dlrm_interaction_gather_forward_f32(self.dense.data_ptr(), self.feat_weights.data_ptr(),
                                                           self.feat_rows.data_ptr(), win, ids.data_ptr(), B, F, D,
                                                           out.data_ptr(), S, err.data_ptr(), _stream()), "gather_forward")
        gbuf = torch.full((B, S), float("nan"), device="cuda")
        gbuf[:, :self.width] = self.grad
        gd = torch.full((B, D), float("nan"), device="cuda")
        gs = torch.full((B, F * D), float("nan"), device="cuda")
        # the backward gathers the same ids again and takes NO counter: an id is counted once
        _check(lib.tbe_dlrm_interaction_gather_backward_f32(self.dense.data_ptr(), self.feat_weights.data_ptr(),
                                                            self.feat_rows.data_ptr(), win, ids.data_ptr(), gbuf.data_ptr(), S,
                                                            B, F, D, gd.data_ptr(), gs.data_ptr(), None, _stream()),
               "gather_backward")
        torch.cuda.synchronize()
        return out, gd, gs, int(err.item())


def _shape_case(B, F, D):
    """The Case of a SHAPES entry."""
    rows = [SMALL_ROW_MIX[f % 4] for f in range(F)] if (B, F, D) in EDGE_SHAPES else None
    return Case(B, F, D, rows=rows)


def _assert_same(a, b, width):
    (out_a, gd_a, gs_a, _), (out_b, gd_b, gs_b, _) = a, b
    assert torch.equal(out_a, out_b)  # pad columns included: both write them as zeros
    assert not torch.isnan(out_a[:, :width]).any()
    assert torch.equal(gd_a, gd_b) and torch.equal(gs_a, gs_b)
    assert not torch.isnan(gd_a).any() and not torch.isnan(gs_a).any()


@pytest.mark.parametrize("pad", [False, True], ids=["dense_rows", "padded_rows"])
@pytest.mark.parametrize("B,F,D", SHAPES)
def test_gather_kernels_bitwise_equal_to_the_unfused_pair(B, F, D, pad):
    c = _shape_case(B, F, D)
    _assert_same(c.fused(pad), c.unfused(pad), c.width)


@pytest.mark.parametrize("pad", [False, True], ids=["dense_rows", "padded_rows"])
@pytest.mark.parametrize("B,F,D", SHAPES)
def test_gather_kernels_bitwise_equal_to_the_oracle(B, F, D, pad):
    """oracle.tbe_forward composed with oracle.interaction_forward / interaction_backward on the same inputs."""
    c = _shape_case(B, F, D)
    tabs = oracle.Tables(c.rows, [D] * F)
    tabs.weights = [np.ascontiguousarray(t.cpu().numpy()) for t in c.tables]
    pooled, bad = oracle.tbe_forward(tabs, c.ids.numpy(), np.arange(F * B + 1, dtype=np.int64))
    assert bad == 0
    dense, sparse = c.dense.cpu().numpy(), pooled.reshape(B, F, D)
    out, gd, gs, err = c.fused(pad)
    assert err == 0
    np.testing.assert_array_equal(out[:, :c.width].cpu().numpy(), oracle.interaction_forward(dense, sparse))
    ogd, ogs = oracle.interaction_backward(dense, sparse, c.grad.cpu().numpy())
    np.testing.assert_array_equal(gd.cpu().numpy(), ogd)
    np.testing.assert_array_equal(gs.view(B, F, D).cpu().numpy(), ogs)


def test_out_of_range_and_skipped_ids_give_zero_rows_and_are_counted_once():
    c = Case(300, 7, 128)
    ids = c.ids.clone().view(c.F, c.B)
    bad = [(0, 5, -1), (1, 17, 3), (2, 0, 1000), (3, 299, 1 << 40), (6, 100, (1 << 63) - 1), (2, 64, -77)]
    for f, b, v in bad:
        ids[f, b] = v
    for f, b in [(0, 9), (4, 250), (5, 0)]:
        ids[f, b] = ID_SKIP  # silently skipped: a zero row, no count
    ids = ids.view(-1)
    for pad in (False, True):
        fused, unfused = c.fused(pad, ids), c.unfused(pad, ids)
        _assert_same(fused, unfused, c.width)
        assert fused[3] == unfused[3] == len(bad)
    # the rows of the bad and skipped ids really are zeros: their gradient is the interaction with the other rows only,
    # and the products with them are zero
    out = c.fused(False, ids)[0]
    R = c.F + 1
    iu = torch.triu_indices(R, R, offset=1)
    for f, b, _ in bad:
        cols = [p for p in range(iu.shape[1]) if f + 1 in (int(iu[0, p]), int(iu[1, p]))]
        assert float(out[b, c.D + torch.tensor(cols)].abs().max()) == 0.0


def test_module_counter_matches_the_unfused_lookup():
    """SplitTableBatchedEmbeddingBagsCodegen.bounds_check_errors() after a deferred lookup consumed by the gather kernels
    (forward with the module's counter, backward with none) equals what the module's own forward reports."""
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from fbgemm_gpu.split_table_batched_embeddings_ops import (
        ComputeDevice, EmbeddingLocation, SplitTableBatchedEmbeddingBagsCodegen)

    rows, D, B = [50, 3, 1000], 64, 130
    F = len(rows)

    def module():
        return SplitTableBatchedEmbeddingBagsCodegen(
            [(r, D, EmbeddingLocation.DEVICE, ComputeDevice.CUDA) for r in rows], device=torch.device("cuda", 0),
            optimizer=EmbOptimType.EXACT_SGD, learning_rate=0.1)

    ids = torch.cat([torch.randint(0, r, (B,)) for r in rows]).to(torch.int64)
    ids[3], ids[B + 7], ids[2 * B + 129], ids[5] = -5, 3, 1000, ID_SKIP
    ids = ids.cuda()
    offsets = torch.arange(F * B + 1, dtype=torch.int64, device="cuda")
    plain, fused = module(), module()
    g = torch.Generator(device="cuda").manual_seed(2)
    for wp, wf in zip(plain.split_embedding_weights(), fused.split_embedding_weights()):
        wp.copy_(torch.randn(wp.shape, generator=g, device="cuda"))
        wf.copy_(wp)
    with torch.no_grad():
        pooled = plain(ids, offsets)
        rec = fused.lookup_deferred(ids, offsets)
    fw, fr, win = fused.gather_layout()
    assert win is None
    dense = torch.randn(B, D, device="cuda")
    width = D + (F + 1) * F // 2
    out, gd, gs = torch.empty(B, width, device="cuda"), torch.empty(B, D, device="cuda"), torch.empty(B, F * D, device="cuda")
    lib = _lib()
    _check(lib.tbe_dlrm_interaction_gather_forward_f32(dense.data_ptr(), fw.data_ptr(), fr.data_ptr(), None,
                                                       rec.indices.data_ptr(), B, F, D, out.data_ptr(), width,
                                                       fused._errors_ptr(), _stream()), "gather_forward")
    grad = torch.randn(B, width, device="cuda")
    _check(lib.tbe_dlrm_interaction_gather_backward_f32(dense.data_ptr(), fw.data_ptr(), fr.data_ptr(), None,
                                                        rec.indices.data_ptr(), grad.data_ptr(), width, B, F, D,
                                                        gd.data_ptr(), gs.data_ptr(), None, _stream()), "gather_backward")
    assert fused.bounds_check_errors() == plain.bounds_check_errors() == 3
    ref = torch.empty(B, width, device="cuda")
    _check(lib.tbe_dlrm_interaction_forward_f32(dense.data_ptr(), pooled.data_ptr(), B, F, D, ref.data_ptr(), width, _stream()),
           "interaction_forward")
    assert torch.equal(out, ref)


def test_row_windows_skip_foreign_rows_silently():
    """Row-wise shard semantics: ids are global rows; those outside the shard's window give a zero row without a count,
    those outside the table are counted."""
    F, D, B = 5, 128, 700
    rows = [1000, 40, 3, 500, 1]
    window = [(500, 3000), (0, 40), (6, 10), (1500, 2000), (0, 1)]
    c = Case(B, F, D, rows=rows, window=window)
    ids = c.ids.clone().view(F, B)
    ids[0, 1], ids[2, 2], ids[3, 3], ids[4, 4] = 3000, -1, 2000, ID_SKIP  # three outside their tables, one skipped
    ids = ids.view(-1)
    local = ((ids.view(F, B) - torch.tensor([w[0] for w in window]).view(F, 1)) >= 0) & \
            ((ids.view(F, B) - torch.tensor([w[0] for w in window]).view(F, 1)) < torch.tensor(rows).view(F, 1))
    assert 0 < int(local[0].sum()) < B  # the case does mix local and foreign rows
    for pad in (False, True):
        fused, unfused = c.fused(pad, ids), c.unfused(pad, ids)
        _assert_same(fused, unfused, c.width)
        assert fused[3] == unfused[3] == 3


# ---- model level -----------------------------------------------------------------------------------------------------
def _train(fused_lookup, steps=5, B=4096, row_cap=20000):
    """DLRMTrain under TrainPipelineSparseDist (eager: no HIP graphs) on Criteo's 26 tables with capped rows."""
    from torchrec_amd.datasets.random import CRITEO_1TB_ROWS, DEFAULT_CAT_NAMES, INT_FEATURE_COUNT, RandomRecDataset
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.train_pipeline import TrainPipelineSparseDist
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.models.dlrm import DLRMTrain
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.optim.keyed import CombinedOptimizer, KeyedOptimizerWrapper

    dev = torch.device("cuda", 0)
    D, lr = 128, 0.05
    rows = [min(r, row_cap) for r in CRITEO_1TB_ROWS]
    torch.manual_seed(11)
    tables = [EmbeddingBagConfig(name=f"t_{n}", embedding_dim=D, num_embeddings=rows[i], feature_names=[n])
              for i, n in enumerate(DEFAULT_CAT_NAMES)]
    ebc = EmbeddingBagCollection(tables=tables, device=torch.device("meta"))
    train_model = DLRMTrain(ebc, INT_FEATURE_COUNT, [512, 256, D], [1024, 1024, 512, 256, 1], dense_device=dev)
    model = DistributedModelParallel(train_model, env=ShardingEnv.from_local(1, 0), device=dev,
                                     sharders=[EmbeddingBagCollectionSharder({"learning_rate": lr})])
    shard = model.sharded_modules()[0]
    shard.reset_parameters_sharding_invariant(3)
    train_model.model.fused_lookup = fused_lookup
    opt = CombinedOptimizer([model.fused_optimizer,
                             KeyedOptimizerWrapper(dict(model.named_parameters()), lambda p: torch.optim.SGD(p, lr=lr))])
    data = RandomRecDataset(DEFAULT_CAT_NAMES, B, rows, manual_seed=5, num_generated_batches=steps + 1,
                            num_batches=steps + 1, device=dev)
    pipe = TrainPipelineSparseDist(model, opt, dev)
    model.train()
    it = iter(data)
    trace = []
    for _ in range(steps):
        loss, logits, _ = pipe.progress(it)
        trace.append((loss.clone(), logits.clone()))
    torch.cuda.synchronize()
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    tabs = {k: w.clone() for k, (w, _) in shard.local_shards().items()}
    assert shard._emb_module.bounds_check_errors() == 0
    return trace, params, tabs, train_model.model.fused_lookup_steps


def _assert_runs_equal(a, b):
    for (la, ga), (lb, gb) in zip(a[0], b[0]):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert a[1].keys() == b[1].keys() and a[2].keys() == b[2].keys() and len(a[2]) == 26
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_training_is_bitwise_the_same_with_the_lookup_fused():
    off1, off2 = _train(False), _train(False)
    assert off1[3] == off2[3] == 0
    _assert_runs_equal(off1, off2)  # the two-kernel path reproduces itself: the comparison below means something
    on = _train(True)
    assert on[3] == 5  # the gather path served every step
    _assert_runs_equal(on, off1)


def _small_dlrm(fused_lookup, D=64, pooling=None, weighted=False, cached=False, dims=None):
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.distributed.planner import EmbeddingShardingPlanner, ParameterConstraints, Topology
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.models.dlrm import DLRM
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig, PoolingType
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    dev = torch.device("cuda", 0)
    rows = [3000, 50, 700]
    keys = [f"f{i}" for i in range(3)]
    dims = dims or [D] * 3
    tables = [EmbeddingBagConfig(name=f"t{i}", embedding_dim=dims[i], num_embeddings=rows[i], feature_names=[keys[i]],
                                 pooling=pooling or PoolingType.SUM) for i in range(3)]
    cons = {"t0": ParameterConstraints(["table_wise"], ["batched_fused_uvm_caching"])} if cached else None
    plan = EmbeddingShardingPlanner(Topology(1), constraints=cons).plan_tables(tables)
    torch.manual_seed(4)
    sebc = ShardedEmbeddingBagCollection(EmbeddingBagCollection(tables, is_weighted=weighted, device=torch.device("meta")),
                                         plan, ShardingEnv.from_local(1, 0),
                                         {"learning_rate": 0.1, "optimizer": EmbOptimType.EXACT_SGD, "cache_sets": 2}, dev)
    sebc.reset_parameters_sharding_invariant(9)
    if len(set(dims)) != 1:
        return sebc, keys, rows
    model = DLRM(sebc, 13, [32, D], [16, 1], dense_device=dev)
    model.fused_lookup = fused_lookup
    return model, keys, rows


def _one_step(model, kjt, dense):
    logits = model(dense, kjt)
    logits.sum().backward()
    torch.cuda.synchronize()
    sebc = model.sparse_arch.embedding_bag_collection
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    return logits.detach().clone(), grads, {k: w.clone() for k, (w, _) in sebc.local_shards().items()}


def _kjt(keys, rows, B, L=1, weighted=False, seed=0):
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    g = torch.Generator().manual_seed(seed)
    vals = torch.cat([torch.randint(0, r, (B * L,), generator=g) for r in rows]).to(torch.int64).cuda()
    w = torch.rand(vals.numel(), generator=g).cuda() if weighted else None
    return KeyedJaggedTensor.from_fixed_lengths(keys, vals, [L] * len(keys), weights=w)


@pytest.mark.parametrize("case", ["eligible", "two_ids_per_bag", "per_sample_weights", "mean_pooling", "cached_table"])
def test_other_configurations_take_the_two_kernel_path_and_give_its_result(case):
    from torchrec_amd.modules.embedding_configs import PoolingType

    B = 96
    kw = {"per_sample_weights": {"weighted": True}, "mean_pooling": {"pooling": PoolingType.MEAN},
          "cached_table": {"cached": True}}.get(case, {})
    dense = torch.randn(B, 13, generator=torch.Generator().manual_seed(1)).cuda()
    results = []
    for fused_lookup in (True, False):
        model, keys, rows = _small_dlrm(fused_lookup, **kw)
        kjt = _kjt(keys, rows, B, L=2 if case == "two_ids_per_bag" else 1, weighted=case == "per_sample_weights")
        results.append(_one_step(model, kjt, dense))
        expected = 1 if (case == "eligible" and fused_lookup) else 0
        assert model.fused_lookup_steps == expected, case
    (la, ga, ta), (lb, gb, tb) = results
    assert torch.equal(la, lb)
    assert ga.keys() == gb.keys() and all(torch.equal(ga[k], gb[k]) for k in ga)
    assert ta.keys() == tb.keys() and all(torch.equal(ta[k], tb[k]) for k in ta)


def test_mixed_dims_are_not_served_by_the_gather_path():
    sebc, keys, rows = _small_dlrm(True, dims=[64, 128, 64])
    kjt = _kjt(keys, rows, 40)
    assert sebc.deferred_lookup_supported(kjt) is False
    out = sebc(kjt).wait().values()
    assert tuple(out.shape) == (40, 256)
    same, _, _ = _small_dlrm(True)
    assert same.sparse_arch.embedding_bag_collection.deferred_lookup_supported(kjt) is True
