"""GPU parity: HIP TBE forward / backward+fused optimizer (through the fbgemm_gpu module surface
and the C ABI) against the CPU oracle and the reference-generated golden vectors.

Tolerances: pooling factor 1 / duplicate-free cases are bit-exact; sums of several rows are
compared at the reference's own tolerance (torch.testing.assert_allclose fp32 defaults,
rtol 1.3e-6, atol 1e-5 — SURVEY.md §8c), scaled for long sums where stated."""
import glob
import os

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
from _util import build_pair, make_inputs, to_dev
from oracle import oracle

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL, ATOL = 1.3e-6, 1e-5


def _opt(name):
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    return getattr(EmbOptimType, name)


def run_fwd(mod, indices, offsets, psw):
    out = mod(to_dev(indices), to_dev(offsets), to_dev(psw))
    torch.cuda.synchronize()
    return out


EBC = sorted(glob.glob(os.path.join(GOLD, "ebc_*.npz")))


@pytest.mark.parametrize("path", EBC, ids=[os.path.basename(p) for p in EBC])
def test_golden_forward_backward_sgd(path):
    """HIP vs the REFERENCE's EmbeddingBagCollection + torch.optim.SGD (golden vectors)."""
    g = np.load(path)
    rows, dims = g["rows"].tolist(), g["dims"].tolist()
    pooling = 1 if str(g["pooling"]) == "mean" else 0
    mod, tabs = build_pair(rows, dims, None, pooling, learning_rate=float(g["lr"]))
    for t, w in enumerate(mod.split_embedding_weights()):
        w.copy_(torch.from_numpy(g[f"w_before_{t}"]))
    psw = g["weights"] if "weights" in g else None
    out = run_fwd(mod, g["values"], g["offsets"], psw)
    if "l1_sum" in path:
        np.testing.assert_array_equal(out.detach().cpu().numpy(), g["out"])
    else:
        np.testing.assert_allclose(out.detach().cpu().numpy(), g["out"], rtol=RTOL, atol=ATOL)
    out.backward(to_dev(g["grad_out"]))
    torch.cuda.synchronize()
    for t, w in enumerate(mod.split_embedding_weights()):
        np.testing.assert_allclose(w.cpu().numpy(), g[f"w_after_{t}"], rtol=RTOL, atol=ATOL)
    assert mod.bounds_check_errors() == 0


CASES = [
    # rows, dims, ftm, B, max_len, fixed_len, weighted, pooling
    dict(rows=[100, 7, 3000], dims=[128, 128, 128], ftm=None, B=300, max_len=1, fixed_len=1, weighted=False, pooling=0),
    dict(rows=[50, 9], dims=[64, 32], ftm=[0, 1, 0], B=65, max_len=5, fixed_len=None, weighted=False, pooling=0),
    dict(rows=[50, 9, 11], dims=[16, 256, 8], ftm=None, B=130, max_len=4, fixed_len=None, weighted=True, pooling=0),
    dict(rows=[33, 200], dims=[512, 40], ftm=None, B=70, max_len=3, fixed_len=None, weighted=False, pooling=1),
    dict(rows=[20, 15], dims=[1024, 12], ftm=None, B=19, max_len=2, fixed_len=None, weighted=True, pooling=1),
    dict(rows=[12, 40], dims=[7, 13], ftm=None, B=37, max_len=4, fixed_len=None, weighted=False, pooling=0),  # D % 4 != 0
    dict(rows=[64], dims=[2048], ftm=None, B=5, max_len=3, fixed_len=None, weighted=False, pooling=0),
    dict(rows=[500, 30], dims=[128, 64], ftm=None, B=33, max_len=60, fixed_len=None, weighted=False, pooling=0),  # long-bag kernel
    dict(rows=[500, 30], dims=[32, 256], ftm=None, B=17, max_len=70, fixed_len=None, weighted=True, pooling=1),  # long-bag, weighted mean
]


@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_forward_vs_oracle(case):
    rng = np.random.default_rng(11)
    mod, tabs = build_pair(case["rows"], case["dims"], case["ftm"], case["pooling"], rng=rng)
    indices, offsets, psw = make_inputs(rng, case["rows"], case["B"], case["max_len"], case["ftm"],
                                        case["fixed_len"], case["weighted"])
    out = run_fwd(mod, indices, offsets, psw).detach().cpu().numpy()
    ref, bad = oracle.tbe_forward(tabs, indices, offsets, psw, case["pooling"])
    assert bad == 0 and mod.bounds_check_errors() == 0
    long_bags = indices.size / max(1, (offsets.size - 1)) >= 3.5
    if case["fixed_len"] == 1 and not case["weighted"]:
        np.testing.assert_array_equal(out, ref)
    elif not long_bags:
        # same accumulation order as the oracle (sequential fmaf): bit-exact
        np.testing.assert_array_equal(out, ref)
    else:
        np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-4)  # different (fixed) association


OPTS = [
    ("EXACT_SGD", {}),
    ("EXACT_ROWWISE_ADAGRAD", dict(eps=1e-3)),
    ("EXACT_ROWWISE_ADAGRAD", dict(eps=1e-3, weight_decay=0.01, weight_decay_mode=1)),  # WeightDecayMode.L2
    ("EXACT_ADAGRAD", dict(eps=1e-3)),
    ("ADAM", dict(eps=1e-3, weight_decay=0.02)),
]


def _states(mod, tabs, code):
    s0 = s1 = None
    if code == oracle.OPT_EXACT_ROWWISE_ADAGRAD:
        s0 = [np.zeros(r, dtype=np.float32) for r in tabs.rows]
    elif code in (oracle.OPT_ADAM, oracle.OPT_EXACT_ADAGRAD):
        s0 = [np.zeros((r, d), dtype=np.float32) for r, d in zip(tabs.rows, tabs.dims)]
        if code == oracle.OPT_ADAM:
            s1 = [np.zeros((r, d), dtype=np.float32) for r, d in zip(tabs.rows, tabs.dims)]
    return s0, s1


@pytest.mark.parametrize("optname,kw", OPTS, ids=[f"{o[0]}{i}" for i, o in enumerate(OPTS)])
@pytest.mark.parametrize("case", CASES[:7], ids=[str(i) for i in range(7)])
def test_backward_fused_vs_oracle(case, optname, kw):
    rng = np.random.default_rng(5)
    code = {"EXACT_SGD": 0, "EXACT_ROWWISE_ADAGRAD": 1, "ADAM": 2, "EXACT_ADAGRAD": 3}[optname]
    lr = 0.05
    mod, tabs = build_pair(case["rows"], case["dims"], case["ftm"], case["pooling"], _opt(optname), rng,
                           learning_rate=lr, **kw)
    s0, s1 = _states(mod, tabs, code)
    for step in range(2):  # two steps so the optimizer state is exercised
        indices, offsets, psw = make_inputs(rng, case["rows"], case["B"], case["max_len"], case["ftm"],
                                            case["fixed_len"], case["weighted"])
        out = mod(to_dev(indices), to_dev(offsets), to_dev(psw))
        grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
        out.backward(to_dev(grad))
        torch.cuda.synchronize()
        oracle.tbe_backward(tabs, indices, offsets, grad, code, lr, psw, case["pooling"],
                            eps=kw.get("eps", 1e-8), weight_decay=kw.get("weight_decay", 0.0),
                            iteration=step + 1, state0=s0, state1=s1)
    for t, w in enumerate(mod.split_embedding_weights()):
        np.testing.assert_allclose(w.cpu().numpy(), tabs.weights[t], rtol=2e-5, atol=2e-5)
    states = mod.split_optimizer_states()
    for t in range(len(tabs.rows)):
        if s0 is not None:
            np.testing.assert_allclose(states[t][0].cpu().numpy(), s0[t], rtol=2e-5, atol=2e-5)
        if s1 is not None:
            np.testing.assert_allclose(states[t][1].cpu().numpy(), s1[t], rtol=2e-5, atol=2e-5)
        if code == 0:
            assert states[t] == ()


def test_backward_sgd_duplicate_free_is_bit_exact():
    """With unique ids every row gets one contribution: w' = fma(-lr, g, w) exactly."""
    rng = np.random.default_rng(2)
    rows, dims = [5000, 3000], [128, 128]
    B = 512
    mod, tabs = build_pair(rows, dims, None, 0, rng=rng, learning_rate=0.3)
    indices = np.concatenate([rng.permutation(rows[0])[:B], rng.permutation(rows[1])[:B]]).astype(np.int64)
    offsets = np.arange(2 * B + 1, dtype=np.int64)
    out = mod(to_dev(indices), to_dev(offsets))
    grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(to_dev(grad))
    torch.cuda.synchronize()
    oracle.tbe_backward(tabs, indices, offsets, grad, oracle.OPT_EXACT_SGD, 0.3)
    for t, w in enumerate(mod.split_embedding_weights()):
        np.testing.assert_array_equal(w.cpu().numpy(), tabs.weights[t])


def test_backward_heavy_duplicates_small_tables_and_determinism():
    """Criteo-like skew: tables with 3 / 4 / 10 rows receive B contributions each -> runs far
    longer than a chunk (fix-up path).  Also: two runs give bitwise identical weights."""
    rows, dims = [3, 4, 10, 100000], [128, 128, 128, 128]
    B = 4096
    results = []
    for rep in range(2):
        rng = np.random.default_rng(9)
        mod, tabs = build_pair(rows, dims, None, 0, rng=rng, learning_rate=0.01)
        indices, offsets, _ = make_inputs(rng, rows, B, 1, fixed_len=1)
        out = mod(to_dev(indices), to_dev(offsets))
        grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
        out.backward(to_dev(grad))
        torch.cuda.synchronize()
        results.append([w.cpu().numpy().copy() for w in mod.split_embedding_weights()])
        if rep == 0:
            oracle.tbe_backward(tabs, indices, offsets, grad, oracle.OPT_EXACT_SGD, 0.01)
            for t in range(len(rows)):
                # ~1400 addends per row for the tiny tables: tolerance scaled with sqrt(n)*eps
                np.testing.assert_allclose(results[0][t], tabs.weights[t], rtol=1e-4, atol=2e-4)
    for a, b in zip(*results):
        np.testing.assert_array_equal(a, b)


def test_dense_variant_gradient_vs_oracle():
    rng = np.random.default_rng(4)
    rows, dims, ftm = [40, 11], [64, 16], [0, 1, 1]
    mod, tabs = build_pair(rows, dims, ftm, 0, rng=rng, dense=True)
    indices, offsets, psw = make_inputs(rng, rows, 33, 4, ftm, weighted=True)
    out = mod(to_dev(indices), to_dev(offsets), to_dev(psw))
    grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(to_dev(grad))
    torch.cuda.synchronize()
    gw = [np.zeros((r, d), dtype=np.float32) for r, d in zip(rows, dims)]
    oracle.tbe_backward(tabs, indices, offsets, grad, oracle.OPT_DENSE_GRAD, 0.0, psw, 0, state0=gw)
    flat = mod.weights.grad.cpu().numpy()
    for t in range(len(rows)):
        o = mod.weights_offsets[t]
        np.testing.assert_allclose(flat[o:o + rows[t] * dims[t]].reshape(rows[t], dims[t]), gw[t], rtol=2e-5, atol=2e-5)


def test_nobag_forward_backward_vs_oracle():
    rng = np.random.default_rng(6)
    rows, dims, ftm = [30, 17], [64, 64], [0, 1, 0]
    mod, tabs = build_pair(rows, dims, ftm, 2, _opt("ADAM"), rng, learning_rate=0.01)
    indices, offsets, _ = make_inputs(rng, rows, 12, 5, ftm)
    out = mod(to_dev(indices), to_dev(offsets))
    ref, _ = oracle.tbe_forward(tabs, indices, offsets, None, oracle.POOL_NONE)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(to_dev(grad))
    torch.cuda.synchronize()
    s0 = [np.zeros((r, d), dtype=np.float32) for r, d in zip(rows, dims)]
    s1 = [np.zeros((r, d), dtype=np.float32) for r, d in zip(rows, dims)]
    oracle.tbe_backward(tabs, indices, offsets, grad, oracle.OPT_ADAM, 0.01, None, oracle.POOL_NONE,
                        state0=s0, state1=s1)
    for t, w in enumerate(mod.split_embedding_weights()):
        np.testing.assert_allclose(w.cpu().numpy(), tabs.weights[t], rtol=2e-5, atol=2e-5)


def test_out_of_range_indices_are_counted_and_contribute_zero():
    rng = np.random.default_rng(8)
    rows, dims = [10, 20], [32, 32]
    mod, tabs = build_pair(rows, dims, None, 0, rng=rng)
    B = 8
    indices = rng.integers(0, 10, size=2 * B).astype(np.int64)
    indices[3] = 10      # == rows -> invalid
    indices[B + 1] = -1  # negative -> invalid
    offsets = np.arange(2 * B + 1, dtype=np.int64)
    out = mod(to_dev(indices), to_dev(offsets))
    ref, bad = oracle.tbe_forward(tabs, indices, offsets)
    assert bad == 2
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    before = [w.clone() for w in mod.split_embedding_weights()]
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    oracle.tbe_backward(tabs, indices, offsets, np.ones(tuple(out.shape), np.float32), 0, 0.01)
    for t, w in enumerate(mod.split_embedding_weights()):
        np.testing.assert_allclose(w.cpu().numpy(), tabs.weights[t], rtol=2e-5, atol=2e-5)
    assert mod.bounds_check_errors() == 4  # 2 in forward + 2 in backward
    del before


def test_empty_batch_and_empty_bags():
    rows, dims = [10], [16]
    mod, tabs = build_pair(rows, dims, None, 0)
    out = mod(torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"))
    assert out.shape == (4, 16) and float(out.abs().sum()) == 0.0
    out.backward(torch.ones_like(out))  # N == 0: no-op
    torch.cuda.synchronize()


def test_full_size_criteo_shape_properties():
    """BASELINE-size properties that need no oracle run: forward is a pure gather at L = 1
    (every output block equals the addressed row), and SGD backward with unit grads moves each
    touched row by -lr * multiplicity."""
    B = 16384
    rows = [45833188 // 64, 36746, 17245, 7413, 3, 62, 10, 4]  # Criteo mix, big table scaled to fit quickly
    dims = [128] * len(rows)
    rng = np.random.default_rng(0)
    from fbgemm_gpu.split_table_batched_embeddings_ops import (
        ComputeDevice, EmbeddingLocation, SplitTableBatchedEmbeddingBagsCodegen)
    mod = SplitTableBatchedEmbeddingBagsCodegen(
        [(r, d, EmbeddingLocation.DEVICE, ComputeDevice.CUDA) for r, d in zip(rows, dims)],
        learning_rate=0.5, device=torch.device("cuda", 0))
    for w in mod.split_embedding_weights():
        w.uniform_(-1, 1)
    indices, offsets, _ = make_inputs(rng, rows, B, 1, fixed_len=1)
    idx_d, off_d = to_dev(indices), to_dev(offsets)
    out = mod(idx_d, off_d)
    ws = mod.split_embedding_weights()
    for t in range(len(rows)):
        expect = ws[t][idx_d[t * B:(t + 1) * B]]
        assert torch.equal(out[:, t * 128:(t + 1) * 128], expect)
    before = [w.clone() for w in ws]
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    for t in range(len(rows)):
        cnt = torch.bincount(idx_d[t * B:(t + 1) * B], minlength=rows[t]).float()
        expect = before[t] - 0.5 * cnt[:, None]
        torch.testing.assert_close(ws[t], expect, rtol=1e-5, atol=1e-3)


def test_a2a_ready_output_layout_matches_standard_layout():
    """Features = (src rank w, local feature f) pairs; the a2a-ready layout [W][B_l][D_local] must
    hold exactly the standard [B_l, W*D_local] output re-sliced, forward and backward."""
    rng = np.random.default_rng(12)
    rows, dims = [300, 5, 77], [128, 64, 32]
    W, Bl = 4, 50
    ftm = [0, 1, 2] * W
    mod_a, tabs = build_pair(rows, dims, ftm, 0, rng=np.random.default_rng(1), learning_rate=0.1)
    mod_b, _ = build_pair(rows, dims, ftm, 0, rng=np.random.default_rng(1), learning_rate=0.1)
    mod_b.set_a2a_output_layout(W)
    indices, offsets, psw = make_inputs(rng, rows, Bl, 3, ftm, weighted=True)
    oa = mod_a(to_dev(indices), to_dev(offsets), to_dev(psw))          # [Bl, W*Dl]
    ob = mod_b(to_dev(indices), to_dev(offsets), to_dev(psw))          # [W*Bl, Dl]
    Dl = sum(dims)
    assert ob.shape == (W * Bl, Dl)
    expect = oa.view(Bl, W, Dl).permute(1, 0, 2).reshape(W * Bl, Dl)
    assert torch.equal(ob, expect)
    g = torch.from_numpy(rng.standard_normal((Bl, W * Dl)).astype(np.float32)).cuda()
    oa.backward(g)
    ob.backward(g.view(Bl, W, Dl).permute(1, 0, 2).reshape(W * Bl, Dl).contiguous())
    torch.cuda.synchronize()
    for wa, wb in zip(mod_a.split_embedding_weights(), mod_b.split_embedding_weights()):
        assert torch.equal(wa, wb)


def test_managed_location_host_mapped_tables_match_device_tables():
    """EmbeddingLocation.MANAGED (the reference's BATCHED_FUSED_UVM kernels,
    torchrec/distributed/embedding_types.py:57-76): tables live in pinned host memory mapped into the
    GPU; the same kernels must give the same forward output and the same updated rows."""
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from fbgemm_gpu.split_table_batched_embeddings_ops import (
        ComputeDevice, EmbeddingLocation, SplitTableBatchedEmbeddingBagsCodegen)

    rng = np.random.default_rng(21)
    rows, dims = [300, 41, 7], [128, 128, 128]
    locs = [EmbeddingLocation.MANAGED, EmbeddingLocation.DEVICE, EmbeddingLocation.MANAGED_CACHING]
    mod = SplitTableBatchedEmbeddingBagsCodegen(
        [(r, d, loc, ComputeDevice.CUDA) for r, d, loc in zip(rows, dims, locs)], device=torch.device("cuda", 0),
        optimizer=EmbOptimType.EXACT_ROWWISE_ADAGRAD, learning_rate=0.1, eps=1e-3)
    tabs = oracle.Tables(rows, dims)
    for t, w in enumerate(mod.split_embedding_weights()):
        init = rng.standard_normal((rows[t], dims[t])).astype(np.float32)
        tabs.weights[t][...] = init
        w.copy_(torch.from_numpy(init))
    assert not mod.split_embedding_weights()[0].is_cuda and mod.split_embedding_weights()[1].is_cuda
    indices, offsets, _ = make_inputs(rng, rows, 64, 3)
    out = mod(to_dev(indices), to_dev(offsets))
    ref, _ = oracle.tbe_forward(tabs, indices, offsets)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(to_dev(grad))
    torch.cuda.synchronize()
    s0 = [np.zeros(r, dtype=np.float32) for r in rows]
    oracle.tbe_backward(tabs, indices, offsets, grad, oracle.OPT_EXACT_ROWWISE_ADAGRAD, 0.1, eps=1e-3, state0=s0)
    for t, w in enumerate(mod.split_embedding_weights()):
        np.testing.assert_allclose(w.cpu().numpy(), tabs.weights[t], rtol=2e-5, atol=2e-5)
    for t, st in enumerate(mod.split_optimizer_states()):
        np.testing.assert_allclose(st[0].cpu().numpy(), s0[t], rtol=2e-5, atol=2e-5)


def test_sharded_ebc_world1_with_replicated_tables_writes_one_buffer():
    """Data-parallel (replicated) tiny tables + fused table-wise tables on one GPU: both TBE modules
    write their column blocks of ONE [B, sum D] matrix (forward_into) and read their gradient columns from
    it; compare with the oracle (fused exact SGD for the sharded tables, dense gradient for the replicas)."""
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.distributed.planner import EmbeddingShardingPlanner, Topology
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    rng = np.random.default_rng(33)
    rows, D, B, lr = [5000, 3, 700, 12, 90000], 128, 300, 0.1
    keys = [f"c{i}" for i in range(len(rows))]
    tables = [EmbeddingBagConfig(name=f"t{i}", embedding_dim=D, num_embeddings=rows[i], feature_names=[keys[i]])
              for i in range(len(rows))]
    ebc = EmbeddingBagCollection(tables, device=torch.device("meta"))
    planner = EmbeddingShardingPlanner(Topology(1), constraints={"t1": ["data_parallel"], "t3": ["data_parallel"]})
    plan = planner.plan_tables(tables)
    assert plan["t1"].sharding_type == "data_parallel" and plan["t0"].sharding_type == "table_wise"
    dev = torch.device("cuda", 0)
    sebc = ShardedEmbeddingBagCollection(ebc, plan, ShardingEnv.from_local(1, 0), {"learning_rate": lr}, dev)
    tabs = oracle.Tables(rows, [D] * len(rows))
    init = [rng.standard_normal((r, D)).astype(np.float32) for r in rows]
    for t in range(len(rows)):
        tabs.weights[t][...] = init[t]
    for name, (w, _) in sebc.local_shards().items():
        w.copy_(torch.from_numpy(init[int(name[1:])]))
    with torch.no_grad():
        for name, w in sebc.dp_tables().items():
            w.copy_(torch.from_numpy(init[int(name[1:])]))
    values = np.concatenate([rng.integers(0, r, size=B) for r in rows]).astype(np.int64)
    kjt = KeyedJaggedTensor.from_fixed_lengths(keys, torch.from_numpy(values).to(dev), [1] * len(keys))
    out = sebc(kjt).wait().values()
    offsets = np.arange(len(rows) * B + 1, dtype=np.int64)
    ref, _ = oracle.tbe_forward(tabs, values, offsets)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(torch.from_numpy(grad).to(dev))
    torch.cuda.synchronize()
    gw = [np.zeros((r, D), dtype=np.float32) for r in rows]
    ref_tabs = oracle.Tables(rows, [D] * len(rows))
    for t in range(len(rows)):
        ref_tabs.weights[t][...] = init[t]
    oracle.tbe_backward(ref_tabs, values, offsets, grad, oracle.OPT_DENSE_GRAD, 0.0, state0=gw)
    oracle.tbe_backward(tabs, values, offsets, grad, oracle.OPT_EXACT_SGD, lr)
    for name, (w, _) in sebc.local_shards().items():   # fused tables: updated in place
        np.testing.assert_allclose(w.cpu().numpy(), tabs.weights[int(name[1:])], rtol=2e-5, atol=2e-5)
    dpm = sebc._dp_module
    flat = dpm.weights.grad.cpu().numpy()
    for i, t in enumerate(sebc._dp_table_ids):          # replicas: untouched weights, dense gradient
        o = dpm.weights_offsets[i]
        np.testing.assert_allclose(flat[o:o + rows[t] * D].reshape(rows[t], D), gw[t], rtol=2e-5, atol=1e-4)
        np.testing.assert_array_equal(dpm.split_embedding_weights()[i].cpu().numpy(), init[t])


def test_malformed_offsets_never_reach_memory():
    """Offsets that run past the ids, go negative or backwards: such bags are empty and counted (forward and
    backward), nothing is read or written through them, every well-formed bag is still exact."""
    from fbgemm_gpu.split_embedding_configs import EmbOptimType

    rng = np.random.default_rng(31)
    rows, dims = [50, 20], [64, 64]
    mod, tabs = build_pair(rows, dims, None, 0, optimizer=EmbOptimType.EXACT_SGD, rng=rng, learning_rate=0.5)
    B = 8
    indices, offsets, _ = make_inputs(rng, rows, B, 3)
    N = indices.size
    bad = offsets.copy()
    bad[3] = -5          # bag 2 starts negative, bag 3 is fine again
    bad[7] = N + 1000    # bag 6 runs far past the ids; bag 7 starts there (also malformed)
    bad[12] = bad[11] - 1 if bad[11] > 0 else bad[11]  # goes backwards
    before = mod.bounds_check_errors()
    out = mod(to_dev(indices), to_dev(bad))
    torch.cuda.synchronize()
    assert mod.bounds_check_errors() > before
    # expectation: the oracle on the same offsets with malformed bags emptied
    good = np.zeros(2 * B, dtype=bool)
    ref = np.zeros((B, 128), dtype=np.float32)
    for bag in range(2 * B):
        s, e = int(bad[bag]), int(bad[bag + 1])
        if 0 <= s <= e <= N:
            good[bag] = True
            f, b = divmod(bag, B)
            for p in range(s, e):
                ref[b, f * 64:(f + 1) * 64] += tabs.weights[f][indices[p]]
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    w_before = [w.clone() for w in mod.split_embedding_weights()]
    g = rng.standard_normal((B, 128)).astype(np.float32)
    out.backward(to_dev(g))
    torch.cuda.synchronize()
    exp = [w.cpu().numpy().copy() for w in w_before]
    acc = [np.zeros_like(e_) for e_ in exp]
    cover = np.zeros(N, dtype=np.int64)
    for bag in range(2 * B):
        if good[bag]:
            cover[int(bad[bag]):int(bad[bag + 1])] += 1
    ambiguous = [set(), set()]  # offsets that go backwards make bags overlap: which bag owns such an id is undefined
    for bag in range(2 * B):
        if good[bag]:
            f, b = divmod(bag, B)
            for p in range(int(bad[bag]), int(bad[bag + 1])):
                if cover[p] > 1:
                    ambiguous[f].add(int(indices[p]))
                acc[f][indices[p]] += g[b, f * 64:(f + 1) * 64]
    for t, w in enumerate(mod.split_embedding_weights()):
        keep = np.array([r not in ambiguous[t] for r in range(rows[t])])
        np.testing.assert_allclose(w.cpu().numpy()[keep], (exp[t] - 0.5 * acc[t])[keep], rtol=1e-5, atol=1e-5)
        assert np.isfinite(w.cpu().numpy()).all()


def test_row_window_skips_other_shards_rows_silently_and_counts_real_errors():
    """`set_row_windows`: a shard of 40 rows holding global rows [100, 140) of a 300-row table, fed with GLOBAL
    ids: in-window ids are looked up at id - 100, other ids of the table are skipped without a bounds error,
    ids outside [0, 300) are counted.  Forward and backward (fused SGD), pooled SUM with ragged bags."""
    rng = np.random.default_rng(77)
    rows, dims = [40, 50], [64, 64]
    mod, tabs = build_pair(rows, dims, None, 0, rng=rng, learning_rate=0.25)
    mod.set_row_windows([100, 0], [300, 50])
    B = 33
    lengths = rng.integers(0, 4, size=2 * B)
    n0, n1 = int(lengths[:B].sum()), int(lengths[B:].sum())
    ids0 = rng.integers(0, 300, size=n0)
    in_win = rng.random(n0) < 0.4
    ids0 = np.where(in_win, rng.integers(100, 140, size=n0), ids0)
    ids1 = rng.integers(0, 50, size=n1)
    bad0, bad1 = [300, 1000, -1, -7], [50, -2]
    ids0[:len(bad0)] = bad0
    ids1[:len(bad1)] = bad1
    indices = np.concatenate([ids0, ids1]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    before = mod.bounds_check_errors()
    with torch.no_grad():
        mod(to_dev(indices), to_dev(offsets))
    assert mod.bounds_check_errors() - before == len(bad0) + len(bad1)
    out = mod(to_dev(indices), to_dev(offsets))
    # expectation: the oracle on shard-local ids, rows of other shards / bad ids -> -1 (zero row)
    local = indices.copy()
    loc0 = ids0 - 100
    local[:n0] = np.where((loc0 >= 0) & (loc0 < 40), loc0, -1)
    local[n0:] = np.where((ids1 >= 0) & (ids1 < 50), ids1, -1)
    ref, _ = oracle.tbe_forward(tabs, local, offsets)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=1e-6, atol=1e-6)
    g = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(to_dev(g))
    torch.cuda.synchronize()
    oracle.tbe_backward(tabs, local, offsets, g, oracle.OPT_EXACT_SGD, 0.25)
    for t, w in enumerate(mod.split_embedding_weights()):
        np.testing.assert_allclose(w.cpu().numpy(), tabs.weights[t], rtol=2e-5, atol=2e-5)
    # the training forward and the backward's linearize each counted the same ids once more
    assert mod.bounds_check_errors() - before == 3 * (len(bad0) + len(bad1))


def test_bounds_check_modes():
    """BoundsCheckMode (public fbgemm enum; parity unpinned): WARNING counts, FATAL raises after
    the lookup, IGNORE / NONE do not count — an out-of-range id is a zero row in every mode."""
    from fbgemm_gpu.split_table_batched_embeddings_ops import (
        BoundsCheckMode, ComputeDevice, EmbeddingLocation, SplitTableBatchedEmbeddingBagsCodegen)

    dev = torch.device("cuda", 0)
    idx = torch.tensor([1, 99, 2, -5], dtype=torch.int64, device=dev)
    off = torch.arange(5, dtype=torch.int64, device=dev)

    def make(mode):
        m = SplitTableBatchedEmbeddingBagsCodegen([(10, 8, EmbeddingLocation.DEVICE, ComputeDevice.CUDA)], device=dev,
                                                  bounds_check_mode=mode)
        m.split_embedding_weights()[0].fill_(1.0)
        return m

    with torch.no_grad():
        m = make(BoundsCheckMode.WARNING)
        out = m(idx, off)
        assert m.bounds_check_errors() == 2 and out.sum().item() == 16.0
        for mode in (BoundsCheckMode.IGNORE, BoundsCheckMode.NONE):
            m = make(mode)
            out = m(idx, off)
            assert m.bounds_check_errors() == 0 and out.sum().item() == 16.0
        m = make(BoundsCheckMode.FATAL)
        with pytest.raises(RuntimeError, match="BoundsCheckMode.FATAL: 2 out-of-range"):
            m(idx, off)
        assert m(torch.tensor([1, 2, 3, 4], dtype=torch.int64, device=dev), off).sum().item() == 32.0  # valid lookups go on


def test_unimplemented_weight_decay_forms_raise():
    """A (weight_decay, mode) pair this build does not implement raises at construction instead of computing another
    form silently (row-wise Adagrad: L2 only; ADAM: decoupled only; SGD / Adagrad: none)."""
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from fbgemm_gpu.split_table_batched_embeddings_ops import (ComputeDevice, EmbeddingLocation,
                                                                SplitTableBatchedEmbeddingBagsCodegen, WeightDecayMode)

    spec = [(10, 8, EmbeddingLocation.DEVICE, ComputeDevice.CUDA)]
    dev = torch.device("cuda", 0)
    for opt, mode in ((EmbOptimType.EXACT_ROWWISE_ADAGRAD, WeightDecayMode.NONE), (EmbOptimType.EXACT_ROWWISE_ADAGRAD, WeightDecayMode.DECOUPLE),
                      (EmbOptimType.ADAM, WeightDecayMode.L2), (EmbOptimType.EXACT_SGD, WeightDecayMode.L2)):
        with pytest.raises(NotImplementedError, match="weight_decay"):
            SplitTableBatchedEmbeddingBagsCodegen(spec, device=dev, optimizer=opt, weight_decay=1e-5, weight_decay_mode=mode)
    SplitTableBatchedEmbeddingBagsCodegen(spec, device=dev, optimizer=EmbOptimType.EXACT_ROWWISE_ADAGRAD, weight_decay=1e-5,
                                          weight_decay_mode=WeightDecayMode.L2)
    SplitTableBatchedEmbeddingBagsCodegen(spec, device=dev, optimizer=EmbOptimType.ADAM, weight_decay=1e-5)  # bert4rec_main.py:488-491
    SplitTableBatchedEmbeddingBagsCodegen(spec, device=dev, optimizer=EmbOptimType.EXACT_ROWWISE_ADAGRAD, weight_decay=0.0)


@pytest.mark.parametrize("weighted", [False, True])
def test_sum_and_mean_tables_in_one_module(weighted):
    """`set_feature_pooling`: SUM and MEAN features share one lookup and one backward (the reference needs one TBE per
    pooling type + cat: embedding_sharding.py:393-490, embedding_lookup.py:219-253).  Ragged bags incl. empty ones, a
    table used by two features, different dims; forward and fused row-wise Adagrad against the oracle's per-type runs."""
    from _util import oracle_backward_mixed, oracle_forward_mixed
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from fbgemm_gpu.split_table_batched_embeddings_ops import PoolingMode

    rng = np.random.default_rng(21)
    rows, dims, ftm = [60, 9, 200, 31], [32, 64, 16, 128], [0, 1, 2, 2, 3]
    feat_mean = [False, True, True, True, False]
    mod, tabs = build_pair(rows, dims, ftm, 0, EmbOptimType.EXACT_ROWWISE_ADAGRAD, rng, learning_rate=0.1, eps=1e-3)
    mod.set_feature_pooling([PoolingMode.MEAN if m else PoolingMode.SUM for m in feat_mean])
    s0 = [np.zeros(r, dtype=np.float32) for r in rows]
    for step in range(2):
        indices, offsets, psw = make_inputs(rng, rows, 19, 6, ftm, None, weighted)
        out = mod(to_dev(indices), to_dev(offsets), to_dev(psw))
        ref = oracle_forward_mixed(tabs, indices, offsets, psw, feat_mean)
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
        grad = rng.standard_normal(ref.shape).astype(np.float32)
        out.backward(to_dev(grad))
        torch.cuda.synchronize()
        oracle_backward_mixed(tabs, indices, offsets, grad, oracle.OPT_EXACT_ROWWISE_ADAGRAD, 0.1, psw, feat_mean, eps=1e-3, state0=s0)
    for t, w in enumerate(mod.split_embedding_weights()):
        np.testing.assert_allclose(w.cpu().numpy(), tabs.weights[t], rtol=3e-5, atol=3e-5)
    for t, st in enumerate(mod.split_optimizer_states()):
        np.testing.assert_allclose(st[0].cpu().numpy(), s0[t], rtol=3e-5, atol=3e-6)
    mod.set_feature_pooling([PoolingMode.SUM] * 5)  # uniform again: plain SUM module
    assert mod.pooling_mode == PoolingMode.SUM and mod._feature_pooling is None


@pytest.mark.parametrize("B", [4096, 65536], ids=["config2_batch4096", "headline_batch65536"])
def test_full_size_criteo_26_tables_properties(B):
    """The REAL workload (BASELINE configs 2 and the headline): all 26 Criteo-1TB tables at full size (177.9 M rows,
    84.85 GiB fp32 in HBM), pooling factor 1, D = 128 — with assertions, not only timed.  Size-independent properties,
    every table, bit-exact:
      * forward is a pure gather: output block (b, t) == row ids[t, b] of table t;
      * backward with an all-ones gradient and lr = 0.5 (lr * count is exact in fp32) moves every touched row by exactly
        -lr * multiplicity and leaves every other row alone (checked on the touched rows + a random sample of the rest)."""
    from fbgemm_gpu.split_table_batched_embeddings_ops import (
        ComputeDevice, EmbeddingLocation, SplitTableBatchedEmbeddingBagsCodegen)

    rows = [45833188, 36746, 17245, 7413, 20243, 3, 7114, 1441, 62, 29275261, 1572176, 345138, 10, 2209, 11267, 128, 4, 974, 14,
            48937457, 11316796, 40094537, 452104, 12606, 104, 35]
    dev = torch.device("cuda", 0)
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 110 * 2**30:
        pytest.skip("needs ~100 GiB of free HBM")
    D, T, lr = 128, len(rows), 0.5
    mod = SplitTableBatchedEmbeddingBagsCodegen([(r, D, EmbeddingLocation.DEVICE, ComputeDevice.CUDA) for r in rows],
                                                learning_rate=lr, device=dev)
    ws = mod.split_embedding_weights()
    assert sum(w.numel() for w in ws) * 4 == 177944275 * 512
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + B)
    for w in ws:
        w.uniform_(-1.0, 1.0, generator=g)
    idx = torch.cat([torch.randint(0, r, (B,), generator=g, device=dev, dtype=torch.int64) for r in rows])
    off = torch.arange(T * B + 1, dtype=torch.int64, device=dev)
    out = mod(idx, off)
    assert tuple(out.shape) == (B, T * D)
    before_rows, probe_ids, probe_before = [], [], []
    for t in range(T):
        ids = idx[t * B:(t + 1) * B]
        rows_t = ws[t][ids]
        assert torch.equal(out[:, t * D:(t + 1) * D], rows_t), f"table {t}: forward is not a pure gather"
        before_rows.append(rows_t.clone())
        p = torch.randint(0, rows[t], (min(rows[t], 4096),), generator=g, device=dev)
        probe_ids.append(p)
        probe_before.append(ws[t][p].clone())
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    assert mod.bounds_check_errors() == 0
    for t in range(T):
        ids = idx[t * B:(t + 1) * B]
        uniq, inv, cnt = torch.unique(ids, return_inverse=True, return_counts=True)
        mult = cnt[inv].float()                                   # multiplicity of every lookup's row
        expect = before_rows[t] - lr * mult[:, None]              # exact: lr * count is a dyadic rational < 2^24
        assert torch.equal(ws[t][ids], expect), f"table {t}: touched rows did not move by -lr * multiplicity"
        touched = torch.zeros(rows[t], dtype=torch.bool, device=dev)
        touched[uniq] = True
        keep = ~touched[probe_ids[t]]
        assert torch.equal(ws[t][probe_ids[t]][keep], probe_before[t][keep]), f"table {t}: an untouched row changed"


@pytest.mark.parametrize("optname", ["EXACT_SGD", "EXACT_ROWWISE_ADAGRAD"])
@pytest.mark.parametrize("case,defer_sort", [(CASES[0], False), (CASES[3], False), (CASES[5], False),
                                             (CASES[0], True), (CASES[2], True)],
                         ids=["0", "3", "5", "0-deferred", "2-deferred"])
def test_lookup_without_autograd_is_the_autograd_path(case, defer_sort, optname):
    """lookup_no_autograd / backward_no_autograd (what the explicit train step of models/dlrm.py drives) against the
    module's own autograd path: same output, same weights and optimizer state after two steps, bit for bit — for the
    fused module and for the dense-gradient module, into a caller's buffer too.
    The `deferred` cases (without and with per-sample weights, which widen the sort's payload): a lookup made with
    defer_sort=True, whose side-stream sort is started afterwards through the record (what the sharded steps do),
    against the explicit lookup that starts its sort itself."""
    def run(explicit, dense, defer=False):
        rng = np.random.default_rng(11)
        if dense:
            mod, _ = build_pair(case["rows"], case["dims"], case["ftm"], case["pooling"], None, rng, dense=True)
        else:
            mod, _ = build_pair(case["rows"], case["dims"], case["ftm"], case["pooling"], _opt(optname), rng, learning_rate=0.05)
        if defer_sort:
            mod.overlap_backward_sort = True  # whatever the environment says: the sort under test runs on the side stream
        outs, grads_w = [], []
        for _ in range(2):
            indices, offsets, psw = make_inputs(rng, case["rows"], case["B"], case["max_len"], case["ftm"],
                                                case["fixed_len"], case["weighted"])
            i, o, w = to_dev(indices), to_dev(offsets), to_dev(psw)
            if defer:
                out, rec = mod.lookup_no_autograd(i, o, w, defer_sort=True)
                assert rec.prepared is None, "the deferred sort started inside the lookup"
            elif explicit:
                out, rec = mod.lookup_no_autograd(i, o, w)
                assert not defer_sort or rec.prepared is not None
            else:
                out = mod(i, o, w)
            grad = to_dev(rng.standard_normal(tuple(out.shape)).astype(np.float32))
            outs.append(out.detach().clone())
            if defer:
                assert mod.start_backward_sort(rec) and rec.prepared is not None
                assert not mod.start_backward_sort(rec), "a record's sort starts once"
            if explicit:
                g = mod.backward_no_autograd(rec, grad)
                if dense:
                    grads_w.append(g.clone())
            else:
                if dense:
                    mod.weights.grad = None
                out.backward(grad)
                if dense:
                    grads_w.append(mod.weights.grad.clone())
        torch.cuda.synchronize()
        state = [] if dense else [tuple(s.clone() for s in st) for st in mod.split_optimizer_states()]
        return outs, [w.clone() for w in mod.split_embedding_weights()], state, grads_w

    for dense in (False, True):
        if dense and optname != "EXACT_SGD":
            continue
        # the explicit lookup (deferred in the `deferred` cases) against autograd, or against the undeferred explicit lookup
        a = run(explicit=defer_sort, dense=dense)
        b = run(explicit=True, dense=dense, defer=defer_sort)
        for x, y in zip(a[0] + a[1] + a[3], b[0] + b[1] + b[3]):
            assert torch.equal(x, y)
        for sa, sb in zip(a[2], b[2]):
            for x, y in zip(sa, sb):
                assert torch.equal(x, y)


def test_sort_give_up_on_the_device_surfaces_as_an_exception_at_the_next_check_point():
    """VERDICT round 2 / ADVICE: a spin-wait give-up inside the pair sort used to bump a device counter nobody read —
    wrong row updates with rc 0.  The kernels now write the library's fault word (GPU-mapped host memory) and the
    module's per-step host call (set_learning_rate, from the fused optimizer's step: batched_embedding_kernel.py:250-257),
    flush(), bounds_check_errors() and split_embedding_weights() raise on any increase.  tbe_debug_inject_sort_giveup
    runs the kernel-side report without a sort that hangs."""
    from fbgemm_gpu import _lib
    from fbgemm_gpu._lib import KernelFaultError, check, stream_ptr
    from torchrec_amd.distributed.embeddingbag import EmbeddingFusedOptimizer

    rng = np.random.default_rng(3)
    rows, dims = [500, 40], [64, 64]
    mod, tabs = build_pair(rows, dims, None, 0, rng=rng, learning_rate=0.1)
    opt = EmbeddingFusedOptimizer(mod, ["a", "b"])
    indices, offsets, _ = make_inputs(rng, rows, 64, 3)
    out = mod(to_dev(indices), to_dev(offsets))
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    opt.step()  # clean: a real backward (with its sort) reports nothing
    mod.flush()
    assert mod.bounds_check_errors() == 0
    dev = torch.device("cuda", 0)
    before = _lib.fault_count()
    check(_lib.load().tbe_debug_inject_sort_giveup(stream_ptr(dev)), "tbe_debug_inject_sort_giveup")
    torch.cuda.synchronize()
    assert _lib.fault_count() == before + 1  # the device's system-scope writes are visible to the host without a copy
    with pytest.raises(KernelFaultError, match="WRONG"):
        opt.step()
    opt.step()  # reported once
    for call in (mod.flush, mod.bounds_check_errors, mod.split_embedding_weights, opt.zero_grad):
        check(_lib.load().tbe_debug_inject_sort_giveup(stream_ptr(dev)), "tbe_debug_inject_sort_giveup")
        torch.cuda.synchronize()
        with pytest.raises(KernelFaultError):
            call()
        call()
