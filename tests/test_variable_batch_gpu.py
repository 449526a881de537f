"""GPU: a different batch size per rank with the real kernels.

* `torch.ops.fbgemm.expand_into_jagged_permute` / `permute_1D_sparse_data` (csrc/sparse_ops.hip), bit-exact against their
  numpy restatements (tests/_vb_ref.py).
* world_size 2 with both ranks on cuda:0 over gloo (the all-to-all staged through the host, exactly as
  tests/test_multirank_gpu.py does): the recorded W = 2 vectors of tests/golden/vb_dist_data.npz through KJTAllToAll and
  PooledEmbeddingsAllToAll on device tensors, forward and backward, and ShardedEmbeddingBagCollection(variable_batch_size=True)
  against the unsharded oracle on the concatenated batch."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _paths  # noqa: F401
import _vb_ref
import _vb_sharded
from _results import ResultStore
from test_multirank_gpu import _free_port, _stage_a2a_through_host

pytestmark = pytest.mark.gpu

DTYPES = {"int32": (np.int32, torch.int32), "int64": (np.int64, torch.int64)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- expand_into_jagged_permute ---------------------------------------------------------------------------------------
def _expand_case(out_lengths, rng, np_dtype):
    P = len(out_lengths)
    permute = rng.permutation(P)
    in_lengths = np.zeros(P, dtype=np.int64)
    in_lengths[permute] = out_lengths  # the caller's contract: input segment permute[i] is as long as output segment i
    in_off = np.concatenate([[0], np.cumsum(in_lengths)]).astype(np_dtype)
    out_off = np.concatenate([[0], np.cumsum(out_lengths)]).astype(np_dtype)
    return permute.astype(np_dtype), in_off, out_off


def _check_expand(permute, in_off, out_off):
    size = int(out_off[-1])
    got = torch.ops.fbgemm.expand_into_jagged_permute(_dev(permute), _dev(in_off), _dev(out_off), size)
    assert got.dtype == _dev(permute).dtype and got.shape == (size,)
    np.testing.assert_array_equal(got.cpu().numpy(), _vb_ref.expand_into_jagged_permute(permute, in_off, out_off, size))
    return got


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_expand_into_jagged_permute_matches_restatement(P, dtype):
    rng = np.random.default_rng(P)
    for _ in range(3):
        out_lengths = rng.choice([0, 1, 2, 63, 64, 65, 200], size=P)
        got = _check_expand(*_expand_case(out_lengths, rng, DTYPES[dtype][0]))
        assert sorted(got.cpu().tolist()) == list(range(int(out_lengths.sum())))  # a permutation of the elements


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_expand_into_jagged_permute_empty_and_one_long_segment(dtype):
    rng = np.random.default_rng(5)
    npd = DTYPES[dtype][0]
    got = _check_expand(*_expand_case(np.zeros(70, dtype=np.int64), rng, npd))  # output_size == 0: nothing is launched
    assert got.numel() == 0
    lone = np.zeros(130, dtype=np.int64)
    lone[77] = 1000  # one segment of 1000 among empties: the wave strides over it
    _check_expand(*_expand_case(lone, rng, npd))


def test_expand_into_jagged_permute_host_checks():
    p, i, o = (_dev(a) for a in _expand_case(np.array([2, 3, 1]), np.random.default_rng(0), np.int32))
    op = torch.ops.fbgemm.expand_into_jagged_permute
    with pytest.raises(RuntimeError, match="input_offset"):
        op(p, i[:-1], o, 6)
    with pytest.raises(RuntimeError, match="output_offset"):
        op(p, i, o.long(), 6)
    with pytest.raises(RuntimeError, match="output_size"):
        op(p, i, o, -1)
    with pytest.raises(RuntimeError, match="dtype"):
        op(p.float(), i.float(), o.float(), 6)


# ---- permute_1D_sparse_data -------------------------------------------------------------------------------------------
def _check_permute_1d(permute, lengths, values, weights):
    want = _vb_ref.permute_1d(permute, lengths, values, weights)
    for given in (True, False):
        l2, v2, w2 = torch.ops.fbgemm.permute_1D_sparse_data(
            _dev(permute.astype(np.int32)), _dev(lengths), _dev(values), _dev(weights) if weights is not None else None,
            int(want[1].size) if given else None)
        assert l2.dtype == _dev(lengths).dtype and v2.dtype == _dev(values).dtype
        np.testing.assert_array_equal(l2.cpu().numpy(), want[0])
        np.testing.assert_array_equal(v2.cpu().numpy(), want[1])
        if weights is None:
            assert w2 is None
        else:
            np.testing.assert_array_equal(w2.cpu().numpy(), want[2])


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("kind", ["identity", "reversal", "one_dropped", "repeats"])
@pytest.mark.parametrize("L", [1, 64, 65, 257])
def test_permute_1d_sparse_data_matches_restatement(L, kind, dtype):
    rng = np.random.default_rng(L)
    npd = DTYPES[dtype][0]
    lengths = rng.integers(0, 5, size=L).astype(npd)  # zeros included
    if L > 1:
        lengths[rng.integers(0, L)] = 0
    N = int(lengths.sum())
    values = rng.integers(0, 1 << 20, size=N).astype(npd)
    weights = rng.random(N).astype(np.float32)
    permute = {"identity": np.arange(L), "reversal": np.arange(L)[::-1].copy(),
               "one_dropped": np.delete(rng.permutation(L), 0), "repeats": rng.integers(0, L, size=2 * L)}[kind]
    assert len(permute) == {"identity": L, "reversal": L, "one_dropped": L - 1, "repeats": 2 * L}[kind]
    for w in (weights, None):
        _check_permute_1d(permute, lengths, values, w)


def test_permute_1d_sparse_data_runs_the_multi_tile_scan():
    """More segments than one scan tile (kScanTile = 2048 in csrc/sparse_ops.hip) holds, on both sides."""
    rng = np.random.default_rng(9)
    L = 2048 * 2 + 77
    lengths = rng.integers(0, 4, size=L).astype(np.int32)
    N = int(lengths.sum())
    _check_permute_1d(rng.permutation(L), lengths, rng.integers(0, 1 << 30, size=N).astype(np.int64),
                      rng.random(N).astype(np.float32))


def test_variable_recat_on_device_equals_the_restatement():
    from torchrec_amd.distributed.dist_data import _get_recat

    # (the last one: few long segments, where the kernel deals one 64-segment range to many waves)
    for local_split, W, bpr in ((4, 8, [65, 1, 0, 64, 63, 7, 200, 2]), (3, 2, [5, 3]), (2, 3, [0, 0, 0]),
                                (4, 8, [8000, 8400, 8192, 7900, 8500, 8192, 8100, 8252])):
        got = _get_recat(local_split, W, 1, torch.device("cuda", 0), bpr)
        assert got.dtype == torch.int32
        np.testing.assert_array_equal(got.cpu().numpy(), _vb_ref.recat(local_split, W, bpr))


# ---- two ranks on one GPU over gloo -------------------------------------------------------------------------------------
def _init(rank, W, port):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    _stage_a2a_through_host()  # gloo has no device all-to-all


def _golden_worker(rank, W, port, ret):
    _init(rank, W, port)
    try:
        z, meta = _vb_sharded.golden()
        ret[rank] = _vb_sharded.run_golden_exchanges(z, meta, W, rank, dist.group.WORLD, torch.device("cuda", 0))
    finally:
        dist.destroy_process_group()


def test_kjt_and_pooled_all_to_all_give_the_golden_results_on_device():
    W = 2
    ret = ResultStore()
    mp.spawn(_golden_worker, args=(W, _free_port(), ret), nprocs=W, join=True)
    z, meta = _vb_sharded.golden()
    assert _vb_sharded.check_golden_exchanges(z, meta, W, ret) >= 4 * W


ROWS = [5000, 7, 230, 90000, 5, 1201]
DIMS = [128, 100, 16, 128, 50, 64]
# t0 and t1 column-wise, t2 replicated, the others table-wise
SHARDING = {0: "column_wise", 1: "table_column_wise", 2: "data_parallel"}
EPS = 1e-3
# (fixed length | 0 = ragged bags of 0..3, weighted, MEAN tables)
VARIANTS = [(0, False, ()), (1, False, ()), (0, True, (0, 3, 5)), (1, True, ())]


def _build(env, weighted, mean_tables, adagrad=False, variable=True):
    from _cw_sharded import LR, tables_and_plan
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    tables, plan = tables_and_plan(env.world_size, ROWS, DIMS, SHARDING, "cuda", mean_tables)
    ebc = EmbeddingBagCollection(tables, is_weighted=weighted, device=torch.device("meta"))
    fused = {"learning_rate": LR}
    if adagrad:
        from fbgemm_gpu.split_embedding_configs import EmbOptimType
        fused.update({"optimizer": EmbOptimType.EXACT_ROWWISE_ADAGRAD, "eps": EPS})
    return plan, ShardedEmbeddingBagCollection(ebc, plan, env, fused, torch.device("cuda", 0), variable_batch_size=variable)


def _step(rank, W, bpr, fixed_len, weighted, mean_tables, adagrad=False, variable=True):
    from _cw_sharded import load_init, train_step
    from torchrec_amd.distributed.types import ShardingEnv

    dev = torch.device("cuda", 0)
    plan, sebc = _build(ShardingEnv.from_process_group(dist.group.WORLD), weighted, mean_tables, adagrad, variable)
    assert sebc._variable_batch == variable
    per_rank, init = _vb_sharded.data(bpr, ROWS, DIMS, fixed_len, weighted)
    load_init(sebc, init)

    def all_reduce(g):
        gc = g.cpu()
        dist.all_reduce(gc)
        return gc.to(dev)

    res = train_step(sebc, per_rank, rank, W, fixed_len, weighted, dev, all_reduce)
    if adagrad:
        res = res + ([(lt.cfg.name, lt.col_offset, st[0].detach().cpu().numpy().copy())
                      for lt, st in zip(sebc._local_tables, sebc._emb_module.split_optimizer_states())],)
    return res, sebc._emb_module.bounds_check_errors(), {n: p.sharding_type for n, p in plan.items()}


def _variants_worker(rank, W, port, bpr, ret):
    _init(rank, W, port)
    try:
        for v, (fixed_len, weighted, mean_tables) in enumerate(VARIANTS):
            res, errors, kinds = _step(rank, W, bpr, fixed_len, weighted, mean_tables)
            ret[f"v{v}_r{rank}"] = (res, errors, kinds)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("bpr", [[5, 3], [4, 0], [65, 1]])
def test_variable_batch_sharded_collection_world2_on_one_gpu(bpr):
    """Column-wise + table-wise + replicated tables, SGD: ragged bags and fixed length 1, weighted and not, SUM and mixed
    SUM / MEAN, one forward + backward each — sharded == unsharded oracle on the concatenated batch, zero bounds errors."""
    W = 2
    ret = ResultStore()
    mp.spawn(_variants_worker, args=(W, _free_port(), bpr, ret), nprocs=W, join=True)
    for v, (fixed_len, weighted, mean_tables) in enumerate(VARIANTS):
        got = [ret[f"v{v}_r{r}"] for r in range(W)]
        kinds = got[0][2]
        assert kinds["t0"] == "column_wise" and kinds["t2"] == "data_parallel" and kinds["t5"] == "table_wise"
        assert all(g[1] == 0 for g in got)
        per_rank, init = _vb_sharded.data(bpr, ROWS, DIMS, fixed_len, weighted)
        _vb_sharded.check_against_unsharded([g[0] for g in got], bpr, ROWS, DIMS, per_rank, init, fixed_len, weighted, kinds,
                                            mean_tables)


def _adagrad_worker(rank, W, port, bpr, ret):
    _init(rank, W, port)
    try:
        ret[rank] = _step(rank, W, bpr, 2, False, (), adagrad=True)
    finally:
        dist.destroy_process_group()


def test_variable_batch_sharded_collection_world2_rowwise_adagrad():
    """EXACT_ROWWISE_ADAGRAD: tables and `momentum1` of every piece equal the oracle on the concatenated batch."""
    W, bpr = 2, [5, 3]
    ret = ResultStore()
    mp.spawn(_adagrad_worker, args=(W, _free_port(), bpr, ret), nprocs=W, join=True)
    got = [ret[r] for r in range(W)]
    assert all(g[1] == 0 for g in got)
    per_rank, init = _vb_sharded.data(bpr, ROWS, DIMS, 2, False)
    _vb_sharded.check_against_unsharded([g[0] for g in got], bpr, ROWS, DIMS, per_rank, init, 2, False, got[0][2], (),
                                        adagrad_eps=EPS)


def _equal_worker(rank, W, port, bpr, ret):
    _init(rank, W, port)
    try:
        for mode in (True, False):
            ret[f"{mode}_{rank}"] = _step(rank, W, bpr, 0, True, (0, 3, 5), variable=mode)
    finally:
        dist.destroy_process_group()


def test_equal_batches_in_variable_mode_agree_with_the_fixed_mode_module():
    W, bpr = 2, [4, 4]
    ret = ResultStore()
    mp.spawn(_equal_worker, args=(W, _free_port(), bpr, ret), nprocs=W, join=True)
    for r in range(W):
        (out_v, pieces_v, repl_v), err_v, _ = ret[f"True_{r}"]
        (out_f, pieces_f, repl_f), err_f, _ = ret[f"False_{r}"]
        assert err_v == 0 and err_f == 0
        np.testing.assert_allclose(out_v, out_f, rtol=1e-5, atol=1e-5)
        assert [(n, r0, c0) for n, _, r0, c0 in pieces_v] == [(n, r0, c0) for n, _, r0, c0 in pieces_f]
        for (_, wv, _, _), (_, wf, _, _) in zip(pieces_v, pieces_f):
            np.testing.assert_allclose(wv, wf, rtol=3e-5, atol=3e-5)
        for n in repl_f:
            np.testing.assert_allclose(repl_v[n], repl_f[n], rtol=3e-5, atol=3e-5)
    per_rank, init = _vb_sharded.data(bpr, ROWS, DIMS, 0, True)
    _vb_sharded.check_against_unsharded([ret[f"True_{r}"][0] for r in range(W)], bpr, ROWS, DIMS, per_rank, init, 0, True,
                                        ret["True_0"][2], (0, 3, 5))
