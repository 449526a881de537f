"""Exact SGD on once-touched rows inside the gather interaction backward (csrc/dlrm_interaction.hip
interaction_gather_bwd_kernel<NT, SGD>, csrc/tbe_backward.hip tbe_backward_single_flags,
tbe_backward_apply_skip_single_f32).

The reference is the pair of calls the new path replaces, through the C ABI: tbe_dlrm_interaction_gather_backward_f32,
then tbe_backward_prepare + tbe_backward_apply_f32 (SGD) on one clone of the flat table buffer.  The new entries run on a
second clone with grad_sparse pre-filled with NaN.  Everything is compared bit for bit: the whole flat buffer with the
guard elements around it, and grad_dense."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
from _bwd_abi import CHUNK, GUARD_ELEMS, opt_args
from test_gather_interaction_gpu import ID_SKIP, SHAPES, Case, _check, _lib, _stream

pytestmark = pytest.mark.gpu

LR = 0.05
GUARD_VALUE = -12345.5


class Tables:
    """One clone of a Case's flat table buffer between two runs of guard elements, with the feat_* arrays that go with it."""

    def __init__(self, c):
        n = c.flat.numel()
        self.buf = torch.full((n + 2 * GUARD_ELEMS,), GUARD_VALUE, device="cuda")
        self.buf[GUARD_ELEMS:GUARD_ELEMS + n] = c.flat
        shift = self.buf.data_ptr() + 4 * GUARD_ELEMS - c.flat.data_ptr()
        assert shift % 16 == 0
        self.feat_weights = (c.feat_weights + shift).contiguous()
        self.inner = self.buf[GUARD_ELEMS:GUARD_ELEMS + n]


def _row_base(c):
    return np.concatenate([[0], np.cumsum(c.rows)[:-1]]).astype(np.int64)


def _key_bits(c):
    return int(sum(c.rows)).bit_length()  # no valid key equals the all-ones sentinel


def _prepare(c, ids):
    """tbe_backward_prepare on the current stream -> (workspace address, bytes, tensors to keep alive, args)"""
    lib, B, F, D = _lib(), c.B, c.F, c.D
    N = F * B
    offsets = torch.arange(N + 1, dtype=torch.int64, device="cuda")
    base = torch.tensor(_row_base(c)).cuda()
    kb = _key_bits(c)
    nbytes = lib.tbe_backward_workspace_bytes(N, F, B, D, kb)
    assert nbytes > 0
    raw = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    ws = (raw.data_ptr() + 255) // 256 * 256
    win = c.feat_window.data_ptr() if c.feat_window is not None else None
    _check(lib.tbe_backward_prepare(c.feat_rows.data_ptr(), base.data_ptr(), F, B, D, kb, ids.data_ptr(), N,
                                    offsets.data_ptr(), 0, 0, ws, nbytes, None, win, _stream()), "tbe_backward_prepare")
    return ws, nbytes, (raw, offsets, base), kb


def _flags(c, ids):
    """tbe_backward_single_flags of the batch -> uint8 [F * B] on the device, pre-filled with a value it must overwrite"""
    lib = _lib()
    ws, nbytes, keep, kb = _prepare(c, ids)
    single = torch.full((c.F * c.B,), 7, dtype=torch.uint8, device="cuda")
    _check(lib.tbe_backward_single_flags(c.F, c.B, c.D, kb, c.F * c.B, ws, nbytes, single.data_ptr(), _stream()),
           "tbe_backward_single_flags")
    torch.cuda.synchronize()
    return single


def _expected_flags(c, ids):
    """numpy: counts[key] == 1 and the id is a row of the feature's shard"""
    F, B = c.F, c.B
    ids = ids.cpu().numpy().reshape(F, B)
    lo = np.zeros(F, dtype=np.int64)
    if c.feat_window is not None:
        lo = c.feat_window.cpu().numpy().reshape(F, 2)[:, 0]
    rows = np.asarray(c.rows, dtype=np.int64)
    with np.errstate(over="ignore"):
        local = ids - lo[:, None]
    valid = (ids != ID_SKIP) & (local >= 0) & (local < rows[:, None])
    keys = np.where(valid, _row_base(c)[:, None] + local, -1)
    uniq, counts = np.unique(keys[valid], return_counts=True)
    once = np.isin(keys, uniq[counts == 1]) & valid
    return once.reshape(-1).astype(np.uint8)


def _run(c, ids, new):
    """One backward on a fresh clone of the tables -> (whole guarded buffer, grad_dense, grad_sparse, flags or None)"""
    lib, B, F, D = _lib(), c.B, c.F, c.D
    N = F * B
    ids = ids.cuda()
    t = Tables(c)
    win = c.feat_window.data_ptr() if c.feat_window is not None else None
    gd = torch.full((B, D), float("nan"), device="cuda")
    gs = torch.full((B, F * D), float("nan"), device="cuda")
    ws, nbytes, keep, kb = _prepare(c, ids)
    offsets, base = keep[1], keep[2]
    single = None
    gather = (c.dense.data_ptr(), t.feat_weights.data_ptr(), c.feat_rows.data_ptr(), win, ids.data_ptr(),
              c.grad.data_ptr(), c.width, B, F, D, gd.data_ptr(), gs.data_ptr(), None)
    if new:
        single = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
        _check(lib.tbe_backward_single_flags(F, B, D, kb, N, ws, nbytes, single.data_ptr(), _stream()),
               "tbe_backward_single_flags")
        _check(lib.tbe_dlrm_interaction_gather_backward_sgd_f32(*gather, single.data_ptr(), LR, _stream()),
               "gather_backward_sgd")
        apply = lib.tbe_backward_apply_skip_single_f32
    else:
        _check(lib.tbe_dlrm_interaction_gather_backward_f32(*gather, _stream()), "gather_backward")
        apply = lib.tbe_backward_apply_f32
    _check(apply(t.feat_weights.data_ptr(), c.feat_D.data_ptr(), c.feat_out_offset.data_ptr(), c.feat_rows.data_ptr(),
                 base.data_ptr(), None, None, F, B, D, kb, ids.data_ptr(), N, offsets.data_ptr(), None, 0, None,
                 gs.data_ptr(), F * D, opt_args(0, LR), 1, ws, nbytes, _stream()), "tbe_backward_apply")
    torch.cuda.synchronize()
    return t.buf, gd, gs, single


def _check_case(c, ids, expect_flagged=None):
    """The required results for one batch; returns the number of flagged contributions."""
    ref_buf, ref_gd, ref_gs, _ = _run(c, ids, new=False)
    assert not torch.isnan(ref_gs).any()
    buf, gd, gs, single = _run(c, ids, new=True)
    want = torch.from_numpy(_expected_flags(c, ids)).cuda()
    assert torch.equal(single, want)
    n_flagged = int(want.sum())
    if expect_flagged is not None:
        assert n_flagged == expect_flagged
    assert torch.equal(buf, ref_buf)  # guard elements before and after the tables included
    assert float(buf[0]) == GUARD_VALUE and float(buf[-1]) == GUARD_VALUE
    assert torch.equal(gd, ref_gd)
    assert not torch.isnan(buf).any()
    # grad_sparse: the rows of flagged contributions are not written, every other row is the plain kernel's
    F, B, D = c.F, c.B, c.D
    written = ~torch.isnan(gs.view(B, F, D)).all(dim=2)  # [B, F]
    assert torch.equal(written, (want.view(F, B).t() == 0))
    assert torch.equal(torch.where(written.unsqueeze(2), gs.view(B, F, D), ref_gs.view(B, F, D)), ref_gs.view(B, F, D))
    buf2, gd2, gs2, _ = _run(c, ids, new=True)
    assert torch.equal(buf2, buf) and torch.equal(gd2, gd)
    assert torch.equal(torch.nan_to_num(gs2, nan=1.5), torch.nan_to_num(gs, nan=1.5))
    return n_flagged


@pytest.mark.parametrize("B,F,D", SHAPES)
def test_new_path_bitwise_equal_to_the_plain_pair_of_calls(B, F, D):
    c = Case(B, F, D)
    n = _check_case(c, c.ids)
    if B == 1:
        assert n == F  # one sample: every row is touched once
    elif F >= 4:
        assert 0 < n < F * B  # the row mix gives both kinds: 1-row tables and a 200000-row one
    else:
        assert n == 0  # (3, 1, 64): one table of one row


@pytest.mark.parametrize("B,F,D", [(257, 26, 128), (4099, 5, 64)])
def test_every_id_distinct_leaves_nothing_to_the_update_kernel(B, F, D):
    c = Case(B, F, D, rows=[B + 5 + f for f in range(F)])
    g = torch.Generator().manual_seed(3)
    ids = torch.cat([torch.randperm(c.rows[f], generator=g)[:B] for f in range(F)]).to(torch.int64)
    _check_case(c, ids, expect_flagged=F * B)


@pytest.mark.parametrize("B,F,D", [(17, 7, 128), (2600, 5, 64)])
def test_one_row_tables_set_no_flag(B, F, D):
    c = Case(B, F, D, rows=[1] * F)
    _check_case(c, c.ids, expect_flagged=0)


def test_skipped_out_of_range_and_foreign_ids_mixed_with_single_rows():
    c = Case(300, 7, 128)
    ids = c.ids.clone().view(c.F, c.B)
    for f, b, v in [(0, 5, -1), (1, 17, 3), (2, 0, 1000), (3, 299, 1 << 40), (6, 100, (1 << 63) - 1), (2, 64, -77)]:
        ids[f, b] = v
    for f, b in [(0, 9), (4, 250), (5, 0), (3, 7)]:
        ids[f, b] = ID_SKIP
    n = _check_case(c, ids.view(-1))
    assert n > 0
    # row windows: ids are global rows; those of other shards are skipped silently, and a single local row next to them
    F, D, B = 5, 128, 700
    rows = [1000, 40, 3, 500, 1]
    window = [(500, 3000), (0, 40), (6, 10), (1500, 2000), (0, 1)]
    c = Case(B, F, D, rows=rows, window=window)
    ids = c.ids.clone().view(F, B)
    ids[0, 1], ids[2, 2], ids[3, 3], ids[4, 4] = 3000, -1, 2000, ID_SKIP
    want = _expected_flags(c, ids.view(-1))
    assert 0 < int(want.sum()) < F * B
    _check_case(c, ids.view(-1))


# Sorted positions of the designed batch (two features, B = 129 ids each, chunks of 32): runs in key order.
#   feature 0: single at 0 (first sorted position); 1..40 a run longer than a chunk; singles at 41 (directly after it) and
#   42; 43..62; singles at 63 and 64 (the two sides of the chunk boundary at 64; 64 is directly before the next long run);
#   65..97 longer than a chunk; single at 98 (directly after); 99..128 (crosses the boundary at 128 into feature 1's chunk)
#   feature 1: single at 129; 130..191 ends on the boundary at 192; singles at 192 (first of its chunk, directly after a
#   run longer than a chunk) and 193; 194..255 ends on the boundary at 256; singles at 256 and 257 (last sorted position)
DESIGNED_RUNS = ([1, 40, 1, 1, 20, 1, 1, 33, 1, 30], [1, 62, 1, 1, 62, 1, 1])


def _designed(D, bad):
    B = 129
    assert CHUNK == 32 and all(sum(r) == B for r in DESIGNED_RUNS)
    rows = [len(r) + 3 for r in DESIGNED_RUNS]
    c = Case(B, 2, D, rows=rows)
    g = torch.Generator().manual_seed(17)
    ids = []
    for runs in DESIGNED_RUNS:
        v = torch.repeat_interleave(torch.arange(len(runs)), torch.tensor(runs))  # row j receives runs[j] contributions
        ids.append(v[torch.randperm(B, generator=g)])
    ids = torch.stack(ids).to(torch.int64)
    n_single = sum(r.count(1) for r in DESIGNED_RUNS)
    if bad:
        # three ids of runs longer than one leave for the sentinel run at the end: the single at the last VALID sorted
        # position is then followed by sentinels, and every position behind a removed id moves up the chunk grid
        for f, row, v in [(0, 1, ID_SKIP), (1, 1, -1), (1, 4, 1 << 40)]:
            b = int((ids[f] == row).nonzero()[0])
            ids[f, b] = v
    return c, ids.view(-1), n_single


@pytest.mark.parametrize("bad", [False, True], ids=["all_valid", "sentinel_tail"])
@pytest.mark.parametrize("D", [64, 128])
def test_singles_placed_against_the_chunk_grid(D, bad):
    c, ids, n_single = _designed(D, bad)
    _check_case(c, ids, expect_flagged=n_single)


@pytest.mark.parametrize("B,F,D", [(257, 26, 128), (2600, 5, 64)])
def test_flag_kernel_matches_numpy(B, F, D):
    c = Case(B, F, D)
    ids = c.ids.clone().view(F, B)
    ids[0, 0], ids[F - 1, B - 1], ids[F // 2, 3] = -1, ID_SKIP, 1 << 50
    ids = ids.view(-1).cuda()
    assert np.array_equal(_flags(c, ids).cpu().numpy(), _expected_flags(c, ids))


def test_entries_validate_before_any_launch():
    lib = _lib()
    assert lib.tbe_backward_single_flags(2, 8, 128, 20, 15, None, 0, None, None) == -1  # N != F * B
    assert b"one id per bag" in lib.tbe_last_error()
    rc = lib.tbe_dlrm_interaction_gather_backward_sgd_f32(None, None, None, None, None, None, 479, 4, 26, 128, None, None,
                                                          None, None, 0.1, None)
    assert rc == -1 and b"null pointer" in lib.tbe_last_error()


# ---- module level ----------------------------------------------------------------------------------------------------
def _dlrm_run(single_row, steps=3, B=257, F=26, D=128):
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.distributed.planner import EmbeddingShardingPlanner, Topology
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.models.dlrm import DLRM
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    dev = torch.device("cuda", 0)
    rows = [[1, 3, 1000, 200000][f % 4] for f in range(F)]
    keys = [f"f{i}" for i in range(F)]
    tables = [EmbeddingBagConfig(name=f"t{i}", embedding_dim=D, num_embeddings=rows[i], feature_names=[keys[i]])
              for i in range(F)]
    plan = EmbeddingShardingPlanner(Topology(1)).plan_tables(tables)
    torch.manual_seed(4)
    sebc = ShardedEmbeddingBagCollection(EmbeddingBagCollection(tables, device=torch.device("meta")), plan,
                                         ShardingEnv.from_local(1, 0),
                                         {"learning_rate": 0.1, "optimizer": EmbOptimType.EXACT_SGD}, dev)
    sebc.reset_parameters_sharding_invariant(9)
    model = DLRM(sebc, 13, [32, D], [16, 1], dense_device=dev)
    assert model.fused_single_row_update is True  # on by default
    model.fused_single_row_update = single_row
    dense_params = [p for p in model.parameters() if p.requires_grad and p.numel() > 0]
    opt = torch.optim.SGD(dense_params, lr=0.05)
    g = torch.Generator().manual_seed(6)
    logits = []
    for _ in range(steps):
        vals = torch.cat([torch.randint(0, r, (B,), generator=g) for r in rows]).to(torch.int64)
        vals[5], vals[B + 2] = -3, ID_SKIP  # one counted, one skipped
        kjt = KeyedJaggedTensor.from_fixed_lengths(keys, vals.cuda(), [1] * F)
        dense = torch.randn(B, 13, generator=g).cuda()
        opt.zero_grad()
        out = model(dense, kjt)
        out.sum().backward()
        opt.step()
        logits.append(out.detach().clone())
    torch.cuda.synchronize()
    m = sebc._emb_module
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    tabs = {k: w.clone() for k, (w, _) in sebc.local_shards().items()}
    return logits, params, tabs, m.bounds_check_errors(), model.fused_lookup_steps, m.single_row_sgd_steps


def test_small_dlrm_trains_bitwise_the_same_with_the_path_on_and_off():
    on, off = _dlrm_run(True), _dlrm_run(False)
    assert on[4] == off[4] == 3  # both took the gather path ...
    assert on[5] == 3 and off[5] == 0  # ... and only one let its backward update the once-touched rows
    assert all(torch.equal(a, b) for a, b in zip(on[0], off[0]))
    assert on[1].keys() == off[1].keys() and on[2].keys() == off[2].keys() and len(on[2]) == 26
    for k in on[1]:
        assert torch.equal(on[1][k], off[1][k]), k
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k
    assert on[3] == off[3] and on[3] >= 1  # the out-of-range id of every step is counted the same way
