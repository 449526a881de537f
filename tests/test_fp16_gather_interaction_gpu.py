"""GPU: tbe_dlrm_interaction_gather_forward_f16w / _gather_backward_f16w (include/tbe_hip.h) through the C ABI, bit for bit
against oracle.interaction_forward / interaction_backward fed float32(table)[ids] with zero rows for bad, foreign and skipped
ids (tests/_gather_cases.py restates classify_id), and the DLRM path to them.  Half to float is exact: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _gather_cases as gc
import _interaction_cases as ic
from _guarded import Buf, TypedBuf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

FWD_WGS_PER_CU = {64: 4, 128: 3}  # f16_wgs_per_cu of csrc/dlrm_interaction.hip; the backward runs 2: grids of 256 of these
SPECIALS = np.array([2.0 ** -24, -2.0 ** -24, 1023 * 2.0 ** -24, -0.0, 65504.0, -65504.0, 2.0 ** -14, 1.0], dtype=np.float16)
POISONED, POISON_ROW = 9, 5  # the sample of the isolation test, and the row of table 0 only it reads


def loop_batch(D):  # twice the waves of the largest grid plus 5: every wave makes two full trips and five a third
    return 2 * 4 * 256 * FWD_WGS_PER_CU[D] + 5


def strides(B, D):  # how far a wave moves between two of its samples, forward and backward
    return {4 * max(1, min((B + 3) // 4, 256 * wgs)) for wgs in (FWD_WGS_PER_CU[D], 2)}


class Case(gc.GatherCase):
    """F features over max(1, F - 1) FP16 tables (the last feature shares table 0) of 16 + 3 t rows; feature f's shard starts
    at global row 7 (f % 3) of a table 5 rows longer than the shard's end.  Halves: normal, every fifth row denormal, SPECIALS
    in row 0 (read by sample 4 of every feature); poison: +Inf in a row one sample reads.  Wave j < 4 meets class j (local,
    foreign, TBE_ID_SKIP, bad) at its first, second and third sample of either kernel, at the first and the last feature."""

    def __init__(self, D, F, B, poison=False):
        rng = np.random.default_rng([16, D, F, B])
        table_of = [f % max(1, F - 1) for f in range(F)]
        rows = np.array([16 + 3 * t for t in table_of])
        starts = np.array([D * sum(16 + 3 * u for u in range(t)) for t in table_of])
        self.half = rng.standard_normal(int(starts.max() + rows[starts.argmax()] * D)).astype(np.float16)
        tables = self.half.reshape(-1, D)
        tables[::5] *= np.float16(2.0 ** -14)
        tables[0, :8], tables[0, D - 8:] = SPECIALS, SPECIALS[::-1]
        if poison:
            tables[POISON_ROW, D // 2] = np.inf
        lo = np.array([7 * (f % 3) for f in range(F)])
        ids = lo[:, None] + rng.integers(0, rows[:, None], (F, B))
        ids[ids == lo[:, None] + POISON_ROW] += 1
        if B > 4:
            ids[:, 4] = lo
        if B > POISONED:
            ids[0, POISONED] = lo[0] + POISON_ROW
        for f in {0, F - 1}:
            classes = (lo[f] + rows[f] - 1, lo[f] + rows[f] + 2, gc.ID_SKIP, lo[f] + rows[f] + 5)
            for b in (j + trip * s for s in strides(B, D) for trip in range(3) for j in range(4)):
                if b < B:  # the strides are multiples of 4: b % 4 == j
                    ids[f, b] = classes[b % 4]
        draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
        super().__init__(B, F, D, rows, starts, self.half.astype(np.float32), ids, draw(B, D), draw(B, D + ic.pairs(F)),
                         np.stack([lo, lo + rows + 5], axis=1))


def run(c, layouts=("dense", "padded")):
    """Both entries on case c in each layout -> every result's bytes; asserts each against the oracle, every byte around
    it, the counter, and that nothing the entries read has changed."""
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    tables = TypedBuf(c.half.size, np.int16, c.half.view(np.int16))
    ids, dense = TypedBuf(c.F * c.B, np.int64, c.ids), Buf(c.B * c.D, c.dense)
    feat = (TypedBuf(c.F, np.int64, tables.ptr + 2 * c.starts), TypedBuf(c.F, np.int64, c.rows), TypedBuf(2 * c.F, np.int64, c.window))
    want_out = c.dot.out if c.B else np.zeros((0, c.D + ic.pairs(c.F)), np.float32)
    want_gd, want_gs = c.dot.grads if c.B else (np.zeros((0, c.D), np.float32), np.zeros((0, c.F, c.D), np.float32))
    results = []
    for name in layouts:
        what = f"D={c.D} F={c.F} B={c.B} {name}"
        _, stride, shift = ic.layout(c.F, c.D, name)
        out, err = ic.RowBuf(c.B, stride, shift), TypedBuf(1, np.int32, [0])
        rc = lib.tbe_dlrm_interaction_gather_forward_f16w(dense.ptr, feat[0].ptr, feat[1].ptr, feat[2].ptr, ids.ptr, c.B, c.F, c.D,
                                                          out.ptr, stride, err.ptr, stream)
        assert rc == 0, lib.tbe_last_error()
        grad = ic.RowBuf(c.B, stride, shift, init=ic.grad_image(c.dot, stride))
        gd, gs = Buf(c.B * c.D), Buf(c.B * c.F * c.D)
        rc = lib.tbe_dlrm_interaction_gather_backward_f16w(dense.ptr, feat[0].ptr, feat[1].ptr, feat[2].ptr, ids.ptr, grad.ptr,
                                                           stride, c.B, c.F, c.D, gd.ptr, gs.ptr, err.ptr, stream)
        assert rc == 0, lib.tbe_last_error()
        torch.cuda.synchronize()
        got = out.get(), gd.get((c.B, c.D)), gs.get((c.B, c.F, c.D))
        gc.assert_same(got[0], ic.expected_out(c.dot, stride, shift, want_out), what)
        gc.assert_same(got[1], want_gd, what)
        gc.assert_same(got[2], want_gs, what)
        assert int(err.get()[0]) == 2 * c.bad  # each entry counts every bad id once
        results += [g.tobytes() for g in got]
    for buf, want in ((tables, c.half.view(np.int16)), (ids, c.ids.reshape(-1)), (dense, c.dense.reshape(-1)),
                      (feat[0], tables.ptr + 2 * c.starts), (feat[1], c.rows), (feat[2], c.window.reshape(-1))):
        np.testing.assert_array_equal(buf.get(), want)
    return results


@pytest.mark.parametrize("F", (1, 16, 27))
@pytest.mark.parametrize("D", (64, 128))
def test_three_trips_of_every_wave(D, F):
    """Ids two samples ahead, rows one, the counted wait behind the 4-byte stores and the 16-byte layout, every id class at a
    wave's first, looping and last sample.  A second run gives the same bits."""
    c = Case(D, F, loop_batch(D))
    assert c.bad > 0 and run(c) == run(c)


def test_every_row_count():
    for F in range(1, 28):  # every slot-to-lane mapping of the copy, R = 16 | 17
        run(Case(64, F, 130), ("odd", "padded"))


@pytest.mark.parametrize("B", (0, 1, 3, 5))
def test_fewer_samples_than_waves(B):
    run(Case(128, 26, B))  # waves with no sample issue nothing; B = 0 leaves the outputs and the counter as they were


@pytest.mark.parametrize("D", (64, 128))
def test_an_infinite_half_stays_in_its_sample(D):
    clean, bad = Case(D, 16, loop_batch(D)), Case(D, 16, loop_batch(D), poison=True)
    others = np.arange(clean.B) != POISONED
    assert not np.isfinite(bad.dot.out[POISONED]).all() and not np.isfinite(bad.dot.grads[1][POISONED]).all()
    for a, b in ((bad.dot.out, clean.dot.out), (bad.dot.grads[0], clean.dot.grads[0]), (bad.dot.grads[1], clean.dot.grads[1])):
        assert a[others].tobytes() == b[others].tobytes()
    run(bad)  # the oracle's result for the poisoned input, NaN for NaN; every other sample as in the clean run


def _train(half_tables, steps=3, B=96, D=64, rows=(3000, 50, 700)):
    """A small DLRM over three FP16 tables, exact SGD with the default stochastic rounding -> (logits of every step and of a
    torch.no_grad() forward behind them, tables, gather steps)."""
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.distributed.planner import EmbeddingShardingPlanner, Topology
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.models.dlrm import DLRM
    from torchrec_amd.modules.embedding_configs import DataType, EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    dev, keys = torch.device("cuda", 0), ["f0", "f1", "f2"]
    cfgs = [EmbeddingBagConfig(name=f"t{i}", embedding_dim=D, num_embeddings=rows[i], feature_names=[keys[i]],
                               data_type=DataType.FP16) for i in range(3)]
    torch.manual_seed(4)
    sebc = ShardedEmbeddingBagCollection(EmbeddingBagCollection(cfgs, device=torch.device("meta")),
                                         EmbeddingShardingPlanner(Topology(1)).plan_tables(cfgs), ShardingEnv.from_local(1, 0),
                                         {"learning_rate": 0.1, "optimizer": EmbOptimType.EXACT_SGD}, dev)
    sebc.reset_parameters_sharding_invariant(9)
    model = DLRM(sebc, 13, [32, D], [16, 1], dense_device=dev)
    model.fused_lookup, model.fused_lookup_half_tables, model.deferred_dense_finish = True, half_tables, False
    opt, g, logits = torch.optim.SGD(model.parameters(), lr=0.05), torch.Generator().manual_seed(0), []
    for step in range(steps + 1):
        vals = torch.cat([torch.randint(0, r, (B,), generator=g) for r in rows]).cuda()
        dense, labels = torch.randn(B, 13, generator=g).cuda(), torch.randint(0, 2, (B,), generator=g).float().cuda()
        kjt = KeyedJaggedTensor.from_fixed_lengths(keys, vals, [1] * 3)
        if step == steps:
            taken = model.fused_lookup_steps
            with torch.no_grad():
                logits.append(model(dense, kjt).cpu())
            break
        out = model(dense, kjt)
        logits.append(out.detach().cpu())
        opt.zero_grad()
        torch.nn.functional.binary_cross_entropy_with_logits(out.view(-1), labels).backward()
        opt.step()
    assert sebc._emb_module.bounds_check_errors() == 0
    return logits, {k: w.cpu() for k, (w, _) in sebc.local_shards().items()}, (taken, model.fused_lookup_steps)


def test_dlrm_over_fp16_tables_trains_to_the_pairs_bits():
    fused, pair = _train(True), _train(False)
    assert fused[2] == (3, 4) and pair[2] == (0, 0)  # the training steps, then the torch.no_grad() forward too
    assert all(torch.equal(a, b) for a, b in zip(fused[0], pair[0]))
    assert all(w.dtype == torch.float16 and torch.equal(w, pair[1][k]) for k, w in fused[1].items())
