"""GPU: tbe_dlrm_interaction_gather_forward_nbit (include/tbe_hip.h) through the C ABI, bit for bit against
oracle.interaction_forward fed the numpy FP32 dequantization of hand-built tables between guards, and the DLRM path to it."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _interaction_cases as ic
from _guarded import Buf, TypedBuf
from fbgemm_gpu import _lib
from oracle import oracle
from torchrec_amd.inference.modules import quantize_embeddings
from torchrec_amd.models.dlrm import DLRM
from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor as KJT

pytestmark = pytest.mark.gpu

WGS_PER_CU = {64: 4, 128: 3}  # nbit_wgs_per_cu of csrc/dlrm_interaction.hip: the grid is capped at 256 of these
SCALES = np.array([0.25, 0.5, 1.0, 2.0, 0.125], dtype=np.float16)
BIASES = np.array([-2.0, -0.5, 0.0, 0.25, 1.5], dtype=np.float16)
POISONED, POISON_ROW = 2, 5  # the sample of the isolation test, and the table row only it reads


def loop_batch(D):  # twice the waves of the largest grid plus 5: every wave makes two full trips and five a third
    return 2 * 4 * 256 * WGS_PER_CU[D] + 5


class Case:
    """F features over max(1, F - 1) tables (the last feature shares table 0) of 16 + 3 t rows, built byte by byte: header
    (scale, bias) halves, data bytes that use every value, 0xFF in every byte the format calls padding; `pad` more bytes
    of row stride.  ids [F, B]: row 0, the last row, -1 and `rows` among them.  poison: +Inf bias in a row one sample reads."""

    def __init__(self, bits, D, F, B, pad=0, poison=False):
        rng = np.random.default_rng([bits, D, F, B])
        self.bits, self.D, self.F, self.B = bits, D, F, B
        epb, nb = 8 // bits, D * bits // 8
        self.row_bytes = -(-(nb + 4) // 16) * 16 + pad
        self.table_of = [f % max(1, F - 1) for f in range(F)]
        self.rows = np.array([16 + 3 * t for t in range(max(1, F - 1))])
        self.raw, deq = [], []
        for t, n in enumerate(self.rows):
            data = rng.integers(0, 256, (n, nb), dtype=np.uint8)
            data.reshape(-1)[:256] = np.arange(256)
            header = np.stack([SCALES[(np.arange(n) + t) % 5], BIASES[(np.arange(n) * 3 + t) % 5]], axis=1)
            if poison and t == 0:
                header[POISON_ROW, 1] = np.inf
            raw = np.full((n, self.row_bytes), 0xFF, dtype=np.uint8)
            raw[:, :4], raw[:, 4:4 + nb] = header.view(np.uint8), data
            j = np.arange(D)
            q = (data[:, j // epb] >> ((j % epb) * bits)) & ((1 << bits) - 1)
            with np.errstate(invalid="ignore"):
                deq.append(q.astype(np.float32) * header[:, :1].astype(np.float32) + header[:, 1:].astype(np.float32))
            self.raw.append(raw)
        limit = self.rows[self.table_of][:, None]
        self.ids = rng.integers(0, limit, (F, B), dtype=np.int64)
        self.ids[self.ids == POISON_ROW] = POISON_ROW + 1
        if B:
            self.ids[:, 0], self.ids[:, B // 2] = 0, limit[:, 0] - 1
            self.ids[0, B - 1], self.ids[F - 1, B // 3] = -1, limit[F - 1, 0]
        if B > POISONED:
            self.ids[0, POISONED] = POISON_ROW
        bad = (self.ids < 0) | (self.ids >= limit)
        self.bad = int(bad.sum())
        self.dense = rng.standard_normal((B, D)).astype(np.float32)
        sparse = np.stack([deq[t][np.where(bad[f], 0, self.ids[f])] for f, t in enumerate(self.table_of)], axis=1)
        sparse[bad.T] = 0.0
        with np.errstate(invalid="ignore"):
            self.out = oracle.interaction_forward(self.dense, sparse) if B else np.zeros((0, D + ic.pairs(F)), np.float32)


def run(c, layouts=("dense", "padded")):
    """The entry on case c in each layout -> the [B, D + P] results; asserts every byte around them and the count."""
    lib = _lib.load()
    flat = np.concatenate([r.reshape(-1) for r in c.raw])
    starts = np.concatenate([[0], np.cumsum([r.size for r in c.raw])])
    tables, ids, dense = TypedBuf(flat.size, np.uint8, flat), TypedBuf(c.F * c.B, np.int64, c.ids), Buf(c.B * c.D, c.dense)
    weights = np.array([tables.ptr + starts[t] for t in c.table_of])
    feat = (TypedBuf(c.F, np.int64, weights), TypedBuf(c.F, np.int32, [c.row_bytes] * c.F),
            TypedBuf(c.F, np.int64, c.rows[c.table_of]))
    results = []
    for name in layouts:
        _, stride, shift = ic.layout(c.F, c.D, name)
        out, err = ic.RowBuf(c.B, stride, shift), TypedBuf(1, np.int32, [0])
        rc = lib.tbe_dlrm_interaction_gather_forward_nbit(dense.ptr, feat[0].ptr, feat[1].ptr, feat[2].ptr, c.bits, ids.ptr,
                                                          c.B, c.F, c.D, out.ptr, stride, err.ptr,
                                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.tbe_last_error()
        torch.cuda.synchronize()
        image = out.get()
        np.testing.assert_array_equal(image, ic.expected_out(c, stride, shift), err_msg=f"bits={c.bits} D={c.D} F={c.F} B={c.B} {name}")
        assert int(err.get()[0]) == c.bad
        results.append(image[:, :c.D + ic.pairs(c.F)])
    for buf, want in ((tables, flat), (ids, c.ids.reshape(-1)), (dense, c.dense.reshape(-1)), (feat[0], weights),
                      (feat[1], [c.row_bytes] * c.F), (feat[2], c.rows[c.table_of])):
        np.testing.assert_array_equal(buf.get(), want)
    return results


@pytest.mark.parametrize("F", (1, 16, 27))
@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("bits", (8, 4, 2))
def test_three_trips_of_every_wave(bits, D, F):
    """Ids two samples ahead, rows one, the counted wait behind the 4-byte stores ("dense": P % 4 != 0 at F = 1, 27) and the
    16-byte layout; at F = 16 a row stride 16 bytes beyond the row.  A second run gives the same bits."""
    c = Case(bits, D, F, loop_batch(D), pad=16 if F == 16 else 0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(run(c), run(c)))


def test_every_row_count():
    for F in range(1, 28):  # INT2 at D = 64: the LDS pitch with a pad chunk; every slot-to-lane mapping, R = 16 | 17
        run(Case(2, 64, F, 130), ("odd", "padded"))


@pytest.mark.parametrize("B", (0, 1, 3, 5))
def test_fewer_samples_than_waves(B):
    run(Case(8, 128, 26, B))  # waves with no sample issue nothing; B = 0 leaves `out` and the counter as they were


@pytest.mark.parametrize("bits,D", ((8, 128), (2, 64)))
def test_an_infinite_bias_stays_in_its_sample(bits, D):
    clean, bad = Case(bits, D, 16, loop_batch(D)), Case(bits, D, 16, loop_batch(D), poison=True)
    others = np.arange(clean.B) != POISONED
    assert not np.isfinite(bad.out[POISONED]).all() and bad.out[others].tobytes() == clean.out[others].tobytes()
    run(bad)  # the oracle's result for the poisoned input, NaN for NaN; every other sample as in the clean run


def _model(weighted=False):
    torch.manual_seed(7)
    dev = torch.device("cuda", 0)
    cfgs = [EmbeddingBagConfig(20 + i, 64, name=f"t{i}", feature_names=[f"f{i}"]) for i in range(3)]
    model = DLRM(EmbeddingBagCollection(cfgs, is_weighted=weighted, device=dev), 13, [32, 64], [32, 1], dense_device=dev)
    return quantize_embeddings(model, torch.quint4x2, inplace=True)


def test_dlrm_takes_the_fused_path_and_gives_the_pairs_bits():
    dev, keys = torch.device("cuda", 0), ["f0", "f1", "f2"]
    dense, ids = torch.randn(5, 13, device=dev), torch.randint(0, 20, (15,), device=dev)
    fixed = KJT.from_fixed_lengths(keys, ids, [1, 1, 1])
    model = _model()
    with torch.no_grad():
        fused = model(dense, fixed)
        assert model.fused_lookup_steps == 1
        model.fused_lookup = False
        pair = model(dense, fixed)
        model.fused_lookup = True
        assert model.fused_lookup_steps == 1 and fused.cpu().numpy().tobytes() == pair.cpu().numpy().tobytes()
        jagged = model(dense, KJT.from_lengths_sync(keys, ids, torch.ones(15, dtype=torch.int32, device=dev)))
        assert model.fused_lookup_steps == 1 and torch.equal(jagged, pair)
    assert torch.equal(model(dense, fixed), pair) and model.fused_lookup_steps == 1  # grad mode on, trainable dense layers
    weighted = _model(weighted=True)
    with torch.no_grad():
        weighted(dense, KJT.from_fixed_lengths(keys, ids, [1, 1, 1], weights=torch.ones(15, device=dev)))
    assert weighted.fused_lookup_steps == 0
