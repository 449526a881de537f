"""GPU: quantized inference tables (csrc/tbe_nbit.hip).  The quantizer bit for bit against the numpy float32 restatement of
include/tbe_hip.h; the lookup through the C ABI bit for bit against float64 sums of tables whose every FP32 sum is exact
(scales 1/8 .. 1/2, biases in eighths, weights 0.5 / 1 / 2, bags of at most 200 ids: tests/_fwd_abi.py's argument); the
modules on top.  Among the quantizer's special rows: float32 has no range of 1e-9 at 1.0 (its spacing there is 1.2e-7), so
one row alternates 1 and 1 + 2^-23 and the row at 2^-10 carries the range of 1e-9 that makes the half scale underflow;
half(-1000.3) = -1000.5 lies BELOW its row, so the row with minimum -1000.2, whose half is -1000.0, is the one whose elements
clamp at 0."""
import functools

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
from _guarded import TypedBuf
from fbgemm_gpu import _lib
from fbgemm_gpu.split_embedding_configs import SparseType
from fbgemm_gpu.split_table_batched_embeddings_ops import (
    EmbeddingLocation, IntNBitTableBatchedEmbeddingBagsCodegen, PoolingMode, rounded_row_size_in_bytes)
from torchrec_amd.inference.modules import quantize_embeddings
from torchrec_amd.models.dlrm import DLRM
from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
from torchrec_amd.quant import EmbeddingBagCollection as QuantEBC
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

pytestmark = pytest.mark.gpu
TY = {8: SparseType.INT8, 4: SparseType.INT4, 2: SparseType.INT2}
NAN_BITS = {np.float32: (np.int32, 0x7FC00000), np.float16: (np.int16, 0x7E00)}


def quantize_ref(x, b):
    """include/tbe_hip.h in numpy float32: (q uint8 [R, D], scale half [R], bias half [R])"""
    qmax = np.float32(2 ** b - 1)
    bias = x.min(1).astype(np.float16)
    minimum = bias.astype(np.float32)
    rng = x.max(1) - minimum
    scale = np.where(rng == 0, np.float32(1), rng / qmax).astype(np.float16).astype(np.float32)
    scale[scale == 0] = 1
    with np.errstate(divide="ignore"):
        inv = np.float32(1) / scale
    scale[np.isinf(inv)], inv[np.isinf(inv)] = 1, 1
    q = np.clip(np.rint((x - minimum[:, None]) * inv[:, None]), 0, qmax).astype(np.uint8)
    return q, scale.astype(np.float16), bias


def layout_rows(q, scale, bias, b, table):
    """the packed rows as uint8: table layout (header, data, zero padding to 16) or compat (data, header)"""
    epb, (R, D) = 8 // b, q.shape
    data = (q.reshape(R, D // epb, epb).astype(np.uint32) << (np.arange(epb) * b)).sum(2).astype(np.uint8)
    hdr = np.stack([scale, bias], 1).astype(np.float16).view(np.uint8)
    if not table:
        return np.concatenate([data, hdr], 1)
    pad = np.zeros((R, rounded_row_size_in_bytes(D, TY[b], 16) - D // epb - 4), np.uint8)
    return np.concatenate([hdr, data, pad], 1)


def quantizer_input(R, D, rng):
    x = rng.standard_normal((R, D)).astype(np.float32)
    last = np.zeros(D, np.float32)
    last[-1] = 5
    special = [np.zeros(D), np.full(D, 3.25), 1 + np.arange(D) % 2 * 2.0 ** -23, 2.0 ** -10 + np.arange(D) % 2 * 1e-9,
               -1000.3 + np.arange(D) % 3 * 0.005, -1000.2 + np.arange(D) % 3 * 0.005, last]
    if R >= len(special):
        x[:len(special)] = np.asarray(special, dtype=np.float32)
    return x


# D: the smallest legal one, either side of the threads-per-row edges 256 and 1024, and the limit
@pytest.mark.parametrize("D_units", [1, 256, 257, 1024, 1025, 4096])
@pytest.mark.parametrize("b", [8, 4, 2])
def test_quantizer_bit_for_bit(b, D_units):
    step = 2 * (8 // b)
    D = step if D_units == 1 else D_units if D_units % step == 0 else (D_units - 1) + step
    lib, rng = _lib.load(), np.random.default_rng(D + b)
    for R in (1, 5, 67):
        x = quantizer_input(R, D, rng)
        q, scale, bias = quantize_ref(x, b)
        wide = torch.zeros((R, D + 8), dtype=torch.float32, device="cuda")  # a row stride wider than D
        wide[:, :D] = torch.from_numpy(x).cuda()
        for src in (wide[:, :D], wide[:, :D].contiguous()):
            got = torch.ops.fbgemm.FloatToFusedNBitRowwiseQuantizedSBHalf(src, b)
            np.testing.assert_array_equal(got.cpu().numpy(), layout_rows(q, scale, bias, b, False), err_msg=f"R={R}")
        # the C entry between guards: compat rows from an address that is only 2-byte aligned, then the table layout
        for table, skip in ((False, 2), (True, 0)):
            want = layout_rows(q, scale, bias, b, table)
            out = TypedBuf(want.size + skip, np.uint8)
            rc = lib.tbe_quantize_nbit_f32(wide.data_ptr(), R, D, D + 8, b, out.ptr + skip, want.shape[1], 4 * table,
                                           0 if table else want.shape[1] - 4, None)
            assert rc == 0, lib.tbe_last_error()
            torch.cuda.synchronize()
            assert (out.get()[:skip] == 0xA5).all()
            np.testing.assert_array_equal(out.get()[skip:].reshape(want.shape), want, err_msg=f"table={table} R={R}")


@functools.lru_cache(maxsize=None)
def problem(b, B, long_bags):
    """One launch's inputs and float64 sums: a feature per D (own table; the last feature shares the first one's), the
    smallest D, 128, and either side of every G edge (row bytes 64 | 80 ... 1024 | 1040: the last rows loop)."""
    rng = np.random.default_rng(1000 * b + 2 * B + long_bags)
    epb = 8 // b
    dims = [2 * epb, 128] + [nb * epb for nb in (60, 62, 124, 126, 252, 254, 508, 510, 1020, 1022) if nb * epb <= 2048]
    dims += [2048] if b == 8 else []  # the third chunk of a lane (row bytes 2064); INT4 rows take two at most, INT2 rows one
    tabs = []
    for D in dims:
        rows = int(rng.integers(3, 9))
        q = rng.integers(0, 2 ** b, size=(rows, D)).astype(np.uint8)
        scale = rng.choice([0.125, 0.25, 0.5], size=rows).astype(np.float16)
        bias = (rng.integers(-32, 33, size=rows) / 8).astype(np.float16)
        tabs.append((layout_rows(q, scale, bias, b, True), q * scale.astype(np.float64)[:, None] + bias.astype(np.float64)[:, None]))
    ftm = list(range(len(dims))) + [0]
    pattern = [0, 1, 5, 63, 64, 65, 200] if long_bags else [1, 0, 1, 2, 1, 5, 1, 0] * 5 + [65]
    lens = np.array([pattern[i % len(pattern)] for i in range(len(ftm) * B)])
    offsets = np.concatenate([[0], np.cumsum(lens)])
    ids = np.concatenate([rng.integers(-1, len(tabs[t][1]) + 1, size=lens[f * B:(f + 1) * B].sum())  # -1 and `rows` included
                          for f, t in enumerate(ftm)]).astype(np.int64)
    psw = rng.choice([0.5, 1.0, 2.0], size=len(ids)).astype(np.float32)
    return tabs, ftm, ids, offsets, psw


def lookup_ref(tabs, ftm, ids, offsets, psw, B):
    """float64 [B, sum D] sums, bag lengths [F, B] and the count of bad ids and bad bags, by the rules of include/tbe_hip.h"""
    errors, cols, lens = 0, [], np.zeros((len(ftm), B), np.int64)
    for f, t in enumerate(ftm):
        W = tabs[t][1]
        out = np.zeros((B, W.shape[1]))
        for j in range(B):
            s, e = int(offsets[f * B + j]), int(offsets[f * B + j + 1])
            if s < 0 or e > len(ids) or s > e:
                errors += 1
                continue
            ok = (ids[s:e] >= 0) & (ids[s:e] < len(W))
            errors, lens[f, j] = errors + int((~ok).sum()), e - s
            out[j] = (psw[s:e][ok, None].astype(np.float64) * W[ids[s:e][ok]]).sum(0)
        cols.append(out)
    return np.concatenate(cols, 1), lens, errors


def expected(sums, lens, dims, mean, ot):
    if not mean:
        return sums.astype(ot)
    with np.errstate(divide="ignore"):
        inv = np.where(lens > 0, np.float32(1) / lens.astype(np.float32), np.float32(0)).astype(np.float32)
    return (sums.astype(np.float32) * np.repeat(inv.T, dims, axis=1)).astype(ot)


def run_lookup(b_of_table, tabs, ftm, ids, offsets, psw, B, mean, ot, it):
    """The entry for id type `it` -> (out [B, sum D] of dtype ot, bounds_errors); canary, guards and a second run checked."""
    lib = _lib.load()
    bufs = [TypedBuf(rows.size, np.uint8, rows) for rows, _ in tabs]
    dims = [tabs[t][1].shape[1] for t in ftm]
    out_off = np.cumsum([0] + [(D + 3) // 4 * 4 for D in dims])  # every block on the 16-byte grid: D % 4 alone picks the path
    stride = int(out_off[-1]) + 8
    cols = np.concatenate([np.arange(o, o + D) for o, D in zip(out_off, dims)])

    def dev(vals, dtype):
        return torch.tensor(np.asarray(vals), dtype=dtype, device="cuda")

    meta = [dev([bufs[t].ptr for t in ftm], torch.int64), dev(dims, torch.int32), dev([b_of_table[t] for t in ftm], torch.int32),
            dev([tabs[t][0].shape[1] for t in ftm], torch.int32), dev([len(tabs[t][1]) for t in ftm], torch.int64),
            dev(out_off[:-1], torch.int64)]
    tt = torch.int32 if it == np.int32 else torch.int64
    ids_d, off_d = dev(ids, tt), dev(offsets, tt)
    psw_d = None if psw is None else dev(psw, torch.float32)
    entry = lib.tbe_forward_nbit_i32 if it == np.int32 else lib.tbe_forward_nbit_i64
    int_type, nan = NAN_BITS[ot]
    runs = []
    for _ in range(2):
        out, err = TypedBuf(B * stride, int_type, nan), TypedBuf(1, np.int32, 0)
        rc = entry(*(m.data_ptr() for m in meta), None, len(ftm), B, ids_d.data_ptr(), len(ids), off_d.data_ptr(),
                   None if psw_d is None else psw_d.data_ptr(), int(mean), out.ptr, int(ot == np.float16), stride, err.ptr, None)
        assert rc == 0, lib.tbe_last_error()
        torch.cuda.synchronize()
        runs.append((out.get((B, stride)), int(err.get()[0])))
    for buf, (rows, _) in zip(bufs, tabs):
        np.testing.assert_array_equal(buf.get(rows.shape), rows)
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1], "two runs differ"
    assert (np.delete(runs[0][0], cols, axis=1) == nan).all(), "columns outside the features' blocks were written"
    return np.ascontiguousarray(runs[0][0][:, cols]).view(ot), runs[0][1]


@pytest.mark.parametrize("long_bags", [False, True])
@pytest.mark.parametrize("B", [1, 17, 65, 130])
@pytest.mark.parametrize("b", [8, 4, 2])
def test_lookup_bit_for_bit(b, B, long_bags):
    tabs, ftm, ids, offsets, psw = problem(b, B, long_bags)
    dims = [tabs[t][1].shape[1] for t in ftm]
    uint = {np.float32: np.uint32, np.float16: np.uint16}
    for weighted, mean in ((False, False), (True, False), (True, True)):
        w = psw if weighted else np.ones_like(psw)
        sums, lens, errors = lookup_ref(tabs, ftm, ids, offsets, w, B)
        for ot in (np.float32, np.float16):
            for it in (np.int32, np.int64):
                got, nbad = run_lookup([b] * len(tabs), tabs, ftm, ids, offsets, psw if weighted else None, B, mean, ot, it)
                want = expected(sums, lens, dims, mean, ot)
                np.testing.assert_array_equal(got.view(uint[ot]), want.view(uint[ot]), err_msg=f"{weighted} {mean} {ot} {it}")
                assert nbad == errors


def test_lookup_mixed_bit_rates_and_malformed_offsets():
    """An INT8, an INT4 and an INT2 feature of different D in one launch, two features on one table; offsets that go
    backwards and past N make empty bags (+0.0) and are counted."""
    picks = [(8, 1), (4, 3), (2, 5)]  # (bit rate, index into that problem's tables): D = 128, 124, 504
    tabs = [problem(b, 17, False)[0][k] for b, k in picks]
    ftm, B = [0, 1, 2, 1], 3
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 3, size=24).astype(np.int64)
    offsets = np.array([0, 2, 4, 6, 9, 7, 12, 12, 14, 30, 14, 20, 24])  # bag (1, 1) goes backwards, (2, 2) ends past N
    psw = rng.choice([0.5, 1.0, 2.0], size=24).astype(np.float32)
    sums, lens, errors = lookup_ref(tabs, ftm, ids, offsets, psw, B)
    assert errors == 3  # 9 > 7;  30 > N;  30 > 14
    got, nbad = run_lookup([b for b, _ in picks], tabs, ftm, ids, offsets, psw, B, True, np.float32, np.int64)
    want = expected(sums, lens, [tabs[t][1].shape[1] for t in ftm], True, np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert nbad == errors


def test_module_from_weight_lists():
    b, B = 4, 17
    tabs, ftm, ids, offsets, psw = problem(b, B, True)
    specs = [(f"t{t}", len(W), W.shape[1], TY[b], EmbeddingLocation.DEVICE) for t, (_, W) in enumerate(tabs)]
    lists = [(torch.from_numpy(rows[:, 4:4 + W.shape[1] * b // 8].copy()).cuda(), torch.from_numpy(rows[:, :4].copy()).cuda())
             for rows, W in tabs]
    m = IntNBitTableBatchedEmbeddingBagsCodegen(specs, feature_table_map=ftm, pooling_mode=PoolingMode.SUM, weight_lists=lists,
                                                device=torch.device("cuda"), row_alignment=16)
    out = m(torch.from_numpy(ids).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(psw).cuda())
    sums, _, errors = lookup_ref(tabs, ftm, ids, offsets, psw, B)
    assert out.dtype == torch.float16
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint16), sums.astype(np.float16).view(np.uint16))
    assert m.bounds_check_errors() == errors
    for (w, ss), (rows, _), (data, hdr) in zip(m.split_embedding_weights(), m.split_embedding_weights(False), lists):
        assert torch.equal(w, data) and torch.equal(ss, hdr) and torch.equal(rows[:, :4], hdr) and ss.data_ptr() == rows.data_ptr()


def _qconfig(dtype):
    q = torch.quantization
    return q.QConfig(activation=q.PlaceholderObserver, weight=q.PlaceholderObserver.with_args(dtype=dtype))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype, b", [(torch.qint8, 8), (torch.quint4x2, 4), (torch.quint2x4, 2)])
def test_quantized_collection_from_float(dtype, b, weighted):
    torch.manual_seed(b)
    rng = np.random.default_rng(b)
    ebc = EmbeddingBagCollection([EmbeddingBagConfig(50, 16, name="t0", feature_names=["f0", "f2"]),
                                  EmbeddingBagConfig(30, 40, name="t1", feature_names=["f1"])],
                                 is_weighted=weighted, device=torch.device("cuda"))
    ebc.qconfig = _qconfig(dtype)
    B, rows = 9, [50, 30, 50]
    lens = rng.integers(0, 6, size=3 * B)
    ids = np.concatenate([rng.integers(0, rows[f], size=lens[f * B:(f + 1) * B].sum()) for f in range(3)]).astype(np.int64)
    w = rng.uniform(-2, 2, size=len(ids)).astype(np.float32) if weighted else None
    kjt = KeyedJaggedTensor.from_lengths_sync(["f0", "f1", "f2"], torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(),
                                              None if w is None else torch.from_numpy(w).cuda())
    want = ebc(kjt)
    qebc = QuantEBC.from_float(ebc)
    got = qebc(kjt)
    assert qebc._get_name() == "QuantizedEmbeddingBagCollection" and qebc.is_weighted == weighted
    assert [c.data_type.name for c in qebc.embedding_bag_configs] == [f"INT{b}"] * 2
    assert list(qebc.state_dict()) == ["embedding_bags.t0.weight", "embedding_bags.t1.weight"]
    assert got.keys() == want.keys() and got.values().shape == want.values().shape and got.values().dtype == torch.float32
    # against the float64 sums of the float tables.  The bound of a pooled value: per id |w| (r / (2 (2^b - 1)) + 2^-10 (r +
    # |min|)) with r the row's range (half a quantization step, the half rounding of scale and bias), summed over the bag, plus
    # the float32 summation error len * 2^-23 * sum of magnitudes
    tables = {k: v.detach().cpu().numpy() for k, v in ebc.table_weights().items()}
    offsets, bound, exact = np.concatenate([[0], np.cumsum(lens)]), {}, {}
    for f, name in enumerate(["t0", "t1", "t0"]):
        W = tables[name]
        r = W.max(1) - W.min(1)
        per_row = r / (2 * (2 ** b - 1)) + 2.0 ** -10 * (r + np.abs(W.min(1)))
        q, scale, bias = quantize_ref(W, b)  # the numpy dequantization itself stays inside the bound
        assert (np.abs(q * scale.astype(np.float64)[:, None] + bias.astype(np.float64)[:, None] - W) <= per_row[:, None]).all()
        bound[f"f{f}"], exact[f"f{f}"] = np.zeros((B, W.shape[1])), np.zeros((B, W.shape[1]))
        for j in range(B):
            s, e = offsets[f * B + j], offsets[f * B + j + 1]
            sw = np.ones(e - s) if w is None else w[s:e].astype(np.float64)
            exact[f"f{f}"][j] = (sw[:, None] * W[ids[s:e]]).sum(0)
            bound[f"f{f}"][j] = ((np.abs(sw) * per_row[ids[s:e]]).sum()
                                 + (e - s) * 2.0 ** -23 * (np.abs(sw)[:, None] * np.abs(W[ids[s:e]])).sum(0))
    bound, exact = (np.concatenate([x[k] for k in want.keys()], 1) for x in (bound, exact))
    err = np.abs(got.values().cpu().numpy().astype(np.float64) - exact)
    print("largest error over its bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), float((err - bound).max())


def test_quantize_embeddings_on_a_small_dlrm():
    dev = torch.device("cuda")
    ebc = EmbeddingBagCollection([EmbeddingBagConfig(20, 16, name=f"t{i}", feature_names=[f"f{i}"]) for i in range(3)], device=dev)
    model = DLRM(ebc, 4, [8, 16], [8, 1], dense_device=dev)
    quantized = quantize_embeddings(model, torch.quint4x2, inplace=False)
    assert type(model.sparse_arch.embedding_bag_collection) is EmbeddingBagCollection
    assert type(quantized.sparse_arch.embedding_bag_collection) is QuantEBC
    dense = {k: v for k, v in model.named_parameters() if "embedding_bag_collection" not in k}
    assert dense and all(torch.equal(v, dict(quantized.named_parameters())[k]) for k, v in dense.items())
    B = 5
    kjt = KeyedJaggedTensor.from_lengths_sync(["f0", "f1", "f2"], torch.arange(3 * B, device=dev) % 20,
                                              torch.ones(3 * B, dtype=torch.int64, device=dev))
    with torch.no_grad():
        logits = quantized(torch.ones(B, 4, device=dev), kjt)
    assert logits.shape[0] == B and bool(torch.isfinite(logits).all())
