"""CPU half of the quantized inference tables (csrc/tbe_nbit.hip, fbgemm_gpu IntNBitTableBatchedEmbeddingBagsCodegen,
torchrec_amd.quant): row sizes, the data-type maps, every refusal of the constructor before any device work, and the C
entries' argument checks before any launch (made-up addresses are never touched)."""
import pytest
import torch

import _paths  # noqa: F401
from fbgemm_gpu import _lib
from fbgemm_gpu.split_embedding_configs import SparseType
from fbgemm_gpu.split_table_batched_embeddings_ops import (
    EmbeddingLocation, IntNBitTableBatchedEmbeddingBagsCodegen, PoolingMode, rounded_row_size_in_bytes)
from torchrec_amd.modules import embedding_configs as ec

INVALID = -1
META = torch.device("meta")


def test_rounded_row_size_in_bytes():
    sizes = {SparseType.INT8: 144, SparseType.INT4: 80, SparseType.INT2: 48, SparseType.FP16: 256, SparseType.FP32: 512}
    for ty, nbytes in sizes.items():
        assert rounded_row_size_in_bytes(128, ty, 16) == nbytes, ty
    assert rounded_row_size_in_bytes(8, SparseType.INT2) == 16


def test_data_type_maps():
    assert [d.name for d in ec.DataType] == ["FP32", "FP16", "INT8", "INT4", "INT2"]
    assert [ec.DATA_TYPE_NUM_BITS[d] for d in ec.DataType] == [32, 16, 8, 4, 2]
    assert [ec.data_type_to_bits(d) for d in ec.DataType] == [32, 16, 8, 4, 2]
    for d in ec.DataType:
        assert ec.data_type_to_sparse_type(d) is SparseType[d.name]
    by_dtype = {torch.qint8: "INT8", torch.quint8: "INT8", torch.quint4x2: "INT4", torch.quint2x4: "INT2"}
    for dtype, name in by_dtype.items():
        assert ec.dtype_to_data_type(dtype) is ec.DataType[name]
    with pytest.raises(ValueError, match="float16"):
        ec.dtype_to_data_type(torch.float16)


def test_sharded_tables_precision_refuses_integer_tables_by_name():
    fp16 = ec.EmbeddingBagConfig(10, 8, name="t_half", data_type=ec.DataType.FP16)
    int8 = ec.EmbeddingBagConfig(10, 8, name="t_int8", data_type=ec.DataType.INT8)
    assert ec.sharded_tables_precision([fp16], [], "test") is SparseType.FP16
    with pytest.raises(NotImplementedError, match="t_int8"):
        ec.sharded_tables_precision([int8], [], "test")


@pytest.mark.parametrize("kwargs, error, match", [
    (dict(index_remapping=[torch.zeros(1)]), NotImplementedError, "index_remapping"),
    (dict(location=EmbeddingLocation.MANAGED), NotImplementedError, "EmbeddingLocation"),
    (dict(location=EmbeddingLocation.HOST), NotImplementedError, "EmbeddingLocation"),
    (dict(ty=SparseType.FP32), NotImplementedError, "weights_ty"),
    (dict(ty=SparseType.FP16), NotImplementedError, "weights_ty"),
    (dict(pooling_mode=PoolingMode.NONE), NotImplementedError, "PoolingMode.NONE"),
    (dict(device=torch.device("cpu")), RuntimeError, "no CPU fallback"),
    (dict(output_dtype=SparseType.INT8), NotImplementedError, "output_dtype"),
    (dict(row_alignment=1), NotImplementedError, "row_alignment"),
])
def test_constructor_refusals(kwargs, error, match):
    kwargs = dict(kwargs)
    spec = ("t", 10, 8, kwargs.pop("ty", SparseType.INT4), kwargs.pop("location", EmbeddingLocation.DEVICE))
    kwargs.setdefault("device", META)
    with pytest.raises(error, match=match):
        IntNBitTableBatchedEmbeddingBagsCodegen([spec], **kwargs)


def test_module_on_meta_carries_the_layout():
    m = IntNBitTableBatchedEmbeddingBagsCodegen(
        [("a", 10, 128, SparseType.INT8, EmbeddingLocation.DEVICE), ("b", 3, 8, SparseType.INT2, EmbeddingLocation.DEVICE)],
        feature_table_map=[0, 1, 0], device=META, row_alignment=16)
    assert m.output_dtype is SparseType.FP16 and m.weights.numel() == 10 * 144 + 3 * 16 and m.total_D == 264
    (wa, sa), (wb, sb) = m.split_embedding_weights()
    assert (tuple(wa.shape), tuple(sa.shape), tuple(wb.shape), tuple(sb.shape)) == ((10, 128), (10, 4), (3, 2), (3, 4))
    assert tuple(m.split_embedding_weights(split_scale_shifts=False)[0][0].shape) == (10, 144)


def test_quantized_collection_refuses_meta_and_cpu_by_name():
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.quant import EmbeddingBagCollection as QuantEBC

    ebc = EmbeddingBagCollection([ec.EmbeddingBagConfig(10, 8, name="t")], device=META)
    ebc.qconfig = torch.quantization.QConfig(activation=torch.quantization.PlaceholderObserver,
                                             weight=torch.quantization.PlaceholderObserver.with_args(dtype=torch.quint4x2))
    with pytest.raises(RuntimeError, match="'meta'"):
        QuantEBC.from_float(ebc)
    with pytest.raises(RuntimeError, match="'cpu'"):
        QuantEBC(None, ebc.embedding_bag_configs, False, torch.device("cpu"))


def test_quantizer_entry_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = 0x1000

    def quantize(R=4, D=128, stride=None, bits=8, src=P, out=P, ostride=144, data_off=4, hdr_off=0):
        rc = lib.tbe_quantize_nbit_f32(src, R, D, D if stride is None else stride, bits, out, ostride, data_off, hdr_off, None)
        return rc, lib.tbe_last_error()

    for bad in (dict(bits=3), dict(D=127), dict(D=6, bits=4), dict(D=4, bits=2), dict(D=4100, ostride=4112),
                dict(R=1 << 61, stride=128), dict(R=1 << 59, ostride=1 << 20), dict(src=None), dict(out=None),
                dict(out=P + 8), dict(ostride=152), dict(data_off=0, hdr_off=128, ostride=132, out=P + 1),
                dict(data_off=2, hdr_off=0), dict(ostride=128), dict(stride=64), dict(R=-1)):
        rc, msg = quantize(**bad)
        assert rc == INVALID and msg, bad
    assert b"D=6" in quantize(D=6, bits=4)[1] and b"bit_rate=4" in quantize(D=6, bits=4)[1]
    assert b"2^63" in quantize(R=1 << 61, stride=128)[1]
    assert b"null" in quantize(src=None)[1] and b"16-B aligned" in quantize(out=P + 8)[1]
    assert quantize(R=0, src=None, out=None)[0] == 0  # nothing to do, nothing launched


@pytest.mark.parametrize("entry", ["tbe_forward_nbit_i32", "tbe_forward_nbit_i64"])
def test_lookup_entries_refuse_bad_arguments_before_any_launch(entry):
    lib = _lib.load()
    P = 0x1000

    def lookup(F=2, B=4, N=8, mode=0, out=P, out_f16=0, stride=16, feat=P, ids=P, offsets=P):
        rc = getattr(lib, entry)(feat, P, P, P, P, P, None, F, B, ids, N, offsets, None, mode, out, out_f16, stride, None, None)
        return rc, lib.tbe_last_error()

    for bad in (dict(F=0), dict(B=-1), dict(N=-1), dict(mode=2), dict(out_f16=2), dict(stride=0), dict(feat=None),
                dict(ids=None), dict(offsets=None), dict(out=None), dict(out=P + 2), dict(out=P + 1, out_f16=1)):
        rc, msg = lookup(**bad)
        assert rc == INVALID and msg, bad
    assert lookup(B=0, out=None)[0] == 0
