"""Table configuration types (torchrec/modules/embedding_configs.py:18-133)."""
import enum
from dataclasses import dataclass, field
from math import sqrt
from typing import Dict, List, Optional

import torch
from fbgemm_gpu.split_embedding_configs import SparseType
from fbgemm_gpu.split_table_batched_embeddings_ops import PoolingMode


@enum.unique
class PoolingType(enum.Enum):
    SUM = "SUM"
    MEAN = "MEAN"
    NONE = "NONE"


@enum.unique
class DataType(enum.Enum):
    FP32 = "FP32"
    FP16 = "FP16"
    INT8 = "INT8"
    INT4 = "INT4"
    INT2 = "INT2"


DATA_TYPE_NUM_BITS: Dict[DataType, int] = {DataType.FP32: 32, DataType.FP16: 16, DataType.INT8: 8, DataType.INT4: 4,
                                           DataType.INT2: 2}
_INTEGER_DATA_TYPES = (DataType.INT8, DataType.INT4, DataType.INT2)


def dtype_to_data_type(dtype: torch.dtype) -> DataType:
    """The table data type a quantization config's weight dtype asks for (torchrec/modules/embedding_configs.py:48-56)."""
    by_dtype = {torch.qint8: DataType.INT8, torch.quint8: DataType.INT8, torch.quint4x2: DataType.INT4,
                torch.quint2x4: DataType.INT2}
    if dtype not in by_dtype:
        raise ValueError(f"Invalid data type {dtype}")
    return by_dtype[dtype]


def pooling_type_to_pooling_mode(p: PoolingType) -> PoolingMode:
    return {PoolingType.SUM: PoolingMode.SUM, PoolingType.MEAN: PoolingMode.MEAN,
            PoolingType.NONE: PoolingMode.NONE}[p]


def data_type_to_sparse_type(d: DataType) -> SparseType:
    return SparseType[d.name]


def data_type_to_bits(d: DataType) -> int:
    """Bits per table element (the reference's DATA_TYPE_NUM_BITS, embedding_configs.py)."""
    return DATA_TYPE_NUM_BITS[d]


def sharded_tables_precision(sharded, replicated, what: str):
    """The one table precision of a sharded module: None when every table is FP32 (nothing is added to the fused
    parameters then), SparseType.FP16 when every sharded (table-wise / row-wise) table is FP16.  One TBE module serves a
    rank here, so a mix raises (the reference groups tables by data type into several TBEs:
    embedding_sharding.py:412-468), and so does an FP16 DATA_PARALLEL table (dense parameters are float32).  Integer
    (quantized inference) tables are not sharded here: they raise by name."""
    quantized = [c.name for c in list(sharded) + list(replicated) if c.data_type in _INTEGER_DATA_TYPES]
    if quantized:
        raise NotImplementedError(f"{what}: tables {quantized} have an integer data type; sharded quantized collections are "
                                  "not implemented (torchrec_amd.quant.EmbeddingBagCollection serves them unsharded)")
    bad_dp = [c.name for c in replicated if c.data_type != DataType.FP32]
    if bad_dp:
        raise NotImplementedError(f"{what}: DATA_PARALLEL tables {bad_dp} ask for {DataType.FP16.value} storage; replicated "
                                  "tables are dense float32 parameters (shard them table-wise / row-wise, or use FP32)")
    kinds = {c.data_type for c in sharded}
    if len(kinds) > 1:
        by = {k.value: [c.name for c in sharded if c.data_type == k] for k in sorted(kinds, key=lambda k: k.value)}
        raise NotImplementedError(f"{what}: sharded tables of different data types on one module ({by}); one fused "
                                  "lookup serves a rank, so all of its tables share one storage precision")
    if kinds == {DataType.FP16}:
        return SparseType.FP16
    return None


@dataclass
class BaseEmbeddingConfig:
    num_embeddings: int
    embedding_dim: int
    name: str = ""
    data_type: DataType = DataType.FP32
    feature_names: List[str] = field(default_factory=list)
    weight_init_max: Optional[float] = None
    weight_init_min: Optional[float] = None

    def get_weight_init_max(self) -> float:
        # default U(-sqrt(1/N), sqrt(1/N)) — embedding_configs.py:102-112
        return sqrt(1 / self.num_embeddings) if self.weight_init_max is None else self.weight_init_max

    def get_weight_init_min(self) -> float:
        return -sqrt(1 / self.num_embeddings) if self.weight_init_min is None else self.weight_init_min

    def num_features(self) -> int:
        return len(self.feature_names)


@dataclass
class EmbeddingBagConfig(BaseEmbeddingConfig):
    pooling: PoolingType = PoolingType.SUM


@dataclass
class EmbeddingConfig(BaseEmbeddingConfig):
    pass
