"""Table configuration types (torchrec/modules/embedding_configs.py:18-133)."""
import enum
from dataclasses import dataclass, field
from math import sqrt
from typing import List, Optional

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


def pooling_type_to_pooling_mode(p: PoolingType) -> PoolingMode:
    return {PoolingType.SUM: PoolingMode.SUM, PoolingType.MEAN: PoolingMode.MEAN,
            PoolingType.NONE: PoolingMode.NONE}[p]


def data_type_to_sparse_type(d: DataType) -> SparseType:
    return {DataType.FP32: SparseType.FP32, DataType.FP16: SparseType.FP16}[d]


def data_type_to_bits(d: DataType) -> int:
    """Bits per table element (the reference's DATA_TYPE_NUM_BITS, embedding_configs.py)."""
    return {DataType.FP32: 32, DataType.FP16: 16}[d]


def sharded_tables_precision(sharded, replicated, what: str):
    """The one table precision of a sharded module: None when every table is FP32 (nothing is added to the fused
    parameters then), SparseType.FP16 when every sharded (table-wise / row-wise) table is FP16.  One TBE module serves a
    rank here, so a mix raises (the reference groups tables by data type into several TBEs:
    embedding_sharding.py:412-468), and so does an FP16 DATA_PARALLEL table (dense parameters are float32)."""
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
