"""Quantized EmbeddingBagCollection for inference on the MI355X path (torchrec/quant/embedding_modules.py:90-286).

Same constructor, `from_float`, `forward(KeyedJaggedTensor) -> KeyedTensor` (float32 values), `embedding_bag_configs`,
`is_weighted` and state-dict keys (`embedding_bags.<table>.weight`) as the reference's module.  The deliberate difference:
the reference builds one IntNBitTableBatchedEmbeddingBagsCodegen per table and loops over features; here ONE module holds
every table of the collection, so a forward is one launch whatever the tables' dims and bit rates, and the
KeyedJaggedTensor's int64 values and offsets go to the kernel as they are.  There is no CPU compute path."""
import copy
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Tuple

import torch
from fbgemm_gpu.split_embedding_configs import SparseType
from fbgemm_gpu.split_table_batched_embeddings_ops import EmbeddingLocation, IntNBitTableBatchedEmbeddingBagsCodegen
from torch import nn

from ..modules.embedding_configs import (DataType, EmbeddingBagConfig, data_type_to_sparse_type, dtype_to_data_type,
                                         pooling_type_to_pooling_mode)
from ..modules.embedding_modules import EmbeddingBagCollection as FloatEmbeddingBagCollection
from ..sparse.jagged_tensor import KeyedJaggedTensor, KeyedTensor

_QUANTIZED = (DataType.INT8, DataType.INT4, DataType.INT2)


class EmbeddingBagCollection(nn.Module):
    def __init__(self, table_name_to_quantized_weights: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]],
                 embedding_configs: List[EmbeddingBagConfig], is_weighted: bool, device: torch.device) -> None:
        super().__init__()
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"quant.EmbeddingBagCollection on device '{device}': quantized tables are served on a HIP "
                               "device only (no CPU compute path, and a 'meta' collection has no weights to quantize)")
        self._is_weighted = is_weighted
        embedding_configs = [copy.copy(cfg) for cfg in embedding_configs]  # feature_names is filled in below: not in the caller's
        self._embedding_bag_configs: List[EmbeddingBagConfig] = embedding_configs
        self._feature_names: List[str] = []
        self._lengths_per_embedding: List[int] = []
        ftm: List[int] = []
        names = set()
        for t, cfg in enumerate(embedding_configs):
            if cfg.name in names:
                raise ValueError(f"Duplicate table name {cfg.name}")
            names.add(cfg.name)
            if cfg.data_type not in _QUANTIZED:
                raise ValueError(f"table {cfg.name}: data_type {cfg.data_type} is not a quantized type")
            if not cfg.feature_names:
                cfg.feature_names = [cfg.name]
            for f in cfg.feature_names:
                self._feature_names.append(f)
                self._lengths_per_embedding.append(cfg.embedding_dim)
                ftm.append(t)
        poolings = {cfg.pooling for cfg in embedding_configs}
        if len(poolings) != 1:
            raise ValueError("all tables of a quantized collection must share one pooling type")
        with torch.cuda.device(device):
            self._tbe = IntNBitTableBatchedEmbeddingBagsCodegen(
                embedding_specs=[(cfg.name, cfg.num_embeddings, cfg.embedding_dim, data_type_to_sparse_type(cfg.data_type),
                                  EmbeddingLocation.DEVICE) for cfg in embedding_configs],
                feature_table_map=ftm, pooling_mode=pooling_type_to_pooling_mode(embedding_configs[0].pooling),
                weight_lists=([table_name_to_quantized_weights[cfg.name] for cfg in embedding_configs]
                              if table_name_to_quantized_weights is not None else None),
                device=device, output_dtype=SparseType.FP32, row_alignment=16)

    def forward(self, features: KeyedJaggedTensor) -> KeyedTensor:
        if features.keys() != self._feature_names:
            features = features.permute([features.keys().index(k) for k in self._feature_names])
        out = self._tbe(features.values(), features.offsets(), features.weights_or_none() if self._is_weighted else None)
        return KeyedTensor(keys=self._feature_names, length_per_key=self._lengths_per_embedding, values=out)

    def gather_interaction(self, features: KeyedJaggedTensor):
        """For a batch the dot interaction can gather itself (models/dlrm.py, tbe_dlrm_interaction_gather_forward_nbit):
        (the fused module's gather_interaction_args(), the ids [F * B] feature-major, B).  None — nothing consumed, the
        caller runs forward() — unless the collection is unweighted, its tables share one bit rate and dim, and the batch
        has this collection's keys in order, exactly one id per bag as host-known metadata (fixed_lengths() all 1) and int64
        values on the tables' device."""
        if self._is_weighted or features.keys() != self._feature_names:
            return None
        fixed = features.fixed_lengths()
        values = features.values()
        if (fixed is None or any(n != 1 for n in fixed) or values.dtype != torch.int64
                or values.device != self._tbe.weights.device):
            return None
        args = self._tbe.gather_interaction_args()
        if args is None:
            return None
        return args, values.contiguous().view(-1), features.stride()

    def state_dict(self, destination: Optional[Dict[str, Any]] = None, prefix: str = "", keep_vars: bool = False):
        if destination is None:
            destination = OrderedDict()
            destination._metadata = OrderedDict()
        rows = self._tbe.split_embedding_weights(split_scale_shifts=False)
        for cfg, (weight, _) in zip(self._embedding_bag_configs, rows):
            destination[prefix + f"embedding_bags.{cfg.name}.weight"] = weight
        return destination

    def _get_name(self) -> str:
        return "QuantizedEmbeddingBagCollection"

    @classmethod
    def from_float(cls, module: FloatEmbeddingBagCollection) -> "EmbeddingBagCollection":
        """The float collection's tables, quantized to the data type its `qconfig` weight observer names.  Each table goes
        through the quantizer kernel once, straight into the fused module's table-layout buffer."""
        assert hasattr(module, "qconfig"), "EmbeddingBagCollection input float module must have qconfig defined"
        data_type = dtype_to_data_type(module.qconfig.weight().dtype)
        configs = copy.deepcopy(module.embedding_bag_configs)
        for cfg in configs:
            cfg.data_type = data_type
        device = getattr(module, "_device", torch.device("cpu"))
        if device.type != "cuda":
            raise RuntimeError(f"quant.EmbeddingBagCollection.from_float: the float collection is on device '{device}'; "
                               "only a collection on a HIP device has weights to quantize (no CPU compute path)")
        quantized = cls(None, configs, module.is_weighted, device)
        weights = module.table_weights()
        for t, cfg in enumerate(configs):
            quantized._tbe.quantize_table_(t, weights[cfg.name])
        return quantized

    @property
    def embedding_bag_configs(self) -> List[EmbeddingBagConfig]:
        return self._embedding_bag_configs

    @property
    def is_weighted(self) -> bool:
        return self._is_weighted
