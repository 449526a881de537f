"""`quantize_embeddings` (torchrec/inference/modules.py:18-45): swaps every float EmbeddingBagCollection of a model for
its quantized counterpart.  PredictModule / PredictFactory and the packager are out of scope."""
from typing import Dict, List, Optional, Type

import torch
import torch.quantization as quant
from torch import nn

from ..modules.embedding_modules import EmbeddingBagCollection
from ..quant import EmbeddingBagCollection as QuantEmbeddingBagCollection


def quantize_embeddings(module: nn.Module, dtype: torch.dtype, inplace: bool,
                        additional_qconfig_spec_keys: Optional[List[Type[nn.Module]]] = None,
                        additional_mapping: Optional[Dict[Type[nn.Module], Type[nn.Module]]] = None) -> nn.Module:
    """`dtype`: torch.qint8 / quint8 (INT8 tables), torch.quint4x2 (INT4) or torch.quint2x4 (INT2)."""
    qconfig = quant.QConfig(activation=quant.PlaceholderObserver, weight=quant.PlaceholderObserver.with_args(dtype=dtype))
    qconfig_spec: Dict[Type[nn.Module], quant.QConfig] = {EmbeddingBagCollection: qconfig}
    mapping: Dict[Type[nn.Module], Type[nn.Module]] = {EmbeddingBagCollection: QuantEmbeddingBagCollection}
    for key in additional_qconfig_spec_keys or ():
        qconfig_spec[key] = qconfig
    mapping.update(additional_mapping or {})
    return quant.quantize_dynamic(module, qconfig_spec=qconfig_spec, mapping=mapping, inplace=inplace)
