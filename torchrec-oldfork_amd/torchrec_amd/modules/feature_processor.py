"""Feature processors: modules that put per-id weights on id-list features before a weighted
EmbeddingBagCollection (torchrec/modules/feature_processor.py:16-74).

Same classes, constructor, call contract and state-dict keys as the reference
(`position_weights.<feature>`, initialised to 1.0).  The position of every id inside its bag comes
from `torch.ops.fbgemm.offsets_range` (a HIP kernel of this repo) and the weight from a
`torch.gather` on the feature's parameter, so the parameter's gradient is torch's gather backward
of the per-sample-weight gradient the TBE computes (`tbe_backward_indice_weights_*`).

One deliberate difference: a bag longer than the feature's `max_length` is not an error here.
Positions `>= max_length` are clamped to the LAST entry of the parameter.  In the reference such a
bag makes `torch.gather` read out of range, which on a GPU is a device-side assert: the card is
faulted for every process that shares it.  Truncate the bags upstream if the reference's contract
(no bag exceeds `max_length`) is wanted exactly; within it the two modules agree.
"""
import abc
from typing import Dict

import torch
from torch import nn

import fbgemm_gpu  # noqa: F401  registers torch.ops.fbgemm.offsets_range

from ..sparse.jagged_tensor import JaggedTensor


class BaseFeatureProcessor(nn.Module):
    """Abstract base: Dict[feature, JaggedTensor] -> Dict[feature, JaggedTensor]."""

    @abc.abstractmethod
    def forward(self, features: Dict[str, JaggedTensor]) -> Dict[str, JaggedTensor]:
        pass


class PositionWeightedModule(BaseFeatureProcessor):
    """Weights every id of an id-list feature by a learned weight of its position in the bag.

    max_feature_lengths: feature name -> `max_length` (truncation size); the feature's parameter
    `position_weights[name]` has `max_length` entries.  Only the listed features are returned.
    """

    def __init__(self, max_feature_lengths: Dict[str, int]) -> None:
        super().__init__()
        self.max_feature_lengths = max_feature_lengths
        self.position_weights = nn.ParameterDict()
        for key, length in max_feature_lengths.items():
            if length < 1:
                raise ValueError(f"max_feature_lengths[{key!r}] = {length}: at least one position is needed")
            self.position_weights[key] = nn.Parameter(torch.ones(length))

    def forward(self, features: Dict[str, JaggedTensor]) -> Dict[str, JaggedTensor]:
        weighted: Dict[str, JaggedTensor] = {}
        for key, pos_weight in self.position_weights.items():
            jt = features[key]
            offsets = jt.offsets()
            seq = torch.ops.fbgemm.offsets_range(offsets.long(), jt.values().numel())
            seq = seq.clamp_(max=pos_weight.numel() - 1)  # see the module docstring
            weighted[key] = JaggedTensor(values=jt.values(), lengths=jt.lengths(), offsets=offsets,
                                         weights=torch.gather(pos_weight, dim=0, index=seq))
        return weighted
