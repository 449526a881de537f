"""`Batch` (torchrec/datasets/utils.py:34-61): what every dataset of this package yields and the train pipelines move."""
from dataclasses import dataclass

import torch

from ..sparse.jagged_tensor import KeyedJaggedTensor

PATH_MANAGER_KEY = "torchrec"  # accepted for signature compatibility; files are opened with plain `open`


@dataclass
class Batch:
    dense_features: torch.Tensor
    sparse_features: KeyedJaggedTensor
    labels: torch.Tensor

    def to(self, device: torch.device, non_blocking: bool = False) -> "Batch":
        return Batch(self.dense_features.to(device, non_blocking=non_blocking),
                     self.sparse_features.to(device, non_blocking=non_blocking),
                     self.labels.to(device, non_blocking=non_blocking))

    def record_stream(self, stream) -> None:
        self.dense_features.record_stream(stream)
        self.sparse_features.record_stream(stream)
        self.labels.record_stream(stream)

    def pin_memory(self) -> "Batch":
        return Batch(self.dense_features.pin_memory(), self.sparse_features.pin_memory(), self.labels.pin_memory())
