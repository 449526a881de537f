"""SimpleDeepFMNN and its arches with the reference's constructors, assertions and module tree (torchrec/models/deepfm.py:
SparseArch :17-66, DenseArch :69-111, FMInteractionArch :114-184, OverArch :187-216, SimpleDeepFMNN :219-346), so a
reference state_dict loads unchanged (`dense_arch.model.0.weight`, `inter_arch.deep_fm.dense_module.0.weight`,
`over_arch.model.0.weight`, `sparse_arch.embedding_bag_collection...`).

FMInteractionArch is where the fusion pays: on a HIP device, for float32 inputs, when `sparse_feature_names` are the
KeyedTensor's keys in order, `dense` and `sparse_features.values()` go as TWO segments through one autograd.Function whose
forward (csrc/deepfm.hip) reads them once and yields both the deep branch's input and the FM term, and whose backward is
one kernel that turns the two output gradients into the two input gradients.  In any other key order the per-feature
views go through the same kernels as a list (modules/deepfm.py), and CPU tensors or other dtypes take the reference's
torch expression.  The nn.Linear layers are torch's."""
from typing import List

import torch
from torch import nn

from ..modules.deepfm import DeepFM, FactorizationMachine, _kernel_inputs, fm_and_cat
from ..modules.embedding_modules import EmbeddingBagCollection
from ..sparse.jagged_tensor import KeyedJaggedTensor, KeyedTensor


class SparseArch(nn.Module):
    """The embedding lookups of every feature (torchrec/models/deepfm.py:17-66)."""

    def __init__(self, embedding_bag_collection: EmbeddingBagCollection) -> None:
        super().__init__()
        self.embedding_bag_collection: EmbeddingBagCollection = embedding_bag_collection

    def forward(self, features: KeyedJaggedTensor) -> KeyedTensor:
        pooled = self.embedding_bag_collection(features)
        # a sharded collection (DistributedModelParallel) hands out an awaitable; the reference's is a LazyAwaitable that
        # resolves itself at first use
        return pooled.wait() if hasattr(pooled, "wait") else pooled


class DenseArch(nn.Module):
    """Linear - ReLU - Linear - ReLU onto the embedding dimension (torchrec/models/deepfm.py:69-111)."""

    def __init__(self, in_features: int, hidden_layer_size: int, embedding_dim: int) -> None:
        super().__init__()
        self.model: nn.Module = nn.Sequential(
            nn.Linear(in_features, hidden_layer_size),
            nn.ReLU(),
            nn.Linear(hidden_layer_size, embedding_dim),
            nn.ReLU(),
        )

    def forward(self, features: torch.Tensor) -> torch.Tensor:
        return self.model(features)


class FMInteractionArch(nn.Module):
    """cat(dense, deep_fm(dense + sparse), fm(dense + sparse)): [B, D + DI + 1] (torchrec/models/deepfm.py:114-184)."""

    def __init__(self, fm_in_features: int, sparse_feature_names: List[str], deep_fm_dimension: int) -> None:
        super().__init__()
        self.sparse_feature_names: List[str] = sparse_feature_names
        self.deep_fm = DeepFM(
            dense_module=nn.Sequential(
                nn.Linear(fm_in_features, deep_fm_dimension),
                nn.ReLU(),
            )
        )
        self.fm = FactorizationMachine()

    def forward(self, dense_features: torch.Tensor, sparse_features: KeyedTensor) -> torch.Tensor:
        if len(self.sparse_feature_names) == 0:
            return dense_features
        if list(self.sparse_feature_names) == list(sparse_features.keys()) and sparse_features.key_dim() == 1:
            flat = _kernel_inputs([dense_features, sparse_features.values()])
            if flat is not None and dense_features.dim() == 2 and sparse_features.values().dim() == 2:
                fm_interaction, deep_input = fm_and_cat(flat, True)  # one read: the deep branch's input and the FM term
                deep_interaction = self.deep_fm.dense_module(deep_input)
                return torch.cat([dense_features, deep_interaction, fm_interaction], dim=1)
        tensor_list: List[torch.Tensor] = [dense_features]
        for feature_name in self.sparse_feature_names:
            tensor_list.append(sparse_features[feature_name])
        deep_interaction = self.deep_fm(tensor_list)
        fm_interaction = self.fm(tensor_list)
        return torch.cat([dense_features, deep_interaction, fm_interaction], dim=1)


class OverArch(nn.Module):
    """Linear to one target, then Sigmoid (torchrec/models/deepfm.py:187-216)."""

    def __init__(self, in_features: int) -> None:
        super().__init__()
        self.model: nn.Module = nn.Sequential(
            nn.Linear(in_features, 1),
            nn.Sigmoid(),
        )

    def forward(self, features: torch.Tensor) -> torch.Tensor:
        return self.model(features)


class SimpleDeepFMNN(nn.Module):
    """Pooled embeddings + a dense projection into the same space, the DeepFM interaction, one logit
    (torchrec/models/deepfm.py:219-346)."""

    def __init__(self, num_dense_features: int, embedding_bag_collection: EmbeddingBagCollection, hidden_layer_size: int,
                 deep_fm_dimension: int) -> None:
        super().__init__()
        assert len(embedding_bag_collection.embedding_bag_configs) > 0, "At least one embedding bag is required"
        for i in range(1, len(embedding_bag_collection.embedding_bag_configs)):
            conf_prev = embedding_bag_collection.embedding_bag_configs[i - 1]
            conf = embedding_bag_collection.embedding_bag_configs[i]
            assert conf_prev.embedding_dim == conf.embedding_dim, "All EmbeddingBagConfigs must have the same dimension"
        embedding_dim: int = embedding_bag_collection.embedding_bag_configs[0].embedding_dim

        feature_names = []
        fm_in_features = embedding_dim
        for conf in embedding_bag_collection.embedding_bag_configs:
            for feat in conf.feature_names:
                feature_names.append(feat)
                fm_in_features += conf.embedding_dim

        self.sparse_arch = SparseArch(embedding_bag_collection)
        self.dense_arch = DenseArch(in_features=num_dense_features, hidden_layer_size=hidden_layer_size,
                                    embedding_dim=embedding_dim)
        self.inter_arch = FMInteractionArch(fm_in_features=fm_in_features, sparse_feature_names=feature_names,
                                            deep_fm_dimension=deep_fm_dimension)
        over_in_features = embedding_dim + deep_fm_dimension + 1
        self.over_arch = OverArch(over_in_features)

    def forward(self, dense_features: torch.Tensor, sparse_features: KeyedJaggedTensor) -> torch.Tensor:
        embedded_dense = self.dense_arch(dense_features)
        embedded_sparse = self.sparse_arch(sparse_features)
        concatenated_dense = self.inter_arch(dense_features=embedded_dense, sparse_features=embedded_sparse)
        logits = self.over_arch(concatenated_dense)
        return logits
