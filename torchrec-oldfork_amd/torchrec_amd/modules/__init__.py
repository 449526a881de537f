from .feature_processor import BaseFeatureProcessor, PositionWeightedModule  # noqa: F401
from .crossnet import CrossNet, LowRankCrossNet, LowRankMixtureCrossNet, VectorCrossNet  # noqa: F401
from .deepfm import DeepFM, FactorizationMachine  # noqa: F401
from .activation import SwishLayerNorm  # noqa: F401
from .utils import extract_module_or_tensor_callable  # noqa: F401
from .loss import CrossEntropyLoss, cross_entropy  # noqa: F401
