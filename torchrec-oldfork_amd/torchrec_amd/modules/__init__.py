from .feature_processor import BaseFeatureProcessor, PositionWeightedModule  # noqa: F401
from .crossnet import CrossNet, LowRankCrossNet, VectorCrossNet  # noqa: F401
