from .feature_processor import BaseFeatureProcessor, PositionWeightedModule  # noqa: F401
