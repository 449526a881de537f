"""Quantized (INT8 / INT4 / INT2) inference modules (torchrec/quant/__init__.py)."""
from .embedding_modules import EmbeddingBagCollection  # noqa: F401
