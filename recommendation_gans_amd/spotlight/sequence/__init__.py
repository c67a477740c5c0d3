"""Sequence models (spotlight/sequence of the reference): the pooling next-item model on the
fused HIP step."""
from .implicit import ImplicitSequenceModel

__all__ = ["ImplicitSequenceModel"]
