"""Drop-in for the reference's ``src/training/classifier.py``: ``ViTClassifierTrainModule`` with the native fused step."""
from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule  # noqa: F401

__all__ = ["ViTClassifierTrainModule"]
