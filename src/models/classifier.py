"""Drop-in for the reference's ``src/models/classifier.py``: ``ViTClassifier`` / ``ClassificationHead`` over the MI355X
engine (the encoder is the engine's ``MaskedAutoencoder(...).encoder.vit`` node)."""
from ssrl_vit_mae_jepa_amd.classifier import ClassificationHead, ViTClassifier  # noqa: F401

__all__ = ["ClassificationHead", "ViTClassifier"]
