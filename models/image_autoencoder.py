"""Reference-name shim: `from models.image_autoencoder import Decoder, Encoder` (train_autoencoder.py:23, and the class
paths inside the reference's encoder_*.pt / decoder_*.pt pickles, train_gan.py:75)."""
from ndivplanning_amd.models.image_autoencoder import Decoder, Encoder, normal_init  # noqa: F401

Encoder.__module__ = __name__
Decoder.__module__ = __name__
