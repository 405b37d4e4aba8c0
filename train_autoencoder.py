#!/usr/bin/env python3
"""Drop-in entry point with the reference's name (`python train_autoencoder.py`); the implementation is
ndivplanning_amd/train_autoencoder.py."""
import models.image_autoencoder  # noqa: F401  (binds the reference class paths for the checkpoints)
from ndivplanning_amd.train_autoencoder import denorm, main, norm, train  # noqa: F401

if __name__ == "__main__":
    main()
