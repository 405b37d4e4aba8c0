#!/usr/bin/env python3
"""Drop-in entry point with the reference's name and CLI (`python generate_trajectories.py --image-shape 128 128 ...`);
the implementation is ndivplanning_amd/generate_trajectories.py.  The normaliser attributes (o_mean, o_std, g_mean,
g_std) live on that module: set them there, or pass args.normalizer."""
from ndivplanning_amd.generate_trajectories import (generate_trajectory, main, process_inputs, render,  # noqa: F401
                                                    write_trajectory)

if __name__ == "__main__":
    main()
