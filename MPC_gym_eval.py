#!/usr/bin/env python3
"""Drop-in entry point with the reference's name and CLI (`python MPC_gym_eval.py --config-file config/evaluation.yaml`);
the implementation is ndivplanning_amd/mpc_gym_eval.py.  With an environment of your own, import
`fetch_push_control_evaluation` from here and pass it as `env`."""
import models.forward_encoder  # noqa: F401  (the class paths inside the training scripts' pickles)
import models.gan  # noqa: F401
import models.image_autoencoder  # noqa: F401
from ndivplanning_amd.mpc_gym_eval import (controlled_reset, denorm, fetch_push_control_evaluation, get_state,  # noqa: F401
                                           main, norm, render, save_image_from_state)

if __name__ == "__main__":
    main()
