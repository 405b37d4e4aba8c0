"""Drop-in for the reference's `mpc_eval.py`: model-predictive control (mpc_eval.py): R rollouts of horizon Th per step, the best one's first action taken.
Same `fetch_push_control_evaluation(image_encoder, fwd_model_autoencoder, generator, dataset, config)` ->
(avg_action_error, avg_image_loss) and CLI; the loop runs on the gfx950 kernels (ndivplanning_amd/evaluation.py)."""
from ._eval_dropin import fetch
from ._eval_io import denorm, norm  # noqa: F401
from .evaluation import script_main


def fetch_push_control_evaluation(image_encoder, fwd_model_autoencoder, generator, dataset, config):
    return fetch("mpc", image_encoder, fwd_model_autoencoder, generator, dataset, config)


def main(argv=None):
    return script_main(fetch_push_control_evaluation, argv)


if __name__ == "__main__":
    main()
