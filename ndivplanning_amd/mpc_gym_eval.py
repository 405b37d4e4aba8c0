"""Drop-in for the reference's `MPC_gym_eval.py`: model-predictive control against a LIVE environment, the evaluation that
yields distance to goal and success rate.  Same `fetch_push_control_evaluation(args, image_encoder,
fwd_model_autoencoder, generator, dataset, config, env)` -> (avg_action_error, avg_image_loss, avg_goal_error,
success_rate), same helper names (`render`, `get_state`, `controlled_reset`, `norm`, `denorm`) and CLI.  Per planning step
the camera frame is resized on the device exactly as PIL's Image.LANCZOS does (ndp_resize_lanczos_u8), the planner runs
on the gfx950 kernels (evaluation.plan_step) and one host synchronisation hands the action to the environment.

The environment is the caller's: `gym` is imported inside main() only.  It is used through what the reference touches and
nothing else: reset(); sim.data.get_joint_qpos / env.sim.data.set_joint_qpos("object0:joint"); sim.forward(); env.goal;
step(action); render(mode="rgb_array"); env._get_obs()["desired_goal"].

Kept from the reference, each on purpose:
  * evaluation.batch_size 1 -- one environment; any other value raises;
  * the first state of a trajectory is the dataset's frame 0, every later one the environment's rendered frame;
  * the planner's semantics (MPC_gym_eval.py:183-225): the full horizon at every step, the last predictions scored against
    the goal image, sentinel 10000000000 with strict `<`;
  * image_error = mse(get_state(env), state_fut), with the goal frame as the last step's target (:174-178, :235);
  * image_error_sum is reset per trajectory while the divisor is (T-1) * len(loader), so avg_image_loss covers only the
    last trajectory (:172, :263);
  * action_error is taken against torch.cat(best_action_list) (:254-257);
  * the goal error is sqrt(sum((DG - OP)^2)) of the desired goal and the object's position after the last step, the
    success rate its share below config.evaluation.threshold (:241-252, :265-267);
  * the seeds (torch.manual_seed, np.random.seed) and the CPU noise stream, drawn in the reference's shapes and order (noise
    kind "mpc_gym": Th pieces [R,1,nz] per planning step; one upload per trajectory).

Deviations:
  * --image-shape other than 128 128 raises: the networks take nothing else;
  * the PNG dump of the first ten trajectories (save_image_from_state, matplotlib, into results/) is behind
    `save_dir=None`: off by default, written with PIL and the reference's min-max scaling;
  * the two malformed logging.info("...", value) calls are well-formed here."""
import logging
import os

import numpy as np
import torch
from torch.utils import data

from . import evaluation as E
from ._eval_io import denorm, norm  # noqa: F401

NUM_TRAJECTORIES_TO_SAVE = 10
IMAGE_SHAPE = (128, 128)
_NO_GYM = ("MPC_gym_eval.main() needs the `gym` package with the FetchPush-v1 (MuJoCo) environment, which this package "
           "neither ships nor requires: the environment is the caller's to supply.  With an environment of your own, "
           "call MPC_gym_eval.fetch_push_control_evaluation(args, image_encoder, fwd_model_autoencoder, generator, "
           "dataset, config, env) directly.")


def render(env):
    """The environment's camera frame as a uint8 [H,W,3] array."""
    return env.render(mode="rgb_array")


def _check_image_shape(args):
    shape = tuple(int(v) for v in getattr(args, "image_shape", IMAGE_SHAPE))
    if shape != IMAGE_SHAPE:
        raise ValueError("--image-shape %d %d: the networks take 128 128 and nothing else" % shape)


_RESIZERS = {}


def _resizer(device):
    from .resize import LanczosResizer
    key = str(device)
    if key not in _RESIZERS:
        _RESIZERS[key] = LanczosResizer(device)
    return _RESIZERS[key]


def get_state(env, args, device=None):
    """The camera frame as the networks' input [1,3,128,128]: render, Image.LANCZOS resize to args.image_shape, norm
    (MPC_gym_eval.py:68-77).  Deviation: the resize runs on the device (PIL's bytes) and the result is a DEVICE tensor
    (`device`, default the current one), where the reference returns a host tensor."""
    _check_image_shape(args)
    frame = torch.from_numpy(np.ascontiguousarray(render(env)))[None]
    return _resizer(device)(frame)[1]


OBJECT_JOINT = "object0:joint"


def controlled_reset(env, states, goal):
    """Start a trajectory where the dataset's one starts (MPC_gym_eval.py:80-89): reset, put the object at the x, y of the
    first recorded state (columns 3:5), let the simulator recompute, and make the trajectory's goal the environment's."""
    env.reset()
    pose = env.sim.data.get_joint_qpos(OBJECT_JOINT)
    if pose.shape != (7,):
        raise ValueError("the object's joint pose has shape %s, expected (7,)" % (pose.shape,))
    first = np.asarray(states, dtype=np.float64)[0, 0]
    pose[0], pose[1] = first[3], first[4]
    env.env.sim.data.set_joint_qpos(OBJECT_JOINT, pose)
    env.sim.forward()
    env.env.goal = np.asarray(goal, dtype=np.float64).reshape(-1)
    return env


def goal_distance(env):
    """Euclidean distance between the desired goal and where the object lies now (MPC_gym_eval.py:241-245)."""
    wanted = np.asarray(env.env._get_obs()["desired_goal"], dtype=np.float64)
    lies = np.asarray(env.sim.data.get_joint_qpos(OBJECT_JOINT), dtype=np.float64)[:3]
    return float(np.sqrt(np.sum((wanted - lies) ** 2)))


def success_rate(distances, threshold):
    """The share of trajectories that ended closer to their goal than `threshold`."""
    return float(np.mean(np.asarray(distances) < threshold))


def save_image_from_state(state, i, image_num, save_dir):
    """results/<i>result<image_num>.png of the reference, min-max scaled, written with PIL."""
    from PIL import Image
    img = state[0].permute(1, 2, 0).cpu().numpy()
    img = (img - np.min(img)) / (np.max(img) - np.min(img))
    os.makedirs(save_dir, exist_ok=True)
    Image.fromarray((img * 255.0 + 0.5).astype(np.uint8)).save(os.path.join(save_dir, "%dresult%d.png" % (i, image_num)))


def _settings(config, dataset, generator):
    ev = config.evaluation
    seed, k, nz, bs = int(config.random_seed), int(ev.num_sample), int(ev.noise_dim), int(ev.batch_size)
    r, th, t = int(config.mpc.rollouts), int(config.mpc.time_horizon), int(dataset.seq_length)
    if bs != 1:
        raise ValueError("MPC_gym_eval drives one environment: evaluation.batch_size must be 1, got %d (several "
                         "environments at once: evaluation.MpcController)" % bs)
    if k != 1:
        raise ValueError("MPC_gym_eval needs evaluation.num_sample == 1 (MPC_gym_eval.py:215 squeezes the sample axis)")
    if r < 2:
        raise ValueError("MPC_gym_eval needs mpc.rollouts >= 2 (MPC_gym_eval.py:200 squeezes a single rollout's codes)")
    if th < 1 or t < 2:
        raise ValueError("mpc.time_horizon must be >= 1 and trajectory_length >= 2")
    if int(generator.noise_dim) != nz:
        raise ValueError("evaluation.noise_dim=%d but the generator was trained with noise_dim %d"
                         % (nz, int(generator.noise_dim)))
    return seed, k, nz, bs, r, th, t


def fetch_push_control_evaluation(args, image_encoder, fwd_model_autoencoder, generator, dataset, config, env,
                                  save_dir=None, record=None):
    """Runs the live-environment MPC evaluation.  record: None, or a list that receives one dict per planning step
    (device tensors: state_u8, rollout_errors, choice, action, image_error) for tests and diagnosis."""
    _check_image_shape(args)
    image_encoder.eval()
    fwd_model_autoencoder.eval()
    generator.eval()
    seed, k, nz, bs, r, th, t = _settings(config, dataset, generator)
    t1 = t - 1
    models = E.EvalModels(image_encoder, fwd_model_autoencoder, generator, E.device_of(config),
                          fm_precision=E.fm_precision_of(config), enc_precision=E.enc_precision_of(config))
    dev = models.device
    torch.manual_seed(seed)
    np.random.seed(seed)
    loader = data.DataLoader(dataset, batch_size=bs, shuffle=False, **E.jpeg.loader_kwargs(dataset))
    shapes = E.noise_piece_shapes("mpc_gym", bs, t, k, nz, r, th)
    per_step = E.plan_step_noise_floats(1, r, th, nz)
    cem = E.cem_from_config(config, r, th)                # the optional `mpc.cem` mapping (absent: the planner as it was)
    grad = E.grad_from_config(config, r, th)              # the optional `mpc.grad` mapping (absent: no gradient stage)
    fut_idx = torch.arange(1, t, dtype=torch.int32, device=dev)
    action_error_sum = torch.zeros(1, dtype=torch.float32, device=dev)
    image_error_sum = None
    distances = []
    ctrl = None
    for i, inputs in enumerate(loader):
        images, states, actions, goal = inputs
        env = controlled_reset(env, states, goal)
        noise = E.draw_noise(shapes, pin=True).to(dev, non_blocking=True)
        imgs, _, _ = E._frames(models, images)                                   # [T,3,128,128] on the device
        image_error_sum = torch.zeros(1, dtype=torch.float32, device=dev)         # reset per trajectory (:172)
        image_errors = torch.empty(t1, dtype=torch.float32, device=dev)
        chosen = torch.empty(t1, 4, dtype=torch.float32, device=dev)
        state = imgs[0:1]                                                         # frame 0 of the dataset (:180-181)
        for image_num in range(t1):
            if ctrl is None:
                ctrl = E.MpcController(models, r, th, seed=seed, cem=cem, grad=grad)   # the first frame tells the camera's size
            if image_num == 0:
                ctrl.reset(imgs[t1:t1 + 1])                                       # the goal, encoded once per trajectory
                ctrl.seed = seed + i * t1                                         # (read only for `cem`'s normal draws)
            take_action, info = ctrl.plan(state, noise=noise[image_num * per_step:(image_num + 1) * per_step])
            env.step(take_action.numpy().ravel())
            chosen[image_num].copy_(info["action"][0])
            state_u8, state = ctrl.observe(np.ascontiguousarray(render(env))[None])      # get_state(env, args)
            if save_dir is not None and i < NUM_TRAJECTORIES_TO_SAVE:
                save_image_from_state(state, i, image_num, save_dir)
            # image_error = mse(state_cur_mpc, state_fut): frame image_num + 1, which at the last step is the goal
            models.mse(state, imgs, 1, E.IMAGE_VALUES, b_idx=fut_idx[image_num:image_num + 1],
                       out=image_errors[image_num:image_num + 1], acc=image_error_sum)
            if record is not None:
                record.append({"state_u8": state_u8, "rollout_errors": info["rollout_errors"], "choice": info["choice"],
                               "action": take_action, "image_error": image_errors[image_num:image_num + 1]})
        distances.append(goal_distance(env))
        logging.info("results of trajectory %d", i + 1)
        logging.info("distance from the goal: %s", distances[-1])
        logging.info("success rate so far: %s", success_rate(distances, config.evaluation.threshold))
        want = actions.to(dev).float()[:, :t1].contiguous()
        models.mse(want, chosen, 1, t1 * 4, acc=action_error_sum)
    if image_error_sum is None:
        raise ValueError("the evaluation dataset is empty")
    models.finish_jpeg()
    avg_action_error = action_error_sum[0] / (t1 * len(loader))
    avg_image_loss = image_error_sum[0] / (t1 * len(loader))
    return (avg_action_error.item(), avg_image_loss.item(), float(np.mean(distances)),
            success_rate(distances, config.evaluation.threshold))


def _import_gym():
    try:
        import gym
    except ImportError as e:
        raise ImportError(_NO_GYM) from e
    return gym


def _add_arguments(parser):
    parser.add_argument("--image-shape", nargs=2, type=int, default=IMAGE_SHAPE,
                        help="Output image shape (WIDTH, HEIGHT) via PIL.Image.resize(); only 128 128 is supported")
    parser.add_argument("--camera-distance", type=float, default=1.0, help="viewer.cam.distance (reference: 1.0)")
    parser.add_argument("--camera-azimuth", type=float, default=130.0, help="viewer.cam.azimuth (reference: 130)")
    parser.add_argument("--camera-elevation", type=float, default=-40.0, help="viewer.cam.elevation (reference: -40.0)")


def _make_environment(args):
    """MPC_gym_eval.py:318-336: FetchPush-v1 with both ranges at 0.30, one render so that the viewer exists, then the
    camera.  Returns what evaluation.script_main wraps around the models: (args,) in front, (env,) behind."""
    _check_image_shape(args)
    gym = _import_gym()
    env = gym.make("FetchPush-v1")
    env.target_range = env.obj_range = 0.30
    env.reset()
    render(env)
    cam = env.viewer.cam
    cam.distance, cam.azimuth, cam.elevation = args.camera_distance, args.camera_azimuth, args.camera_elevation
    return (args,), (env,)


def main(argv=None):
    """MPC_gym_eval.py:274-349 on evaluation.script_main: the common CLI plus --image-shape and the camera, the
    environment, then the evaluation."""
    return E.script_main(fetch_push_control_evaluation, argv, add_arguments=_add_arguments, prepare=_make_environment)


if __name__ == "__main__":
    main()
