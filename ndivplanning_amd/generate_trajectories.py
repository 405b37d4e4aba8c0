"""Drop-in for the reference's `generate_trajectories.py`: roll a HER actor out in a live environment and store the
trajectories (JPEG frames, states, actions, goal) as HDF5 bundles -- the data every training and evaluation script here
reads -- or, with `--bundle-format ndpt`, as the project's own bundles (ndivplanning_amd/bundle.py; no h5py).  Same `process_inputs`, `render`, `generate_trajectory(env, actor_network, args)` -> (image_frames: list of T
bytes, states [T,25], actions [T,4], desired_goal) and CLI, including the `simplify_task` / `goal_inline` branch and the
reference's order of np.random draws.

The environment steps on the host, as it must.  What the reference does per frame on the host -- PIL resize (LANCZOS) and
PIL save (`format="jpeg", quality=95`) -- happens on the device, once per trajectory: the T rendered frames go up in one
batch, ndp_resize_lanczos_u8 and ndp_jpeg_encode_u8 run on them (`LanczosResizer` -> `JpegEncoder`, both byte-identical
to PIL), and only the streams come back (`JpegEncoder.encode_to_bytes`).

Kept from the reference: the normaliser (o_mean, o_std, g_mean, g_std) is read from this module's attributes, which
`main()` sets from the pretrained model file (generate_trajectories.py:235-237); `args.normalizer`, a 4-tuple, takes
precedence when present.  The `shape` attribute of the images dataset says 500 x 500 whatever was stored
(generate_trajectories.py:199-201, :283-286).

Deviations:
  * `args.image_shape` other than (128, 128) raises ValueError: the encoder, the decoder and the networks are 128x128;
    the reference's default of 500 x 500 is not supported (the CLI's default here is 128 128);
  * `gym`, `h5py` and the HER actor (`hindsight_experience_replay`) are imported inside `main()` only and reported
    plainly when missing; nothing at import time needs them."""
import argparse
import importlib
import os

import numpy as np
import torch

from .utils.argparse_util import dir_exists_write_privileges, file_exists

IMAGE_SHAPE = (128, 128)
RECORDED_FRAME = (500, 500, 3)          # the images dataset's `shape` attribute names the camera's size, not the stored one
STATE_DIM = 25
ACTION_DIM = 4

o_mean = o_std = g_mean = g_std = None          # set by main() (or by the caller), as in the reference

_MISSING = ("generate_trajectories.main() needs the `%s` package (%s), which this package neither ships nor requires.  "
            "With an environment and an actor of your own, call generate_trajectories.generate_trajectory(env, "
            "actor_network, args) and write_trajectory(h5file, ix, image_frames, states, actions, goal) directly.")

_codec = {}


def _device_codec(device=None):
    """(LanczosResizer, JpegEncoder) of a device, made once."""
    from .jpeg import JpegEncoder
    from .resize import LanczosResizer
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _codec:
        _codec[key] = (LanczosResizer(dev), JpegEncoder(dev))
    return _codec[key]


def _standardise(values, mean, std, args):
    """Bound to +-clip_obs, standardise, bound to +-clip_range."""
    bounded = np.clip(values, -args.clip_obs, args.clip_obs)
    return np.clip((bounded - mean) / std, -args.clip_range, args.clip_range)


def process_inputs(o, g, o_mean, o_std, g_mean, g_std, args):
    """The actor's input: standardised observation, then standardised goal, as one fp32 vector."""
    halves = (_standardise(o, o_mean, o_std, args), _standardise(g, g_mean, g_std, args))
    return torch.from_numpy(np.concatenate(halves)).to(torch.float32)


def render(env):
    """The camera frame of `env` as a uint8 [H,W,3] array."""
    return env.render(mode="rgb_array")


def _check_image_shape(args):
    shape = tuple(int(v) for v in args.image_shape)
    if shape != IMAGE_SHAPE:
        raise ValueError("image_shape %s is not supported: the device JPEG encoder, the decoder and the networks are "
                         "128x128 only (the reference's default of 500 500 included); pass --image-shape 128 128" % (shape,))


def _normalizer(args):
    norm = getattr(args, "normalizer", None)
    if norm is None:
        norm = (o_mean, o_std, g_mean, g_std)
    if len(norm) != 4 or any(v is None for v in norm):
        raise ValueError("no normaliser: set generate_trajectories.o_mean / o_std / g_mean / g_std (main() reads them "
                         "from the pretrained model file) or pass args.normalizer = (o_mean, o_std, g_mean, g_std)")
    return norm


def encode_frames(frames, device=None):
    """T rendered frames (uint8 [H,W,3] each, one size) -> list of T JPEG streams: PIL's LANCZOS resize to 128x128 and
    PIL's quality-95 save, both done on the device in one batch."""
    resizer, encoder = _device_codec(device)
    batch = torch.from_numpy(np.ascontiguousarray(np.stack(frames), dtype=np.uint8))
    small, _ = resizer(batch, floats=False)
    return encoder.encode_to_bytes(small)


def _heading(angle):
    return np.array([np.cos(angle), np.sin(angle)])


def _simplified_start(env, args):
    """The `simplify_task` start: the block one block-width (0.056) from the gripper's rest position in a random
    direction, the goal further along -- on that very line 0.10-0.11 beyond the block (`goal_inline`), or 0.16-0.18 from
    the gripper within 60 degrees of it.  np.random is drawn in the reference's order: rand() for the direction, then
    uniform() once (in line) or twice (bearing, then distance).  Returns the observation of the rearranged scene."""
    rest = env.initial_gripper_xpos[:2].copy()
    angle = np.random.rand() * (2 * np.pi)
    along = _heading(angle)
    block = rest + along * 0.056
    if args.goal_inline:
        target = block + along * np.random.uniform(0.1, 0.11)
    else:
        bearing = np.random.uniform(angle - np.pi / 3, angle + np.pi / 3)
        target = rest + _heading(bearing) * np.random.uniform(0.16, 0.18)
    env.env.goal = np.hstack([target, env.height_offset])
    pose = env.sim.data.get_joint_qpos("object0:joint")
    if pose.shape != (7,):
        raise ValueError("object0:joint has a pose of shape %s, not (7,)" % (pose.shape,))
    pose[:2] = block
    env.env.sim.data.set_joint_qpos("object0:joint", pose)
    env.sim.forward()
    return env.env._get_obs()


def generate_trajectory(env, actor_network, args):
    """One rollout of `actor_network` in `env` over args.trajectory_length steps.  Returns (image_frames: list of T
    JPEG streams as bytes, states float64 [T,25], actions float64 [T,4], the desired goal of the start)."""
    _check_image_shape(args)
    norm = _normalizer(args)
    start = env.reset()
    if args.simplify_task:
        start = _simplified_start(env, args)
    state, goal = start["observation"], start["desired_goal"]
    steps = args.trajectory_length
    camera = []
    states, actions = np.empty((steps, STATE_DIM)), np.empty((steps, ACTION_DIM))
    for t in range(steps):
        camera.append(np.array(render(env), dtype=np.uint8))      # a copy: resized and encoded after the last step
        with torch.no_grad():
            action = actor_network(process_inputs(state, goal, *norm, args)).numpy().squeeze()
        states[t], actions[t] = state, action
        state = env.step(action)[0]["observation"]
    return encode_frames(camera, getattr(args, "device", None)), states, actions, start["desired_goal"]


# dataset -> (shape after T, dtype, description attribute); generate_trajectories.py:275-324
_DATASETS = (("images", (), None, "raw_pixels"),
             ("states", (STATE_DIM,), "float32", "gripper_and_object_position_velocity_rotation"),
             ("actions", (ACTION_DIM,), "float32", "action_tensor"))


def write_trajectory(h5file, ix, image_frames, states, actions, goal):
    """Group trajectory_{ix:05d} of an open h5py file, as the reference lays it out: `images` (T variable-length byte
    strings), `states` [T,25] and `actions` [T,4] in float32, each with a `description` and an int32 `shape` attribute,
    and `goal` [3] float32 without attributes; all gzip level 9."""
    steps = len(image_frames)
    packing = {"compression": "gzip", "compression_opts": 9}
    group = h5file.create_group("trajectory_{:05d}".format(ix))
    payload = {"images": image_frames, "states": states, "actions": actions}
    for name, tail, dtype, description in _DATASETS:
        typed = {} if dtype is None else {"dtype": dtype}
        ds = group.create_dataset(name, (steps,) + tail, data=payload[name], **typed, **packing)
        ds.attrs["description"] = np.bytes_(description)
        recorded = (steps,) + RECORDED_FRAME if name == "images" else payload[name].shape
        ds.attrs["shape"] = np.array(recorded, dtype="int32")
    group.create_dataset("goal", (3,), dtype="float32", data=goal, **packing)
    return group


# flag -> argparse keywords: the reference's flags and defaults (but --image-shape, see the module docstring)
_FLAGS = (
    ("--env-name", dict(type=str, default="FetchPush-v1", help="gym environment to roll out in")),
    ("--trajectory-length", dict(type=int, default=20, help="steps (and frames) per trajectory")),
    ("--simplify-task", dict(dest="simplify_task", action="store_true",
                             help="start with the block next to the gripper and the goal beyond it")),
    ("--goal-inline", dict(dest="goal_inline", action="store_true",
                           help="with --simplify-task: the goal on the line from the gripper through the block")),
    ("--pretrained_model_path", dict(type=file_exists, default="models/her_pretrained/FetchPush-v1/model.pt",
                                     help="HER checkpoint: (o_mean, o_std, g_mean, g_std, actor state)")),
    ("--clip-obs", dict(type=float, default=200, help="observations and goals are bounded to +- this")),
    ("--clip-range", dict(type=float, default=5, help="standardised actor inputs are bounded to +- this")),
    ("--num_trajectory_per_file", dict(type=int, default=1000, help="trajectories per HDF5 bundle")),
    ("--num_files", dict(type=int, default=1, help="bundles to write")),
    ("--filename_start_idx", dict(type=int, default=1, help="number of the first bundle (trajectory_bundle_00001.h5)")),
    ("--image-shape", dict(nargs=2, type=int, default=IMAGE_SHAPE,
                           help="stored frame size; only 128 128 is supported (the reference's default is 500 500)")),
    ("--outdir", dict(default="data", type=dir_exists_write_privileges, help="existing, writable directory for the bundles")),
    ("--bundle-format", dict(choices=("h5", "ndpt"), default="h5",
                             help="h5: the reference's HDF5 bundles (needs h5py); ndpt: the project's own bundles "
                                  "(ndivplanning_amd/bundle.py), trajectory_bundle_NNNNN.ndpt, no h5py")),
)


def _parser():
    parser = argparse.ArgumentParser(description="Roll a HER actor out in a gym environment and store the trajectories.")
    for flag, keywords in _FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


def _import(name, what):
    try:
        return importlib.import_module(name)
    except ImportError as e:
        raise SystemExit(_MISSING % (name.split(".")[0], what)) from e


def _make_environment(gym, name):
    """The reference's scene: both sampling ranges at 0.30 and the camera at distance 1.0, azimuth 130, elevation -40
    (the viewer exists only after a first render).  Returns (env, the sizes the HER actor is built from)."""
    env = gym.make(name)
    env.target_range = env.obj_range = 0.30
    first = env.reset()
    sizes = {"obs": first["observation"].shape[0], "goal": first["desired_goal"].shape[0],
             "action": env.action_space.shape[0], "action_max": env.action_space.high[0]}
    render(env)
    cam = env.viewer.cam
    cam.distance, cam.azimuth, cam.elevation = 1.0, 130, -40.0
    return env, sizes


def _bundle_format(argv):
    """The value of --bundle-format, read ahead of the full parse: it decides whether h5py is imported at all."""
    import sys
    ahead = argparse.ArgumentParser(add_help=False)
    ahead.add_argument("--bundle-format", choices=("h5", "ndpt"), default="h5")
    return ahead.parse_known_args(sys.argv[1:] if argv is None else argv)[0].bundle_format


def write_bundles(args, make_trajectory, open_h5=None):
    """args.num_files bundles of args.num_trajectory_per_file trajectories each, from make_trajectory() -> (image_frames,
    states, actions, goal).  A trajectory that fails is reported and left out; the bundle goes on.  open_h5: h5py.File
    for --bundle-format h5; an ndpt bundle is collected and written by ndivplanning_amd.bundle.write_bundle (a bundle
    none of whose trajectories succeeded is reported and not written)."""
    def fill(number, write):
        for ix in range(args.num_trajectory_per_file):
            try:
                write(ix, *make_trajectory())
            except Exception as e:          # the reference skips a failed trajectory too
                print("trajectory {:05d} of bundle {:05d} was not written: {}".format(ix, number, e))

    for number in range(args.filename_start_idx, args.filename_start_idx + args.num_files):
        stem = os.path.join(args.outdir, "trajectory_bundle_{:05d}".format(number))
        if args.bundle_format == "ndpt":
            from .bundle import SUFFIX, write_bundle
            kept = []
            fill(number, lambda ix, *item: kept.append(item))
            if kept:
                write_bundle(stem + SUFFIX, kept)
            else:
                print("bundle {:05d} was not written: no trajectory succeeded".format(number))
        else:
            with open_h5(stem + ".h5", "w") as bundle:
                fill(number, lambda ix, *item: write_trajectory(bundle, ix, *item))


def main(argv=None):
    """The reference's command line: args.num_files bundles of args.num_trajectory_per_file trajectories each.  A
    trajectory that fails is reported and left out; the bundle goes on."""
    global o_mean, o_std, g_mean, g_std
    fmt = _bundle_format(argv)
    gym = _import("gym", "with the FetchPush-v1 MuJoCo environment")
    h5py = _import("h5py", "to write the trajectory bundles") if fmt == "h5" else None
    her = _import("hindsight_experience_replay.rl_modules.models", "the HER actor network of the pretrained model")
    args = _parser().parse_args(argv)
    _check_image_shape(args)
    env, sizes = _make_environment(gym, args.env_name)
    o_mean, o_std, g_mean, g_std, weights = torch.load(args.pretrained_model_path, map_location="cpu")
    policy = her.actor(sizes)
    policy.load_state_dict(weights)
    policy.eval()
    write_bundles(args, lambda: generate_trajectory(env, policy, args), h5py.File if h5py is not None else None)


if __name__ == "__main__":
    main()
