"""A batched push world of the project's own (include/ndp.h "push world"): a gripper, a block and a
goal on a table, the reference's 4-component actions, n environments at once ON THE DEVICE.  One launch per environment
step (ndp_world_step_render) advances the physics and writes the camera frames as the [n,S,S,3] bytes every kernel here
reads; there is no host round trip.

    world = PushWorld(n, "cuda:0")                 # seeded starts, "simplified" or "scattered"
    frames = world.step(actions)                   # [n,S,S,3] bytes on the device
    actions = expert_actions(world.state)          # the scripted expert, torch ops (CPU or device tensors)
    env = GymPushEnv(world)                        # the gym protocol MPC_gym_eval / generate_trajectories use
    generate(1000, "data")                         # .ndpt bundles for every trainer
    evaluate_mpc(models, 16, 14, rollouts, horizon)   # expert / random / MPC goal distances and success rates

Command line:
    python -m ndivplanning_amd.push_world generate N DIR [--steps T --seed S --epsilon E --start KIND]
    python -m ndivplanning_amd.push_world mpc --config-file config/evaluation.yaml [--envs B --steps T --start KIND]
"""
import os
import sys

import numpy as np
import torch

from . import _capi

# include/ndp.h, NDP_WORLD_*
X0, Y0, SIDE = 1.09, 0.50, 0.50
REST = (1.34, 0.75)
Z_MIN, Z_MAX, Z_CONTACT = 0.42, 0.60, 0.47
OBJECT_Z = 0.425
R_G, R_O = 0.02, 0.03
R = R_G + R_O
STEP, SUB = 0.05, 4
MAX_ENVS = 65535
STARTS = ("simplified", "scattered")
Z_LOW, Z_HIGH = 0.44, 0.53            # the heights the starts and the expert use: pushing and carrying
STATE_DIM = 8
OBS_DIM = 25
SUCCESS_THRESHOLD = 0.05              # config/evaluation.yaml: evaluation.threshold


# ------------------------------------------------------------------------------------------------------------ checks
def _check_size(frame_size):
    s = int(frame_size)
    if s != frame_size or s < 32 or s > 1024 or s % 4:
        raise ValueError("frame_size=%r: a multiple of 4 in 32..1024" % (frame_size,))
    return s


def _check_n(n):
    if int(n) != n or int(n) < 1 or int(n) > MAX_ENVS:
        raise ValueError("n=%r environments: 1..%d" % (n, MAX_ENVS))
    return int(n)


def _check_start(start):
    if start not in STARTS:
        raise ValueError("start=%r: one of %s" % (start, ", ".join(STARTS)))
    return start


def _check_epsilon(epsilon):
    e = float(epsilon)
    if not 0.0 <= e <= 1.0:
        raise ValueError("epsilon=%r outside [0, 1]" % (epsilon,))
    return e


def _check_actions(actions, n):
    a = torch.as_tensor(actions)
    if tuple(a.shape) != (n, 4):
        raise ValueError("actions must be [%d,4], got %s" % (n, tuple(a.shape)))
    return a


# ------------------------------------------------------------------------------------------------------------ starts
def _heading(angle):
    return np.array([np.cos(angle), np.sin(angle)])


def _start(kind, seed, index):
    rng = np.random.default_rng([int(seed), int(index)])
    rest = np.array(REST)
    if kind == "simplified":
        # what the reference's simplify_task does (generate_trajectories._simplified_start)
        angle = rng.random() * (2 * np.pi)
        along = _heading(angle)
        block = rest + 0.056 * along
        if rng.random() < 0.5:
            goal = block + along * rng.uniform(0.10, 0.11)
        else:
            bearing = rng.uniform(angle - np.pi / 3, angle + np.pi / 3)
            goal = rest + _heading(bearing) * rng.uniform(0.16, 0.18)
        gripper = (rest[0], rest[1], Z_LOW)
    else:
        block = rest + rng.uniform(-0.12, 0.12, size=2)
        offset = rng.uniform(0.06, 0.15, size=2) * rng.choice([-1.0, 1.0], size=2)
        goal = block + offset
        lo, hi = np.array([X0 + R_O, Y0 + R_O]), np.array([X0 + SIDE - R_O, Y0 + SIDE - R_O])
        goal = np.where((goal < lo) | (goal > hi), block - offset, goal)        # mirrored where it leaves the table
        near = rest + rng.uniform(-0.02, 0.02, size=2)
        gripper = (near[0], near[1], Z_HIGH)
    return [gripper[0], gripper[1], gripper[2], block[0], block[1], OBJECT_Z, goal[0], goal[1]]


def starts(kind, seed, indices):
    """Start states float32 [m,8] of the environments `indices`: a function of (kind, seed, index) alone, whatever the
    number of environments."""
    _check_start(kind)
    if int(seed) < 0:
        raise ValueError("seed=%r must be >= 0" % (seed,))
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    if idx.size and idx.min() < 0:
        raise ValueError("start indices must be >= 0")
    return np.array([_start(kind, seed, i) for i in idx], dtype=np.float32).reshape(-1, STATE_DIM)


# ------------------------------------------------------------------------------------------------------------ expert
def _towards(delta):
    """A move of `delta` [n,3] metres as an action: delta / STEP, scaled down where a component would exceed 1 (the
    direction stays, and a move that fits lands exactly on the target)."""
    a = delta / STEP
    return a / a.abs().amax(dim=1, keepdim=True).clamp_min(1.0)


def expert_actions(state, uniform=None, epsilon=0.0):
    """The scripted expert: state [n,8] -> actions [n,4], torch ops on whatever device `state` is on, stateless.

    With u the unit vector block -> goal and pre = o - u * (R + 0.02), in this order: within 1 cm of the goal rise; low,
    behind the block and less than 12 mm off the line, move towards goal - u * R (push); at pre (within 8 mm) descend;
    low with the straight path to pre passing closer than R + 5 mm to the block, rise; otherwise move towards pre.
    epsilon: with that probability per environment the action is 2 * uniform[:, 0:4] - 1 instead; uniform [n,5] in
    [0,1) (column 4 decides), drawn with torch.rand on the state's device where None."""
    epsilon = _check_epsilon(epsilon)
    s = torch.as_tensor(state)
    if s.dim() != 2 or int(s.shape[1]) != STATE_DIM:
        raise ValueError("state must be [n,8], got %s" % (tuple(s.shape),))
    s = s.to(torch.float64)
    n = int(s.shape[0])
    g, gz, o, t = s[:, 0:2], s[:, 2], s[:, 3:5], s[:, 6:8]
    to_goal = t - o
    dist = to_goal.norm(dim=1)
    u = to_goal / dist.clamp_min(1e-9)[:, None]
    pre = o - u * (R + 0.02)
    low = gz < Z_CONTACT
    rel = o - g
    behind = (rel * u).sum(dim=1) > 0
    off_line = (rel[:, 0] * u[:, 1] - rel[:, 1] * u[:, 0]).abs()
    to_pre = pre - g
    at_pre = to_pre.norm(dim=1) < 0.008
    # the distance from the block to the segment g -> pre
    seg2 = (to_pre * to_pre).sum(dim=1)
    frac = ((rel * to_pre).sum(dim=1) / seg2.clamp_min(1e-18)).clamp(0.0, 1.0)
    blocked = (rel - frac[:, None] * to_pre).norm(dim=1) < R + 0.005

    zero = torch.zeros_like(gz)
    rise = torch.stack([zero, zero, (Z_HIGH - gz).clamp_min(0.0)], dim=1)
    push = torch.cat([t - u * R - g, zero[:, None]], dim=1)
    descend = torch.cat([to_pre, (Z_LOW - gz)[:, None]], dim=1)
    approach = torch.cat([to_pre, zero[:, None]], dim=1)
    delta = approach
    delta = torch.where((low & blocked)[:, None], rise, delta)
    delta = torch.where(at_pre[:, None], descend, delta)
    delta = torch.where((low & behind & (off_line < 0.012))[:, None], push, delta)
    delta = torch.where((dist < 0.01)[:, None], rise, delta)
    act = torch.cat([_towards(delta), zero[:, None]], dim=1).to(torch.float32)
    if epsilon > 0.0:
        if uniform is None:
            uniform = torch.rand(n, 5, device=s.device)
        uni = torch.as_tensor(uniform).to(device=s.device, dtype=torch.float32)
        if tuple(uni.shape) != (n, 5):
            raise ValueError("uniform must be [%d,5], got %s" % (n, tuple(uni.shape)))
        act = torch.where((uni[:, 4] < epsilon)[:, None], 2.0 * uni[:, 0:4] - 1.0, act)
    return act


# ------------------------------------------------------------------------------------------------------------- world
class PushWorld:
    """n push environments on `device`.  The state [n,8] (gx, gy, gz, ox, oy, oz, tx, ty) is double-buffered on the
    device; step() is ONE launch that reads one buffer, writes the other and draws the frames of the new state."""

    def __init__(self, n, device, frame_size=128, seed=0, start="simplified"):
        self.n, self.size, self.start = _check_n(n), _check_size(frame_size), _check_start(start)
        if int(seed) < 0:
            raise ValueError("seed=%r must be >= 0" % (seed,))
        self.seed = int(seed)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _capi.NdpError("PushWorld runs on a ROCm GPU only (got %s)" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _capi.load()
        self._buffers = [torch.zeros(self.n, STATE_DIM, dtype=torch.float32, device=self.device) for _ in range(2)]
        self._cur = 0
        self.start_index = np.arange(self.n, dtype=np.int64)
        self.reset(render=False)

    # -- state
    @property
    def state(self):
        """The current state [n,8] on the device (a view of the current buffer: clone it to keep it across a step)."""
        return self._buffers[self._cur]

    def set_state(self, state):
        s = torch.as_tensor(state, dtype=torch.float32)
        if tuple(s.shape) != (self.n, STATE_DIM):
            raise ValueError("state must be [%d,8], got %s" % (self.n, tuple(s.shape)))
        self._buffers[self._cur].copy_(s)

    def reset(self, seed=None, index=None, render=True):
        """Put every environment at its seeded start.  index: None (environment i starts at start i), an int (i starts
        at start index + i) or n start indices.  Returns the frames unless render is False."""
        if seed is not None:
            if int(seed) < 0:
                raise ValueError("seed=%r must be >= 0" % (seed,))
            self.seed = int(seed)
        if index is None:
            idx = np.arange(self.n, dtype=np.int64)
        elif np.ndim(index) == 0:
            idx = int(index) + np.arange(self.n, dtype=np.int64)
        else:
            idx = np.asarray(index, dtype=np.int64).reshape(-1)
            if idx.shape != (self.n,):
                raise ValueError("index must hold %d start indices, got %d" % (self.n, idx.size))
        self.start_index = idx
        self.set_state(torch.from_numpy(starts(self.start, self.seed, idx)))
        return self.render() if render else None

    def observation(self):
        """[n,25] on the device, the reference's layout: 0:3 gripper, 3:6 object, 6:9 object - gripper, the rest zero."""
        s = self.state
        obs = torch.zeros(self.n, OBS_DIM, dtype=torch.float32, device=self.device)
        obs[:, 0:6] = s[:, 0:6]
        obs[:, 6:9] = s[:, 3:6] - s[:, 0:3]
        return obs

    def goal3(self):
        s = self.state
        return torch.cat([s[:, 6:8], torch.full((self.n, 1), OBJECT_Z, dtype=torch.float32, device=self.device)], dim=1)

    def goal_distance(self):
        s = self.state
        return (s[:, 3:5] - s[:, 6:8]).norm(dim=1)

    def success(self, threshold=SUCCESS_THRESHOLD):
        return self.goal_distance() < float(threshold)

    # -- launches
    def _frames(self, out):
        shape = (self.n, self.size, self.size, 3)
        if out is None:
            return torch.empty(shape, dtype=torch.uint8, device=self.device)
        if (out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != self.device or not out.is_contiguous()
                or out.data_ptr() % 4):
            raise ValueError("out must be a contiguous, 4-byte aligned uint8 %s tensor on %s" % (shape, self.device))
        return out

    def render(self, out=None):
        """The frames [n,S,S,3] of the current state, one launch."""
        frames = self._frames(out)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_world_render(_capi.ptr(self.state), self.n, self.size, _capi.ptr(frames),
                                                  _capi.stream_ptr(self.device)), "ndp_world_render")
        return frames

    def step(self, actions, out=None, render=True):
        """Advance every environment by actions [n,4] (host or device) and return the new frames [n,S,S,3] (None with
        render=False: the step then writes no frame).  One launch."""
        a = _check_actions(actions, self.n)
        a = a.to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
        frames = self._frames(out) if render else None
        nxt = 1 - self._cur
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_world_step_render(_capi.ptr(self._buffers[self._cur]), _capi.ptr(a), self.n, self.size,
                                                       _capi.ptr(self._buffers[nxt]), _capi.ptr(frames),
                                                       _capi.stream_ptr(self.device)), "ndp_world_step_render")
        self._cur = nxt
        return frames


# --------------------------------------------------------------------------------------------------- the gym protocol
OBJECT_JOINT = "object0:joint"


class _Data:
    def __init__(self, env):
        self._env = env

    def get_joint_qpos(self, name):
        if name != OBJECT_JOINT:
            raise KeyError(name)
        row = self._env._row()
        return np.array([row[3], row[4], row[5], 1.0, 0.0, 0.0, 0.0], dtype=np.float64)

    def set_joint_qpos(self, name, value):
        if name != OBJECT_JOINT:
            raise KeyError(name)
        pose = np.asarray(value, dtype=np.float64).reshape(7)
        self._env._write({3: pose[0], 4: pose[1], 5: pose[2]})


class _Sim:
    def __init__(self, env):
        self.data = _Data(env)

    def forward(self):
        pass                                     # nothing is derived from the state: there is nothing to recompute


class GymPushEnv:
    """Environment `index` of a PushWorld behind the gym protocol that MPC_gym_eval and generate_trajectories use, and
    nothing more: reset(), step(action) -> (obs, 0.0, False, {}), render(mode="rgb_array"), sim.data.get_joint_qpos /
    env.sim.data.set_joint_qpos("object0:joint"), sim.forward(), a settable env.goal, env._get_obs(),
    initial_gripper_xpos and height_offset.  The other environments of the world get zero actions.  Every reset() takes
    the next seeded start of the world's kind."""

    def __init__(self, world, index=0):
        if not 0 <= int(index) < world.n:
            raise ValueError("index=%r outside the world's %d environments" % (index, world.n))
        self.world, self.index = world, int(index)
        self.env = self                          # gym's wrapper and the wrapped environment in one
        self.sim = _Sim(self)
        self.initial_gripper_xpos = np.array([REST[0], REST[1], Z_LOW], dtype=np.float64)
        self.height_offset = OBJECT_Z
        self.episodes = 0

    def _row(self):
        return self.world.state[self.index].cpu().numpy().astype(np.float64)

    def _write(self, columns):
        state = self.world.state.clone()
        for col, value in columns.items():
            state[self.index, col] = float(value)
        self.world.set_state(state)

    @property
    def goal(self):
        row = self._row()
        return np.array([row[6], row[7], OBJECT_Z], dtype=np.float64)

    @goal.setter
    def goal(self, value):
        v = np.asarray(value, dtype=np.float64).reshape(-1)
        self._write({6: v[0], 7: v[1]})

    def reset(self):
        first = int(self.world.start_index[self.index])
        row = starts(self.world.start, self.world.seed, [first + self.episodes * self.world.n])[0]
        self.episodes += 1
        self._write({c: row[c] for c in range(STATE_DIM)})
        return self._get_obs()

    def _get_obs(self):
        row = self._row()
        obs = np.zeros(OBS_DIM, dtype=np.float64)
        obs[0:6] = row[0:6]
        obs[6:9] = row[3:6] - row[0:3]
        return {"observation": obs, "achieved_goal": row[3:6].copy(),
                "desired_goal": np.array([row[6], row[7], OBJECT_Z], dtype=np.float64)}

    def step(self, action):
        a = np.asarray(action, dtype=np.float32).reshape(-1)
        if a.shape != (4,):
            raise ValueError("action must have 4 components, got %s" % (a.shape,))
        actions = torch.zeros(self.world.n, 4, dtype=torch.float32)
        actions[self.index] = torch.from_numpy(a)
        self.world.step(actions, render=False)
        return self._get_obs(), 0.0, False, {}

    def render(self, mode="human"):
        if mode != "rgb_array":
            raise ValueError("render(mode=%r): only \"rgb_array\"" % (mode,))
        return self.world.render()[self.index].cpu().numpy()


# ------------------------------------------------------------------------------------------------------ data generator
def _check_generate(n, steps, epsilon, start, batch, per_file, frame_size):
    if int(n) != n or int(n) < 1:
        raise ValueError("n=%r trajectories: at least 1" % (n,))
    if int(steps) < 1 or int(batch) < 1 or int(per_file) < 1:
        raise ValueError("steps, batch and per_file must be >= 1")
    _check_n(min(int(batch), int(n)))
    _check_start(start)
    if _check_size(frame_size) != 128:
        raise ValueError("frame_size=%r: the JPEG encoder, the decoder and the networks take 128 and nothing else"
                         % (frame_size,))
    return _check_epsilon(epsilon)


def rollout(world, steps, epsilon=0.0, generator=None, frames=None):
    """`steps` frames of the expert from the world's current state, as generate_trajectory records them: frame t is
    rendered before action t is applied; the last action is recorded and not applied.  frames: None, or a uint8
    [steps,n,S,S,3] device tensor to draw into.  Returns (states [steps,n,25], actions [steps,n,4]) on the device."""
    n, dev = world.n, world.device
    states = torch.empty(steps, n, OBS_DIM, dtype=torch.float32, device=dev)
    actions = torch.empty(steps, n, 4, dtype=torch.float32, device=dev)
    if frames is not None:
        world.render(out=frames[0])
    for t in range(steps):
        uniform = None
        if epsilon > 0.0:
            uniform = torch.rand(n, 5, generator=generator).to(dev, non_blocking=True)
        act = expert_actions(world.state, uniform=uniform, epsilon=epsilon)
        states[t] = world.observation()
        actions[t] = act
        if t + 1 < steps:
            world.step(act, out=None if frames is None else frames[t + 1], render=frames is not None)
    return states, actions


def generate(n, out_dir, steps=15, seed=0, epsilon=0.2, start="simplified", batch=256, per_file=1000, device=None,
             frame_size=128):
    """n expert trajectories (epsilon-randomised) of `steps` frames as trajectory_bundle_{:05d}.ndpt files of `per_file`
    trajectories in out_dir: `batch` environments at a time run on the device, their [steps,batch,128,128,3] frames go
    through JpegEncoder, the bundles through bundle.write_bundle.  Trajectory i starts at start i of (start, seed).
    Returns the paths written."""
    epsilon = _check_generate(n, steps, epsilon, start, batch, per_file, frame_size)
    n, steps, batch, per_file = int(n), int(steps), int(batch), int(per_file)
    from . import bundle
    from .jpeg import JpegEncoder
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    encoder = JpegEncoder(dev)
    os.makedirs(out_dir, exist_ok=True)
    written, pending, number = [], [], 0

    def flush(count):
        nonlocal number
        number += 1
        path = os.path.join(out_dir, "trajectory_bundle_{:05d}{}".format(number, bundle.SUFFIX))
        bundle.write_bundle(path, pending[:count])
        del pending[:count]
        written.append(path)

    for lo in range(0, n, batch):
        m = min(batch, n - lo)
        world = PushWorld(m, dev, frame_size=frame_size, seed=seed, start=start)
        world.reset(index=lo, render=False)
        goal = world.goal3().cpu().numpy()
        frames = torch.empty(steps, m, frame_size, frame_size, 3, dtype=torch.uint8, device=dev)
        gen = torch.Generator().manual_seed(int(seed) * 1000003 + lo)
        states, actions = rollout(world, steps, epsilon, gen, frames)
        buffer, offsets = encoder.encode(frames)                                   # streams in [t][i] order
        blob, off = buffer.cpu().numpy(), offsets.cpu().numpy()
        states, actions = states.cpu().numpy(), actions.cpu().numpy()
        for i in range(m):
            streams = [blob[off[t * m + i]:off[t * m + i + 1]] for t in range(steps)]
            pending.append((streams, states[:, i], actions[:, i], goal[i]))
        while len(pending) >= per_file:
            flush(per_file)
    if pending:
        flush(len(pending))
    return written


# ---------------------------------------------------------------------------------------------------- closed-loop MPC
def closed_loop_mpc(models, world, goal_frames, steps, rollouts, horizon, cem=None, seed=0, threshold=SUCCESS_THRESHOLD,
                    grad=None):
    """MPC on the world's n live environments from its current state: MpcController.reset(goal_frames), then per step
    ctrl.act(world.render()) -> world.step(actions).  goal_frames: uint8 [n,S,S,3].  Returns {"distance" [n],
    "success" [n] bool, "actions" [steps,n,4]} on the host.  cem, grad: the controller's CemSettings / GradSettings."""
    from .evaluation import MpcController
    ctrl = MpcController(models, rollouts, horizon, frame_shape=(world.size, world.size), seed=seed, cem=cem, grad=grad)
    goal = torch.as_tensor(goal_frames)
    if goal.dtype != torch.uint8 or tuple(goal.shape) != (world.n, world.size, world.size, 3):
        raise ValueError("goal_frames must be uint8 %s, got %s %s"
                         % ((world.n, world.size, world.size, 3), goal.dtype, tuple(goal.shape)))
    if world.size != 128:
        goal = ctrl.resizer(goal, floats=False)[0]
    ctrl.reset(goal)
    taken = torch.empty(int(steps), world.n, 4, dtype=torch.float32)
    frames = world.render()
    for t in range(int(steps)):
        actions, _ = ctrl.act(frames)
        taken[t] = actions
        frames = world.step(actions, out=frames)
    return {"distance": world.goal_distance().cpu(), "success": world.success(threshold).cpu(), "actions": taken}


def evaluate_mpc(models, n, steps, rollouts, horizon, cem=None, seed=0, start="simplified", frame_size=128,
                 threshold=SUCCESS_THRESHOLD, grad=None):
    """Three policies from the same n seeded starts: the expert (the ceiling), uniform random actions (the floor) and
    MPC towards the expert's last frame -- what frame T-1 of a generated dataset is, and what the reference uses as the
    goal image.  Returns {policy: {"distance": mean final block-goal distance, "success": rate}} and "mpc_actions"."""
    world = PushWorld(n, models.device, frame_size=frame_size, seed=seed, start=start)
    steps = int(steps)

    def report():
        return {"distance": float(world.goal_distance().mean()), "success": float(world.success(threshold).float().mean())}

    for _ in range(steps):
        world.step(expert_actions(world.state), render=False)
    goal_frames = world.render()
    result = {"expert": report()}
    world.reset(render=False)
    gen = torch.Generator().manual_seed(int(seed))
    for _ in range(steps):
        world.step(torch.rand(world.n, 4, generator=gen) * 2.0 - 1.0, render=False)
    result["random"] = report()
    world.reset(render=False)
    run = closed_loop_mpc(models, world, goal_frames, steps, rollouts, horizon, cem=cem, seed=seed, threshold=threshold,
                          grad=grad)
    result["mpc"] = report()
    result["mpc_actions"] = run["actions"]
    return result


# -------------------------------------------------------------------------------------------------------- command line
def _mpc_main(argv):
    """`mpc`: the model paths and the mpc.* / mpc.cem / mpc.grad keys of the configuration, as mpc_eval reads them."""
    from argparse import ArgumentParser

    from . import evaluation as E
    from ._eval_io import config_cli, load_eval_models
    from .utils.cli_arguments.common_arguments import add_common_arguments
    parser = add_common_arguments(ArgumentParser(description="closed-loop MPC in the push world"))
    parser.add_argument("--envs", type=int, default=16)
    parser.add_argument("--steps", type=int, default=14)
    parser.add_argument("--start", default="simplified")
    parser.add_argument("--fm-precision", choices=E.FM_PRECISIONS, default=None,
                        help="operand precision of the forward model's passes (default: evaluation.fm_precision, else fp32)")
    parser.add_argument("--enc-precision", choices=E.ENC_PRECISIONS, default=None,
                        help="precision of the image encoder's passes (default: evaluation.enc_precision, else fp32)")

    def check(ns):
        _check_n(ns.envs)
        _check_start(ns.start)

    namespace, config, _ = config_cli(parser, argv, "the push world", prepare=check)
    image_encoder, generator, fwd_model_autoencoder, gpu_id = load_eval_models(config)
    for module in (image_encoder, generator, fwd_model_autoencoder):
        module.eval()
    models = E.EvalModels(image_encoder, fwd_model_autoencoder, generator, gpu_id, fm_precision=E.fm_precision_of(config),
                          enc_precision=E.enc_precision_of(config))
    r, th = int(config.mpc.rollouts), int(config.mpc.time_horizon)
    result = evaluate_mpc(models, namespace.envs, namespace.steps, r, th, cem=E.cem_from_config(config, r, th),
                          seed=int(config.random_seed), start=namespace.start,
                          threshold=float(config.evaluation.threshold), grad=E.grad_from_config(config, r, th))
    for policy in ("expert", "random", "mpc"):
        print("%-6s mean goal distance %.4f  success rate %.3f" % (policy, result[policy]["distance"],
                                                                   result[policy]["success"]))
    return result


def main(argv=None):
    from argparse import ArgumentParser
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "mpc":
        return _mpc_main(argv[1:])
    parser = ArgumentParser(prog="python -m ndivplanning_amd.push_world", description=__doc__.split("\n\n")[0])
    sub = parser.add_subparsers(dest="command", required=True)
    gen = sub.add_parser("generate", help="write N expert trajectories as .ndpt bundles into DIR")
    gen.add_argument("n", type=int)
    gen.add_argument("out_dir")
    gen.add_argument("--steps", type=int, default=15)
    gen.add_argument("--seed", type=int, default=0)
    gen.add_argument("--epsilon", type=float, default=0.2)
    gen.add_argument("--start", default="simplified")
    gen.add_argument("--batch", type=int, default=256)
    gen.add_argument("--per-file", type=int, default=1000)
    sub.add_parser("mpc", help="expert, random and MPC goal distances (--config-file, --envs, --steps, --start)")
    args = parser.parse_args(argv)
    written = generate(args.n, args.out_dir, steps=args.steps, seed=args.seed, epsilon=args.epsilon, start=args.start,
                       batch=args.batch, per_file=args.per_file)
    for path in written:
        print(path)
    return written


if __name__ == "__main__":
    main()
