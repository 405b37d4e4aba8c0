"""A deterministic stand-in for gym's FetchPush-v1, with exactly the protocol MPC_gym_eval.py uses and nothing more:
reset(); sim.data.get_joint_qpos / env.sim.data.set_joint_qpos("object0:joint"); sim.forward(); env.goal; step(action);
render(mode="rgb_array"); env._get_obs()["desired_goal"].  A helper for the tests and for
tests/golden/make_golden_mpc_gym.py, not a conftest.

The world: a gripper and an object block on a table.  step(action) moves the gripper by 0.05 * clip(action[:3], -1, 1);
a gripper within 0.08 of the object in the table plane carries it along.  render draws a gradient that follows the
gripper's height, a gripper disc and an object block at those positions into a 120-row x 160-column frame: not square, so
that the resize runs both passes.

Replay mode (`replay=frames [N,120,160,3]`): render returns the recorded frames in the order of the calls, whatever the
actions were; the world still moves, so distances to the goal stay defined.  `rendered` holds every frame handed out and
`actions` every action taken."""
import numpy as np

HEIGHT, WIDTH = 120, 160
TABLE = ((0.8, 1.8), (0.3, 1.3))       # x and y range the camera sees


class _Data:
    def __init__(self, world):
        self._w = world

    def get_joint_qpos(self, name):
        assert name == "object0:joint", name
        return self._w.object_qpos.copy()

    def set_joint_qpos(self, name, value):
        assert name == "object0:joint", name
        self._w.object_qpos = np.array(value, dtype=np.float64).reshape(7)


class _Sim:
    def __init__(self, world):
        self.data = _Data(world)
        self.forwards = 0

    def forward(self):
        self.forwards += 1


class FakePushEnv:
    def __init__(self, replay=None):
        self.env = self                 # gym's wrapper and the wrapped environment in one
        self.sim = _Sim(self)
        self.replay = None if replay is None else np.asarray(replay, np.uint8)
        self.rendered, self.actions = [], []
        self.goal = np.zeros(3)
        self.reset()

    def reset(self):
        self.gripper = np.array([1.34, 0.75, 0.53])
        self.object_qpos = np.array([1.25, 0.65, 0.42, 1.0, 0.0, 0.0, 0.0])
        return self._get_obs()

    def _get_obs(self):
        return {"observation": np.concatenate([self.gripper, self.object_qpos[:3]]),
                "achieved_goal": self.object_qpos[:3].copy(), "desired_goal": np.asarray(self.goal, np.float64).copy()}

    def step(self, action):
        action = np.asarray(action, np.float64).reshape(-1)
        assert action.shape == (4,), action.shape
        self.actions.append(action.copy())
        move = 0.05 * np.clip(action[:3], -1.0, 1.0)
        if np.hypot(*(self.gripper[:2] - self.object_qpos[:2])) < 0.08:
            self.object_qpos[:2] += move[:2]
        self.gripper = self.gripper + move
        return self._get_obs(), 0.0, False, {}

    def _pixel(self, pos):
        (x0, x1), (y0, y1) = TABLE
        return (pos[0] - x0) / (x1 - x0) * (WIDTH - 1), (pos[1] - y0) / (y1 - y0) * (HEIGHT - 1)

    def draw(self):
        yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
        lift = int(round(float(self.gripper[2]) * 100.0))
        img = np.stack([(xx * 255) // (WIDTH - 1), (yy * 255) // (HEIGHT - 1), (xx + 2 * yy + lift) % 256], axis=2)
        img = img.astype(np.uint8)
        ox, oy = self._pixel(self.object_qpos)
        block = (np.abs(xx - ox) <= 7) & (np.abs(yy - oy) <= 7)
        img[block] = (20, 20, 235)
        gx, gy = self._pixel(self.gripper)
        disc = (xx - gx) ** 2 + (yy - gy) ** 2 <= 10 ** 2
        img[disc] = (250, 245, 10)
        return img

    def render(self, mode="human"):
        assert mode == "rgb_array", mode
        if self.replay is not None:
            frame = self.replay[len(self.rendered)].copy()
        else:
            frame = self.draw()
        self.rendered.append(frame)
        return frame
