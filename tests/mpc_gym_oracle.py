"""The recipe of tests/golden/mpc_gym_case.npz and a plain fp32 / fp64 restatement of MPC_gym_eval.py's loop on the oracle
package, with the reference's call pattern (the reset and the goal distance are the package's own helpers,
ndivplanning_amd.mpc_gym_eval.controlled_reset / goal_distance: one statement of the environment protocol) (the goal encoded at every horizon step, R copies of the state), its inline CPU
noise draws and PIL's resize of the environment's frames.  tests/golden/make_golden_mpc_gym.py ran the reference's own
script on the same data; the tests compare."""
import numpy as np
import torch

import eval_oracle as EV
from ndivplanning_amd.mpc_gym_eval import controlled_reset, goal_distance, success_rate

# trajectories, T, rollouts, horizon, seed of the run
N_TRAJ, SEQ, ROLLOUTS, HORIZON, RUN_SEED = 2, 3, 2, 2, 17
THRESHOLD = 0.05
MIN_ERROR = 10000000000


class GymTrajectories(torch.utils.data.Dataset):
    """(images, states, actions, goal) as PushDataset yields them: seeded frames (tests/eval_oracle.case_frames), an
    object position in states[:, 3:5] and a goal position, both within the fake environment's table."""

    def __init__(self, data_seed, n=N_TRAJ, seq_length=SEQ):
        self.frames, self.seq_length = EV.case_frames(n, seq_length, seed=data_seed), seq_length
        g = torch.Generator().manual_seed(data_seed * 77 + 5)
        self.states = torch.zeros(n, seq_length, 25)
        self.states[:, :, 3] = 1.30 + 0.08 * torch.rand(n, 1, generator=g)
        self.states[:, :, 4] = 0.71 + 0.08 * torch.rand(n, 1, generator=g)
        self.goals = torch.stack([1.2 + 0.3 * torch.rand(n, generator=g), 0.6 + 0.3 * torch.rand(n, generator=g),
                                  torch.full((n,), 0.42)], dim=1)

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i][1], self.states[i], self.frames[i][2], self.goals[i]


def pil_state(frame, dtype=torch.float32):
    """MPC_gym_eval.get_state on one rendered frame: (resized bytes [128,128,3], norm'ed [1,3,128,128])."""
    from PIL import Image
    u8 = np.array(Image.fromarray(frame).resize((128, 128), Image.LANCZOS))
    t = torch.from_numpy(u8)[None].permute(0, 3, 1, 2)
    return u8, ((t / 255.0 - 0.5) * 2.0).to(dtype)


def run(encode, generate, forward, dataset, env, seed=RUN_SEED, rollouts=ROLLOUTS, horizon=HORIZON, noise_dim=EV.NOISE_DIM,
        dtype=torch.float32, choices=None):
    """Returns ((avg_action_error, avg_image_loss, avg_goal_error, success_rate), record)."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    loader = torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False)
    t1 = dataset.seq_length - 1
    rec = {"pieces": [], "gen_out": [], "fm_out_sums": [], "rollout_errors": [], "choices": [], "margins": [], "image_errors": [], "actions": [],
           "states_u8": [], "goal_errors": []}
    action_error_sum = 0
    image_error_sum = 0
    step = 0
    for images, states, actions, goal in loader:
        images, actions = images.to(dtype), actions.to(dtype)[:, :t1]
        env = controlled_reset(env, states, goal)
        target = images[:, t1]
        image_error_sum = 0
        state_mpc = images[:, 0]
        chosen = []
        for i in range(t1):
            fut = images[:, i + 1]
            state_fwd = state_mpc.repeat(rollouts, 1, 1, 1)
            for ts in range(horizon):                        # the full horizon at every step
                codes = torch.cat([encode(state_fwd), encode(target.repeat(rollouts, 1, 1, 1))], dim=1)
                piece = torch.FloatTensor(rollouts, 1, noise_dim).uniform_()
                rec["pieces"].append(piece.clone())
                z = torch.cat([codes[:, None, :], piece.to(dtype)], 2)
                act = generate(z.reshape(-1, 256 + noise_dim)).view(rollouts, -1, 4)
                rec["gen_out"].append(act.detach().double().reshape(rollouts, 4))
                if ts == 0:
                    taken = act
                state_fwd = forward(state_fwd, act.squeeze(1))
                rec["fm_out_sums"].append([float(state_fwd.double().sum()), float(state_fwd.double().abs().sum())])
            errs = [float(((state_fwd[ro] - target[0]) ** 2).mean()) for ro in range(rollouts)]
            best, min_error = 0, MIN_ERROR
            for ro, e in enumerate(errs):
                if e < min_error:
                    min_error, best = e, ro
            rest = sorted(e for ro, e in enumerate(errs) if ro != best)
            rec["rollout_errors"].append(errs)
            rec["margins"].append(rest[0] - errs[best])
            if choices is not None:
                best = int(choices[step])
            rec["choices"].append(best)
            step += 1
            chosen.append(taken[best])
            env.step(taken[best].detach().to(torch.float32).numpy().ravel())
            u8, state_mpc = pil_state(env.render(mode="rgb_array"), dtype)
            rec["states_u8"].append(u8)
            err = ((state_mpc - fut) ** 2).mean()
            rec["image_errors"].append(float(err))
            image_error_sum = image_error_sum + err
        rec["goal_errors"].append(goal_distance(env))
        action_hat = torch.cat(chosen, dim=0)
        rec["actions"].append(action_hat.detach().double().reshape(-1))
        action_error_sum = action_error_sum + ((actions - action_hat) ** 2).mean()
    n = t1 * len(loader)
    ge = rec["goal_errors"]
    return (float(action_error_sum / n), float(image_error_sum / n), float(np.mean(ge)), success_rate(ge, THRESHOLD)), rec
