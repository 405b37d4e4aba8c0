#!/usr/bin/env python3
"""Golden vectors for the live-environment MPC evaluation, from the REFERENCE's own MPC_gym_eval.py: its
`fetch_push_control_evaluation` runs on CPU, unedited, with the reference's Encoder, ForwardAutoencoder and gan.Decoder
loaded with the seeded states of tests/eval_oracle.py, a small in-memory dataset (tests/mpc_gym_oracle.GymTrajectories)
and the deterministic environment of tests/fake_push_env.py.  Runs only where the reference checkout is (its path is the
first argument); the .npz travels.  gym, matplotlib, dotmap, torchvision, h5py and vis_tools are stubbed (the script imports
them; on CPU it uses matplotlib's imsave only, which writes nothing here).

Recorded, without editing the script: every noise piece (the last noise_dim columns of every generator input), every
generator output and every forward-model output (as its sum and absolute sum: the maps themselves are 3 MB), every
rollout's error as MPC_gym_eval.py:221 computes it, the choice (the row of the
ts = 0 generator output the environment was stepped with), the actions taken, the rendered frames, the resized states
(get_state's result, wrapped), the per-step image errors and the returned 4-tuple; beside them the fp64 restatement
(tests/mpc_gym_oracle.run) teacher-forced to the recorded choices.  Weights are not stored: seeds and checksums are.

The data seed is searched until, at every planning step, the best and the second-best rollout error differ by at least
100 x the distance between the fp32 reference's errors and the fp64 ones: the choice does not ride on rounding.

Usage: python tests/golden/make_golden_mpc_gym.py REFERENCE_CHECKOUT
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import eval_oracle as EV  # noqa: E402
import mpc_gym_oracle as MG  # noqa: E402
from fake_push_env import FakePushEnv  # noqa: E402
from make_golden_eval import Recorder, _stub, _stubs, reference_modules  # noqa: E402


def config():
    ns = types.SimpleNamespace
    return ns(random_seed=MG.RUN_SEED, gpu_id=0, log_port=8081,
              evaluation=ns(num_sample=1, noise_dim=EV.NOISE_DIM, batch_size=1, threshold=MG.THRESHOLD),
              mpc=ns(rollouts=MG.ROLLOUTS, time_horizon=MG.HORIZON))


def one_case(ref, script, data_seed):
    enc, fm, g, states = reference_modules(ref)
    log, resized = [], []
    dataset = MG.GymTrajectories(data_seed)
    env = FakePushEnv()
    inner = script.get_state

    def get_state(e, a):
        out = inner(e, a)
        resized.append(out.detach().clone())
        return out
    script.get_state = get_state
    try:
        with torch.no_grad():
            four = script.fetch_push_control_evaluation(types.SimpleNamespace(image_shape=(128, 128)), Recorder(enc, log, "enc"),
                                                        Recorder(fm, log, "fm"), Recorder(g, log, "gen"), dataset, config(),
                                                        env)
    finally:
        script.get_state = inner
    gens = [e for e in log if e[0] == "gen"]
    fms = [e for e in log if e[0] == "fm"]
    mse = torch.nn.MSELoss()
    r, th, t1 = MG.ROLLOUTS, MG.HORIZON, MG.SEQ - 1
    assert len(gens) == len(fms) == MG.N_TRAJ * t1 * th and len(env.rendered) == len(resized) == MG.N_TRAJ * t1
    errs, choices, margins, image_errors, actions = [], [], [], [], []
    for traj in range(MG.N_TRAJ):
        imgs = dataset.frames[traj][1]
        for i in range(t1):
            k = traj * t1 + i
            g0 = gens[k * th][2].view(r, 4)
            preds = fms[k * th + th - 1][2]
            e = [float(mse(preds[ro], imgs[t1])) for ro in range(r)]
            taken = torch.from_numpy(env.actions[k]).float()
            hit = [ro for ro in range(r) if torch.equal(g0[ro], taken)]
            c = hit[0]
            rest = sorted(v for ro, v in enumerate(e) if ro != c)
            errs.append(e)
            choices.append(c)
            margins.append(rest[0] - e[c])
            image_errors.append(float(mse(resized[k], imgs[i + 1:i + 2])))
            actions.append(taken.double().numpy())
    u8 = np.stack([MG.pil_state(f)[0] for f in env.rendered])
    for k in range(len(resized)):                                 # get_state's floats are norm() of PIL's bytes
        assert torch.equal(resized[k], MG.pil_state(env.rendered[k])[1])
    rec = {"four": np.array(four, dtype=np.float64),
           "noise": torch.cat([e[1][0][:, 256:].reshape(-1) for e in gens]).numpy(),
           "gen_out": torch.stack([e[2].view(r, 4) for e in gens]).numpy(),
           "fm_out_sums": np.array([[float(e[2].double().sum()), float(e[2].double().abs().sum())] for e in fms]),
           "meta": np.array([MG.N_TRAJ, MG.SEQ, r, th, MG.RUN_SEED, EV.NOISE_DIM, data_seed]),
           "state_checksums": np.stack([EV.checksum(s) for s in states]),
           "frames": np.stack(env.rendered), "states_u8": u8,
           "rollout_errors": np.array(errs), "choices": np.array(choices), "margins": np.array(margins),
           "image_errors": np.array(image_errors), "actions": np.concatenate(actions)}
    # the fp64 restatement on the recorded frames, teacher-forced to the reference's choices
    four64, r64 = MG.run(*EV.oracle_callables(*EV.case_states(), torch.float64), dataset, FakePushEnv(replay=rec["frames"]),
                         dtype=torch.float64, choices=rec["choices"])
    assert np.array_equal(torch.cat([p.reshape(-1) for p in r64["pieces"]]).numpy(), rec["noise"])
    rec["four_fp64"] = np.array(four64)
    rec["image_errors_fp64"] = np.array(r64["image_errors"])
    rec["actions_fp64"] = torch.cat(r64["actions"]).numpy()
    rec["rollout_errors_fp64"] = np.array(r64["rollout_errors"])
    rec["goal_errors"] = np.array(r64["goal_errors"])
    rec["gen_out_fp64"] = torch.stack(r64["gen_out"]).numpy()
    rec["fm_out_sums_fp64"] = np.array(r64["fm_out_sums"])
    return rec


def decisive(rec):
    bound = np.abs(rec["rollout_errors"] - rec["rollout_errors_fp64"]).max(axis=1)
    return bool((rec["margins"] >= 100 * bound).all() and (rec["margins"] > 0).all())


def main(ref):
    import logging
    logging.raiseExceptions = False          # MPC_gym_eval.py:246-253 pass a value without a format field
    _stubs()
    _stub("gym")
    sys.modules["matplotlib.pyplot"].imsave = lambda *a, **k: None
    sys.path.insert(0, ref)
    import MPC_gym_eval
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for data_seed in range(41, 61):
        rec = one_case(ref, MPC_gym_eval, data_seed)
        print("data seed", data_seed, "choices", rec["choices"], "margins", rec["margins"], "four", rec["four"], rec["four_fp64"])
        if decisive(rec):
            break
    else:
        raise SystemExit("no data seed gave decisive margins")
    assert decisive(rec)
    path = os.path.join(HERE, "mpc_gym_case.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "../reference")
