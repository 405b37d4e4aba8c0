#!/usr/bin/env python3
"""Golden vector for the generate_trajectories drop-in, from the REFERENCE's own generate_trajectories.py: its
`generate_trajectory` runs on the CPU, unedited (PIL resize with LANCZOS, PIL save at quality 95), on the stand-ins of
tests/test_gpu_generate_trajectories.py (PushEnv25, the seeded two-layer actor, the normaliser, set as the script's module
globals as its __main__ does).  Runs only where the reference checkout is (its path is the first argument); the .npz
travels.  gym, h5py, dotmap, matplotlib and hindsight_experience_replay are stubbed: the script imports them, and
generate_trajectory uses none of them.

Stored (tests/golden/generate_case.npz), per case `plain`, `simplified`, `simplified_inline`:
  <case>.streams uint8, <case>.offsets int64 [T+1]   the T JPEG streams the reference returned
  <case>.states [T,25], <case>.actions [T,4] float64, <case>.goal [3]
  <case>.rendered_digest [16] uint8                   blake2b of the T frames the environment rendered

Usage: python tests/golden/make_golden_generate.py REFERENCE_CHECKOUT
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_generate_trajectories as S  # noqa: E402
from make_golden_eval import _stub  # noqa: E402


def main(ref):
    _stub("gym")
    _stub("h5py")
    _stub("dotmap", DotMap=dict)
    mpl = _stub("matplotlib")
    mpl.pyplot = _stub("matplotlib.pyplot")
    her = _stub("hindsight_experience_replay")
    her.rl_modules = _stub("hindsight_experience_replay.rl_modules")
    her.rl_modules.models = _stub("hindsight_experience_replay.rl_modules.models", actor=object)
    mine = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "utils" or k.startswith("utils.")}
    sys.path.insert(0, ref)
    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_generate_trajectories", os.path.join(ref, "generate_trajectories.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    sys.path.remove(ref)
    sys.modules.update(mine)
    script.o_mean, script.o_std, script.g_mean, script.g_std = S.normalizer()
    rec = {}
    for name, simplify, inline in S.CASES:
        env, frames, states, actions, goal = S.run(script.generate_trajectory, simplify, inline)
        assert len(frames) == S.T and states.shape == (S.T, 25) and actions.shape == (S.T, 4)
        assert np.abs(actions).max() > 0 and len({a.tobytes() for a in actions}) == S.T, actions
        assert np.array_equal(states * 64, np.round(states * 64)), "states are not on the 1/64 grid"
        rec[name + ".streams"] = np.frombuffer(b"".join(frames), np.uint8)
        rec[name + ".offsets"] = np.concatenate([[0], np.cumsum([len(b) for b in frames])]).astype(np.int64)
        rec[name + ".states"], rec[name + ".actions"] = states, actions
        rec[name + ".goal"] = np.asarray(goal, np.float64)
        rec[name + ".rendered_digest"] = S.digest(np.stack(env.rendered))
        print(name, [len(b) for b in frames], "goal", goal, "actions", actions.tolist())
    assert not np.array_equal(rec["plain.goal"], rec["simplified.goal"])
    path = os.path.join(HERE, "generate_case.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "../reference")
