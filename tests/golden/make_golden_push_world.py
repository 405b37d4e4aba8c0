"""Writes tests/golden/push_world_case.npz: a dozen states of the push world, the actions taken in them, their successor
states, the frames of both at S = 32 and one frame at S = 128, all produced by the numpy restatement of include/ndp.h's
definition (tests/world_common.py).  The file pins the definition against a silent change of either side: the
restatement must reproduce it (tests/test_push_world.py), and the kernels must match the restatement.  Run from the
repository root:
    python tests/golden/make_golden_push_world.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import world_common as W  # noqa: E402

NAMES = ("r2 == 0", "at Z_CONTACT, the fp32 below it", "a NaN action component", "actions beyond +-1",
         "the block into the wall", "the block into the corner", "gripper in corner 00", "gripper in corner 11",
         "raised over the block", "descending onto the block", "three sixteenths, pushing", "a state from outside the window")


def build():
    by_name = {name: (state, action) for name, state, action in W.cases()}
    states = np.stack([by_name[n][0] for n in NAMES])
    actions = np.stack([by_name[n][1] for n in NAMES])
    after = W.step(states, actions)
    return {"names": np.array(NAMES), "states": states, "actions": actions, "successors": after,
            "frames32": W.render(states, 32), "successor_frames32": W.render(after, 32),
            "frame128": W.render(after[10:11], 128)[0]}


def main():
    out = build()
    path = os.path.join(HERE, "push_world_case.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
