"""Shared by the trajectory-store tests (tests/test_store_gather_host.py, tests/test_gpu_trajectory_store.py): the
random-byte corpora, the gather cases, what a gather must give -- `pack_jpegs` of the selected streams in batch order plus
numpy slices of the tables -- and the run of tests/host_drivers/store_gather.inc through tests/host_driver.py."""
import numpy as np

import host_driver
from ndivplanning_amd.bundle import ACTION_DIM, GOAL_DIM, STATE_DIM

CHUNK_BYTES = 4096                  # one workgroup's chunk (ndp::store::kChunkBytes)
LONG_STREAM = 70001                 # longer than a chunk and than 65,537 bytes: split over 18 workgroups
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 255, 256, 257, 4093, 4099, LONG_STREAM)
CANARY = 0xC5
BAD_INDEX, CAPACITY = 1, 2          # NDP_STORE_* (include/ndp.h)


def make_corpus(n_traj, steps, lengths, seed):
    """A store of n_traj x steps streams of random bytes with the given lengths, and random float tables."""
    rng = np.random.RandomState(seed)
    lengths = np.asarray(lengths, np.int64)
    assert lengths.size == n_traj * steps
    offsets = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=offsets[1:])
    tables = [rng.randn(n_traj, steps, STATE_DIM).astype(np.float32), rng.randn(n_traj, steps, ACTION_DIM).astype(np.float32),
              rng.randn(n_traj, GOAL_DIM).astype(np.float32)]
    tables[0][0, 0, 0] = np.nan                                      # bits, not values, are compared
    tables[1][-1, -1, -1] = -0.0
    return dict(n=n_traj, steps=steps, offsets=offsets, blob=rng.randint(0, 256, int(offsets[-1])).astype(np.uint8),
                states=tables[0], actions=tables[1], goal=tables[2], max_len=int(lengths.max()))


def main_corpus():
    """40 trajectories of 8 streams.  Trajectory 0 starts with a 17-byte stream; the required lengths follow, the long one
    in trajectory 2; the rest are short odd-and-even lengths that walk the source offsets through every residue mod 16;
    the last stream of the last trajectory (4,099 bytes) ends with the blob."""
    rng = np.random.RandomState(11)
    n_traj, steps = 40, 8
    short = [l for l in LENGTHS if l <= 257]
    lengths = [int(rng.choice(short)) if rng.rand() < 0.5 else int(rng.randint(1, 41)) for _ in range(n_traj * steps)]
    lengths[0] = 17
    lengths[1:1 + len(LENGTHS)] = LENGTHS
    lengths[-1] = 4099
    lengths[-2] = 0
    return make_corpus(n_traj, steps, lengths, seed=12)


def single_corpus():
    """3 trajectories of ONE stored stream each (T = 1), 33, 0 and 5 bytes."""
    return make_corpus(3, 1, [33, 0, 5], seed=17)


def single_cases(corpus):
    """(B, T stored, seq_start, T') = (1, 1, 0, 1), and the three of them with the empty one in the middle."""
    return [("1x1 of T=1", np.array([2], np.int64), 0, 1), ("3x1 of T=1", np.array([0, 1, 2], np.int64), 0, 1)]


def tiny_corpus():
    """1,024 trajectories of 20 streams of 1..40 bytes: 20,480 streams, the largest batch the trainers form."""
    rng = np.random.RandomState(13)
    return make_corpus(1024, 20, rng.randint(1, 41, 1024 * 20), seed=14)


def main_cases(corpus):
    """[(name, indices int64 [B], seq_start, seq_length)] on main_corpus()."""
    n = corpus["n"]
    rng = np.random.RandomState(15)
    pick = lambda b: rng.randint(0, n, b).astype(np.int64)            # noqa: E731  (with duplicates)
    return [("one", np.array([5], np.int64), 0, 1),
            ("3x5", np.array([7, 0, 2], np.int64), 2, 5),
            ("first and last", np.array([0, n - 1], np.int64), 0, 8),
            ("long", np.array([2, 1, 2], np.int64), 0, 8),
            ("duplicates", np.array([3, 3, 9, 3, 9], np.int64), 1, 6),
            ("out of range", np.array([4, n, 6, -1, 2 ** 40, 1], np.int64), 3, 4),
            ("residues", pick(150), 0, 8),                            # fills the table of residue pairs (asserted)
            ("63", pick(9), 1, 7), ("64", pick(8), 0, 8), ("65", pick(13), 3, 5),
            ("1023", pick(341), 4, 3), ("1025", pick(205), 2, 5)]


def tiny_cases(corpus):
    return [("20480", np.random.RandomState(16).permutation(corpus["n"]).astype(np.int64), 0, 20)]


def selected(corpus, indices, seq_start, seq_length):
    """[(source offset, length)] of the batch's streams in batch order; an index out of range gives (0, 0) streams."""
    out = []
    for i in indices:
        for t in range(seq_start, seq_start + seq_length):
            if 0 <= i < corpus["n"]:
                f = int(i) * corpus["steps"] + t
                out.append((int(corpus["offsets"][f]), int(corpus["offsets"][f + 1] - corpus["offsets"][f])))
            else:
                out.append((0, 0))
    return out


def expected(corpus, indices, seq_start, seq_length):
    """(buffer uint8, offsets int64 [n+1], states, actions, goal, status): pack_jpegs of the selected streams, slices of
    the tables (zero rows for an index out of range)."""
    from ndivplanning_amd.jpeg import pack_jpegs
    sel = selected(corpus, indices, seq_start, seq_length)
    buffer, offsets = pack_jpegs([corpus["blob"][o:o + l] for o, l in sel], pin=False)
    b = len(indices)
    states = np.zeros((b, seq_length, STATE_DIM), np.float32)
    actions = np.zeros((b, seq_length, ACTION_DIM), np.float32)
    goal = np.zeros((b, GOAL_DIM), np.float32)
    status = 0
    for r, i in enumerate(indices):
        if 0 <= i < corpus["n"]:
            states[r] = corpus["states"][i, seq_start:seq_start + seq_length]
            actions[r] = corpus["actions"][i, seq_start:seq_start + seq_length]
            goal[r] = corpus["goal"][i]
        else:
            status |= BAD_INDEX
    return buffer.numpy(), offsets.numpy(), states, actions, goal, status


def residue_pairs(corpus, case_list):
    """{(source offset mod 16, destination offset mod 16)} over every stream that holds a byte, over all cases."""
    pairs = set()
    for _, indices, seq_start, seq_length in case_list:
        dst = 0
        for o, l in selected(corpus, indices, seq_start, seq_length):
            if l:
                pairs.add((o % 16, dst % 16))
            dst += l
    return pairs


def capacity(corpus, indices, seq_length):
    return len(indices) * seq_length * corpus["max_len"]


def check(name, got, want):
    """got, want: (buffer, offsets, states, actions, goal, status); byte for byte."""
    for what, g, w in zip(("buffer", "offsets", "states", "actions", "goal"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (name, what, np.flatnonzero(g.view(np.uint8).ravel() != w.view(np.uint8).ravel())[:8])
    assert int(got[5]) == int(want[5]), (name, "status", got[5], want[5])


# ------------------------------------------------------------------------------------------ the host driver
def build_driver(out_dir=None, sanitize=True):
    return host_driver.build(sanitize)


def run_driver(exe, corpus, case_list, work_dir, timeout=600):
    """Asserts that the child exits 0 with no sanitizer report.  Returns per case ((buffer, offsets, states, actions,
    goal, status), bytes changed past offsets[-1])."""
    parts = [np.array([corpus["n"], corpus["steps"], corpus["blob"].size], np.int64).tobytes()]
    parts += [np.ascontiguousarray(corpus[k]).tobytes() for k in ("offsets", "states", "actions", "goal", "blob")]
    parts.append(np.int64(len(case_list)).tobytes())
    for _, indices, seq_start, seq_length in case_list:
        parts += [np.array([len(indices), seq_start, seq_length, capacity(corpus, indices, seq_length)], np.int64).tobytes(),
                  np.ascontiguousarray(indices, np.int64).tobytes()]
    raw = np.frombuffer(host_driver.run("store_gather", b"".join(parts), work_dir, timeout=timeout, exe=exe), np.uint8)
    results, pos = [], 0

    def take(count, dtype):
        nonlocal pos
        size = count * np.dtype(dtype).itemsize
        out = raw[pos:pos + size].copy().view(dtype)
        pos += size
        return out

    for _, indices, seq_start, seq_length in case_list:
        b, n = len(indices), len(indices) * seq_length
        status, changed = (int(v) for v in take(2, np.int64))
        offsets = take(n + 1, np.int64)
        states = take(n * STATE_DIM, np.float32).reshape(b, seq_length, STATE_DIM)
        actions = take(n * ACTION_DIM, np.float32).reshape(b, seq_length, ACTION_DIM)
        goal = take(b * GOAL_DIM, np.float32).reshape(b, GOAL_DIM)
        buffer = take(int(offsets[-1]), np.uint8)
        results.append(((buffer, offsets, states, actions, goal, status), changed))
    assert pos == raw.size, (pos, raw.size)
    return results
