"""Run tests/host_drivers/jpeg_enc.inc, the JPEG encoder's core on the CPU, through tests/host_driver.py, and rebuild the encoder corpus of
tests/golden/jpeg_encode_case.npz (used by tests/test_jpeg_encode_core_host.py, tests/test_jpeg_encode_golden.py,
tests/test_gpu_jpeg_encode.py and tests/golden/make_golden_jpeg_encode.py)."""
import numpy as np

import host_driver

FIELDS = ("len", "len_serial", "equal", "total_bits", "entropy_bytes", "stuffed", "last_ff", "zrl", "eob_only", "max_dc_cat",
          "max_stream", "reserved")
CENSUS = ("total_bits", "entropy_bytes", "stuffed", "last_ff", "zrl", "eob_only", "max_dc_cat")
HEADER = 623
BLOCKS = 384
STORED, UNIFORM_NOISE, BINARY_NOISE, CORNER_NOISE = 0, 1, 2, 3      # `kind` of a corpus frame
ENV_ACTIONS = ((1.0, 0.5, -0.5, 0.0), (-1.0, -1.0, 1.0, 0.0), (0.3, -0.9, 0.2, 0.0))


def build_driver(out_dir=None, sanitize=True):
    return host_driver.build(sanitize)


def run_driver(exe, frames, coefs, work_dir, timeout=900):
    """Encode `frames` (uint8 [nf,128,128,3]) and then the coefficient sets `coefs` (int16 [nc,384,64]) in a child
    process; asserts that it exits 0 with no sanitizer report.  Returns (records {field: int32 [nf+nc]}, streams: list of
    bytes, the scheduled writer's)."""
    frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, 128, 128, 3)
    coefs = np.ascontiguousarray(coefs, np.int16).reshape(-1, BLOCKS, 64)
    payload = np.int32(len(frames)).tobytes() + frames.tobytes() + np.int32(len(coefs)).tobytes() + coefs.tobytes()
    raw = host_driver.run("jpeg_enc", payload, work_dir, timeout=timeout, exe=exe)
    n = len(frames) + len(coefs)
    rec = {k: np.zeros(n, np.int32) for k in FIELDS}
    streams, at = [], 0
    for i in range(n):
        ints = np.frombuffer(raw, np.int32, len(FIELDS), at)
        for j, k in enumerate(FIELDS):
            rec[k][i] = ints[j]
        at += 4 * len(FIELDS)
        streams.append(raw[at:at + int(ints[0])])
        at += int(ints[0])
    assert at == len(raw), (at, len(raw))
    return rec, streams


def pil_encode(frame):
    """The reference writer (generate_trajectories.py:113-122)."""
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame, np.uint8)).save(buf, format="jpeg", quality=95)
    return buf.getvalue()


def seeded_frame(kind, seed):
    rng = np.random.RandomState(int(seed))
    if kind == UNIFORM_NOISE:
        return rng.randint(0, 256, (128, 128, 3)).astype(np.uint8)
    if kind == BINARY_NOISE:
        return (rng.randint(0, 2, (128, 128, 3)) * 255).astype(np.uint8)
    if kind == CORNER_NOISE:                                  # flat, the last MCU of 0 / 255 noise: a short stream whose
        frame = np.full((128, 128, 3), 128, np.uint8)         # last bits vary with the seed
        frame[112:, 112:] = (rng.randint(0, 2, (16, 16, 3)) * 255).astype(np.uint8)
        return frame
    raise ValueError(kind)


def corpus_frames(g):
    """The frames uint8 [n,128,128,3] of a loaded jpeg_encode_case.npz: stored ones, and seeded noise made again."""
    out = np.zeros((len(g["kind"]), 128, 128, 3), np.uint8)
    for i, (kind, ref) in enumerate(zip(g["kind"], g["ref"])):
        out[i] = g["frames"][ref] if kind == STORED else seeded_frame(kind, ref)
    return out


def corpus_streams(g):
    o = g["offsets"]
    return [g["streams"][o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]


def env_frames():
    """The 120x160 frames of tests/fake_push_env.py the corpus holds (resized by PIL): the start and three steps."""
    from fake_push_env import FakePushEnv
    env = FakePushEnv()
    frames = [env.draw()]
    for a in ENV_ACTIONS:
        env.step(np.array(a))
        frames.append(env.draw())
    return np.stack(frames)


def check_classes(g):
    """The class conditions of the encoder corpus, on the arrays of a loaded (or about to be written)
    jpeg_encode_case.npz: each must be met by at least one frame."""
    names = [str(n) for n in g["names"]]
    assert len(set(names)) == len(names) >= 36
    n = len(names)
    lens = np.diff(g["offsets"])
    assert g["streams"].size == g["offsets"][-1] and len(lens) == n
    for k in CENSUS:
        assert g[k].shape == (n,), k
    assert (g["entropy_bytes"] == lens - HEADER - 2).all()
    assert (g["zrl"] > 0).any(), "no ZRL symbol"
    assert (g["stuffed"] > 0).any(), "no stuffed 0xFF"
    assert (g["last_ff"] == 1).any(), "no final padded byte of 0xFF"
    assert ((g["total_bits"] % 8 == 0) & (g["total_bits"] > 0)).any(), "no stream without padding"
    assert (g["eob_only"] == BLOCKS).any(), "no all-EOB frame"
    assert (g["max_dc_cat"] >= 10).any(), "no DC category of 10"
    assert (g["entropy_bytes"] > 20000).any(), "no entropy segment above 20,000 bytes"
    s = g["streams"]
    for i in range(n):
        a, b = int(g["offsets"][i]), int(g["offsets"][i + 1])
        assert np.array_equal(s[a:a + HEADER], g["header"]), names[i]
        assert s[b - 2] == 0xFF and s[b - 1] == 0xD9, names[i]
        if g["last_ff"][i]:
            assert s[b - 4] == 0xFF and s[b - 3] == 0x00, names[i]
    assert g["header"].shape == (HEADER,) and g["env_index"].shape == (1 + len(ENV_ACTIONS),)
