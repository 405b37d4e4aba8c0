"""Build and run tests/jpeg_enc_host_driver.hip, the JPEG encoder's core on the CPU, and rebuild the encoder corpus of
tests/golden/jpeg_encode_case.npz (used by tests/test_jpeg_encode_core_host.py, tests/test_jpeg_encode_golden.py,
tests/test_gpu_jpeg_encode.py and tests/golden/make_golden_jpeg_encode.py).  The driver is an ordinary program: it is
started as a child process, nothing is preloaded and nothing of it is loaded into Python.  The build recipe, the
sanitizer flags and the test for a toolchain without the runtimes are tests/jpeg_core_host.py's."""
import os
import subprocess

import numpy as np

import jpeg_core_host as H

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "jpeg_enc_host_driver.hip")
FIELDS = ("len", "len_serial", "equal", "total_bits", "entropy_bytes", "stuffed", "last_ff", "zrl", "eob_only", "max_dc_cat",
          "max_stream", "reserved")
CENSUS = ("total_bits", "entropy_bytes", "stuffed", "last_ff", "zrl", "eob_only", "max_dc_cat")
HEADER = 623
BLOCKS = 384
STORED, UNIFORM_NOISE, BINARY_NOISE, CORNER_NOISE = 0, 1, 2, 3      # `kind` of a corpus frame
ENV_ACTIONS = ((1.0, 0.5, -0.5, 0.0), (-1.0, -1.0, 1.0, 0.0), (0.3, -0.9, 0.2, 0.0))


def build_driver(out_dir, sanitize=True):
    """jpeg_core_host.build_driver for the encoder's driver."""
    exe = os.path.join(str(out_dir), "jpeg_enc_host_driver")
    cmd = [H._hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17"] + (H.SANITIZE if sanitize else [])
    cmd += ["-Wno-unused-value", "-Wno-pass-failed", "-Wno-invalid-offsetof", "-Wno-dangling-else", SOURCE, "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        if sanitize and H._RUNTIME_MISSING.search(res.stdout):
            raise H.NoSanitizerRuntime(res.stdout[-2000:])
        raise RuntimeError("hipcc failed:\n" + res.stdout[-4000:])
    return exe


def run_driver(exe, frames, coefs, work_dir, timeout=900):
    """Encode `frames` (uint8 [nf,128,128,3]) and then the coefficient sets `coefs` (int16 [nc,384,64]) in a child
    process; asserts that it exits 0 with no sanitizer report.  Returns (records {field: int32 [nf+nc]}, streams: list of
    bytes, the scheduled writer's)."""
    frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, 128, 128, 3)
    coefs = np.ascontiguousarray(coefs, np.int16).reshape(-1, BLOCKS, 64)
    src, dst = os.path.join(str(work_dir), "frames.bin"), os.path.join(str(work_dir), "streams.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(frames)).tobytes())
        f.write(frames.tobytes())
        f.write(np.int32(len(coefs)).tobytes())
        f.write(coefs.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, src, dst], env=env, capture_output=True, text=True, timeout=timeout)
    text = p.stdout + p.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert p.returncode == 0, (p.returncode, text[-2000:])
    raw = open(dst, "rb").read()
    os.remove(src)
    os.remove(dst)
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
