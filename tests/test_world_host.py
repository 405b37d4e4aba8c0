"""The push world's kernels (k_world_step_render, k_world_render, csrc/ndp_world.inc) on the CPU, under AddressSanitizer
and UndefinedBehaviorSanitizer.  tests/host_drivers/world_main.hip is a stand-alone program beside main.hip: it includes
the library's source and replays both kernels' schedules thread by thread with the library's own __host__ __device__
functions (namespace ndp::world), the LDS hand-over included, every buffer in an allocation of exactly its size.  It is
compiled with host_driver's command line, once per session, and runs as an ordinary child process: nothing is preloaded
and nothing of it is loaded into Python.  The expected values are the numpy restatement of include/ndp.h's definition
(tests/world_common.py): every state and every frame bit for bit.  No GPU involved (the same cases on the GPU:
tests/test_gpu_push_world.py)."""
import os
import subprocess

import numpy as np
import pytest

import host_driver
import world_common as W

SOURCE = os.path.join(host_driver.HERE, "host_drivers", "world_main.hip")


@pytest.fixture(scope="session")
def world_driver(tmp_path_factory):
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    exe = str(tmp_path_factory.mktemp("world_driver") / "world")
    cmd = [host_driver._hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17"] + host_driver.SANITIZE
    cmd += ["-Wno-unused-value", "-Wno-pass-failed", "-Wno-invalid-offsetof", "-Wno-dangling-else", SOURCE, "-o", exe]
    print("world driver:", " ".join(cmd), flush=True)
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "hipcc failed:\n" + res.stdout[-4000:]
    with open(exe, "rb") as f:
        assert b"__asan_init" in f.read(), "the program was linked without AddressSanitizer's runtime"
    return exe


@pytest.fixture(scope="module")
def report(world_driver, tmp_path_factory):
    runs = W.host_runs()
    raw = host_driver.run("world", W.pack(runs), tmp_path_factory.mktemp("world_cases"), exe=world_driver)
    return runs, W.unpack(runs, raw)


def test_the_runs_cover_the_shapes_and_every_case():
    runs = W.host_runs()
    assert {(size, len(states)) for size, _, states, _ in runs} >= {(s, n) for s in (32, 36, 128) for n in (1, 3)}
    assert (36 * 36 // 4) % 256 != 0                                  # S = 36: the second workgroup is partial
    every = {st.tobytes() + ac.tobytes() for _, st, ac in W.cases()}
    for size in W.HOST_SIZES:
        seen = {s.tobytes() + a.tobytes() for sz, _, states, actions in runs if sz == size for s, a in zip(states, actions)}
        assert every <= seen, size
    assert any(not with_frames for _, with_frames, _, _ in runs)


def test_states_are_bit_equal_to_the_restatement(report):
    runs, results = report
    for (size, _, states, actions), got in zip(runs, results):
        assert W.bits_equal(got["state_out"], W.step(states, actions)), (size, len(states))


def test_frames_are_bit_equal_to_the_restatement(report):
    runs, results = report
    for (size, with_frames, states, actions), got in zip(runs, results):
        want = W.render(states, size)
        assert W.bits_equal(got["render_frames"], want), (size, np.argwhere(got["render_frames"] != want)[:4])
        if with_frames:
            want = W.render(W.step(states, actions), size)
            assert W.bits_equal(got["step_frames"], want), (size, np.argwhere(got["step_frames"] != want)[:4])
        else:
            assert got["step_frames"] is None


def test_the_driver_refuses_a_bad_header(world_driver, tmp_path):
    states, actions = W.case_arrays(1)
    for size, n_flag in ((34, 1), (28, 1), (32, 2)):                  # not a multiple of 4, too small, with_frames = 2
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(W.pack([(size, n_flag, states, actions)]))
        p = subprocess.run([world_driver, "world", src, dst], env=dict(os.environ), capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 2, (size, n_flag, p.returncode, p.stderr[-2000:])
