"""The push world's kernels (k_world_step_render, k_world_render, csrc/ndp_world.inc) on the CPU, under AddressSanitizer
and UndefinedBehaviorSanitizer.  tests/host_drivers/world.inc follows the library's source in main.hip and replays both
kernels' schedules thread by thread with the library's own __host__ __device__ functions (namespace ndp::world), the LDS
hand-over included, every buffer in an allocation of exactly its size.  The program is host_driver's, built once per
process, and runs as an ordinary child process: nothing is preloaded and nothing of it is loaded into Python.  The
expected values are the numpy restatement of include/ndp.h's definition (tests/world_common.py): every state and every
frame bit for bit.  No GPU involved (the same cases on the GPU: tests/test_gpu_push_world.py)."""
import numpy as np
import pytest

import host_driver
import world_common as W


@pytest.fixture(scope="module")
def driver():
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    return host_driver.build()


@pytest.fixture(scope="module")
def report(driver, tmp_path_factory):
    runs = W.host_runs()
    raw = host_driver.run("world", W.pack(runs), tmp_path_factory.mktemp("world_cases"), exe=driver)
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


def test_the_driver_refuses_a_bad_header(driver, tmp_path):
    states, actions = W.case_arrays(1)
    for size, n_flag in ((34, 1), (28, 1), (32, 2)):                  # not a multiple of 4, too small, with_frames = 2
        host_driver.run("world", W.pack([(size, n_flag, states, actions)]), tmp_path, timeout=300, exe=driver, expect=2)
