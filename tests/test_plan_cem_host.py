"""The planner's cross-entropy update (k_plan_cem_update, csrc/ndp_plan.inc) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer.  tests/host_drivers/plan_cem_main.hip is a stand-alone program beside main.hip: it includes
the library's source and replays the workgroup's schedule thread by thread with the library's own __host__ __device__
functions (namespace ndp::plan), every buffer (inputs, outputs, each LDS array) in an allocation of exactly its size.
It is compiled with host_driver's command line, once per session, and runs as an ordinary child process.  The expected
values are the plain numpy restatement of include/ndp.h's definition (tests/plan_common.py): every output bit for bit.
No GPU involved (the same cases on the GPU: tests/test_gpu_plan_cem.py)."""
import os
import subprocess

import numpy as np
import pytest

import host_driver
import plan_common as C

SOURCE = os.path.join(host_driver.HERE, "host_drivers", "plan_cem_main.hip")


@pytest.fixture(scope="session")
def plan_cem_driver(tmp_path_factory):
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    exe = str(tmp_path_factory.mktemp("plan_cem_driver") / "plan_cem")
    cmd = [host_driver._hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17"] + host_driver.SANITIZE
    cmd += ["-Wno-unused-value", "-Wno-pass-failed", "-Wno-invalid-offsetof", "-Wno-dangling-else", SOURCE, "-o", exe]
    print("plan_cem driver:", " ".join(cmd), flush=True)
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "hipcc failed:\n" + res.stdout[-4000:]
    with open(exe, "rb") as f:
        assert b"__asan_init" in f.read(), "the program was linked without AddressSanitizer's runtime"
    return exe


@pytest.fixture(scope="module")
def report(plan_cem_driver, tmp_path_factory):
    case_list = C.cases()
    raw = host_driver.run("plan_cem", C.pack(case_list), tmp_path_factory.mktemp("plan_cem_cases"), exe=plan_cem_driver)
    return case_list, C.unpack(case_list, raw)


def test_the_cases_cover_the_shapes_and_edges():
    case_list = C.cases()
    shapes = {(c["seq_in"].shape[1], c["seq_in"].shape[2], c["elites"], c["seq_in"].shape[0]) for c in case_list}
    assert set(C.SHAPES) <= shapes
    assert {c["first"] for c in case_list} == {0, 1}
    assert {c["name"][0] for c in case_list} >= {"shape", "edges", "clamp", "min_std binds", "one elite"}


def test_every_case_is_bit_equal_to_the_restatement(report):
    case_list, results = report
    for c, got in zip(case_list, results):
        want = C.cem_update(c)
        for o in C.OUTPUTS:
            if o == "elite_idx" and not c["with_idx"]:
                assert (got[o] == -7).all(), c["name"]
                continue
            assert C.bits_equal(got[o], want[o]), (c["name"], o, np.flatnonzero(got[o].reshape(-1) != want[o].reshape(-1))[:8])


def test_edge_cases(report):
    case_list, results = report
    seen = set()
    for c, got in zip(case_list, results):
        if c["with_idx"]:
            C.check_special(c, got)
            seen.add(c["name"][0])
    assert {"edges", "clamp", "min_std binds", "one elite", "inf inside"} <= seen


def test_an_absent_elite_idx_leaves_the_other_outputs_alone(report):
    case_list, results = report
    c, got = case_list[-1], results[-1]
    assert not c["with_idx"]
    want = C.cem_update(c)
    for o in ("mean", "std", "seq_out", "best_err"):
        assert C.bits_equal(got[o], want[o]), o


def test_the_driver_refuses_a_bad_header(plan_cem_driver, tmp_path):
    c = dict(C.cases()[0], elites=5)                                  # E > R
    env = dict(os.environ)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(C.pack([c]))
    p = subprocess.run([plan_cem_driver, "plan_cem", src, dst], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
