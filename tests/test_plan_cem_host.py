"""The planner's cross-entropy update (k_plan_cem_update, csrc/ndp_plan.inc) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer.  tests/host_drivers/plan_cem.inc follows the library's source in main.hip and replays the
workgroup's schedule thread by thread with the library's own __host__ __device__ functions (namespace ndp::plan), every
buffer (inputs, outputs, each LDS array) in an allocation of exactly its size.  The program is host_driver's, built once
per process, and runs as an ordinary child process.  The expected values are the plain numpy restatement of
include/ndp.h's definition (tests/plan_common.py): every output bit for bit.  No GPU involved (the same cases on the
GPU: tests/test_gpu_plan_cem.py)."""
import numpy as np
import pytest

import host_driver
import plan_common as C


@pytest.fixture(scope="module")
def driver():
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    return host_driver.build()


@pytest.fixture(scope="module")
def report(driver, tmp_path_factory):
    case_list = C.cases()
    raw = host_driver.run("plan_cem", C.pack(case_list), tmp_path_factory.mktemp("plan_cem_cases"), exe=driver)
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


def test_the_driver_refuses_a_bad_header(driver, tmp_path):
    c = dict(C.cases()[0], elites=5)                                  # E > R
    host_driver.run("plan_cem", C.pack([c]), tmp_path, timeout=300, exe=driver, expect=2)
