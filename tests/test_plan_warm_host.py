"""The planner's update with MPPI weighting and the two flags (k_plan_update) and the warm-start launch (k_plan_warm, both
csrc/ndp_plan.inc) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.  tests/host_drivers/plan_warm.inc
follows the library's source in plan_warm_main.hip, a program of its own, and replays both kernels' schedules thread by
thread with the library's own __host__ __device__ functions (namespace ndp::plan), every buffer (inputs, outputs, each
LDS array) in an allocation of exactly its size.  The program is built once per process by host_driver.build itself
(plan_warm_common.build_driver hands it the other source) and runs as an ordinary child process, nothing preloaded
(host_driver.run).  It is a program of its own because a change that adds a feature leaves every existing test file,
main.hip among them, exactly as it is.  The expected values are the numpy restatements of include/ndp.h's definitions (tests/plan_warm_common.py).  Exact: the rank
order (elite_idx), best_err, row 0 of seq_out, every output of the warm launch, every case with weighting = elites.  What
passes through exp -- the MPPI mean and std -- may differ by the fp32 rounding of two fp64 results that agree to a few fp64
ulp (numpy's, glibc's and the device's exp are each within about an ulp and are not the same function): 1 fp32 ulp there,
and ulp(mean) + |n| ulp(std) + ulp(result) for seq_out.  No GPU involved (the same cases on the GPU:
tests/test_gpu_plan_warm.py)."""
import numpy as np
import pytest

import host_driver
import plan_common as C
import plan_warm_common as W


@pytest.fixture(scope="module")
def driver():
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    return W.build_driver()


@pytest.fixture(scope="module")
def report(driver, tmp_path_factory):
    updates, warms = W.update_cases(), W.warm_cases()
    raw = host_driver.run("plan_warm", W.pack(updates, warms), tmp_path_factory.mktemp("plan_warm_cases"), exe=driver)
    return (updates, warms) + W.unpack(updates, warms, raw)


def test_the_cases_cover_the_shapes_and_edges():
    updates, warms = W.update_cases(), W.warm_cases()
    for shape in C.SHAPES:
        for weighting in (W.MPPI, W.ELITES):
            mine = [c for c in updates if c["name"][1] == shape and c["weighting"] == weighting]
            assert {c["name"][0] for c in mine} == {"flags", "ties", "nan", "inf", "e0 inf", "fewer", "all nan",
                                                    "min_std binds", "clamp"}
            assert {(c["smooth"], c["first"]) for c in mine if c["name"][0] == "flags"} == {(0, 0), (0, 1), (1, 0), (1, 1)}
            assert all((c["seq_in"].shape[1], c["seq_in"].shape[2], c["elites"], c["seq_in"].shape[0]) == shape for c in mine)
    assert {c["name"][1] for c in warms} == set(W.WARM_SHAPES)
    for shape in W.WARM_SHAPES:
        assert {c["name"][0] for c in warms if c["name"][1] == shape} == {"floor binds", "floor idle", "nan std", "clamp"}


def test_update_cases_against_the_restatement(report):
    updates, _, got_u, _ = report
    differ = total = 0
    for c, got in zip(updates, got_u):
        d, n = W.compare_update(c, got, W.plan_update(c))
        if c["weighting"] == W.MPPI:
            differ, total = differ + d, total + n
    print("MPPI mean / std / seq_out: %d of %d elements differ from the restatement" % (differ, total))


def test_update_edge_cases(report):
    updates, _, got_u, _ = report
    for c, got in zip(updates, got_u):
        tag, (b, r, e, th) = c["name"][0], c["name"][1]
        if tag == "ties":
            assert (got["elite_idx"][:, 0] == 0).all()                # the minimum twice: the lower index wins
            assert C.bits_equal(got["seq_out"][:, :, 0], c["seq_in"][:, :, 0])
            if e > 1:
                assert (got["elite_idx"][:, 1] == r - 1).all()
        if tag == "inf":
            # one finite error: with MPPI the infinite elites weigh 0 and the fit is that row and the floor
            assert (got["elite_idx"][:, 0] == 0).all()
            if c["weighting"] == W.MPPI:
                assert C.bits_equal(got["mean"], np.moveaxis(c["seq_in"][:, :, 0], 0, 1))
                assert (got["std"] == np.float32(c["min_std"])).all()
        if tag == "e0 inf":
            assert np.isinf(got["best_err"]).all() or not c["first"]
            assert np.isfinite(got["mean"]).all() and np.isfinite(got["std"]).all()       # never inf - inf
        if tag == "fewer":
            assert (got["elite_idx"][:, 0] == r // 2).all() and (got["elite_idx"][:, 1:] == -1).all()
            assert C.bits_equal(got["mean"], np.moveaxis(c["seq_in"][:, :, r // 2], 0, 1))
        if tag == "all nan":
            assert (got["elite_idx"] == -1).all()
            if c["smooth"]:
                assert C.bits_equal(got["mean"], c["mean"]) and C.bits_equal(got["std"], c["std"])
                assert np.isnan(got["best_err"]).all()                # first = 1: only written
            else:
                assert (got["mean"] == 0).all() and (got["std"] == np.float32(c["min_std"])).all()
                assert C.bits_equal(got["best_err"], c["best_err"])   # first = 0: a NaN replaces nothing
        if tag == "min_std binds":
            assert (got["std"] == np.float32(2.0)).all()
        if tag == "clamp":
            rest = got["seq_out"][:, :, 1:]
            assert (rest >= c["low"]).all() and (rest <= c["high"]).all()


def test_elites_through_the_new_entry_equal_the_old_restatement(report):
    """weighting = elites with smooth = !first is ndp_plan_cem_update: plan_common's restatement, bit for bit."""
    updates, _, got_u, _ = report
    seen = 0
    for c, got in zip(updates, got_u):
        if c["weighting"] == W.ELITES and c["smooth"] == 1 - c["first"]:
            want = C.cem_update(c)
            for o in C.OUTPUTS:
                assert C.bits_equal(got[o], want[o]), (c["name"], o)
            seen += 1
    assert seen >= 2 * len(C.SHAPES)


def test_warm_cases_are_bit_equal_to_the_restatement(report):
    _, warms, _, got_w = report
    for c, got in zip(warms, got_w):
        W.compare_warm(c, got, W.plan_warm(c))
        W.check_warm_special(c, got)


def test_the_two_exact_limits_of_the_temperature(driver, tmp_path):
    pairs = W.limit_cases()
    flat = [c for pair in pairs for c in pair if c is not None]
    got, _ = W.unpack(flat, [], host_driver.run("plan_warm", W.pack(flat, []), tmp_path, exe=driver))
    at = 0
    for pair in pairs:
        twin = None if pair[1] is None else got[at + 1]
        W.check_limits(pair, got[at], twin)
        at += 1 if pair[1] is None else 2


def test_the_driver_refuses_a_bad_header(driver, tmp_path):
    c = dict(W.update_cases()[0], weighting=2)
    host_driver.run("plan_warm", W.pack([c], []), tmp_path, timeout=300, exe=driver, expect=2)
    w = dict(W.warm_cases()[0], warm_std=-1.0)
    host_driver.run("plan_warm", W.pack([], [w]), tmp_path, timeout=300, exe=driver, expect=2)
