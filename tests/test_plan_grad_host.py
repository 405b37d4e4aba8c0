"""The three launches of the planner's gradient stage (k_plan_goal_grad, k_plan_grad_gather, k_plan_grad_step,
csrc/ndp_plan.inc) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.  tests/host_drivers/plan_grad.inc
follows the library's source in plan_grad_main.hip, a program of its own, and replays the kernels' schedules thread by
thread with the library's own __host__ __device__ functions (namespace ndp::plan), every buffer (inputs, outputs, each LDS
array) in an allocation of exactly its size.  The program is built once per process by host_driver.build itself
(plan_grad_common.build_driver hands it the other source) and runs as an ordinary child process, nothing preloaded
(host_driver.run).  The expected values are the numpy restatements of include/ndp.h's definitions
(tests/plan_grad_common.py), and every output is bit-equal to them: the fp64 sum of err follows the documented order with
its fused multiply-add, and fp64 sqrt and division are correctly rounded in numpy and in C alike.  No GPU involved (the
same cases on the GPU: tests/test_gpu_plan_grad.py)."""
import numpy as np
import pytest

import host_driver
import plan_common as C
import plan_grad_common as G


@pytest.fixture(scope="module")
def driver():
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    return G.build_driver()


@pytest.fixture(scope="module")
def report(driver, tmp_path_factory):
    cases = G.goal_cases(), G.gather_cases(), G.step_cases()
    raw = host_driver.run("plan_grad", G.pack(*cases), tmp_path_factory.mktemp("plan_grad_cases"), exe=driver)
    return cases, G.unpack(*cases, raw)


def test_the_cases_cover_the_tags_and_shapes():
    goals, gathers, steps = G.goal_cases(), G.gather_cases(), G.step_cases()
    for shape in G.GOAL_SHAPES:
        assert {c["name"][0] for c in goals if c["name"][1] == shape} == set(G.GOAL_TAGS)
    assert {(c["rows_per_goal"], c["inplace"]) for c in goals} >= {(1, 0), (2, 0), (2, 1)}       # rows_per_goal 1 and G
    for shape in G.GATHER_SHAPES:
        mine = [c for c in gathers if c["name"][1] == shape]
        assert {c["name"][0] for c in mine} == {"plain", "ties", "nan", "inf", "all nan"}
        assert all((c["seq"].shape[1], c["seq"].shape[2], c["rows"], c["seq"].shape[0]) == shape for c in mine)
    shapes = set(G.GATHER_SHAPES)
    assert {s[1] for s in shapes} >= {4, 5} and {s[2] for s in shapes} >= {1, 2} and {s[3] for s in shapes} >= {1, 2, 3}
    assert any(r % 2 == 1 and g == r // 2 for _, r, g, _ in shapes)                              # odd R with G = R // 2
    for shape in G.STEP_SHAPES:
        mine = [c for c in steps if c["name"][1] == shape]
        assert {c["name"][0] for c in mine} == {"sgd", "adam t1", "adam t3", "nan grad", "inf grad", "zero grad", "clamp",
                                                "no dst"}
    by_tag = {c["name"][0]: c for c in steps}
    assert by_tag["adam t1"]["t"] == 1 and by_tag["adam t3"]["t"] == 3 and by_tag["adam t3"]["optimizer"] == G.ADAM
    assert np.isnan(by_tag["nan grad"]["grad"]).sum() == 1 and np.isinf(by_tag["inf grad"]["grad"]).sum() == 1
    assert (by_tag["zero grad"]["grad"][:, 0, 0] == 0).all() and by_tag["no dst"]["dst"] is None
    assert any(c["seq_g"].shape[1] * c["seq_g"].shape[2] > 256 for c in steps)                   # more than one block


def test_the_vectorised_fma_is_the_exact_one():
    g = np.random.default_rng(1)
    a = np.concatenate([g.standard_normal(400), g.standard_normal(100) * 1e-7, [0.0, 1.0, 3.0, 1.0 + 2.0 ** -30]])
    s = np.concatenate([g.random(400) * 50, g.random(100), [0.0, 2.0 ** -60, 1.0, 1.0]])
    got = G.fma(a, a, s)
    want = np.array([G.fma_exact(float(x), float(x), float(y)) for x, y in zip(a, s)])
    assert got.tobytes() == want.tobytes()
    assert (got != a * a + s).any()                                   # the single rounding is seen on these operands


def test_goal_grad_against_the_restatement(report):
    (goals, _, _), (got, _, _) = report
    for c, one in zip(goals, got):
        want = G.goal_grad(c)
        G.compare(c, one, want, G.GOAL_OUTPUTS)
        n = c["pred"].shape[0]
        if c["name"][0] == "nan":
            assert np.isnan(one["err"][n - 1]) and np.isnan(one["d_pred"][n - 1, 12345])
            assert np.isnan(one["d_pred"][n - 1]).sum() == 1 and np.isinf(one["err"][0])
        else:
            assert np.isfinite(one["err"]).all() and (one["err"] > 0).all()


def test_in_place_equals_out_of_place(report):
    (goals, _, _), (got, _, _) = report
    pairs = {}
    for c, one in zip(goals, got):
        pairs.setdefault((c["name"][0], c["name"][1][:3]), {})[c["inplace"]] = (c, one)
    seen = 0
    for both in pairs.values():
        if len(both) == 2:                                            # the same operands, d_pred apart and in pred
            assert C.bits_equal(both[0][0]["pred"], both[1][0]["pred"])
            for o in G.GOAL_OUTPUTS:
                assert both[0][1][o].tobytes() == both[1][1][o].tobytes(), o
            seen += 1
    assert seen == len(G.GOAL_TAGS)


def test_gather_against_the_restatement(report):
    (_, gathers, _), (_, got, _) = report
    for c, one in zip(gathers, got):
        G.compare(c, one, G.grad_gather(c), G.GATHER_OUTPUTS)
        b, r, g, th = c["name"][1]
        for i in range(b):
            assert not set(one["src"][i]) & set(one["dst"][i])        # disjoint: G <= R // 2
        if c["name"][0] == "ties":
            assert (one["src"][:, 0] == 0).all()                      # the minimum twice: the lower index wins
            assert (one["dst"][:, g - 1] == 2).all()                  # the maximum twice: the higher index ranks last
        if c["name"][0] == "nan":
            assert all(k % 2 == 0 for k in one["dst"][:, g - 1])      # NaNs rank after every number
            assert (one["src"][:, 0] % 2 == 1).all()
        if c["name"][0] == "all nan":
            assert (one["src"] == np.arange(g)).all() and (one["dst"] == np.arange(r - g, r)).all()
        assert (one["m"] == 0).all() and (one["v"] == 0).all()


def test_step_against_the_restatement(report):
    (_, _, steps), (_, _, got) = report
    for c, one in zip(steps, got):
        G.compare(c, one, G.grad_step(c), G.step_outputs(c))
        G.check_step_special(c, one)
        assert C.bits_equal(one["curve"], c["err_g"])
        if c["optimizer"] == G.SGD:
            assert C.bits_equal(one["m"], c["m"]) and C.bits_equal(one["v"], c["v"])
