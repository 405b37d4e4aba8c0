"""The generator scoring kernel's core (k_gan_score, csrc/ndp_eval.inc) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer.  tests/host_drivers/gan_score.inc follows the library's source in main.hip and scores every case by the
kernel's schedule with the library's own __host__ __device__ functions (namespace ndp::gan_score), every buffer (inputs,
outputs, each LDS array) in an allocation of exactly its size.  The expected values are the plain numpy restatement of the
stated definition (tests/gan_eval_common.py).  The sanitizers are on the host half of the stand-alone driver only; it runs
as an ordinary child process.  No GPU involved (the same cases on the GPU: tests/test_gpu_gan_eval.py)."""
import numpy as np
import pytest

import gan_eval_common as C
import host_driver


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    driver = host_driver.build()
    case_list = C.cases()
    return case_list, C.run_driver(driver, case_list, tmp_path_factory.mktemp("gan_score_cases"))


def test_every_case_matches_the_plain_restatement(report):
    case_list, results = report
    assert [c["x"].shape[:2] + (c["noise"].shape[2],) for c, _ in case_list[:7]] == list(C.SHAPES)
    worst = {}
    for (c, wanted), got in zip(case_list, results):
        for o, m in C.check_scores(c, got, wanted).items():
            worst[o] = tuple(max(a, b) for a, b in zip(worst.get(o, (0, 0, 0)), m))
    for o, (dist, ref, tol) in sorted(worst.items()):
        print("%s: driver to fp64 %.3g, torch fp32 to fp64 %.3g, bound %.3g" % (o, dist, ref, tol))


def test_special_rows(report):
    case_list, results = report
    for (c, _), got in zip(case_list, results):
        if c["name"][0] != "special":
            continue
        k = c["x"].shape[1]
        # row 0: samples 1 and 3 are equal and the closest: the first of the tie wins, for the error and for the logit
        assert got["best_k"][0] == 1 and got["d_pick_k"][0] == 1
        assert got["sample_err"][0, 1] == got["sample_err"][0, 3] == got["best_err"][0] == got["d_pick_err"][0]
        assert np.isfinite(got["ndiv"][0]) and np.isfinite(got["spread"][0])
        # row 1: sample 0 is NaN: the curve starts NaN, is finite from sample 1 on, and the NaN is chosen by nothing
        assert np.isnan(got["sample_err"][1, 0]) and np.isfinite(got["sample_err"][1, 1:]).all()
        assert np.isnan(got["best_curve"][1, 0]) and np.isfinite(got["best_curve"][1, 1:]).all()
        assert got["best_k"][1] >= 1 and got["d_pick_k"][1] >= 1 and np.isfinite(got["best_err"][1])
        assert np.isnan(got["mean_err"][1]) and np.isnan(got["spread"][1]) and np.isnan(got["ndiv"][1])
        assert np.isnan(got["d_fake_prob"][1])
        # row 2: all NaN: k = 0 and NaN
        assert got["best_k"][2] == 0 and got["d_pick_k"][2] == 0
        assert np.isnan(got["best_err"][2]) and np.isnan(got["best_curve"][2]).all() and np.isnan(got["d_pick_err"][2])
        # row 3 is ordinary, and the curve falls
        assert np.isfinite(got["best_curve"][3]).all() and (np.diff(got["best_curve"][3]) <= 0).all()
        assert got["best_curve"][3, k - 1] == got["best_err"][3]


def test_k_of_one_gives_nan_spread_and_ndiv(report):
    case_list, results = report
    got = results[0]
    assert case_list[0][0]["x"].shape[:2] == (1, 1)
    assert np.isnan(got["spread"]).all() and np.isnan(got["ndiv"]).all()
    assert got["best_k"][0] == 0 and got["sample_err"][0, 0] == got["best_err"][0] == got["mean_err"][0]


def test_absent_inputs_and_outputs_leave_the_others_bits_alone(report):
    case_list, results = report
    full = results[2]
    seen = 0
    for (c, wanted), got in zip(case_list[9:], results[9:]):
        wanted = C.available(c) if wanted is None else wanted
        for o in C.OUTPUTS:
            if o in wanted:
                assert got[o].tobytes() == full[o].tobytes(), (c["name"], o)
            else:
                assert (got[o] == -7).all(), (c["name"], o)
        seen += 1
    assert seen == 3 + len(C.OUTPUTS)
