"""The forward-model scoring kernel's core (k_fm_score, csrc/ndp_eval.inc) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer.  tests/host_drivers/fm_score.inc follows the library's source in main.hip and scores n = 1, 3, 5
predictions by the kernel's schedule with the library's own __host__ __device__ functions, every buffer (inputs, index
maps, outputs, each LDS array) in an allocation of exactly its size.  The expected values are the plain numpy restatement
of the stated definition (tests/fm_eval_common.py).  The sanitizers are on the host half of the stand-alone driver only;
it runs as an ordinary child process.  No GPU involved (the same cases on the GPU: tests/test_gpu_forward_model_eval.py)."""
import numpy as np
import pytest

import fm_eval_common as C
import host_driver


@pytest.fixture(scope="module")
def driver():
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    return host_driver.build()


def _cases():
    rng = np.random.RandomState(3)
    cases = []
    for n in (1, 3, 5):
        pred = C.boundary_images(n, seed=n)
        n_target, n_base = n + 1, n + 2
        tgt_u8 = rng.randint(0, 256, (n_target, 128, 128, 3)).astype(np.uint8)
        base_u8 = rng.randint(0, 256, (n_base, 128, 128, 3)).astype(np.uint8)
        # index maps with repeats; for n >= 3 one index of -1 and one of n_target (target), one of n_base (base)
        tidx = rng.randint(0, n_target, n).astype(np.int32)
        bidx = rng.randint(0, n_base, n).astype(np.int32)
        tidx[0] = tidx[-1]
        if n >= 3:
            tidx[1], tidx[2], bidx[0] = -1, n_target, n_base
        if n >= 5:
            bidx[3], bidx[4] = -1, bidx[1]
        for tk in ("u8", "f32"):
            for bk in ("u8", "f32", None):
                tgt = tgt_u8 if tk == "u8" else C.as_float_images(tgt_u8)
                base = None if bk is None else base_u8 if bk == "u8" else C.as_float_images(base_u8)
                cases.append(dict(pred=pred, target=tgt, base=base, target_idx=tidx, base_idx=None if base is None else bidx,
                                  bytes=True, name=(n, tk, bk, "maps")))
        # no index maps: image i uses row i of both
        cases.append(dict(pred=pred, target=tgt_u8, base=C.as_float_images(base_u8), target_idx=None, base_idx=None,
                          bytes=False, name=(n, "u8", "f32", "identity")))
    return cases


@pytest.fixture(scope="module")
def report(driver, tmp_path_factory):
    cases = _cases()
    return cases, C.run_driver(driver, cases, tmp_path_factory.mktemp("fm_score_cases"))


def test_bytes_errors_and_bad_indices_match_the_plain_restatement(report):
    cases, results = report
    assert len(cases) == 3 * 7
    for c, (err, base_err, by) in zip(cases, results):
        n = len(c["pred"])
        tidx = c["target_idx"] if c["target_idx"] is not None else np.arange(n)
        tgt = C.as_float_images(c["target"])
        want = C.want_mse(c["pred"], np.arange(n), tgt, tidx)
        bad = np.isnan(want)
        # the noise images hold no NaN, image 0 does: its error is NaN by arithmetic, as the definition's
        assert np.array_equal(np.isnan(err), bad), c["name"]
        assert (C.ulps(err[~bad], want[~bad]) <= 1).all(), (c["name"], err, want)
        if c["base"] is not None:
            bidx = c["base_idx"] if c["base_idx"] is not None else np.arange(n)
            want_b = C.want_mse(C.as_float_images(c["base"]), bidx, tgt, tidx)
            bad_b = np.isnan(want_b)
            assert np.array_equal(np.isnan(base_err), bad_b), (c["name"], base_err, want_b)
            assert (C.ulps(base_err[~bad_b], want_b[~bad_b]) <= 1).all(), c["name"]
        else:
            assert (base_err == -7).all()
        if c["bytes"]:
            assert np.array_equal(by, C.want_bytes(c["pred"])), c["name"]
        else:
            assert (by == 0xA5).all()


def test_out_of_range_indices_give_nan_for_that_image_only(report):
    cases, results = report
    c, (err, base_err, _) = next((c, r) for c, r in zip(cases, results) if c["name"] == (5, "u8", "u8", "maps"))
    # image 0 holds NaN values itself; images 1 and 2 have a target index of -1 and of n_target
    assert np.isnan(err[[0, 1, 2]]).all() and np.isfinite(err[[3, 4]]).all()
    # base_err: NaN where the target index is bad (1, 2) or the base index is (0: n_base, 3: -1); image 4 is fine
    assert np.isnan(base_err[[0, 1, 2, 3]]).all() and np.isfinite(base_err[4])


def test_byte_and_float_targets_of_the_same_bytes_give_identical_bits(report):
    cases, results = report
    by_name = {c["name"]: r for c, r in zip(cases, results)}
    for n in (1, 3, 5):
        a, b = by_name[(n, "u8", "u8", "maps")], by_name[(n, "f32", "f32", "maps")]
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert by_name[(n, "u8", "f32", "maps")][1].tobytes() == a[1].tobytes()
