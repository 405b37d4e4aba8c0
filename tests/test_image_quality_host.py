"""The image-quality kernels' core (k_image_quality, k_image_quality_finish, csrc/ndp_eval.inc) on the CPU, under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/host_drivers/image_quality.inc follows the library's source in main.hip and
scores n = 1, 3, 5 pairs by the kernels' schedule with the library's own __host__ __device__ functions, with 16 and with 32
output rows per band (8 and 4 bands, the kernel's two instantiations), every buffer (inputs, index maps, workspace,
outputs, each LDS array) in an allocation of exactly its size.  The expected values are the golden file's (tests/golden/image_quality_case.npz: SSIM by
scipy's gaussian_filter in fp64, a route that is not the kernel's) and the fp64 evaluation of the stated PSNR.  The SSIM
allowance is 4 * d32, d32 being the plain fp32 numpy restatement's own worst distance from fp64, read from the file: the
margin DESIGN 5j gives a kernel over an fp32 CPU path (the kernel contracts the taps to fmaf chains).  The sanitizers are on
the host half of the stand-alone driver only; it runs as an ordinary child process.  No GPU involved (the same pairs on the
GPU: tests/test_gpu_image_quality.py)."""
import numpy as np
import pytest

import host_driver
import quality_common as Q

ROWS = (16, 32)


@pytest.fixture(scope="module")
def driver():
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    return host_driver.build()


@pytest.fixture(scope="module")
def rec(golden):
    return golden("image_quality_case")


def _cases(rec):
    pairs = {name: (a, b) for name, a, b in Q.golden_pairs(rec)}
    pool = rec["images_u8"]                                  # 9 byte frames
    names = [str(n) for n in rec["image_names"]]
    at = names.index
    n_pool = len(pool)
    both = lambda a: {"u8": a, "f32": Q.as_float_images(a)}                 # noqa: E731
    cases = []
    for rows in ROWS:
        # n = 1, identity maps: the identical pair, bytes
        a = pool[[at("scene0")]]
        cases.append(dict(name=("identical", "u8", rows), a=a, b=a.copy(), n=1, rows=rows, pairs=["identical"]))
        # n = 3, identity maps, every operand kind: light noise, heavy noise, black against white
        a3 = pool[[at("scene0"), at("scene0"), at("black")]]
        b3 = pool[[at("scene0_light"), at("scene0_heavy"), at("white")]]
        for ka, kb in (("u8", "u8"), ("f32", "f32"), ("u8", "f32"), ("f32", "u8")):
            cases.append(dict(name=("three", ka + kb, rows), a=both(a3)[ka], b=both(b3)[kb], n=3, rows=rows,
                              pairs=["light_noise", "heavy_noise", "black_white"]))
        # n = 3, index maps with repeats into the pool
        cases.append(dict(name=("three_mapped", "u8", rows), a=pool, b=pool, n=3, rows=rows,
                          a_idx=np.array([at("scene0")] * 3, np.int32),
                          b_idx=np.array([at("scene0_light"), at("scene0_heavy"), at("scene0_inverse")], np.int32),
                          pairs=["light_noise", "heavy_noise", "inverse"]))
        # n = 5, index maps with a repeat, -1, n_a and n_b
        a_idx = np.array([at("scene0"), at("scene0"), -1, at("noise0"), n_pool], np.int32)
        b_idx = np.array([at("scene1"), n_pool, at("noise1"), at("noise1"), at("scene0")], np.int32)
        for kind in ("u8", "f32"):
            cases.append(dict(name=("five_mapped", kind, rows), a=both(pool)[kind], b=both(pool)[kind], n=5, rows=rows,
                              a_idx=a_idx, b_idx=b_idx, pairs=["unrelated", None, None, "byte_noise", None]))
        # n = 5 float pairs: identical as floats, the flat grey frame, the two pairs outside [-1, 1], the NaN
        order = ["grey", "outside_1", "outside_2", "one_nan"]
        s0 = Q.as_float(pool[at("scene0")])
        cases.append(dict(name=("five_float", "f32", rows), a=np.stack([s0] + [pairs[k][0] for k in order]),
                          b=np.stack([s0] + [pairs[k][1] for k in order]), n=5, rows=rows, pairs=["identical"] + order))
    # one output alone
    a, b = pool[[at("scene0")]], pool[[at("scene1")]]
    cases.append(dict(name=("ssim_only", "u8", 16), a=a, b=b, n=1, rows=16, psnr=False, pairs=["unrelated"]))
    cases.append(dict(name=("psnr_only", "u8", 32), a=a, b=b, n=1, rows=32, ssim=False, pairs=["unrelated"]))
    # +-Inf clamp to the ends: the same bits as finite values beyond the ends
    inf, big = Q.as_float(pool[at("scene0")]).copy(), Q.as_float(pool[at("scene0")]).copy()
    inf[0, 3, 3], inf[2, 100, 100] = np.inf, -np.inf
    big[0, 3, 3], big[2, 100, 100] = 5.0, -5.0
    light = Q.as_float_images(pool[[at("scene0_light")]])
    cases.append(dict(name=("inf", "f32", 32), a=inf[None], b=light, n=1, rows=32, pairs=[None]))
    cases.append(dict(name=("big", "f32", 32), a=big[None], b=light, n=1, rows=32, pairs=[None]))
    return cases


@pytest.fixture(scope="module")
def report(driver, rec, tmp_path_factory):
    cases = _cases(rec)
    results = Q.run_driver(driver, cases, tmp_path_factory.mktemp("image_quality_cases"))
    return {c["name"]: (c, r) for c, r in zip(cases, results)}


def test_golden_pairs_within_the_allowance_and_psnr_within_one_ulp(report, rec):
    allow = 4.0 * float(rec["d32"])
    assert 1e-6 < allow < 1e-5                                # about 6e-6: the restatement's own distance, times 4
    seen = set()
    for name, (c, (ssim, psnr)) in report.items():
        for p, pair in enumerate(c["pairs"]):
            if pair is None:
                continue
            k = Q.NAMES.index(pair)
            want_s, want_p = float(rec["ssim64"][k]), float(rec["psnr64"][k])
            seen.add(pair)
            if c.get("ssim", True):
                if np.isnan(want_s):
                    assert np.isnan(ssim[p]), (name, pair)
                else:
                    assert abs(float(ssim[p]) - want_s) <= allow, (name, pair, ssim[p], want_s)
            else:
                assert ssim[p] == -7
            if c.get("psnr", True):
                if np.isnan(want_p):
                    assert np.isnan(psnr[p]), (name, pair)
                elif np.isinf(want_p):
                    assert psnr[p] == np.inf, (name, pair)
                else:
                    assert Q.ulps(psnr[p], want_p) <= 1, (name, pair, psnr[p], want_p)
            else:
                assert psnr[p] == -7
    assert seen == set(Q.NAMES)


def test_identical_images_give_exactly_one_and_infinite_psnr(report):
    for rows in ROWS:
        ssim, psnr = report[("identical", "u8", rows)][1]
        assert ssim[0] == np.float32(1.0) and psnr[0] == np.inf
        ssim, psnr = report[("five_float", "f32", rows)][1]
        assert ssim[0] == np.float32(1.0) and psnr[0] == np.inf


def test_results_do_not_depend_on_the_band_count(report):
    by_rows = {}
    for (what, kind, rows), (_, (ssim, psnr)) in report.items():
        if what in ("ssim_only", "psnr_only", "inf", "big"):
            continue
        by_rows.setdefault((what, kind), {})[rows] = ssim.tobytes() + psnr.tobytes()
    assert len(by_rows) == 9
    for key, got in by_rows.items():
        assert got[16] == got[32], key
    # and one output alone gives the bits it has beside the other
    both = report[("five_mapped", "u8", 16)][1]
    assert report[("ssim_only", "u8", 16)][1][0][0].tobytes() == both[0][0].tobytes()
    assert report[("psnr_only", "u8", 32)][1][1][0].tobytes() == both[1][0].tobytes()


def test_byte_and_float_operands_of_the_same_bytes_give_identical_bits(report):
    for rows in ROWS:
        want = report[("three", "u8u8", rows)][1]
        for kinds in ("f32f32", "u8f32", "f32u8"):
            got = report[("three", kinds, rows)][1]
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (kinds, rows)
        a, b = report[("five_mapped", "u8", rows)][1], report[("five_mapped", "f32", rows)][1]
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        # the mapped pairs are the unmapped ones
        m = report[("three_mapped", "u8", rows)][1]
        assert m[0][:2].tobytes() == want[0][:2].tobytes() and m[1][:2].tobytes() == want[1][:2].tobytes()


def test_index_and_nan_rules(report):
    for rows in ROWS:
        for kind in ("u8", "f32"):
            ssim, psnr = report[("five_mapped", kind, rows)][1]
            # pairs 1, 2, 4: b index n_b, a index -1, a index n_a
            assert np.isnan(ssim[[1, 2, 4]]).all() and np.isnan(psnr[[1, 2, 4]]).all()
            assert np.isfinite(ssim[[0, 3]]).all() and np.isfinite(psnr[[0, 3]]).all()
        ssim, psnr = report[("five_float", "f32", rows)][1]
        assert np.isnan(ssim[4]) and np.isnan(psnr[4])          # one NaN value: both results of that pair
        assert np.isfinite(ssim[:4]).all() and np.isfinite(psnr[1:4]).all()
    inf, big = report[("inf", "f32", 32)][1], report[("big", "f32", 32)][1]
    assert np.isfinite(inf[0][0]) and np.isfinite(inf[1][0])
    assert inf[0].tobytes() == big[0].tobytes() and inf[1].tobytes() == big[1].tobytes()
