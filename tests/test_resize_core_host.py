"""The Lanczos resize (csrc/ndp_resize.inc) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer (signed
overflow included).  tests/host_drivers/resize.inc follows the library's source in main.hip, builds the coefficient tables with the
library's own function and resizes every frame by the kernel's schedule (every band split a launch can choose), with the
frame, each raw row, each band's tile and the tables in allocations of exactly their size.  The expected bytes are this
machine's PIL's, computed here.  The sanitizers are on the host half of the stand-alone driver only; it runs as an ordinary
child process.  No GPU involved (the same frames on the GPU: tests/test_gpu_resize.py).

Also here, CPU-only: the committed pin against a Pillow change (tests/golden/resize_case.npz), `norm` on bytes against the
kernels' 256-entry table, and the argument checks of the new entries through the library."""
import ctypes

import numpy as np
import pytest
import torch

import host_driver
import resize_core_host as R
from conftest import load_golden


@pytest.fixture(scope="module")
def driver():
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    return host_driver.build()


@pytest.fixture(scope="module")
def cases():
    out = []
    for h, w in R.SIZES:
        for content in R.CONTENTS:
            frame = R.make_frame(h, w, content)
            out.append(((h, w, content), frame, R.pil_resize(frame)))
    return out


@pytest.fixture(scope="module")
def report(driver, cases, tmp_path_factory):
    return R.run_driver(driver, [(f, want) for _, f, want in cases], tmp_path_factory.mktemp("resize_frames"))


def test_every_band_split_of_every_frame_gives_pil_s_bytes(cases, report):
    rec, got = report
    for i, (name, _, want) in enumerate(cases):
        assert rec["equal"][i] == 1 and rec["mismatches"][i] == 0, (name, int(rec["mismatches"][i]))
        assert np.array_equal(got[i], want), name
        assert rec["schedules"][i] >= 1
    # 500 -> 128: 25 taps; 2048 -> 128: 97; enlarging (37, 1): 7
    by_name = {n[:2]: i for i, (n, _, _) in enumerate(cases)}
    assert rec["kx"][by_name[(500, 500)]] == 25 and rec["ky"][by_name[(500, 500)]] == 25
    assert rec["kx"][by_name[(2048, 2048)]] == 97 and rec["max_tile_rows"][by_name[(2048, 2048)]] == 96
    assert rec["kx"][by_name[(37, 53)]] == 7 and rec["ky"][by_name[(1, 1)]] == 7
    assert rec["schedules"][by_name[(500, 500)]] >= 2          # the band splits of one image and of many
    # finish()'s two clamps did fire in what the driver reproduced: where a frame is enlarged Lanczos overshoots next to
    # an edge between 0 and 255, and the enlarged binary frame's bytes hold clamped values of both kinds
    i = next(j for j, c in enumerate(cases) if c[0] == (37, 53, "binary"))
    assert (got[i] == 0).mean() > 0.05 and (got[i] == 255).mean() > 0.05 and ((got[i] > 0) & (got[i] < 255)).mean() > 0.2


def test_no_accumulator_can_overflow_int32(cases, report):
    rec, _ = report
    worst = rec["worst_lo"].astype(np.int64) & 0xFFFFFFFF | (rec["worst_hi"].astype(np.int64) << 32)
    print("largest accumulator magnitude over the tables: %d (%.3f x 2^31)" % (worst.max(), worst.max() / 2.0 ** 31))
    assert (worst > 255 << 22).all()                           # the coefficients of a row sum to about 2^22
    assert (worst < 255 * 1.5 * 2 ** 22 + 2 ** 21).all() and (worst < 2 ** 31).all()


def test_committed_frames_still_resize_to_the_committed_bytes():
    """The pin against a Pillow change: frames and PIL 12.2.0's results of tests/golden/make_golden_resize.py."""
    g = load_golden("resize_case")
    assert g["frame_a"].shape == (53, 37, 3) and g["frame_b"].shape == (120, 160, 3)
    for k in ("a", "b"):
        assert np.array_equal(R.pil_resize(g["frame_" + k]), g["resized_" + k]), \
            "this Pillow resizes differently from %s" % str(g["pillow_version"])


def test_norm_on_bytes_is_the_kernels_table():
    """MPC_gym_eval.norm on a uint8 tensor against u8_norm_table's expression ((float)i / 255.0f - 0.5f) * 2.0f, which
    ndp_eval_frames_u8 and the resize kernel's float output use, on all 256 values."""
    import MPC_gym_eval
    values = torch.arange(256, dtype=torch.uint8)
    table = (np.arange(256, dtype=np.float32) / np.float32(255.0) - np.float32(0.5)) * np.float32(2.0)
    got = MPC_gym_eval.norm(values)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), table)
    assert np.array_equal(MPC_gym_eval.denorm(got).round().numpy(), np.arange(256, dtype=np.float32))


@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


def test_workspace_sizes_and_table_builder_check_their_arguments(lib):
    assert lib.ndp_resize_workspace_bytes(500, 500) == 4 * (8 + 512 + 128 * 50)
    assert lib.ndp_resize_workspace_bytes(128, 128) == 4 * (8 + 512 + 128 * 14)
    for h, w in ((0, 128), (128, 0), (2049, 128), (128, 2049), (-1, -1)):
        assert lib.ndp_resize_workspace_bytes(h, w) == 0
    need = lib.ndp_resize_workspace_bytes(37, 53)
    buf = (ctypes.c_int32 * (need // 4))()
    assert lib.ndp_resize_build_tables(37, 53, None, need) == 1 and b"null" in lib.ndp_last_error()
    assert lib.ndp_resize_build_tables(37, 53, buf, need - 1) == 1 and b"below" in lib.ndp_last_error()
    assert lib.ndp_resize_build_tables(0, 53, buf, need) == 1 and b"outside" in lib.ndp_last_error()
    assert lib.ndp_resize_build_tables(37, 2049, buf, need) == 1
    assert lib.ndp_resize_build_tables(37, 53, buf, need) == 0
    t = np.frombuffer(buf, np.int32)
    assert t[1] == 37 and t[2] == 53 and t[3] == 7 and t[4] == 7
    xb = t[8:8 + 256].reshape(128, 2)
    assert xb[:, 0].min() == 0 and (xb[:, 0] + xb[:, 1]).max() == 53 and (xb[:, 1] <= 7).all()
    kx = t[8 + 512:8 + 512 + 128 * 7].reshape(128, 7)
    assert (np.abs(kx.sum(axis=1) - (1 << 22)) <= 7).all()     # a normalised row, each tap rounded once


def test_resize_entry_rejects_bad_arguments_before_launching(lib):
    p = ctypes.c_void_p(4096)                                  # never dereferenced: every call fails its checks
    need = lib.ndp_resize_workspace_bytes(500, 500)
    f = lib.ndp_resize_lanczos_u8
    assert f(None, 1, 500, 500, p, need, 0, p, None, None) == 1 and b"null" in lib.ndp_last_error()
    assert f(p, 1, 500, 500, None, need, 0, p, None, None) == 1
    assert f(p, 1, 500, 500, p, need, 0, None, None, None) == 1
    assert f(p, 0, 500, 500, p, need, 0, p, None, None) == 1 and b"image count" in lib.ndp_last_error()
    assert f(p, 65537, 500, 500, p, need, 0, p, None, None) == 1
    assert f(p, 1, 0, 500, p, need, 0, p, None, None) == 1 and b"outside" in lib.ndp_last_error()
    assert f(p, 1, 500, 2049, p, need, 0, p, None, None) == 1
    assert f(p, 1, 500, 500, p, need - 4, 0, p, None, None) == 1 and b"below" in lib.ndp_last_error()
    assert f(ctypes.c_void_p(4097), 1, 500, 500, p, need, 0, p, None, None) == 1 and b"aligned" in lib.ndp_last_error()
    assert f(p, 1, 500, 500, p, need, 0, ctypes.c_void_p(4098), None, None) == 1
    assert f(p, 1, 500, 500, p, need, 3, p, None, None) == 1 and b"rows_per_band" in lib.ndp_last_error()
    # 2048 rows: only one output row per band fits LDS
    need = lib.ndp_resize_workspace_bytes(2048, 2048)
    assert f(p, 1, 2048, 2048, p, need, 2, p, None, None) == 1 and b"LDS" in lib.ndp_last_error()
