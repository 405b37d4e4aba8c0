"""The JPEG encoder's core (csrc/ndp_jpeg_enc.inc) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer
(signed overflow included).  tests/host_drivers/jpeg_enc.inc follows the library's source in main.hip and runs the __host__ __device__
functions the kernels call by the kernels' schedule, serially: colour conversion, downsampling, DCT and quantisation per
block; bit counts per block, scan, bits ORed into words of a buffer of exactly its own size, padding, stuffing by lane.
Every stream must be the fixture's (PIL's) bytes and must equal what a plain one-lane bit writer in the same driver gives.
Crafted coefficient sets go straight to the pack stage: the only way to the derived size bound.  The sanitizers are on the
host half of the stand-alone driver only; it runs as an ordinary child process.  No GPU involved (the same corpus on the
GPU: tests/test_gpu_jpeg_encode.py).  Most of the time is the one compilation."""
import numpy as np
import pytest

import host_driver
import jpeg_enc_core_host as E
from conftest import load_golden


@pytest.fixture(scope="module")
def driver():
    try:
        return host_driver.build()
    except host_driver.NoSanitizerRuntime as e:
        pytest.skip("this toolchain cannot link the sanitizers' runtimes: " + str(e)[-300:])


@pytest.fixture(scope="module")
def corpus():
    return load_golden("jpeg_encode_case")


def crafted():
    """Coefficient sets [384][64] (scan order, zig-zag, DC as values) and their names."""
    worst = np.full((E.BLOCKS, 64), 1023, np.int16)
    worst[:, 1::2] = -1023
    worst[:, 0] = 1016
    for first in (0, 4, 5):                                   # DC alternates per component: every difference is 2032
        own = np.array([g for g in range(E.BLOCKS) if (g % 6 < 4 if first == 0 else g % 6 == first)])
        worst[own[1::2], 0] = -1016
    zero = np.zeros((E.BLOCKS, 64), np.int16)
    last = np.zeros((E.BLOCKS, 64), np.int16)
    last[:, 63] = 1                                           # 62 zeros, then one coefficient: three ZRL each, no EOB
    wild = np.random.RandomState(5).randint(-32768, 32768, (E.BLOCKS, 64)).astype(np.int16)   # beyond any frame: the clamps
    return ["all_1023", "all_zero", "only_zz63", "any_int16"], np.stack([worst, zero, last, wild])


@pytest.fixture(scope="module")
def report(driver, corpus, tmp_path_factory):
    return E.run_driver(driver, E.corpus_frames(corpus), crafted()[1], tmp_path_factory.mktemp("jpeg_enc_corpus"))


def test_the_scheduled_writer_gives_the_fixture_s_bytes_for_every_frame(corpus, report):
    rec, streams = report
    want = E.corpus_streams(corpus)
    for i, name in enumerate(corpus["names"]):
        assert streams[i] == want[i], "%s: %d bytes, PIL %d" % (name, len(streams[i]), len(want[i]))
    for k in E.CENSUS:
        assert rec[k][:len(want)].tolist() == corpus[k].tolist(), k


def test_the_scheduled_writer_agrees_with_the_serial_one(corpus, report):
    rec, _ = report
    assert (rec["equal"] == 1).all() and (rec["len"] == rec["len_serial"]).all(), np.flatnonzero(rec["equal"] != 1)


def test_crafted_coefficients_reach_the_bound_and_stay_within_it(corpus, report):
    rec, streams = report
    names, _ = crafted()
    n = len(corpus["names"])
    bound = int(rec["max_stream"][0])
    row = {name: n + j for j, name in enumerate(names)}
    assert (rec["len"] <= bound).all()
    # the bound: a DC code with 11 more bits (20 for Y, 22 for chroma) and 63 x (16 + 10) AC bits per block, every byte stuffed
    assert bound == E.HEADER + 2 * ((256 * (20 + 63 * 26) + 128 * (22 + 63 * 26) + 7) // 8) + 2
    # what the set takes: +-1023 after no run is 16 + 10 bits in the Y table and 12 + 10 in the chroma table; the first
    # block of each component has a difference of 1016, category 10, whose code is 2 bits shorter
    assert rec["total_bits"][row["all_1023"]] == 256 * (20 + 63 * 26) + 128 * (22 + 63 * 22) - 3 * 2
    assert rec["len"][row["all_1023"]] > 75000
    assert rec["max_dc_cat"][row["all_1023"]] == 11 and rec["total_bits"][row["any_int16"]] <= rec["total_bits"][row["all_1023"]]
    assert rec["eob_only"][row["all_zero"]] == E.BLOCKS and rec["total_bits"][row["all_zero"]] == 256 * (2 + 4) + 128 * (2 + 2)
    assert rec["zrl"][row["only_zz63"]] == 3 * E.BLOCKS and rec["eob_only"][row["only_zz63"]] == 0
    for j in row.values():
        assert streams[j][:E.HEADER] == corpus["header"].tobytes() and streams[j][-2:] == b"\xff\xd9"
