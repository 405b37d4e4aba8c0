"""GPU tests of the device JPEG decoder (ndp_jpeg_decode_u8) on the edge corpus tests/golden/jpeg_edges.npz (made by
tests/golden/make_golden_jpeg_edges.py): the streams that need up to chunks + 1 sync rounds, the two sides of the 24 KB LDS
split and of the 128-bit chunk floor, flat frames, symbol extremes, header variants, rejected streams in between.  The
fixture holds no frames: PIL's bytes are checked by a 16-byte blake2b digest and by the byte sums per 16x16 MCU, which
say where a wrong frame differs (from some MCU on: the entropy stage lost its place; isolated MCUs: IDCT, upsampling or
colour).  The same corpus goes through the decoder's core on the CPU in tests/test_jpeg_core_host.py."""
import numpy as np
import pytest
import torch

import jpeg_core_host as H
from conftest import load_golden
from test_gpu_jpeg import _decoder, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus():
    g = load_golden("jpeg_edges")
    o = g["offsets"]
    g["list"] = [g["streams"][o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]
    return g


def _check(g, i, frame, status, how):
    """Frame and status of corpus stream i against the fixture."""
    where = "%s (%s, %d host rounds of %d chunks) %s" % (g["names"][i], g["classes"][i], g["rounds"][i], g["nchunks"][i], how)
    assert int(status) == int(g["status"][i]), "%s: status %d, expected %d" % (where, int(status), int(g["status"][i]))
    frame = frame.numpy()
    if g["status"][i] != 0:
        assert not frame.any(), where + ": a rejected frame is not all zero"
        return
    same = np.array_equal(H.mcu_sums(frame), g["mcu_sums"][i]) and np.array_equal(H.digest(frame), g["digest"][i])
    assert same, "%s: not PIL's bytes, %s" % (where, H.differing_mcus(frame, g["mcu_sums"][i]))


def test_every_edge_stream_alone(corpus):
    dec = _decoder()
    for i, s in enumerate(corpus["list"]):
        frames, st = _run(dec, [s])
        _check(corpus, i, frames[0], st[0], "alone")


def test_all_edge_streams_in_one_batch_twice(corpus):
    dec = _decoder()
    f1, s1 = _run(dec, corpus["list"])
    for i in range(len(corpus["list"])):
        _check(corpus, i, f1[i], s1[i], "in the batch")
    f2, s2 = _run(dec, corpus["list"])
    assert torch.equal(f1, f2) and torch.equal(s1, s2)


def test_the_batch_shuffled_at_unaligned_offsets_with_junk_between(corpus):
    dec = _decoder()
    rng = np.random.RandomState(1)
    n = len(corpus["list"])
    order = rng.permutation(n)
    pad = rng.randint(0, 7, n)
    frames, st = _run(dec, [corpus["list"][i] for i in order], pad=pad, lead=3)
    for j, i in enumerate(order):
        _check(corpus, int(i), frames[j], st[j], "shuffled, at place %d after %d junk bytes" % (j, 3 + int(pad[:j].sum())))


def test_print_the_entropy_stage_s_time_of_the_slowest_single_stream(corpus):
    """Not asserted: the figure DESIGN.md section 5f quotes (run with -s).  Device events around k_jpeg_entropy, one frame
    per decode, the second decode of each stream."""
    from ndivplanning_amd import _capi
    dec = _decoder()
    times = {}
    ok = [i for i in range(len(corpus["list"])) if corpus["status"][i] == 0]
    _run(dec, [corpus["list"][ok[0]]])
    _capi.timing_enable(True)
    try:
        for i in ok:
            for _ in range(2):
                _run(dec, [corpus["list"][i]])
                torch.cuda.synchronize()
                t = _capi.timing_collect()
            times[i] = t["k_jpeg_entropy"][0]
    finally:
        _capi.timing_enable(False)
    by_time = sorted(times, key=times.get)
    slow = by_time[-1]
    print("\nk_jpeg_entropy, one frame: slowest %s %.3f ms (%d host rounds of %d chunks, %d bytes); median %.3f ms; "
          "fastest %s %.3f ms" % (corpus["names"][slow], times[slow], corpus["rounds"][slow], corpus["nchunks"][slow],
                                  corpus["ncompact"][slow], times[by_time[len(by_time) // 2]], corpus["names"][by_time[0]],
                                  times[by_time[0]]))
    for i in by_time[-5:]:
        print("  %-40s %.3f ms, %d rounds" % (corpus["names"][i], times[i], corpus["rounds"][i]))
    assert len(times) == len(ok) and all(t > 0 for t in times.values())
