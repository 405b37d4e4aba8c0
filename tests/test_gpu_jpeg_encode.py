"""ndp_jpeg_encode_u8 on the MI355X: the streams of `JpegEncoder` are PIL's bytes (tests/golden/jpeg_encode_case.npz, made by
tests/golden/make_golden_jpeg_encode.py; every comparison is byte equality), at batch sizes around the offset scan's tile,
twice the same, decodable by `JpegDecoder` into PIL's pixels, within `capacity` whatever it is, and fed by `LanczosResizer`."""
import numpy as np
import pytest
import torch

import jpeg_core_host as H
import jpeg_enc_core_host as E
from conftest import load_golden

pytestmark = pytest.mark.gpu

SCAN_TILE = 1024                      # kScanTile of csrc/ndp_jpeg_enc.inc


@pytest.fixture(scope="module")
def corpus():
    g = load_golden("jpeg_encode_case")
    g["all_frames"] = E.corpus_frames(g)
    g["list"] = E.corpus_streams(g)
    return g


@pytest.fixture(scope="module")
def encoder():
    from ndivplanning_amd.jpeg import JpegEncoder
    return JpegEncoder()


def expected(corpus, rows):
    streams = [corpus["list"][i] for i in rows]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    return np.frombuffer(b"".join(streams), np.uint8), offsets


def assert_streams(corpus, rows, buffer, offsets, status):
    want_buf, want_off = expected(corpus, rows)
    got_off = offsets.cpu().numpy()
    assert not status.cpu().numpy().any()
    assert np.array_equal(got_off, want_off), [(corpus["names"][rows[i]], int(a), int(b)) for i, (a, b) in
                                                enumerate(zip(np.diff(got_off), np.diff(want_off))) if a != b][:8]
    got = buffer.cpu().numpy()[:int(want_off[-1])]
    if not np.array_equal(got, want_buf):
        bad = [corpus["names"][r] for i, r in enumerate(rows)
               if not np.array_equal(got[want_off[i]:want_off[i + 1]], want_buf[want_off[i]:want_off[i + 1]])]
        raise AssertionError("streams differ from PIL's: %s" % bad[:8])


@pytest.mark.parametrize("n", [1, 3, 17, None])
def test_encode_gives_pil_s_bytes(corpus, encoder, n):
    total = len(corpus["list"])
    rows = list(range(total)) if n is None else [(5 * j + n) % total for j in range(n)]
    buffer, offsets = encoder.encode(torch.from_numpy(corpus["all_frames"][rows]))
    assert buffer.is_cuda and buffer.dtype == torch.uint8 and offsets.dtype == torch.int64
    assert buffer.numel() == int(offsets[-1])
    assert_streams(corpus, rows, buffer, offsets, encoder.status)


def test_one_frame_more_than_the_offset_scan_s_tile(corpus, encoder):
    total = len(corpus["list"])
    small = [i for i in range(total) if len(corpus["list"][i]) < 8000]       # keeps the batch a few MB
    rows = [small[j % len(small)] for j in range(SCAN_TILE + 1)]
    rows[SCAN_TILE - 1], rows[SCAN_TILE] = int(np.argmax(np.diff(corpus["offsets"]))), small[3]
    frames = torch.from_numpy(corpus["all_frames"])[rows]
    buffer, offsets = encoder.encode(frames)
    assert_streams(corpus, rows, buffer, offsets, encoder.status)


def test_two_runs_give_the_same_bytes(corpus, encoder):
    frames = torch.from_numpy(corpus["all_frames"]).cuda()
    a, ao = encoder.encode(frames)
    b, bo = encoder.encode(frames)
    assert torch.equal(a, b) and torch.equal(ao, bo)
    lists = encoder.encode_to_bytes(frames)
    assert lists == corpus["list"]
    five = frames.view(2, 19, 128, 128, 3)
    jf = encoder.encode_frames(five)
    assert jf.shape == (2, 19, 128, 128, 3) and torch.equal(jf.buffer, a) and torch.equal(jf.offsets, ao)


def test_the_decoder_reads_the_encoder_s_streams_into_pil_s_pixels(corpus, encoder):
    from ndivplanning_amd.jpeg import JpegDecoder
    frames = JpegDecoder().decode(*encoder.encode(torch.from_numpy(corpus["all_frames"]))).cpu().numpy()
    for i, name in enumerate(corpus["names"]):
        assert np.array_equal(H.digest(frames[i]), corpus["digest"][i]), name


@pytest.mark.parametrize("cut", ["last", "middle", "nothing"])
def test_capacity_is_respected(corpus, encoder, cut):
    rows = list(range(12, 24))
    want_buf, want_off = expected(corpus, rows)
    total = int(want_off[-1])
    capacity = {"last": total - 1, "middle": int(want_off[5]) + 700, "nothing": 600}[cut]
    fit = int(np.searchsorted(want_off, capacity, side="right")) - 1          # frames that fit
    assert fit == {"last": 11, "middle": 5, "nothing": 0}[cut]
    x = encoder._frames(torch.from_numpy(corpus["all_frames"][rows]))
    guard = 4096
    # a larger allocation: the capacity's bytes, then guard bytes the encoder must not touch
    big = torch.full((capacity + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.full((len(rows) + 1,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    from ndivplanning_amd import _capi
    ws = encoder._workspace(len(rows))
    _capi.check(encoder.lib.ndp_jpeg_encode_u8(_capi.ptr(x), len(rows), _capi.ptr(big), capacity, _capi.ptr(off), _capi.ptr(st),
                                               _capi.ptr(ws), int(ws.numel()), _capi.stream_ptr(big.device)), "ndp_jpeg_encode_u8")
    off, st, big = off.cpu().numpy(), st.cpu().numpy(), big.cpu().numpy()
    assert st.tolist() == [0] * fit + [4] * (len(rows) - fit)
    assert np.array_equal(off[:fit + 1], want_off[:fit + 1]) and (off[fit + 1:] == want_off[fit]).all()
    assert np.array_equal(big[:want_off[fit]], want_buf[:want_off[fit]])
    assert (big[want_off[fit]:] == 0xA5).all(), "bytes beyond the last frame that fits were written"


def test_a_default_capacity_that_is_too_small_is_retried_at_the_sum_of_the_lengths(corpus, monkeypatch):
    from ndivplanning_amd.jpeg import JpegEncoder
    enc = JpegEncoder()
    monkeypatch.setattr(enc, "DEFAULT_FRAME_BYTES", 3000)         # the corpus averages 6.5 KB a frame
    monkeypatch.setattr(enc, "EAGER_FRAME_BYTES", 1000)
    rows = list(range(len(corpus["list"])))
    frames = corpus["all_frames"]                                 # numpy input
    buffer, offsets = enc.encode(frames)
    assert buffer.numel() == corpus["offsets"][-1] == enc._needed(len(rows))
    assert_streams(corpus, rows, buffer, offsets, enc.status)
    assert enc.encode_to_bytes(frames) == corpus["list"]
    jf = enc.encode_frames(frames.reshape(2, 19, 128, 128, 3))
    assert jf.shape == (2, 19, 128, 128, 3) and torch.equal(jf.buffer, buffer)


def test_bad_arguments_are_refused_without_launching(encoder):
    from ndivplanning_amd import _capi
    lib = encoder.lib
    assert lib.ndp_jpeg_encode_workspace_bytes(0) == 0 and lib.ndp_jpeg_encode_workspace_bytes(65537) == 0
    assert lib.ndp_jpeg_encode_lengths_offset(0) == -1 and lib.ndp_jpeg_encode_lengths_offset(3) == 3 * 384 * 64 * 2
    assert lib.ndp_jpeg_encode_workspace_bytes(2) >= 2 * 384 * 64 * 2 + 16
    x = torch.zeros(1, 128, 128, 3, dtype=torch.uint8, device="cuda")
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = encoder._workspace(1)
    args = lambda **k: [k.get("x", _capi.ptr(x)), k.get("n", 1), _capi.ptr(out), k.get("cap", 4096), _capi.ptr(off), _capi.ptr(st),
                        _capi.ptr(ws), k.get("wsb", int(ws.numel())), _capi.stream_ptr(x.device)]
    for bad in (dict(x=None), dict(n=0), dict(n=65537), dict(cap=-1), dict(wsb=100)):
        assert lib.ndp_jpeg_encode_u8(*args(**bad)) == 1, bad
    with pytest.raises(_capi.NdpError):
        encoder.encode(torch.zeros(2, 64, 64, 3, dtype=torch.uint8))


def test_resizer_into_encoder_equals_pil_resize_and_pil_save(corpus, encoder):
    from ndivplanning_amd.resize import LanczosResizer
    small, _ = LanczosResizer()(torch.from_numpy(E.env_frames()), floats=False)
    rows = [int(i) for i in corpus["env_index"]]
    assert np.array_equal(small.cpu().numpy(), corpus["all_frames"][rows])
    buffer, offsets = encoder.encode(small)
    assert_streams(corpus, rows, buffer, offsets, encoder.status)
    assert encoder.encode_to_bytes(small) == [corpus["list"][i] for i in rows]
