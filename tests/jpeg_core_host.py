"""Run tests/host_drivers/jpeg.inc, the JPEG decoder's core on the CPU, through tests/host_driver.py (used by
tests/test_jpeg_core_host.py and tests/golden/make_golden_jpeg_edges.py)."""
import hashlib

import numpy as np

import host_driver

FIELDS = ("status", "status_serial", "frames_equal", "rounds", "nchunks", "ncompact", "max_dc_cat", "zrl", "no_eob", "slow",
          "max_abs", "reserved")
CENSUS = ("rounds", "nchunks", "ncompact", "max_dc_cat", "zrl", "no_eob", "slow", "max_abs")
FRAME = 128 * 128 * 3
OK = 0
LDS = 24576                                                  # kStreamLdsBytes of csrc/ndp_jpeg.inc


def build_driver(out_dir=None, sanitize=True):
    return host_driver.build(sanitize)


def run_driver(exe, streams, work_dir, frames=False, timeout=900):
    """Decode `streams` (bytes each) in a child process; asserts that it exits 0 with no sanitizer report.  Returns
    (records: {field: int32 [n]}, chunked, serial) where the last two are uint8 [n,128,128,3], or None without `frames`."""
    payload = np.int32(len(streams)).tobytes() + b"".join(np.int32(len(s)).tobytes() + bytes(s) for s in streams)
    raw = np.frombuffer(host_driver.run("jpeg", payload, work_dir, ["frames"] if frames else [], timeout, exe), np.uint8)
    n, per = len(streams), 4 * len(FIELDS) + (2 * FRAME if frames else 0)
    assert raw.size == n * per, (raw.size, n, per)
    raw = raw.reshape(n, per)
    ints = raw[:, :4 * len(FIELDS)].copy().view(np.int32)
    rec = {k: ints[:, i].copy() for i, k in enumerate(FIELDS)}
    if not frames:
        return rec, None, None
    pix = raw[:, 4 * len(FIELDS):].reshape(n, 2, 128, 128, 3)
    return rec, pix[:, 0], pix[:, 1]


def digest(frame):
    """16-byte blake2b of a frame's bytes, as uint8 [16]."""
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(frame, np.uint8).tobytes(), digest_size=16).digest(), np.uint8)


def mcu_sums(frame):
    """Byte sums per 16x16 MCU and channel, uint32 [8,8,3]: which MCUs of a wrong frame differ."""
    return np.asarray(frame, np.uint32).reshape(8, 16, 8, 16, 3).sum(axis=(1, 3), dtype=np.uint32)


def differing_mcus(frame, sums):
    """The (row, column) MCUs whose sums differ from `sums`, as a short string."""
    bad = np.argwhere((mcu_sums(frame) != sums).any(axis=2))
    if len(bad) == 0:
        return "no MCU sum differs (the digest does)"
    head = ", ".join("(%d,%d)" % (r, c) for r, c in bad[:12])
    return "%d of 64 MCUs differ, first %s%s" % (len(bad), head, " ..." if len(bad) > 12 else "")


def segments(data):
    """[(marker, start, end)] of the marker segments SOI .. SOS (start at the first 0xFF), end exclusive."""
    assert data[:2] == b"\xff\xd8"
    out, p = [], 2
    while True:
        q = p
        while data[q + 1] == 0xFF:                           # fill bytes
            q += 1
        assert data[q] == 0xFF and data[q + 1] != 0x00, q
        m = data[q + 1]
        n = int.from_bytes(data[q + 2:q + 4], "big")
        out.append((m, p, q + 2 + n))
        p = q + 2 + n
        if m == 0xDA:
            return out


def check_edge_classes(g):
    """The class conditions, on the arrays of a loaded (or about to be written) jpeg_edges.npz.
    tests/test_jpeg_core_host.py calls this on the committed file."""
    names, classes = [str(n) for n in g["names"]], [str(c) for c in g["classes"]]
    idx = {n: i for i, n in enumerate(names)}
    assert len(idx) == len(names), "stream names repeat"
    ok = g["status"] == OK
    rej = [i for i, c in enumerate(classes) if c == "rejected"]
    assert all(ok[i] == (classes[i] != "rejected") for i in range(len(names)))
    assert len(rej) >= 5 and min(rej) > 5 and max(rej) < len(names) - 5 and np.diff(rej).min() > 1, \
        "rejected ones not interleaved"
    tiny = [i for i, c in enumerate(classes) if c == "tiny"]
    assert len(tiny) == 15
    for i in tiny:                                           # 32 bits per MCU, plus the first DC values: 128-bit chunks
        assert 256 <= g["ncompact"][i] <= 264 and g["nchunks"][i] in (16, 17) and 384 / g["nchunks"][i] >= 20, names[i]
    assert any(g["ncompact"][i] == 256 and g["nchunks"][i] == 16 for i in tiny)
    for n in (4096, 4097, LDS, LDS + 1):
        assert g["ncompact"][idx["unstuffed_%d" % n]] == n
    assert g["nchunks"][idx["unstuffed_4096"]] == 256 and g["nchunks"][idx["unstuffed_4097"]] < 256
    i = idx["short_not_flat_q30"]
    assert 256 < g["ncompact"][i] < 1024 and g["nchunks"][i] < 256
    assert LDS - 4 < g["ncompact"][idx["unstuffed_%d" % (LDS - 2)]] < LDS
    assert g["ncompact"][idx["noise_q100_above_32000"]] > 32000
    rounds = g["rounds"]
    assert (rounds >= 200).sum() >= 3 and (rounds > 100).sum() >= 10, sorted(rounds.tolist())[-12:]
    assert (rounds[ok] <= g["nchunks"][ok] + 1).all() and (rounds[ok] >= 1).all()
    assert g["max_dc_cat"][idx["checker8_q100"]] == 11
    assert any(g["zrl"][idx["stripes_q%d" % q]] > 0 for q in (5, 25, 60, 100)) and g["max_abs"].max() >= 1024
    assert g["no_eob"][idx["noise_q100_no_eob"]] >= 300
    longc = [i for i, n in enumerate(names) if n.startswith("long_codes_")]
    assert len(longc) >= 3 and all(g["slow"][i] > 0 for i in longc)
    assert sum(c == "colour" for c in classes) == 25 and sum(c == "sync" for c in classes) == 84
    assert sum(c == "header" for c in classes) == 10
