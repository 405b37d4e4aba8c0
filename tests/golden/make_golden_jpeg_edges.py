#!/usr/bin/env python3
"""Edge corpus for the device JPEG decoder (ndp_jpeg_decode_u8): the streams at which the
decoder takes another path than on tests/golden/jpeg_case.npz.

Every stream is written by PIL on libjpeg-turbo (asserted), 128x128, 4:2:0; some then have bytes edited by hand, and for
those PIL must still decode the stream, to the bytes asserted here.  Each class's property is asserted with the report of
the host driver of the decoder's core (tests/host_drivers/jpeg.inc, run by tests/jpeg_core_host.py), so the coverage is
proven, not assumed.

Stored (tests/golden/jpeg_edges.npz):
  streams [bytes] uint8, offsets [n+1] int64   every stream, back to back
  names [n] str, classes [n] str                what each stream is, and the class below it belongs to
  status [n] int32                              the expected NDP_JPEG_* status (include/ndp.h)
  digest [n,16] uint8                           blake2b (16 bytes) of PIL's 128x128x3 bytes; zeros for a rejected stream
  mcu_sums [n,8,8,3] uint32                     PIL's byte sums per 16x16 MCU and channel: a failing test names the MCUs
  rounds, nchunks, ncompact, max_dc_cat, zrl, no_eob, slow, max_abs [n] int32
                                                the host driver's report: sync rounds, chunks, unstuffed bytes, and the
                                                census (largest DC category, ZRL symbols, blocks without EOB, symbols with
                                                a code longer than 9 bits, largest |coefficient|)
No decoded frames are stored.

Classes: tiny (flat frames: 256 unstuffed bytes and 16 chunks, or a few bytes and one chunk more), geometry (unstuffed
length exactly 4,096 and 4,097, where the chunks grow from 128 to 160 bits; a short stream that is not flat),
lds (exactly 24,576 and 24,577 unstuffed bytes, the two sides of the LDS split; one within a word below; one above 32,000), sync (a 16x16 random tile repeated, and
uniform noise of amplitude 1 .. 128 around grey, plain and optimize=True: the streams that need the most sync rounds),
symbols (DC category 11, ZRL runs and ringing, blocks without EOB, long Huffman codes), colour (the scenes of
make_golden_jpeg.py at qualities 3, 15 and 88; chroma that changes every 2x2 pixels up to the borders), header (16-bit
DQT + SOF1, ICC profiles that push SOS past the 2 KB staged in LDS, a long COM, fill bytes, DRI 0, merged DHT / DQT),
rejected (4:4:4, progressive, restart markers, a long stream truncated in its far part, SOS followed by EOI).

Usage: python tests/golden/make_golden_jpeg_edges.py   (compiles the host driver first: about a minute)
"""
import os
import sys
import tempfile

import numpy as np
from PIL import features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_core_host as H                                   # noqa: E402
from jpeg_core_host import LDS, OK, segments                 # noqa: E402
from make_golden_jpeg import encode, pil_decode, scene       # noqa: E402

UNSUPPORTED, SIZE, CORRUPT = 1, 2, 3
MAX_FILE = 2_000_000


def unstuffed_len(data):
    """Bytes of entropy data after unstuffing (the search below steers by it; the driver's report is what is asserted)."""
    e0 = segments(data)[-1][2]
    body = data[e0:]
    end = len(body)
    p = body.find(b"\xff")
    while p >= 0:
        if p + 1 >= len(body) or body[p + 1] != 0:
            end = p
            break
        p = body.find(b"\xff", p + 2)
    return end - body[:end].count(b"\xff\x00")


def noise(seed, amp=128):
    rng = np.random.RandomState(seed)
    return np.clip(128 + rng.randint(-amp, amp + 1, (128, 128, 3)), 0, 255).astype(np.uint8)


def hit_length(target, seed, quality=100):
    """A frame whose stream at `quality` has exactly `target` unstuffed bytes: from noise, blank 8x8 blocks while the
    stream is too long (or re-randomise blanked ones while it is too short), then change single pixels, keeping every
    change that does not move the length away from the target."""
    rng = np.random.RandomState(seed)
    img = noise(seed)
    length = unstuffed_len(encode(img, quality=quality))
    assert length > target, (length, target)
    order = rng.permutation(256)
    encodes = 1
    for b in order:
        if length <= target + 150:
            break
        y, x = 8 * (b // 16), 8 * (b % 16)
        img[y:y + 8, x:x + 8] = 128
        length = unstuffed_len(encode(img, quality=quality))
        encodes += 1
    for _ in range(20000):
        if length == target:
            return img, encodes
        y, x, c = rng.randint(0, 128), rng.randint(0, 128), rng.randint(0, 3)
        old = img[y, x, c]
        img[y, x, c] = rng.randint(0, 256)
        new = unstuffed_len(encode(img, quality=quality))
        encodes += 1
        if abs(new - target) <= abs(length - target):
            length = new
        else:
            img[y, x, c] = old
    raise AssertionError("the search missed %d unstuffed bytes (at %d after %d encodes)" % (target, length, encodes))


def insert_before(data, marker, extra, which=0):
    """`extra` inserted before the `which`-th segment with `marker`."""
    segs = [s for s in segments(data) if s[0] == marker]
    p = segs[which][1]
    return data[:p] + extra + data[p:]


def merged(data, marker):
    """The segments with `marker` merged into one at the place of the first."""
    segs = [s for s in segments(data) if s[0] == marker]
    assert len(segs) >= 2, "PIL wrote one segment only"
    body = b"".join(data[a + 4:b] for _, a, b in segs)
    out, p = b"", 0
    for i, (_, a, b) in enumerate(segs):
        out += data[p:a]
        if i == 0:
            out += bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
        p = b
    return out + data[p:]


def same_as(edited, original):
    """PIL must decode the edited stream to the original's bytes."""
    assert np.array_equal(pil_decode(edited), pil_decode(original)), "an edit changed what PIL decodes"
    return edited


def max_code_length(data):
    longest = 0
    for m, a, b in segments(data):
        if m == 0xC4:
            q = a + 4
            while q < b:
                counts = data[q + 1:q + 17]
                longest = max(longest, max(l + 1 for l in range(16) if counts[l]))
                q += 17 + sum(counts)
    return longest


def cases():
    """[(name, class, stream, expected status)]."""
    out = []
    # tiny: flat frames
    flats = {"black": (0, 0, 0), "white": (255, 255, 255), "grey128": (128, 128, 128), "red": (255, 0, 0),
             "teal": (23, 141, 97)}
    for name, rgb in flats.items():
        for q in (1, 50, 100):
            img = np.zeros((128, 128, 3), np.uint8) + np.array(rgb, np.uint8)
            out.append(("flat_%s_q%d" % (name, q), "tiny", encode(img, quality=q), OK))
    # chunk geometry
    for target in (4096, 4097):
        img, _ = hit_length(target, seed=target)
        out.append(("unstuffed_%d" % target, "geometry", encode(img, quality=100), OK))
    small = np.zeros((128, 128, 3), np.uint8) + 90
    small[40:72, 24:88] = noise(3)[40:72, 24:88]
    out.append(("short_not_flat_q30", "geometry", encode(small, quality=30), OK))
    # LDS split
    for target in (LDS, LDS + 1, LDS - 2):
        img, _ = hit_length(target, seed=target)
        out.append(("unstuffed_%d" % target, "lds", encode(img, quality=100), OK))
    long_stream = encode(noise(99, 128), quality=100)
    out.append(("noise_q100_above_32000", "lds", long_stream, OK))
    # sync adversaries
    tile = np.random.RandomState(16).randint(0, 256, (16, 16, 3)).astype(np.uint8)
    tiled = np.tile(tile, (8, 8, 1))
    for q in (20, 50, 95, 100):
        out.append(("tile16_q%d" % q, "sync", encode(tiled, quality=q), OK))
    for amp in (1, 2, 4, 8, 16, 32, 64, 128):
        for q in (5, 30, 75, 95, 100):
            img = noise(1000 + amp, amp)
            out.append(("noise_amp%d_q%d" % (amp, q), "sync", encode(img, quality=q), OK))
            out.append(("noise_amp%d_q%d_optimize" % (amp, q), "sync", encode(img, quality=q, optimize=True), OK))
    # symbol extremes
    yy, xx = np.mgrid[0:128, 0:128]
    checker = ((((yy // 8) + (xx // 8)) % 2) * 255).astype(np.uint8)[..., None].repeat(3, axis=2)
    out.append(("checker8_q100", "symbols", encode(checker, quality=100), OK))
    stripes = np.zeros((128, 128, 3), np.uint8)
    pal = np.array([[255, 0, 0], [0, 255, 255], [0, 255, 0], [255, 0, 255], [0, 0, 255], [255, 255, 0]], np.uint8)
    stripes[:, :] = pal[(2 * ((xx // 32) % 3) + xx % 2)]
    for q in (5, 25, 60, 100):
        out.append(("stripes_q%d" % q, "symbols", encode(stripes, quality=q), OK))
    out.append(("noise_q100_no_eob", "symbols", encode(noise(7, 128), quality=100), OK))
    for name, img, q in (("scene3", scene(3), 95), ("noise_amp128", noise(8, 128), 90), ("scene7", scene(7), 95)):
        out.append(("long_codes_%s_q%d_optimize" % (name, q), "symbols", encode(img, quality=q, optimize=True), OK))
    # colour and upsampling edges
    for q in (3, 15, 88):
        for i in range(8):
            out.append(("scene%d_q%d" % (i, q), "colour", encode(scene(i), quality=q), OK))
    rng = np.random.RandomState(22)
    chroma = np.repeat(np.repeat(rng.randint(0, 256, (64, 64, 3)), 2, axis=0), 2, axis=1).astype(np.uint8)
    out.append(("chroma_2x2_q95", "colour", encode(chroma, quality=95), OK))
    # header variants
    base_img = scene(2)
    base = encode(base_img, quality=75)
    qt = [[min(1000, 8 + 40 * (i // 8 + i % 8) + (300 if i in (10, 27, 63) else 0)) for i in range(64)],
          [min(2000, 16 + 60 * (i // 8 + i % 8)) for i in range(64)]]
    wide = encode(base_img, qtables=qt)
    segs = segments(wide)
    assert any(m == 0xC1 for m, _, _ in segs) and any(m == 0xDB and wide[a + 4] >> 4 == 1 for m, a, _ in segs), \
        "PIL did not write 16-bit tables and SOF1"
    out.append(("dqt16_sof1", "header", wide, OK))
    icc = bytes(np.random.RandomState(5).randint(0, 256, 5000).astype(np.uint8))
    straddle = None
    for n in range(1000, 2200):
        s = encode(base_img, quality=75, icc_profile=icc[:n])
        if any(m == 0xC4 and a < 2048 < b - 1 for m, a, b in segments(s)):
            straddle = n
            break
    assert straddle is not None, "no ICC size puts a DHT segment across byte 2,048"
    for n in (1000, straddle, 3000, 5000):
        s = encode(base_img, quality=75, icc_profile=icc[:n])
        assert (segments(s)[-1][1] > 2048) == (n >= straddle)
        out.append(("icc_%d%s" % (n, "_dht_across_2048" if n == straddle else ""), "header", same_as(s, base), OK))
    com = encode(base_img, quality=75, comment=b"c" * 3000)
    assert any(m == 0xFE and b - a >= 3000 for m, a, b in segments(com)), "PIL wrote no COM segment"
    out.append(("com_3000", "header", same_as(com, base), OK))
    fill = insert_before(insert_before(insert_before(base, 0xDA, b"\xff" * 3), 0xC4, b"\xff" * 2, which=1), 0xDB, b"\xff")
    out.append(("fill_bytes_before_dqt_dht_sos", "header", same_as(fill, base), OK))
    out.append(("dri_0_before_sos", "header", same_as(insert_before(base, 0xDA, b"\xff\xdd\x00\x04\x00\x00"), base), OK))
    out.append(("dht_merged", "header", same_as(merged(base, 0xC4), base), OK))
    out.append(("dqt_merged", "header", same_as(merged(base, 0xDB), base), OK))
    # rejected
    e0 = segments(long_stream)[-1][2]
    cut = long_stream[:e0 + 28000]
    if cut.endswith(b"\xff"):
        cut = cut[:-1]
    rejected = [("scene2_444", encode(base_img, quality=95, subsampling=0), UNSUPPORTED),
                ("scene2_progressive", encode(base_img, quality=95, progressive=True), UNSUPPORTED),
                ("scene2_restart", encode(base_img, quality=95, restart_marker_blocks=4), UNSUPPORTED),
                ("noise_q100_truncated_in_far_part", cut, CORRUPT),
                ("noise_q100_truncated_in_far_part_then_eoi", cut + b"\xff\xd9", CORRUPT),
                ("sos_then_eoi", base[:segments(base)[-1][2]] + b"\xff\xd9", CORRUPT)]
    # interleaved with the rest
    step = len(out) // (len(rejected) + 1)
    for j, (name, data, st) in enumerate(rejected):
        out.insert((j + 1) * step + j, (name, "rejected", data, st))
    return out


def main():
    assert features.check_feature("libjpeg_turbo"), "the oracle is PIL on libjpeg-turbo (IJG libjpeg upsamples differently)"
    rows = cases()
    for name, cls, data, st in rows:
        if name.startswith("long_codes_"):
            assert max_code_length(data) >= 10, (name, max_code_length(data))
    streams = [r[2] for r in rows]
    with tempfile.TemporaryDirectory() as tmp:
        exe = H.build_driver(tmp)
        rec, chunked, serial = H.run_driver(exe, streams, tmp, frames=True)
    n = len(rows)
    digests, sums = np.zeros((n, 16), np.uint8), np.zeros((n, 8, 8, 3), np.uint32)
    for i, (name, cls, data, st) in enumerate(rows):
        assert rec["status"][i] == st and rec["status_serial"][i] == st, (name, rec["status"][i], rec["status_serial"][i], st)
        if st == OK:
            want = pil_decode(data)
            assert np.array_equal(chunked[i], want) and np.array_equal(serial[i], want), name + ": the host decode is not PIL's"
            digests[i], sums[i] = H.digest(want), H.mcu_sums(want)
        else:
            assert not chunked[i].any() and not serial[i].any(), name
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([len(s) for s in streams])
    g = dict(streams=np.frombuffer(b"".join(streams), np.uint8), offsets=offsets, names=np.array([r[0] for r in rows]),
             classes=np.array([r[1] for r in rows]), status=np.array([r[3] for r in rows], np.int32), digest=digests,
             mcu_sums=sums)
    for k in H.CENSUS:
        g[k] = rec[k].astype(np.int32)
    H.check_edge_classes(g)
    path = os.path.join(HERE, "jpeg_edges.npz")
    np.savez_compressed(path, **g)
    size = os.path.getsize(path)
    assert size <= MAX_FILE, size
    r = np.sort(g["rounds"][g["status"] == OK])
    top = np.argsort(-g["rounds"])[:6]
    print("wrote %s: %d streams (%d decodable), %d bytes" % (path, n, int((g["status"] == OK).sum()), size))
    print("sync rounds: median %d, maximum %d; most: %s" % (r[len(r) // 2], r[-1], ", ".join(
        "%s %d of %d chunks" % (g["names"][i], g["rounds"][i], g["nchunks"][i]) for i in top)))


if __name__ == "__main__":
    main()
