"""The JPEG decoder's core (csrc/ndp_jpeg.inc) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer (signed
overflow included).  tests/host_drivers/jpeg.inc follows the library's source in main.hip and calls the __host__ __device__ functions
the kernels call; it decodes every stream twice, by k_jpeg_entropy's schedule of chunks and sync rounds run serially and by
one lane from bit 0, and the two must agree for every stream, valid or not (every chunk's entry is
exact by induction).  The streams: the edge corpus tests/golden/jpeg_edges.npz (made by
tests/golden/make_golden_jpeg_edges.py), where both decodes must give PIL's bytes, and seeded mutations of it, where the
decoder must stay inside its buffers.  The sanitizers are on the host half of the stand-alone driver only; it runs as an
ordinary child process.  No GPU involved (the same corpus on the GPU: tests/test_gpu_jpeg_edges.py).  About a minute, most
of it the one compilation."""
import io

import numpy as np
import pytest

import host_driver
import jpeg_core_host as H
from conftest import load_golden

N_MUTATIONS = 3200


@pytest.fixture(scope="module")
def driver():
    try:
        return host_driver.build()
    except host_driver.NoSanitizerRuntime as e:
        pytest.skip("this toolchain cannot link the sanitizers' runtimes: " + str(e)[-300:])


@pytest.fixture(scope="module")
def corpus():
    g = load_golden("jpeg_edges")
    o = g["offsets"]
    g["list"] = [g["streams"][o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]
    return g


@pytest.fixture(scope="module")
def report(driver, corpus, tmp_path_factory):
    return H.run_driver(driver, corpus["list"], tmp_path_factory.mktemp("jpeg_corpus"), frames=True)


def test_both_host_decodes_of_every_corpus_stream_are_pil_s_bytes(corpus, report):
    rec, chunked, serial = report
    g = corpus
    for i, name in enumerate(g["names"]):
        where = "%s (%s, %d rounds)" % (name, g["classes"][i], g["rounds"][i])
        assert rec["status"][i] == g["status"][i] and rec["status_serial"][i] == g["status"][i], \
            (where, int(rec["status"][i]), int(rec["status_serial"][i]), int(g["status"][i]))
        assert np.array_equal(chunked[i], serial[i]), where + ": chunked and serial differ, " + \
            H.differing_mcus(chunked[i], H.mcu_sums(serial[i]))
        if g["status"][i] == 0:
            for kind, frame in (("chunked", chunked[i]), ("serial", serial[i])):
                assert np.array_equal(H.mcu_sums(frame), g["mcu_sums"][i]) and np.array_equal(H.digest(frame), g["digest"][i]), \
                    "%s, %s: %s" % (where, kind, H.differing_mcus(frame, g["mcu_sums"][i]))
        else:
            assert not chunked[i].any() and not g["digest"][i].any()


def test_the_committed_corpus_meets_its_class_conditions_and_the_driver_s_report_is_the_stored_one(corpus, report):
    rec = report[0]
    H.check_edge_classes(corpus)
    assert corpus["streams"].size == corpus["offsets"][-1] and len(corpus["list"]) == len(corpus["names"]) >= 150
    for k in H.CENSUS:
        assert rec[k].tolist() == corpus[k].tolist(), k


def test_corpus_digests_agree_with_this_machine_s_pil(corpus):
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this PIL is not built on libjpeg-turbo")
    for i, s in enumerate(corpus["list"]):
        if corpus["status"][i] == 0:
            frame = np.array(Image.open(io.BytesIO(s)))
            assert np.array_equal(H.digest(frame), corpus["digest"][i]), corpus["names"][i]
            assert np.array_equal(H.mcu_sums(frame), corpus["mcu_sums"][i]), corpus["names"][i]


def _set_length(s, seg, rng):
    """A segment length raised or lowered, a little or a lot."""
    at = seg[3]
    old = int.from_bytes(s[at:at + 2], "big")
    new = old + int(rng.choice([-300, -17, -2, -1, 1, 2, 17, 300, 30000])) if rng.randint(0, 4) else int(rng.randint(0, 65536))
    s[at:at + 2] = int(min(65535, max(0, new))).to_bytes(2, "big")


def mutations(corpus, count, seed=2024):
    """`count` seeded mutations of corpus streams, as (kind, bytes): byte flips anywhere (the headers included),
    truncations, segment lengths raised and lowered, DHT counts, SOF and SOS fields, and the ICC streams cut around the
    2 KB staged in LDS."""
    rng = np.random.RandomState(seed)
    names = [str(n) for n in corpus["names"]]
    ok = [i for i in range(len(names)) if corpus["status"][i] == 0]
    # mostly the short streams (the mutations are about the parser and the symbol loop, not about length), some of all
    short = [i for i in ok if corpus["ncompact"][i] <= 6000]
    out = []
    for name in names:
        if name.startswith("icc_"):
            s = corpus["list"][names.index(name)]
            for cut in (2047, 2048, 2049):
                out.append(("icc_cut", s[:cut]))
                out.append(("icc_cut_eoi", s[:cut] + b"\xff\xd9"))
    kinds = ("flip", "flip_header", "flip_entropy", "truncate", "length", "dht_counts", "sof_sos")
    while len(out) < count:
        kind = kinds[len(out) % len(kinds)]
        i = int(rng.choice(short if rng.randint(0, 8) else ok))
        s = bytearray(corpus["list"][i])
        # (marker, start, end, offset of the length field), fill bytes skipped
        segs = []
        for m, a, b in H.segments(bytes(s)):
            q = a
            while s[q + 1] == 0xFF:
                q += 1
            segs.append((m, a, b, q + 2))
        e0 = segs[-1][2]
        if kind == "flip":
            for _ in range(rng.randint(1, 5)):
                s[rng.randint(0, len(s))] ^= 1 << rng.randint(0, 8)
        elif kind == "flip_header":
            for _ in range(rng.randint(1, 4)):
                s[rng.randint(2, e0)] = rng.randint(0, 256)
        elif kind == "flip_entropy":
            for _ in range(rng.randint(1, 6)):
                s[rng.randint(e0, len(s))] ^= 1 << rng.randint(0, 8)
        elif kind == "truncate":
            s = s[:rng.randint(0, len(s))]
            if rng.randint(0, 2):
                s += b"\xff\xd9"
        elif kind == "length":
            _set_length(s, segs[rng.randint(0, len(segs))], rng)
        elif kind == "dht_counts":
            dht = [g for g in segs if g[0] == 0xC4]
            g = dht[rng.randint(0, len(dht))]
            at = g[3] + 2 + 1 + rng.randint(0, 16)           # a count of the segment's first table
            if rng.randint(0, 2):                            # a code moved to another length: the table stays as long
                to = g[3] + 2 + 1 + rng.randint(0, 16)
                if s[at] > 0 and s[to] < 255:
                    s[at] -= 1
                    s[to] += 1
            else:
                s[at] = (s[at] + int(rng.choice([-2, -1, 1, 2, 7, 100, 255]))) % 256
            if rng.randint(0, 4) == 0:
                s[g[3] + 2] = rng.randint(0, 256)           # the table's class and id
        else:
            sel = [g for g in segs if g[0] in (0xC0, 0xC1, 0xDA)]
            g = sel[rng.randint(0, len(sel))]
            at = rng.randint(g[3] + 2, g[2])
            s[at] = rng.randint(0, 256) if rng.randint(0, 2) else (s[at] ^ (1 << rng.randint(0, 8)))
        out.append((kind, bytes(s)))
    return out


def test_hostile_streams_stay_in_bounds_and_chunked_equals_serial(driver, corpus, tmp_path):
    muts = mutations(corpus, N_MUTATIONS)
    assert len(muts) >= 3000
    rec, _, _ = H.run_driver(driver, [m[1] for m in muts], tmp_path)      # asserts: exit 0, no sanitizer report
    st = rec["status"]
    assert np.isin(st, (0, 1, 2, 3)).all(), sorted(set(st.tolist()))
    bad = np.flatnonzero((rec["status_serial"] != st) | (rec["frames_equal"] != 1))
    assert bad.size == 0, [(int(i), muts[i][0], int(st[i]), int(rec["status_serial"][i])) for i in bad[:10]]
    # the mutations reach every outcome, and the entropy stage of streams that are then rejected
    per_kind = {k: st[[j for j, m in enumerate(muts) if m[0] == k]] for k in sorted({m[0] for m in muts})}
    assert all(len(v) >= 6 for v in per_kind.values())
    assert (st == 0).sum() >= 100 and (st == 1).sum() >= 20 and (st == 2).sum() >= 5 and (st == 3).sum() >= 1000
    assert ((st == 3) & (rec["rounds"] > 0)).sum() >= 100
    print("hostile streams: %d, by status %s, accepted %d" % (len(muts), np.bincount(st, minlength=4).tolist(), (st == 0).sum()))
