"""The launch arguments the host derives from the network tables (csrc/ndp_forward_model.inc: fm_geom, fm_layer_views and
the per-network FmMaps) against the recorded ones, before anything runs on a GPU: a wrong size, stride or tensor offset
in a layer launch is an out-of-bounds gather, not a failing result.  tests/host_drivers/fm_geometry.inc reports, for every
layer of the forward model, the autoencoder and its folded decoder and every direction that network launches, what the
layer helpers hand to fm_gemm, fm_deconv32 and fm_wgrad; tests/golden/fm_layer_geometry.json holds the same tuples as
the hand-written call sites stated them before the launches were derived from the tables (transcribed from those
argument lists, one row per call site and batch size: 15 and 16 images where k_fm_deconv32 may take over).  Host
arithmetic only; the program is host_driver's, an ordinary child process under AddressSanitizer and UBSan."""
import json
import os
import struct

import pytest

import host_driver

HERE = os.path.dirname(os.path.abspath(__file__))
NETS = {"fm": 0, "ae": 1, "aed": 2}
DIRS = {"fwd": 0, "dgrad": 1, "wgrad": 2}
KERNELS = {"gemm": 0, "deconv32": 1, "wgrad": 2}
# the workspace tensors in the order of FmTensor / AeTensor / AeDecTensor
TENSORS = {
    "fm": ("COLS CAT6 CAT5 CAT4 CAT3 CAT2 Z RAW1 RAW2 RAW3 RAWU1 RAWU2 RAWU3 RAWU4 RAWU5 RAWU6 UP6 RAWR1 R1 Y2 "
           "DCAT6 DCAT5 DCAT4 DCAT3 DCAT2 DZ DUP6 DR1").split(),
    "ae": ("COLS RAW1 A1 RAW2 A2 RAW3 A3 A4 A5 Z RAWU1 U1 RAWU2 U2 RAWU3 U3 RAWU4 U4 RAWU5 U5 G6 "
           "DU5 DU4 DU3 DU2 DU1 DZ DA5 DA4 DA3 DA2 DA1").split(),
    "aed": "U1 U2 U3 U4 U5".split(),
}
LAYERS = {"fm": 14, "ae": 12, "aed": 6}
BN_LAYERS = {"fm": {0, 1, 2, 6, 7, 8, 9, 10, 11, 12}, "ae": {0, 1, 2, 6, 7, 8, 9, 10}, "aed": set()}
FIELDS = 21


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "fm_layer_geometry.json")) as f:
        doc = json.load(f)
    return [dict(zip(doc["fields"], row)) for row in doc["rows"]]


@pytest.fixture(scope="module")
def report(golden, tmp_path_factory):
    payload = struct.pack("<i", len(golden))
    for r in golden:
        payload += struct.pack("<4i", NETS[r["net"]], r["layer"], DIRS[r["dir"]], r["n"])
    raw = host_driver.run("fm_geometry", payload, tmp_path_factory.mktemp("fm_geometry"), exe=host_driver.build())
    rows, at = [], 0
    for _ in golden:
        rows.append((struct.unpack_from("<%di" % FIELDS, raw, at), raw[at + 4 * FIELDS:at + 4 * FIELDS + 32].rstrip(b"\0").decode()))
        at += 4 * FIELDS + 32
    maps = {}
    for net in ("fm", "ae", "aed"):
        (layers,) = struct.unpack_from("<i", raw, at)
        at += 4
        assert layers == LAYERS[net]
        maps[net] = [struct.unpack_from("<12i", raw, at + 48 * l) for l in range(layers)]
        at += 48 * layers
    assert at == len(raw)
    return rows, maps


def view(net, v):
    """(tensor index, offset, stride) as the driver names the fixture's [tensor name, channel offset, stride]"""
    return (-2 if v[0] == "codes" else TENSORS[net].index(v[0]), v[1], v[2])


def test_the_fixture_covers_every_launch_of_every_network(golden):
    seen = {(r["net"], r["dir"], r["layer"]) for r in golden}
    want = set()
    want |= {("fm", "fwd", l) for l in range(12)} | {("fm", "dgrad", l) for l in range(1, 12)} | {("fm", "wgrad", l) for l in range(13)}
    want |= {("ae", "fwd", l) for l in range(11)} | {("ae", "dgrad", l) for l in range(1, 11)} | {("ae", "wgrad", l) for l in range(11)}
    want |= {("aed", "fwd", l) for l in range(5)}
    assert seen == want
    # both sides of the k_fm_deconv32 threshold for every stride-2 transposed convolution's forward launch
    for net, layers in (("fm", range(7, 12)), ("ae", range(7, 11)), ("aed", range(1, 5))):
        for l in layers:
            assert {r["n"] for r in golden if (r["net"], r["dir"], r["layer"]) == (net, "fwd", l)} == {15, 16}
    assert len(golden) == 86
    assert len({r["label"] for r in golden}) == len(seen)              # one label per launch, none shared


def test_every_launch_gets_the_recorded_arguments(golden, report):
    rows, _ = report
    names = ["kernel", "mode", "SH", "ss", "OH", "GH", "C", "N", "KH", "pad", "p2", "DH", "J", "columns"]
    for want, (got, label) in zip(golden, rows):
        where = (want["net"], want["dir"], want["layer"], want["n"])
        assert label == want["label"], where
        g = dict(zip(names, got))
        assert g["kernel"] == KERNELS[want["kernel"]], where
        assert g["p2"] == (want["weights"] == "P2"), where
        for k in ("mode", "SH", "ss", "OH", "GH", "C", "N", "KH", "pad", "DH", "J", "columns"):
            if want[k] is not None:                                    # (null: the call site has no such argument)
                assert g[k] == want[k], (where, k, g[k], want[k])
        assert tuple(got[15:18]) == view(want["net"], want["a"]), (where, "first map")
        assert tuple(got[18:21]) == view(want["net"], want["b"]), (where, "second map")


def test_each_layers_output_is_the_next_layers_input(golden, report):
    rows, maps = report
    for net in ("fm", "ae", "aed"):
        for l, v in enumerate(maps[net]):
            inp, raw, din, nxt = v[0:3], v[3:6], v[6:9], v[9:12]
            if l + 1 < LAYERS[net]:
                assert nxt == maps[net][l + 1][0:3], (net, l)          # in[l + 1] is one view, seen from both layers
                assert nxt[0] != -1, (net, l)
            if l in BN_LAYERS[net]:
                assert raw[0] != -1 and raw[:2] != nxt[:2], (net, l)   # BatchNorm reads the raw map, writes the next input
            else:
                assert raw == nxt, (net, l)                            # no BatchNorm: the launch writes the next input
            if din[0] != -1:
                assert din[2] == inp[2], (net, l)                      # a gradient map has its map's stride
    # the BatchNorm index the helpers use for a layer, and the forward launches' destination: the raw map
    for want, (got, _) in zip(golden, rows):
        bn = sorted(BN_LAYERS[want["net"]])
        assert got[14] == (bn.index(want["layer"]) if want["layer"] in bn else -1)
        if want["dir"] == "fwd":
            assert tuple(got[18:21]) == maps[want["net"]][want["layer"]][3:6]


def test_the_driver_refuses_a_launch_the_network_does_not_have(tmp_path):
    for net, layer, direction in ((0, 13, 0), (0, 0, 1), (1, 11, 2), (2, 5, 0), (0, 14, 0)):
        payload = struct.pack("<5i", 1, net, layer, direction, 16)
        host_driver.run("fm_geometry", payload, tmp_path, timeout=300, exe=host_driver.build(), expect=2)
