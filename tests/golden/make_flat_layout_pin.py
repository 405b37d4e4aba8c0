#!/usr/bin/env python3
"""Pin of everything the host side of the forward model and of the image autoencoder computes about their flat
vectors and workspaces (include/ndp.h): sizes, ndp_*_layout for every valid query, workspace sizes and tensor offsets,
and the gradient buckets.  Every call is host-only, so this needs the built library and no GPU.

The file was written once, from the commit BEFORE the two networks' host helpers were merged into one set driven by
a network table; tests/test_forward_model_layout.py compares the built library against it.  Regenerate it only when a
layout is meant to change.

Usage: python tests/golden/make_flat_layout_pin.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

WORKSPACE_N = (1, 3, 16, 65, 240, 8192)
OFFSET_N = (1, 3, 65)
# family -> (layers, BatchNorms): the valid indices of ndp_*_layout(what, index)
FAMILIES = {"fm": (14, 10), "ae": (12, 8)}


def family(lib, tag, buckets):
    layers, bns = FAMILIES[tag]
    fn = lambda name: getattr(lib, "ndp_%s_%s" % (tag, name))
    out = {"param_floats": fn("param_floats")(), "stat_floats": fn("stat_floats")(), "layout": {}}
    off, dims = ctypes.c_int64(), (ctypes.c_int64 * 6)()
    for what in range(6):
        for i in range(layers if what < 2 else bns):
            assert fn("layout")(what, i, ctypes.byref(off), dims) == 0
            out["layout"]["%d,%d" % (what, i)] = [off.value] + list(dims)
    out["workspace_floats"] = {str(n): fn("workspace_floats")(n) for n in WORKSPACE_N}
    out["workspace_offset"] = {}
    for n in OFFSET_N:
        offs, t = [], 0
        while fn("workspace_offset")(n, t) >= 0:                       # -1 past the last tensor
            offs.append(fn("workspace_offset")(n, t))
            t += 1
        out["workspace_offset"][str(n)] = offs
    out["buckets"] = [list(b) for b in buckets]
    return out


def collect():
    """The pin's content from the built library (also what the test compares the file with)."""
    from ndivplanning_amd import _build, _capi
    _build.build()
    lib = _capi.load()
    pin = {"fm": family(lib, "fm", _capi.fm_grad_buckets()), "ae": family(lib, "ae", _capi.ae_grad_buckets())}
    pin["ae"]["workspace_floats"]["8193"] = lib.ndp_ae_workspace_floats(8193)
    return pin


if __name__ == "__main__":
    path = os.path.join(HERE, "flat_layout_pin.json")
    with open(path, "w") as f:
        json.dump(collect(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(path)
