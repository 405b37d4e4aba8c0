"""CPU: the flat parameter vector of the forward-model kernels (include/ndp.h, ndp_fm_layout) against the module's own
tensors -- packing and unpacking are inverse, padded entries are zero, every float of the vector belongs to exactly one
tensor -- the pin of both networks' host-side numbers (tests/golden/flat_layout_pin.json), and the host-side refusals
that need no GPU."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

from ndivplanning_amd import _capi
from ndivplanning_amd.models import forward_encoder as FE
from oracle import forward_model_oracle as FO


@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build
    _build.build()
    return _capi.load()


def test_layout_tiles_the_vector_and_round_trips(lib):
    total = lib.ndp_fm_param_floats()
    spans = []
    for what, count in ((0, 14), (1, 14), (2, 10), (3, 10)):
        for i in range(count):
            off, d = FE._layout(lib, what, i)
            spans.append((off, off + d[0] * d[1] * d[2]))
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))          # back to back, no overlap
    assert all(s[0] % 4 == 0 for s in spans)                             # float4 loads
    state = FO.init_forward_model_state(1)
    model = FE.ForwardAutoencoder()
    model.load_state_dict(state)
    with torch.no_grad():                                                # make every tensor distinguishable
        for i, bn in enumerate(FE.BN_NAMES):
            FE._module_tensor(model, bn).weight.add_(0.01 * i)
            FE._module_tensor(model, bn).running_var.add_(0.1 * i)
    params, stats = FE.pack_module(model, "cpu")
    back = FE.unpack_vector(params, model)
    sd = model.state_dict()
    assert sorted(back) == sorted(k for k in sd if "running_" not in k and "num_batches" not in k
                                  and not k.startswith(("encoder.conv4_bn", "encoder.conv5_bn")))
    assert all(torch.equal(v, sd[k]) for k, v in back.items())
    # the real entries account for every non-zero of the vector: the padding is zero
    assert int((params != 0).sum()) == sum(int((v != 0).sum()) for v in back.values())
    # reference layouts: Conv2d [co][ci][kh][kw] -> [co][kh][kw][ci pad], ConvTranspose2d [ci][co][kh][kw] -> [ci pad][kh][kw][co]
    off, d = FE._layout(lib, 0, 0)
    assert d[:3] == [64, 9, 32] and params[off + (5 * 9 + 3 * 1 + 2) * 32 + 1] == sd["encoder.conv1.weight"][5, 1, 1, 2]
    off, d = FE._layout(lib, 0, 6)
    assert d[:3] == [160, 16, 1024] and params[off + (7 * 16 + 4 * 2 + 3) * 1024 + 9] == sd["decoder.deconv1.weight"][7, 9, 2, 3]
    clone = FE.ForwardAutoencoder()
    FE.unpack_into_module(clone, params, stats, batches_tracked=3)
    assert torch.equal(clone.decoder.deconv6.weight, model.decoder.deconv6.weight)
    assert torch.equal(clone.decoder.conv_refine_1_bn.running_var, model.decoder.conv_refine_1_bn.running_var)
    assert int(clone.encoder.conv2_bn.num_batches_tracked) == 3


def test_sizes_layouts_workspaces_and_buckets_are_the_pinned_ones(lib):
    """Every number the host side derives from the two network tables -- vector sizes, ndp_*_layout of every valid query,
    workspace sizes and tensor offsets, gradient buckets -- against the file written before the two networks' host code
    was merged (tests/golden/make_flat_layout_pin.py): entry by entry."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "flat_layout_pin.json")) as f:
        pin = json.load(f)
    spec = importlib.util.spec_from_file_location("make_flat_layout_pin", os.path.join(golden, "make_flat_layout_pin.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    now = json.loads(json.dumps(maker.collect()))                        # (tuples -> lists, integer keys -> strings)
    assert sorted(now) == sorted(pin) == ["ae", "fm"]
    for tag in pin:
        assert sorted(now[tag]) == sorted(pin[tag])
        for key, want in pin[tag].items():
            if isinstance(want, dict):
                assert sorted(now[tag][key]) == sorted(want), (tag, key)
                for sub, value in want.items():
                    assert now[tag][key][sub] == value, (tag, key, sub)
            else:
                assert now[tag][key] == want, (tag, key)
    # the figures the refactoring was pinned on
    assert (pin["fm"]["param_floats"], pin["fm"]["stat_floats"]) == (33366548, 4960)
    assert (pin["ae"]["param_floats"], pin["ae"]["stat_floats"]) == (21633796, 4864)
    assert pin["fm"]["workspace_floats"]["3"] == 100110800 and pin["ae"]["workspace_floats"]["3"] == 77552400
    assert pin["ae"]["workspace_floats"]["8193"] == 0
    assert pin["fm"]["workspace_offset"]["3"][27] == 52399824 and pin["ae"]["workspace_offset"]["3"][31] == 30519312
    assert len(pin["fm"]["layout"]) == 2 * 14 + 4 * 10 and len(pin["ae"]["layout"]) == 2 * 12 + 4 * 8
    assert pin["fm"]["buckets"][0] == [31979328, 1382260] and pin["fm"]["buckets"][-1] == [33361588, 4960]
    assert pin["ae"]["buckets"][0] == [18871872, 2757060] and pin["ae"]["buckets"][-1] == [21628932, 4864]


def test_host_side_refusals(lib):
    off, dims = ctypes.c_int64(), (ctypes.c_int64 * 6)()
    assert lib.ndp_fm_layout(0, 14, ctypes.byref(off), dims) == 1 and b"out of range" in lib.ndp_last_error()
    assert lib.ndp_fm_workspace_floats(0) == 0 and lib.ndp_fm_workspace_floats(8) > lib.ndp_fm_workspace_floats(1) > 0
    assert lib.ndp_fm_workspace_offset(8, 999) == -1
    assert lib.ndp_fm_forward(None, None, None, None, 1, 1, None, None, None) == 1
    model = FE.ForwardAutoencoder().eval()
    with pytest.raises(_capi.NdpError):                                  # no CPU path for the kernels' case
        model(torch.zeros(1, 3, 128, 128), torch.zeros(1, 4))
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    with pytest.raises(_capi.NdpError):
        ForwardModelTrainer(model, batch=2)
    model.train()
    x, a = torch.rand(1, 3, 128, 128) * 2 - 1, torch.rand(1, 4)
    with pytest.raises(_capi.NdpError):                                  # training mode neither
        model(x, a)
    # the operator composition the mirror keeps for Encoder / Decoder called on their own is the oracle's arithmetic
    y = model._forward_torch(x, a)
    want = FO.forward({k: v.clone() for k, v in model.state_dict().items()}, x, a, training=True)
    assert y.requires_grad and float((y.detach() - want).abs().max()) <= 1e-6
