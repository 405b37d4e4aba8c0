"""GPU tests of the Lanczos resize (csrc/ndp_resize.inc, ndivplanning_amd/resize.py): PIL's bytes on every size and
content of tests/resize_core_host.py (the CPU twin of these tests runs the same frames through the kernel's schedule on
the host: tests/test_resize_core_host.py)."""
import numpy as np
import pytest
import torch

import resize_core_host as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = [s for s in R.SIZES if s != (2048, 2048)]


@pytest.fixture(scope="module")
def resizer():
    from ndivplanning_amd import _build
    from ndivplanning_amd.resize import LanczosResizer
    _build.build()
    return LanczosResizer(DEV)


def _frames_u8(bytes_dev):
    """ndp_eval_frames_u8 of resized bytes: what the float output must equal bit for bit."""
    from ndivplanning_amd import _capi
    n = int(bytes_dev.shape[0])
    out = torch.empty(n, 3, 128, 128, device=DEV)
    _capi.check(_capi.load().ndp_eval_frames_u8(_capi.ptr(bytes_dev), n, _capi.ptr(out), _capi.stream_ptr()), "frames_u8")
    return out


def _check(resizer, frames, want):
    """frames uint8 [n,H,W,3] (host), want [n,128,128,3]: bytes, floats, a second run, a device-resident input."""
    host = torch.from_numpy(frames)
    got, img = resizer(host)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and tuple(img.shape) == (len(frames), 3, 128, 128)
    bad = np.argwhere(got.cpu().numpy() != want)
    assert len(bad) == 0, "%d bytes differ from PIL's, first at %s" % (len(bad), bad[:4].tolist())
    assert torch.equal(img, _frames_u8(got))
    again, img2 = resizer(host)
    assert torch.equal(again, got) and torch.equal(img2, img)
    resident, img3 = resizer(host.to(DEV))
    assert torch.equal(resident, got) and torch.equal(img3, img)
    only_bytes, none = resizer(host, floats=False)
    assert none is None and torch.equal(only_bytes, got)
    return got


@pytest.mark.parametrize("h,w", SMALL)
def test_bytes_are_pil_s_singly_and_in_a_batch(resizer, h, w):
    frames = np.stack([R.make_frame(h, w, c) for c in R.CONTENTS])
    want = np.stack([R.pil_resize(f) for f in frames])
    batch = _check(resizer, frames, want)                                       # n = 3
    for i in range(3):                                                          # n = 1: a batch equals its frames singly
        one = _check(resizer, frames[i:i + 1], want[i:i + 1])
        assert torch.equal(one[0], batch[i])
    if (h, w) == (128, 128):
        assert np.array_equal(want, frames)                                     # the copy path


@pytest.mark.parametrize("content", R.CONTENTS)
def test_the_largest_frame(resizer, content):
    frame = R.make_frame(2048, 2048, content)
    _check(resizer, frame[None], R.pil_resize(frame)[None])


@pytest.mark.parametrize("h,w", [(500, 500), (129, 127), (128, 300), (300, 128), (37, 53)])
def test_the_band_split_does_not_change_a_bit(resizer, h, w):
    """Every rows_per_band the entry takes, and the one it picks for 1, 8, 16 and 40 images."""
    frames = torch.from_numpy(np.stack([R.make_frame(h, w, R.CONTENTS[i % 3], seed=i) for i in range(40)]))
    want, wimg = resizer(frames, rows_per_band=1)
    assert np.array_equal(want[:3].cpu().numpy(), np.stack([R.pil_resize(f.numpy()) for f in frames[:3]]))
    for rb in (2, 4, 8, 16):
        got, img = resizer(frames, rows_per_band=rb)
        assert torch.equal(got, want) and torch.equal(img, wimg), rb
    for n in (1, 8, 16, 40):
        got, img = resizer(frames[:n])
        assert torch.equal(got, want[:n]) and torch.equal(img, wimg[:n]), n


def test_a_view_off_a_dword_boundary_and_bad_frames(resizer):
    from ndivplanning_amd import _capi
    flat = torch.from_numpy(R.make_frame(1, 37 * 53 * 3 + 1, "noise")[0, :, 0].copy()).to(DEV)
    view = flat[1:].view(1, 37, 53, 3)
    assert view.data_ptr() % 4 == 1
    got, _ = resizer(view)
    assert np.array_equal(got[0].cpu().numpy(), R.pil_resize(view[0].cpu().numpy()))
    with pytest.raises(_capi.NdpError):
        resizer(torch.zeros(1, 2049, 8, 3, dtype=torch.uint8))
    with pytest.raises(_capi.NdpError):
        resizer(torch.zeros(1, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(_capi.NdpError):
        resizer(torch.zeros(1, 8, 8, 3))
    with pytest.raises(_capi.NdpError, match="LDS"):
        resizer(torch.zeros(1, 2048, 16, 3, dtype=torch.uint8), rows_per_band=8)


def test_committed_frames_resize_to_the_committed_bytes(resizer):
    g = load_golden("resize_case")
    for k in ("a", "b"):
        got, img = resizer(torch.from_numpy(g["frame_" + k])[None])
        assert np.array_equal(got[0].cpu().numpy(), g["resized_" + k]), k
        want = (torch.from_numpy(g["resized_" + k]).permute(2, 0, 1).float().div(255) - 0.5) * 2.0
        assert torch.equal(img[0].cpu(), want)


def test_the_resize_kernel_launches_once(resizer):
    from ndivplanning_amd import _capi
    frames = torch.from_numpy(R.make_frame(120, 160, "noise")[None]).to(DEV)
    _capi.timing_enable(True)
    try:
        resizer(frames)
        torch.cuda.synchronize()
        seen = _capi.timing_collect()
    finally:
        _capi.timing_enable(False)
    assert seen == {"k_resize_lanczos": (seen["k_resize_lanczos"][0], 1)}, seen
