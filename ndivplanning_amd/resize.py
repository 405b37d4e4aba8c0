"""Device-side Lanczos resize of camera frames (ndp_resize_lanczos_u8, include/ndp.h).

A live environment renders frames of its own size (MuJoCo: 500x500); the reference resizes them on the host with
`Image.fromarray(frame).resize((128, 128), Image.LANCZOS)` (MPC_gym_eval.py:68-77, generate_trajectories.py:113-118).
`LanczosResizer` does it on the device, bit-identical to Pillow, and can hand back the normalised floats the networks
take from the same launch.  The coefficient tables of a frame size are built on the host (in double, once) and cached
per (H, W, device)."""
import ctypes

import torch

from . import _capi

OUT = 128
MAX_SIDE = 2048
TABLE_MAGIC = 0x525a4c33          # resize::kMagic (csrc/ndp_resize.inc): the tables' first int, then H and W
_TABLES = {}


def host_tables(height, width):
    """The coefficient tables of one frame size as a host int32 tensor (ndp_resize_build_tables)."""
    lib = _capi.load()
    need = int(lib.ndp_resize_workspace_bytes(int(height), int(width)))
    if need <= 0:
        raise _capi.NdpError("frames of %d x %d cannot be resized: both sides must lie in 1..%d" % (height, width, MAX_SIDE))
    t = torch.empty(need // 4, dtype=torch.int32)
    _capi.check(lib.ndp_resize_build_tables(int(height), int(width), ctypes.c_void_p(t.data_ptr()), need),
                "ndp_resize_build_tables")
    if t[:3].tolist() != [TABLE_MAGIC, int(height), int(width)]:
        raise _capi.NdpError("ndp_resize_build_tables wrote the header %s for %d x %d" % (t[:5].tolist(), height, width))
    return t


class LanczosResizer:
    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise _capi.NdpError("LanczosResizer runs on a ROCm GPU only (got %s)" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _capi.load()

    def tables(self, height, width):
        key = (int(height), int(width), self.device.index)
        if key not in _TABLES:
            host = host_tables(height, width)
            _TABLES[key] = (host.to(self.device), host[:3].tolist())
        dev, header = _TABLES[key]
        if header != [TABLE_MAGIC, int(height), int(width)]:          # the cached tables are this size's
            raise _capi.NdpError("cached resize tables %s do not belong to %d x %d" % (header, height, width))
        return dev

    def __call__(self, frames, floats=True, rows_per_band=0):
        """frames: uint8 [n,H,W,3], host or device -> (uint8 [n,128,128,3], fp32 [n,3,128,128] in [-1,1] or None) on the
        device.  rows_per_band: 0 (chosen from n), or 1, 2, 4, 8, 16 -- the bytes do not depend on it."""
        if frames.dtype != torch.uint8 or frames.dim() != 4 or int(frames.shape[3]) != 3:
            raise _capi.NdpError("frames must be uint8 [n,H,W,3], got %s %s" % (frames.dtype, tuple(frames.shape)))
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        tab = self.tables(h, w)
        x = frames.to(self.device, non_blocking=True).contiguous()
        if x.data_ptr() % 4:
            x = x.clone()                         # a view that starts off a dword boundary
        out = torch.empty(n, OUT, OUT, 3, dtype=torch.uint8, device=self.device)
        img = torch.empty(n, 3, OUT, OUT, dtype=torch.float32, device=self.device) if floats else None
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_resize_lanczos_u8(_capi.ptr(x), n, h, w, _capi.ptr(tab), int(tab.numel()) * 4,
                                                       int(rows_per_band), _capi.ptr(out), _capi.ptr(img),
                                                       _capi.stream_ptr(self.device)), "ndp_resize_lanczos_u8")
        return out, img
