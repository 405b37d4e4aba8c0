"""Device-side JPEG decode and encode of trajectory frames (ndp_jpeg_decode_u8, ndp_jpeg_encode_u8, include/ndp.h;
DESIGN.md sections 5f and 5i).

The reference stores every camera frame as a JPEG (generate_trajectories.py:113-122: PIL, quality 95, 4:2:0, 128x128)
and decodes it with PIL on the host (utils/hdf5_load.py:9-11).  Here the loader workers only pack the streams
(`pack_jpegs` / `collate_jpeg`: one byte buffer plus int64 offsets, about a sixth of the decoded bytes), and
`JpegDecoder.decode` turns them into the [n,128,128,3] uint8 frames the *_u8 entry points take, bit-identical to PIL.

Formats other than the reference writer's (progressive, restart intervals, other sampling factors or sizes, ...) are
not decoded: each frame has a status (STATUS below), and `check` decides when a nonzero one raises.

`JpegEncoder` is the other direction: [n,128,128,3] uint8 frames -> the streams the reference's writer gives
(generate_trajectories.py:113-122), byte for byte, in the packed layout above.
"""
import numpy as np
import torch

from . import _capi

FRAME_SHAPE = (128, 128, 3)
STATUS = {0: "ok", 1: "unsupported format", 2: "not 128x128", 3: "corrupt or truncated",
          4: "stream does not fit the workspace"}


class JpegDecodeError(_capi.NdpError):
    """A frame did not decode: `index` is its position in the batch, `status` its NDP_JPEG_* code."""

    def __init__(self, index, status):
        self.index, self.status = int(index), int(status)
        super().__init__("JPEG frame %d did not decode: status %d (%s)"
                         % (self.index, self.status, STATUS.get(self.status, "?")))


def pack_jpegs(streams, pin=True):
    """Concatenate JPEG streams (bytes-like) into (buffer uint8 [total], offsets int64 [n+1]) host tensors: stream i is
    buffer[offsets[i]:offsets[i+1]].  pin: page-locked, for an asynchronous upload (only where a GPU is present; in
    DataLoader workers leave it off and let `DataLoader(pin_memory=True)` pin in the main process)."""
    views = [np.frombuffer(memoryview(s), dtype=np.uint8) for s in streams]
    if not views:
        raise ValueError("pack_jpegs: no streams")
    offsets = np.zeros(len(views) + 1, dtype=np.int64)
    np.cumsum([v.size for v in views], out=offsets[1:])
    buffer = torch.from_numpy(np.concatenate(views))
    offsets = torch.from_numpy(offsets)
    if pin and torch.cuda.is_available():
        buffer, offsets = buffer.pin_memory(), offsets.pin_memory()
    return buffer, offsets


class JpegFrames:
    """A batch of B trajectories x T frames as JPEG streams: what `collate_jpeg` yields in place of the frame tensor.
    `frames[lo:hi]` keeps trajectories lo..hi-1 (the same buffer, a slice of the offsets)."""

    def __init__(self, buffer, offsets, batch, steps):
        self.buffer, self.offsets, self.batch, self.steps = buffer, offsets, int(batch), int(steps)

    @property
    def shape(self):
        return (self.batch, self.steps) + FRAME_SHAPE

    def __len__(self):
        return self.batch

    def __getitem__(self, rows):
        if not isinstance(rows, slice):
            raise TypeError("JpegFrames supports slices of trajectories only")
        lo, hi, step = rows.indices(self.batch)
        if step != 1:
            raise ValueError("JpegFrames: slice step must be 1")
        hi = max(hi, lo)
        return JpegFrames(self.buffer, self.offsets[lo * self.steps:hi * self.steps + 1], hi - lo, self.steps)

    def pin_memory(self):                # DataLoader(pin_memory=True)
        return JpegFrames(self.buffer.pin_memory(), self.offsets.pin_memory(), self.batch, self.steps)


def collate_jpeg(batch):
    """DataLoader collate for datasets that yield (list of T JPEG streams, states, actions, goal): the B x T frames are
    packed into one JpegFrames (not pinned: see pack_jpegs), the rest stacked as default_collate does."""
    frames = [s for item in batch for s in item[0]]
    steps = len(batch[0][0])
    if any(len(item[0]) != steps for item in batch):
        raise ValueError("collate_jpeg: trajectories of different lengths")
    buffer, offsets = pack_jpegs(frames, pin=False)
    rest = torch.utils.data.default_collate([tuple(item[1:]) for item in batch])
    return (JpegFrames(buffer, offsets, len(batch), steps),) + tuple(rest)


def is_jpeg(dataset):
    return getattr(dataset, "mode", None) == "jpeg"


def loader_kwargs(dataset):
    """Extra DataLoader arguments for `dataset`: the JPEG collate for a dataset in jpeg mode, nothing otherwise."""
    return {"collate_fn": collate_jpeg} if is_jpeg(dataset) else {}


class JpegDecoder:
    """Holds the decode workspace of one device.  check: True -> every decode synchronises and raises JpegDecodeError
    naming the first failed frame; "deferred" -> the statuses are copied to pinned memory behind an event and checked at
    the next decode() or at finish() (no host synchronisation on the hot path); False -> never raises (see `status`)."""

    def __init__(self, device=None, check=True):
        if check not in (True, False, "deferred"):
            raise ValueError("check must be True, False or 'deferred'")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise _capi.NdpError("JpegDecoder decodes on a ROCm GPU only (got %s)" % self.device)
        self.lib = _capi.load()
        self.check = check
        self.status = None              # int32 [n] device tensor of the last decode
        self._ws = None
        self._pending = None

    def _workspace(self, n, stream_bytes):
        need = int(self.lib.ndp_jpeg_workspace_bytes(int(n), int(stream_bytes)))
        if need <= 0:
            raise _capi.NdpError("ndp_jpeg_workspace_bytes(%d, %d) refused the batch" % (n, stream_bytes))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def decode(self, buffer, offsets, check=None):
        """buffer: uint8 [bytes] (host or device), offsets: int64 [n+1] (frame i = buffer[offsets[i]:offsets[i+1]];
        device offsets must lie within the buffer, host ones are checked).  Returns the [n,128,128,3] uint8 frames on the device; frames that did not decode are all zero."""
        check = self.check if check is None else check
        self._raise_pending()
        if buffer.dtype != torch.uint8 or buffer.dim() != 1:
            raise _capi.NdpError("JPEG buffer must be a 1-D uint8 tensor")
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2:
            raise _capi.NdpError("JPEG offsets must be a 1-D int64 tensor of n+1 >= 2 entries")
        n = int(offsets.numel()) - 1
        if not offsets.is_cuda:            # free on the host (pack_jpegs, collate_jpeg): the kernels cannot check it
            if int(offsets[0]) < 0 or int(offsets[-1]) > buffer.numel() or bool((offsets[1:] < offsets[:-1]).any()):
                raise _capi.NdpError("JPEG offsets must be non-decreasing within the %d-byte buffer" % buffer.numel())
        buf = buffer.to(self.device, non_blocking=True).contiguous()
        off = offsets.to(self.device, non_blocking=True).contiguous()
        ws = self._workspace(n, max(int(buf.numel()), 1))
        frames = torch.empty((n,) + FRAME_SHAPE, dtype=torch.uint8, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_jpeg_decode_u8(_capi.ptr(buf), _capi.ptr(off), n, _capi.ptr(frames),
                                                    _capi.ptr(status), _capi.ptr(ws), int(ws.numel()),
                                                    _capi.stream_ptr(self.device)), "ndp_jpeg_decode_u8")
            self.status = status
            if check is True:
                self._raise_first(status.cpu())
            elif check == "deferred":
                host = torch.empty(n, dtype=torch.int32, pin_memory=True)
                host.copy_(status, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                self._pending = (host, event)
        return frames

    def decode_frames(self, frames, check=None):
        """JpegFrames [B,T] -> uint8 [B,T,128,128,3] on the device."""
        return self.decode(frames.buffer, frames.offsets, check=check).view(frames.shape)

    def decode_images(self, frames, check=None):
        """JpegFrames [B,T] -> fp32 [B,T,3,128,128] in [-1,1] on the device: the decoded bytes normalised as the
        reference's loader does (utils/hdf5_load.py:9-11), by ndp_eval_frames_u8."""
        x = self.decode(frames.buffer, frames.offsets, check=check)
        n = int(x.shape[0])
        out = torch.empty(n, 3, 128, 128, dtype=torch.float32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_eval_frames_u8(_capi.ptr(x), n, _capi.ptr(out), _capi.stream_ptr(self.device)),
                        "ndp_eval_frames_u8")
        return out.view(frames.batch, frames.steps, 3, 128, 128)

    def finish(self):
        """Raise for a deferred check that is still outstanding."""
        self._raise_pending()

    def _raise_pending(self):
        if self._pending is not None:
            host, event = self._pending
            self._pending = None
            event.synchronize()
            self._raise_first(host)

    @staticmethod
    def _raise_first(host_status):
        bad = torch.nonzero(host_status).flatten()
        if bad.numel():
            i = int(bad[0])
            raise JpegDecodeError(i, int(host_status[i]))


class JpegEncodeError(_capi.NdpError):
    pass


class JpegEncoder:
    """Holds the encode workspace of one device.  The streams are the reference writer's, byte for byte (PIL,
    `format="jpeg", quality=95`: baseline, 4:2:0, standard Huffman tables); only 128x128 frames are encoded.

    Capacity: a stream is 0.9-24 KB (24 KB: noise of only 0 and 255) but the bound that holds for every pixel array is
    `max_stream_bytes` (about 160 KB), so by default a batch gets DEFAULT_FRAME_BYTES a frame.  If a frame did not fit
    (status 4 on the last frame; only hand-made worst cases get there), the lengths of all frames, which every call leaves
    in the workspace, are summed and the batch is encoded again into exactly that many bytes."""

    DEFAULT_FRAME_BYTES = 32768
    EAGER_FRAME_BYTES = 8192            # encode_to_bytes: what its first (usually only) download takes per frame

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise _capi.NdpError("JpegEncoder encodes on a ROCm GPU only (got %s)" % self.device)
        self.lib = _capi.load()
        self.max_stream_bytes = int(self.lib.ndp_jpeg_encode_max_stream_bytes())
        self.status = None              # int32 [n] device tensor of the last encode
        self._ws = None

    def _workspace(self, n):
        need = int(self.lib.ndp_jpeg_encode_workspace_bytes(int(n)))
        if need <= 0:
            raise _capi.NdpError("ndp_jpeg_encode_workspace_bytes(%d) refused the batch" % n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _frames(self, frames):
        if not isinstance(frames, torch.Tensor):
            frames = torch.as_tensor(frames)
        if frames.dtype != torch.uint8 or frames.dim() not in (4, 5) or tuple(frames.shape[-3:]) != FRAME_SHAPE:
            raise _capi.NdpError("frames must be uint8 [n,128,128,3] or [B,T,128,128,3], got %s %s"
                                 % (frames.dtype, tuple(frames.shape)))
        x = frames.to(self.device, non_blocking=True).contiguous().view((-1,) + FRAME_SHAPE)
        if x.shape[0] < 1:
            raise _capi.NdpError("no frames to encode")
        return x.clone() if x.data_ptr() % 4 else x

    def _launch(self, x, capacity):
        """One allocation: offsets int64 [n+1], status int32 [n], padding to 16 bytes, then `capacity` stream bytes.
        Returns (blob, offsets, status, streams), the last three views of the first."""
        n = int(x.shape[0])
        meta = (8 * (n + 1) + 4 * n + 15) // 16 * 16
        blob = torch.empty(meta + int(capacity), dtype=torch.uint8, device=self.device)
        offsets = blob[:8 * (n + 1)].view(torch.int64)
        status = blob[8 * (n + 1):8 * (n + 1) + 4 * n].view(torch.int32)
        streams = blob[meta:]
        ws = self._workspace(n)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_jpeg_encode_u8(_capi.ptr(x), n, _capi.ptr(streams), int(capacity), _capi.ptr(offsets),
                                                    _capi.ptr(status), _capi.ptr(ws), int(ws.numel()),
                                                    _capi.stream_ptr(self.device)), "ndp_jpeg_encode_u8")
        self.status = status
        return blob, offsets, status, streams

    def _needed(self, n):
        """The bytes the last batch of n frames takes: the sum of the lengths the call left in the workspace."""
        at = int(self.lib.ndp_jpeg_encode_lengths_offset(n))
        return int(self._ws[at:at + 8 * n].view(torch.int64).sum())

    @staticmethod
    def _tail(blob, n):
        """(offsets[n], status[n-1]) of a launch's blob, in one small copy."""
        host = blob[8 * n:8 * (n + 1) + 4 * n].cpu()
        return int(host[:8].view(torch.int64)), int(host[-4:].view(torch.int32))

    def encode(self, frames, capacity=None):
        """frames: uint8 [n,128,128,3] or [B,T,128,128,3], host or device -> (buffer uint8 [bytes], offsets int64 [n+1])
        on the device: stream i is buffer[offsets[i]:offsets[i+1]], what pack_jpegs makes and JpegDecoder.decode takes.

        capacity None: the default a frame; the total and the last status are read back in one copy (one
        synchronisation) and the buffer is exactly that long.  A batch that did not fit is encoded again into the sum of
        its lengths (one more read).  capacity given: no host synchronisation and no retry; the buffer is `capacity`
        long, a frame that did not fit and every later one have length 0 and `self.status` 4."""
        x = self._frames(frames)
        n = int(x.shape[0])
        if capacity is not None:
            _, offsets, _, streams = self._launch(x, int(capacity))
            return streams, offsets
        capacity = n * self.DEFAULT_FRAME_BYTES
        for attempt in range(2):
            blob, offsets, _, streams = self._launch(x, capacity)
            total, last = self._tail(blob, n)       # a frame that fits has every earlier one fit too
            if last == 0:
                return streams[:total], offsets
            capacity = self._needed(n)
        raise JpegEncodeError("%d frames did not fit the %d bytes their own lengths add up to" % (n, capacity))

    def encode_frames(self, frames, capacity=None):
        """uint8 [B,T,128,128,3], host or device -> JpegFrames [B,T] on the device (what JpegDecoder.decode_frames
        takes)."""
        shape = tuple(torch.as_tensor(frames).shape) if not isinstance(frames, torch.Tensor) else tuple(frames.shape)
        if len(shape) != 5:
            raise _capi.NdpError("encode_frames takes [B,T,128,128,3], got %s" % (shape,))
        buffer, offsets = self.encode(frames, capacity=capacity)
        return JpegFrames(buffer, offsets, shape[0], shape[1])

    def encode_to_bytes(self, frames):
        """-> list of n bytes objects, what generate_trajectories.py stores per frame.  One download and one
        synchronisation while the streams average EAGER_FRAME_BYTES or less (camera frames are 4-7 KB): offsets,
        statuses and the head of the stream buffer come back in one copy; a longer batch takes a second copy for the
        rest, and one that did not fit the default capacity is encoded again as in `encode`."""
        x = self._frames(frames)
        n = int(x.shape[0])
        capacity = n * self.DEFAULT_FRAME_BYTES
        for attempt in range(2):
            blob, offsets, status, streams = self._launch(x, capacity)
            meta = int(blob.numel() - streams.numel())
            head = blob[:meta + min(capacity, n * self.EAGER_FRAME_BYTES)].cpu().numpy()
            off = head[:8 * (n + 1)].view(np.int64)
            st = head[8 * (n + 1):8 * (n + 1) + 4 * n].view(np.int32)
            if int(st[-1]) != 0:
                capacity = self._needed(n)
                continue
            data = head[meta:]
            if int(off[-1]) > data.size:
                data = np.concatenate([data, streams[data.size:int(off[-1])].cpu().numpy()])
            return [data[off[i]:off[i + 1]].tobytes() for i in range(n)]
        raise JpegEncodeError("%d frames did not fit the %d bytes their own lengths add up to" % (n, capacity))
