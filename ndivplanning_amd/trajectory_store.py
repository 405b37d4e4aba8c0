"""A directory of trajectory bundles (bundle.py) resident in device memory, and batches assembled from it on the device
(ndp_store_gather, include/ndp.h).

`DeviceTrajectoryStore` uploads every bundle once -- the streams as one blob, one frame-offset table rebased across the
files, states, actions and goals.  `store.gather(indices, seq_start, seq_length)` returns what a `DataLoader` over
`BundleDataset(raw_jpeg=True)` with `collate_jpeg` returns for the same trajectories -- a `JpegFrames` whose buffer and
offsets are byte-identical to `pack_jpegs` of the same streams, and the float tensors -- with everything on the device
and only the B indices travelling there.  `StoreLoader` is the `DataLoader` replacement: the same batches in the same
order for the same `torch.manual_seed`, the order drawn by torch's own samplers on the host."""
import numpy as np
import torch
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler

from . import _capi, bundle
from .jpeg import JpegFrames

BAD_INDEX, CAPACITY = 1, 2              # NDP_STORE_* (include/ndp.h)


def store_bytes(bundles):
    """The device bytes a list of open bundles takes as a store."""
    return sum(b.blob.size + 8 * b.offsets.size + 4 * (b.states.size + b.actions.size + b.goal.size) for b in bundles)


class DeviceTrajectoryStore:
    """Every bundle of `datadir`, in sorted file order, in the memory of `device`.  `len(store)` trajectories of
    `store.steps` frames; `store.max_stream_bytes` is the longest stream.  max_bytes: refuse a larger directory (default:
    a quarter of the device's free memory now).  The blob is not padded: the kernel reads nothing outside it."""

    def __init__(self, datadir, device=None, max_bytes=None):
        bundles = bundle.open_dir(datadir)
        steps = {b.steps for b in bundles}
        if len(steps) != 1:
            raise ValueError("%s holds bundles of different trajectory lengths %s: a store needs one" % (datadir, sorted(steps)))
        need = store_bytes(bundles)
        if max_bytes is None:
            self.device = self._device(device)
            max_bytes = torch.cuda.mem_get_info(self.device)[0] // 4
        if need > int(max_bytes):
            raise ValueError("%s takes %d bytes as a device-resident store, more than max_bytes = %d: read it with the host "
                             "loader instead (PushDataset / BundleDataset with a DataLoader; leave device_store off)"
                             % (datadir, need, int(max_bytes)))
        self.device = self._device(device)
        self.lib = _capi.load()
        self.datadir = datadir
        self.n, self.steps = sum(b.n for b in bundles), steps.pop()
        self.max_stream_bytes = max(b.max_stream_bytes() for b in bundles)
        offsets, base = [], 0
        for b in bundles:
            offsets.append(np.asarray(b.offsets[:-1], np.int64) + base)
            base += int(b.offsets[-1])
        offsets.append(np.array([base], np.int64))
        up = lambda arrays: torch.from_numpy(np.concatenate([np.asarray(a) for a in arrays])).to(self.device)   # noqa: E731
        self.blob = up([b.blob for b in bundles])
        self.offsets = up(offsets)
        self.states = up([b.states for b in bundles])
        self.actions = up([b.actions for b in bundles])
        self.goal = up([b.goal for b in bundles])
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)      # of the last gather (NDP_STORE_*)
        self.nbytes = need

    @staticmethod
    def _device(device):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise _capi.NdpError("DeviceTrajectoryStore lives on a ROCm GPU only (got %s)" % dev)
        return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev

    def __len__(self):
        return self.n

    def check_window(self, seq_start, seq_length):
        if seq_start < 0 or seq_length < 1 or seq_start + seq_length > self.steps:
            raise ValueError("%s holds trajectories of %d steps: seq_start %d + seq_length %d does not fit"
                             % (self.datadir, self.steps, seq_start, seq_length))

    def gather(self, indices, seq_start, seq_length):
        """indices: int64 [B], host (validated here, then uploaded) or device (guarded by the kernel: an index out of
        range gives empty streams and zero rows and sets `store.status`).  Returns (JpegFrames [B, seq_length], states
        [B,seq_length,25], actions [B,seq_length,4], goal [B,3]) on the device.  The frames' buffer has the capacity
        B * seq_length * max_stream_bytes; its part past offsets[-1] is not written.  No host synchronisation."""
        seq_start, seq_length = int(seq_start), int(seq_length)
        self.check_window(seq_start, seq_length)
        if not isinstance(indices, torch.Tensor):
            indices = torch.as_tensor(indices, dtype=torch.int64)
        if indices.dim() != 1 or indices.numel() < 1 or indices.dtype != torch.int64:
            raise ValueError("indices must be a 1-D int64 tensor of at least one trajectory index")
        if not indices.is_cuda:
            if int(indices.min()) < 0 or int(indices.max()) >= self.n:
                raise IndexError("trajectory indices must lie in 0..%d, got %d..%d" % (self.n - 1, int(indices.min()), int(indices.max())))
            indices = indices.to(self.device, non_blocking=True)
        indices = indices.contiguous()
        b = int(indices.numel())
        n, dev = b * seq_length, self.device
        capacity = n * self.max_stream_bytes
        buffer = torch.empty(capacity, dtype=torch.uint8, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        states = torch.empty(b, seq_length, bundle.STATE_DIM, dtype=torch.float32, device=dev)
        actions = torch.empty(b, seq_length, bundle.ACTION_DIM, dtype=torch.float32, device=dev)
        goal = torch.empty(b, bundle.GOAL_DIM, dtype=torch.float32, device=dev)
        with _capi.on_device(dev):
            _capi.check(self.lib.ndp_store_gather(
                _capi.ptr(self.blob), int(self.blob.numel()), _capi.ptr(self.offsets), _capi.ptr(self.states),
                _capi.ptr(self.actions), _capi.ptr(self.goal), self.n, self.steps, _capi.ptr(indices), b, seq_start,
                seq_length, _capi.ptr(buffer), capacity, _capi.ptr(offsets), _capi.ptr(states), _capi.ptr(actions),
                _capi.ptr(goal), _capi.ptr(self.status), _capi.stream_ptr(dev)), "ndp_store_gather")
        return JpegFrames(buffer, offsets, b, seq_length), states, actions, goal


class StoreLoader:
    """Iterable with `__len__` over a store: yields what `DataLoader(BundleDataset(datadir, seq_start, seq_length,
    raw_jpeg=True), batch_size, shuffle, collate_fn=collate_jpeg)` yields, in the same order for the same
    `torch.manual_seed` (torch's own RandomSampler / BatchSampler on the host, after the one draw a DataLoader's iterator
    takes from the global generator first), the ragged final batch included -- on the device.  world > 1: only rows
    `dp.shard_bounds(batch_size, rank, world)` of every full batch are gathered and the ragged batch is skipped, as the
    trainers do with a DataLoader's batches."""

    def __init__(self, store, batch_size, seq_start, seq_length, shuffle=True, rank=0, world=1):
        from . import dp
        self.store, self.batch_size = store, int(batch_size)
        self.seq_start, self.seq_length = int(seq_start), int(seq_length)
        self.rank, self.world = int(rank), int(world)
        if self.batch_size < 1 or not 0 <= self.rank < self.world:
            raise ValueError("StoreLoader: batch_size %d, rank %d of %d" % (self.batch_size, self.rank, self.world))
        if hasattr(store, "check_window"):
            store.check_window(self.seq_start, self.seq_length)
        self.shard = dp.shard_bounds(self.batch_size, self.rank, self.world) if self.world > 1 else (0, self.batch_size)
        rows = range(len(store))
        self.batch_sampler = BatchSampler(RandomSampler(rows) if shuffle else SequentialSampler(rows), self.batch_size,
                                          drop_last=False)

    def __len__(self):
        return len(self.batch_sampler) if self.world == 1 else len(self.store) // self.batch_size

    def index_batches(self):
        """The epoch's index lists, one per yielded batch (this rank's rows of it)."""
        torch.empty((), dtype=torch.int64).random_()            # DataLoader's iterator draws its base seed first
        for indices in self.batch_sampler:
            if self.world > 1:
                if len(indices) != self.batch_size:
                    continue
                indices = indices[self.shard[0]:self.shard[1]]
            yield indices

    def __iter__(self):
        for indices in self.index_batches():
            yield self.store.gather(torch.tensor(indices, dtype=torch.int64), self.seq_start, self.seq_length)


def require_bundle_dir(path, what):
    """The `device_store` switch of the trainers: `path` must be a directory of bundles."""
    path = str(path)
    if "synthetic:" in path or not bundle.is_bundle_dir(path):
        raise ValueError("%s needs a directory of %s trajectory bundles (python -m ndivplanning_amd.bundle convert | "
                         "synth), got %r" % (what, bundle.SUFFIX, path))
    return path
