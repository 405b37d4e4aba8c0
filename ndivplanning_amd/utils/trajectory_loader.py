"""Trajectory datasets with the reference's `PushDataset.__getitem__` contract
(utils/trajectory_loader.py:38-72): (images [T,3,H,W] f32 in [-1,1], states [T,25],
actions [T,4], goal [3]).

`PushDataset` reads a trajectory directory: the project's own `.ndpt` bundles (ndivplanning_amd/bundle.py: numpy for the
container, PIL only to decode to pixels on the host, no h5py) or the reference's HDF5 bundles
(generate_trajectories.py:275-324), which need h5py -- where that is missing it raises a clear error at construction
(`python -m ndivplanning_amd.bundle convert` turns HDF5 directories into bundles on a machine that has it).
`SyntheticPushDataset` has the same output contract without any stored data, plus a `codes` mode that yields per-frame
128-d codes instead of images (what a cache of the frozen encoder's outputs would hold)."""
import numpy as np
import torch

from .argparse_util import listdir_nohidden


class SyntheticPushDataset(torch.utils.data.Dataset):
    """Seeded random trajectories.  mode 'images': frames ~ U[-1,1) [T,3,128,128];
    mode 'codes': frame codes ~ N(0,1) [T,128] in place of the images; mode 'frames_u8': decoded camera frames as the
    JPEG decoder leaves them, bytes [T,128,128,3] (what `PushDataset(raw_uint8=True)` yields); mode 'jpeg': a list of T
    JPEG streams of seeded scenes, encoded as the reference encodes its frames (PIL, quality 95; what
    `PushDataset(raw_jpeg=True)` yields -- batch them with `ndivplanning_amd.jpeg.collate_jpeg`)."""

    def __init__(self, num_trajectories, seq_length=8, mode="codes", seed=0, image_size=128):
        if mode not in ("codes", "images", "frames_u8", "jpeg"):
            raise ValueError("mode must be 'codes', 'images', 'frames_u8' or 'jpeg'")
        if mode == "jpeg":
            try:
                from PIL import Image  # noqa: F401
            except ImportError as e:  # pragma: no cover - depends on the image
                raise RuntimeError("SyntheticPushDataset(mode='jpeg') encodes its scenes with PIL, which is missing "
                                   "(%s)" % e)
        self.n, self.seq_length, self.mode, self.seed, self.hw = int(num_trajectories), int(seq_length), mode, seed, image_size

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        gen = torch.Generator().manual_seed(self.seed * 1000003 + int(index))
        t = self.seq_length
        if self.mode == "codes":
            frames = torch.randn(t, 128, generator=gen)
        elif self.mode == "frames_u8":
            frames = torch.randint(0, 256, (t, self.hw, self.hw, 3), generator=gen, dtype=torch.uint8)
        elif self.mode == "jpeg":
            frames = [encode_jpeg(synthetic_scene(gen, self.hw)) for _ in range(t)]
        else:
            frames = torch.rand(t, 3, self.hw, self.hw, generator=gen) * 2.0 - 1.0
        states = torch.randn(t, 25, generator=gen)
        actions = torch.rand(t, 4, generator=gen) * 2.0 - 1.0
        goal = torch.randn(3, generator=gen)
        return frames, states, actions, goal


def synthetic_scene(gen, size=128):
    """A seeded camera-like frame, bytes [size,size,3]: a gradient, a few discs and a block, mild texture."""
    yy = torch.arange(size, dtype=torch.float32).view(-1, 1).expand(size, size)
    xx = torch.arange(size, dtype=torch.float32).view(1, -1).expand(size, size)
    base = torch.rand(3, generator=gen) * 120
    img = torch.stack([base[0] + 0.9 * xx, base[1] + 0.8 * yy, base[2] + 0.4 * (xx + yy)], dim=2)
    for _ in range(4):
        cy, cx, r = (torch.rand(3, generator=gen) * torch.tensor([size, size, size / 5.0])).tolist()
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < (r + 3) ** 2] = torch.rand(3, generator=gen) * 255
    y0, x0 = (torch.rand(2, generator=gen) * (size - 24)).long().tolist()
    img[y0:y0 + 24, x0:x0 + 20] = torch.rand(3, generator=gen) * 255
    img += torch.randn(size, size, 3, generator=gen) * 3
    return img.clamp(0, 255).to(torch.uint8).numpy()


def encode_jpeg(frame, quality=95):
    """bytes [H,W,3] -> a JPEG stream, as the reference writes its frames (generate_trajectories.py:113-122)."""
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="jpeg", quality=quality)
    return buf.getvalue()


def norm_frame(image):
    """utils/hdf5_load.py:9-11, `(ToTensor()(image) - 0.5) * 2.0`, without torchvision: ToTensor is bytes HWC -> CHW,
    float32, divided by 255."""
    t = torch.from_numpy(np.array(image, dtype=np.uint8)).permute(2, 0, 1).contiguous()
    return (t.to(torch.float32).div(255) - 0.5) * 2.0


class PushDataset(torch.utils.data.Dataset):
    """The reference's HDF5 + JPEG dataset (utils/trajectory_loader.py:17-72).  A directory whose files all end in .ndpt
    is read by `bundle.BundleDataset` instead (same contract, no h5py); a directory that mixes the two is an error."""

    def __init__(self, datadir, seq_start=0, seq_length=15, transform=None, raw_uint8=False, raw_jpeg=False):
        from ..bundle import BundleDataset, is_bundle_dir
        self._bundles = None
        if is_bundle_dir(datadir):
            self._bundles = BundleDataset(datadir, seq_start, seq_length, transform, raw_uint8, raw_jpeg)
            for name, value in vars(self._bundles).items():      # mode (jpeg only), seq_length, files, total_seq_ct, ...
                setattr(self, name, value)
            return
        # raw_uint8: images as the decoder's bytes [T,H,W,3] instead of the normalised float tensor [T,3,H,W]; the
        # kernels apply the reference's normalisation (utils/hdf5_load.py:9-11) as they read (a quarter of the upload)
        # raw_jpeg: images as the stored JPEG streams, a list of T bytes objects, untouched (no PIL); batch them with
        # ndivplanning_amd.jpeg.collate_jpeg and decode on the device (JpegDecoder)
        self.raw_uint8, self.raw_jpeg = bool(raw_uint8), bool(raw_jpeg)
        if self.raw_jpeg:
            self.mode = "jpeg"
        try:
            import h5py  # noqa: F401
            if not self.raw_jpeg:
                from PIL import Image  # noqa: F401
        except ImportError as e:  # pragma: no cover - depends on the image
            raise RuntimeError("PushDataset needs h5py%s to read the reference's trajectory bundles "
                               "(%s); use a `synthetic:` train_data_path instead" % ("" if self.raw_jpeg else " and PIL", e))
        import h5py
        self.datadir, self.transform = datadir, transform
        self.seq_start, self.seq_length = seq_start, seq_length
        self.files = listdir_nohidden(datadir)
        counts = []
        for f in self.files:
            with h5py.File(f, "r") as h:
                counts.append(len(h))
        self.file_seq_cts = np.cumsum(counts)
        self.total_seq_ct = int(self.file_seq_cts[-1]) if counts else 0

    def __len__(self):
        return self.total_seq_ct

    def __getitem__(self, index):
        import io

        if self._bundles is not None:
            return self._bundles[index]
        import h5py
        file_index = int(np.argmax(self.file_seq_cts > index))
        seq_index = index if file_index == 0 else index - int(self.file_seq_cts[file_index - 1])
        sl = slice(self.seq_start, self.seq_start + self.seq_length)
        with h5py.File(self.files[file_index], "r") as f:
            seq = f["trajectory_{:05d}".format(seq_index)]
            raw = [bytes(b.tobytes() if hasattr(b, "tobytes") else b) for b in seq["images"][sl]]
            if self.raw_jpeg:
                images = raw
            else:
                from PIL import Image
                frames = []
                for b in raw:
                    img = Image.open(io.BytesIO(b))
                    frames.append(torch.from_numpy(np.array(img, dtype=np.uint8)) if self.raw_uint8 else norm_frame(img))
                images = torch.stack(frames)
            states = torch.from_numpy(seq["states"][sl])
            actions = torch.from_numpy(seq["actions"][sl])
            goal = torch.from_numpy(np.array(seq["goal"]))
        if self.transform:
            images = self.transform(images)
        return images, states, actions, goal


def open_dataset(path, seq_length, seed, default_mode, modes=None, mode_error=None, push=None):
    """The one way from a data path to a dataset, for every trainer and evaluation script.  `synthetic:<N>[:mode]`, at
    the start of the path or behind a directory prefix (what `make_paths_absolute` makes of it), gives
    `SyntheticPushDataset(N, seq_length, mode or default_mode, seed)`; a mode outside `modes` (None: any the class takes)
    is a ValueError with the caller's own text, `mode_error` (`%(mode)r` in it stands for the mode).  Any other path is a
    trajectory directory: `PushDataset(path, **push)`, the caller's keyword arguments and nothing else."""
    path = str(path)
    if path.startswith("synthetic:") or "/synthetic:" in path:
        spec = path[path.index("synthetic:"):].split(":")
        mode = spec[2] if len(spec) > 2 else default_mode
        if modes is not None and mode not in modes:
            raise ValueError(mode_error % {"mode": mode})
        return SyntheticPushDataset(int(spec[1]), seq_length=seq_length, mode=mode, seed=seed)
    return PushDataset(path, **(push or {}))
