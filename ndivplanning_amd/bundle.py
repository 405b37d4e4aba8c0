"""Trajectory bundles the project reads and writes itself (`.ndpt`): what the reference keeps in
one HDF5 file (generate_trajectories.py:275-324 -- per trajectory T JPEG streams, states [T,25], actions [T,4], goal [3])
in a flat little-endian file that numpy maps: no h5py anywhere.  PIL is needed only to decode to pixels on the host
(`BundleDataset` without raw_jpeg).

File layout (every section starts at a multiple of 64 bytes; the gaps are zero):

    header, 64 bytes
        0   8 bytes   magic  b"NDPTRAJ\\0"
        8   uint32    version (1)
        12  uint32    header bytes (64)
        16  int64     N, trajectories
        24  int64     T, steps (frames) per trajectory
        32  uint32    state width (25)
        36  uint32    action width (4)
        40  uint32    goal width (3)
        44  uint32    0
        48  int64     blob bytes
        56  int64     0
    offsets   int64 [N*T + 1]: frame t of trajectory i is blob[offsets[i*T + t] : offsets[i*T + t + 1]];
              offsets[0] = 0, non-decreasing, offsets[N*T] = blob bytes
    states    float32 [N, T, 25]
    actions   float32 [N, T, 4]
    goal      float32 [N, 3]
    blob      the N*T streams back to back; the file ends with its last byte

Command line:  python -m ndivplanning_amd.bundle convert SRC_DIR DST_DIR | synth N DST_DIR --steps T --seed S
[--per-file M] | info PATH
"""
import argparse
import os
import struct
import sys

import numpy as np
import torch

MAGIC = b"NDPTRAJ\0"
VERSION = 1
HEADER_BYTES = 64
ALIGN = 64
SUFFIX = ".ndpt"
STATE_DIM, ACTION_DIM, GOAL_DIM = 25, 4, 3
_HEADER = struct.Struct("<8sIIqqIIIIqq")
assert _HEADER.size == HEADER_BYTES


def _align(n):
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


def section_layout(n, steps, blob_bytes):
    """{section: (byte offset, byte count)} of a bundle of n trajectories of `steps` frames, and the file's size."""
    sizes = (("offsets", 8 * (n * steps + 1)), ("states", 4 * n * steps * STATE_DIM), ("actions", 4 * n * steps * ACTION_DIM),
             ("goal", 4 * n * GOAL_DIM), ("blob", int(blob_bytes)))
    layout, at = {}, HEADER_BYTES
    for name, size in sizes:
        at = _align(at)
        layout[name] = (at, size)
        at += size
    return layout, at


class Bundle:
    """An open bundle: `offsets` int64 [N*T+1], `states` [N,T,25], `actions` [N,T,4], `goal` [N,3] float32 and `blob`
    uint8 [bytes], all views of one read-only memory map of the file; `n`, `steps`, `path`."""

    def __init__(self, path, n, steps, offsets, states, actions, goal, blob):
        self.path, self.n, self.steps = path, int(n), int(steps)
        self.offsets, self.states, self.actions, self.goal, self.blob = offsets, states, actions, goal, blob

    def __len__(self):
        return self.n

    def stream(self, index, t):
        """Frame t of trajectory `index` as a uint8 view of the blob."""
        f = int(index) * self.steps + int(t)
        return self.blob[int(self.offsets[f]):int(self.offsets[f + 1])]

    def max_stream_bytes(self):
        return int(np.diff(self.offsets).max()) if self.offsets.size > 1 else 0


def write_bundle(path, trajectories):
    """Write the iterable of (streams: T bytes-like, states [T,25], actions [T,4], goal [3]) to `path` as one bundle.
    All trajectories must have the same T >= 1.  Returns the number written."""
    streams, states, actions, goals, steps = [], [], [], [], None
    for item in trajectories:
        frames, s, a, g = item
        frames = [np.frombuffer(memoryview(f), dtype=np.uint8) for f in frames]
        s = np.asarray(s, dtype="<f4")
        a = np.asarray(a, dtype="<f4")
        g = np.asarray(g, dtype="<f4").reshape(-1)
        if steps is None:
            steps = len(frames)
        if len(frames) != steps or steps < 1:
            raise ValueError("%s: trajectory %d has %d frames, the bundle's trajectories have %s"
                             % (path, len(goals), len(frames), steps))
        if s.shape != (steps, STATE_DIM) or a.shape != (steps, ACTION_DIM) or g.shape != (GOAL_DIM,):
            raise ValueError("%s: trajectory %d has states %s, actions %s, goal %s; expected (%d,%d), (%d,%d), (%d,)"
                             % (path, len(goals), s.shape, a.shape, g.shape, steps, STATE_DIM, steps, ACTION_DIM, GOAL_DIM))
        streams.extend(frames)
        states.append(s)
        actions.append(a)
        goals.append(g)
    n = len(goals)
    if n == 0:
        raise ValueError("%s: no trajectories to write" % path)
    offsets = np.zeros(n * steps + 1, dtype="<i8")
    np.cumsum([f.size for f in streams], out=offsets[1:])
    blob_bytes = int(offsets[-1])
    layout, size = section_layout(n, steps, blob_bytes)
    header = _HEADER.pack(MAGIC, VERSION, HEADER_BYTES, n, steps, STATE_DIM, ACTION_DIM, GOAL_DIM, 0, blob_bytes, 0)
    parts = {"offsets": [offsets], "states": states, "actions": actions, "goal": goals, "blob": streams}
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(header)
        for name in ("offsets", "states", "actions", "goal", "blob"):
            at, _ = layout[name]
            f.write(b"\0" * (at - f.tell()))
            for piece in parts[name]:
                f.write(np.ascontiguousarray(piece).tobytes())
        if f.tell() != size:
            raise AssertionError("%s: wrote %d bytes, laid out %d" % (path, f.tell(), size))
    os.replace(tmp, path)
    return n


def read_bundle(path):
    """Open and validate a bundle; returns a `Bundle` of memory-mapped views.  A truncated or inconsistent file raises
    ValueError naming the file; nothing outside a validated section is ever read."""
    def bad(why):
        return ValueError("%s is not a valid trajectory bundle: %s" % (path, why))

    size = os.path.getsize(path)
    if size < HEADER_BYTES:
        raise bad("%d bytes, shorter than the %d-byte header" % (size, HEADER_BYTES))
    with open(path, "rb") as f:
        head = f.read(HEADER_BYTES)
    magic, version, header_bytes, n, steps, sd, ad, gd, zero, blob_bytes, _ = _HEADER.unpack(head)
    if magic != MAGIC:
        raise bad("wrong magic %r" % magic)
    if version != VERSION:
        raise bad("version %d, this reader knows version %d" % (version, VERSION))
    if header_bytes != HEADER_BYTES or (sd, ad, gd) != (STATE_DIM, ACTION_DIM, GOAL_DIM):
        raise bad("header of %d bytes with widths %s, expected %d and %s"
                  % (header_bytes, (sd, ad, gd), HEADER_BYTES, (STATE_DIM, ACTION_DIM, GOAL_DIM)))
    if n < 1 or steps < 1 or blob_bytes < 0 or n * steps > size:          # (every frame has an 8-byte offset: n*T < size)
        raise bad("N = %d, T = %d, blob of %d bytes in a file of %d bytes" % (n, steps, blob_bytes, size))
    layout, want = section_layout(n, steps, blob_bytes)
    if want != size:
        raise bad("the header describes %d bytes, the file has %d" % (want, size))
    raw = np.memmap(path, dtype=np.uint8, mode="r")

    def view(name, dtype, shape):
        at, count = layout[name]
        return raw[at:at + count].view(dtype).reshape(shape)

    offsets = view("offsets", "<i8", (n * steps + 1,))
    if int(offsets[0]) != 0 or int(offsets[-1]) != blob_bytes:
        raise bad("frame offsets run from %d to %d, the blob has %d bytes" % (offsets[0], offsets[-1], blob_bytes))
    if bool((offsets[1:] < offsets[:-1]).any()):
        raise bad("frame offsets decrease at frame %d" % int(np.argmax(offsets[1:] < offsets[:-1])))
    return Bundle(path, n, steps, offsets, view("states", "<f4", (n, steps, STATE_DIM)),
                  view("actions", "<f4", (n, steps, ACTION_DIM)), view("goal", "<f4", (n, GOAL_DIM)),
                  view("blob", np.uint8, (blob_bytes,)))


def list_bundles(datadir):
    """The directory's entries (dot-files skipped) as paths, in sorted name order."""
    names = sorted(e for e in os.listdir(datadir) if not e.startswith("."))
    return [os.path.join(datadir, e) for e in names]


def is_bundle_dir(datadir):
    """True: every entry ends in .ndpt; False: none does (or not a directory); a mixture raises ValueError."""
    if not os.path.isdir(datadir):
        return False
    files = list_bundles(datadir)
    flags = [f.endswith(SUFFIX) for f in files]
    if files and all(flags):
        return True
    if any(flags):
        raise ValueError("%s mixes %s bundles with other files (%s): keep one kind per directory"
                         % (datadir, SUFFIX, os.path.basename(files[flags.index(False)])))
    return False


def open_dir(datadir):
    """Every bundle of the directory, opened, in sorted name order."""
    if not is_bundle_dir(datadir):
        raise ValueError("%s is not a directory of %s trajectory bundles" % (datadir, SUFFIX))
    return [read_bundle(f) for f in list_bundles(datadir)]


class BundleDataset(torch.utils.data.Dataset):
    """`PushDataset`'s output contract (utils/trajectory_loader.py) over a directory of bundles: (images, states [T',25],
    actions [T',4], goal [3]) with images the normalised floats [T',3,H,W], the decoded bytes [T',H,W,3] (raw_uint8) or
    the list of T' stored streams as bytes (raw_jpeg; `.mode == "jpeg"`).  Files in sorted name order, the reference's
    index arithmetic across them; a window that does not fit a file's T raises at construction."""

    def __init__(self, datadir, seq_start=0, seq_length=15, transform=None, raw_uint8=False, raw_jpeg=False):
        self.raw_uint8, self.raw_jpeg = bool(raw_uint8), bool(raw_jpeg)
        if self.raw_jpeg:
            self.mode = "jpeg"
        else:
            try:
                from PIL import Image  # noqa: F401
            except ImportError as e:  # pragma: no cover - depends on the image
                raise RuntimeError("BundleDataset decodes frames on the host with PIL, which is missing (%s); use "
                                   "raw_jpeg=True and decode on the device" % e)
        self.datadir, self.transform = datadir, transform
        self.seq_start, self.seq_length = int(seq_start), int(seq_length)
        self.bundles = open_dir(datadir)
        self.files = [b.path for b in self.bundles]
        for b in self.bundles:
            if self.seq_start < 0 or self.seq_length < 1 or self.seq_start + self.seq_length > b.steps:
                raise ValueError("%s holds trajectories of %d steps: seq_start %d + seq_length %d does not fit"
                                 % (b.path, b.steps, self.seq_start, self.seq_length))
        self.file_seq_cts = np.cumsum([b.n for b in self.bundles])
        self.total_seq_ct = int(self.file_seq_cts[-1])

    def __len__(self):
        return self.total_seq_ct

    def locate(self, index):
        """(bundle, trajectory within it) of dataset index `index` (utils/trajectory_loader.py:38-47)."""
        index = int(index)
        if not 0 <= index < self.total_seq_ct:
            raise IndexError("trajectory %d of %d" % (index, self.total_seq_ct))
        file_index = int(np.argmax(self.file_seq_cts > index))
        seq_index = index if file_index == 0 else index - int(self.file_seq_cts[file_index - 1])
        return self.bundles[file_index], seq_index

    def __getitem__(self, index):
        import io
        bundle, seq = self.locate(index)
        sl = slice(self.seq_start, self.seq_start + self.seq_length)
        raw = [bundle.stream(seq, t).tobytes() for t in range(sl.start, sl.stop)]
        if self.raw_jpeg:
            images = raw
        else:
            from PIL import Image

            from .utils.trajectory_loader import norm_frame
            frames = []
            for b in raw:
                img = Image.open(io.BytesIO(b))
                frames.append(torch.from_numpy(np.array(img, dtype=np.uint8)) if self.raw_uint8 else norm_frame(img))
            images = torch.stack(frames)
        states = torch.from_numpy(np.array(bundle.states[seq, sl]))
        actions = torch.from_numpy(np.array(bundle.actions[seq, sl]))
        goal = torch.from_numpy(np.array(bundle.goal[seq]))
        if self.transform:
            images = self.transform(images)
        return images, states, actions, goal


# ---------------------------------------------------------------------------------------------------- command line
def convert(src_dir, dst_dir):
    """Every HDF5 bundle of src_dir (the reference's layout) -> dst_dir/<same name>.ndpt; groups in sorted name order."""
    try:
        import h5py
    except ImportError as e:
        raise SystemExit("bundle convert needs the `h5py` package (to read the reference's HDF5 bundles), which this "
                         "package neither ships nor requires: %s" % e)
    written = []
    for name in sorted(e for e in os.listdir(src_dir) if not e.startswith(".")):
        with h5py.File(os.path.join(src_dir, name), "r") as h:
            def items():
                for key in sorted(h.keys()):
                    g = h[key]
                    frames = [bytes(b.tobytes() if hasattr(b, "tobytes") else b) for b in g["images"][:]]
                    yield frames, np.asarray(g["states"][:]), np.asarray(g["actions"][:]), np.asarray(g["goal"][:])
            dst = os.path.join(dst_dir, os.path.splitext(name)[0] + SUFFIX)
            write_bundle(dst, items())
        written.append(dst)
    return written


def synth(n, dst_dir, steps=8, seed=0, per_file=None):
    """n seeded synthetic trajectories (`SyntheticPushDataset(mode="jpeg")`) as trajectory_bundle_{:05d}.ndpt files of
    `per_file` trajectories each (default: one file)."""
    from .utils.trajectory_loader import SyntheticPushDataset
    n, per_file = int(n), int(per_file) if per_file else int(n)
    if n < 1 or per_file < 1 or steps < 1:
        raise ValueError("synth: N, --per-file and --steps must be positive")
    dataset = SyntheticPushDataset(n, seq_length=int(steps), mode="jpeg", seed=int(seed))
    os.makedirs(dst_dir, exist_ok=True)
    written = []
    for number, lo in enumerate(range(0, n, per_file), start=1):
        path = os.path.join(dst_dir, "trajectory_bundle_{:05d}{}".format(number, SUFFIX))
        write_bundle(path, ((f, s.numpy(), a.numpy(), g.numpy())
                            for f, s, a, g in (dataset[i] for i in range(lo, min(lo + per_file, n)))))
        written.append(path)
    return written


def info(path):
    """Lines describing a bundle file or every bundle of a directory."""
    bundles = open_dir(path) if os.path.isdir(path) else [read_bundle(path)]
    lines = []
    for b in bundles:
        lengths = np.diff(b.offsets)
        lines.append("%s: version %d, %d trajectories x %d steps, %d stream bytes (stream min %d, mean %.0f, max %d), "
                     "%d bytes in all" % (b.path, VERSION, b.n, b.steps, b.blob.size, lengths.min(), lengths.mean(),
                                          lengths.max(), os.path.getsize(b.path)))
    if len(bundles) > 1:
        lines.append("%d bundles, %d trajectories" % (len(bundles), sum(b.n for b in bundles)))
    return lines


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m ndivplanning_amd.bundle", description="Trajectory bundles (.ndpt).")
    sub = parser.add_subparsers(dest="command", required=True)
    p = sub.add_parser("convert", help="HDF5 bundles of the reference's layout -> .ndpt (needs h5py)")
    p.add_argument("src_dir")
    p.add_argument("dst_dir")
    p = sub.add_parser("synth", help="seeded synthetic bundles")
    p.add_argument("n", type=int)
    p.add_argument("dst_dir")
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--per-file", type=int, default=None)
    p = sub.add_parser("info", help="describe a bundle file or directory")
    p.add_argument("path")
    args = parser.parse_args(argv)
    if args.command == "convert":
        os.makedirs(args.dst_dir, exist_ok=True)
        for path in convert(args.src_dir, args.dst_dir):
            print(path)
    elif args.command == "synth":
        for path in synth(args.n, args.dst_dir, steps=args.steps, seed=args.seed, per_file=args.per_file):
            print(path)
    else:
        try:
            print("\n".join(info(args.path)))
        except ValueError as e:
            raise SystemExit(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main())
