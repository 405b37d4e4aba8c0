"""The HDF5 side of the loader without h5py: a dict-backed stand-in for the part of the `h5py.File` mapping protocol the
project uses (len, keys, [] on files, groups and datasets; `with`) is installed as sys.modules["h5py"].  It drives the
existing HDF5 `PushDataset` -- the reference's index arithmetic at the file boundary, in all three image modes -- then
`bundle convert` over the same files, and checks that the converted directory read through `BundleDataset` equals the
stand-in read through `PushDataset`, item by item.  The generator's writer choice is driven as far as it goes without gym.
What stays unpinned is only the real h5py library behind the same calls."""
import io
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

from ndivplanning_amd import bundle
from ndivplanning_amd import generate_trajectories as GT
from ndivplanning_amd.utils import trajectory_loader as TL

FILES, PER_FILE, STEPS = 2, 3, 5


class _Dataset:
    """h5py.Dataset as the project reads it: slicing gives an array (of bytes objects for `images`)."""

    def __init__(self, value):
        self.value = value

    def __getitem__(self, key):
        return self.value[key]

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self.value, dtype=dtype)


class _Group(dict):
    def __getitem__(self, key):
        v = dict.__getitem__(self, key)
        return v if isinstance(v, _Group) else _Dataset(v)


class _File(_Group):
    """h5py.File(path, "r"): the pickled {group: {dataset: array}} of `path`."""

    def __init__(self, path, mode="r"):
        assert mode == "r"
        with open(path, "rb") as f:
            super().__init__({k: _Group(v) for k, v in pickle.load(f).items()})

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _standin():
    mod = types.ModuleType("h5py")
    mod.File = _File
    return mod


@pytest.fixture(scope="module")
def h5dir(tmp_path_factory):
    """FILES files of PER_FILE groups trajectory_{:05d}; returns (directory, {file name: [trajectory tuples]})."""
    root = tmp_path_factory.mktemp("h5")
    gen = torch.Generator().manual_seed(31)
    content = {}
    for f in range(FILES):
        name = "trajectory_bundle_%05d.h5" % (f + 1)
        groups, items = {}, []
        for ix in range(PER_FILE):
            frames = np.empty(STEPS, dtype=object)
            frames[:] = [TL.encode_jpeg(TL.synthetic_scene(gen)) for _ in range(STEPS)]
            item = (frames, torch.randn(STEPS, 25, generator=gen).numpy(), torch.randn(STEPS, 4, generator=gen).numpy(),
                    torch.randn(3, generator=gen).numpy())
            groups["trajectory_%05d" % ix] = dict(zip(("images", "states", "actions", "goal"), item))
            items.append(item)
        with open(str(root / name), "wb") as out:
            pickle.dump(groups, out)
        content[name] = items
    return str(root), content


def _decode(stream):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(stream)), dtype=np.uint8)


def _expected(ds, content, index):
    """The trajectory that dataset index `index` names, by the reference's arithmetic over ds.files in ds's own order."""
    for path in ds.files:
        items = content[os.path.basename(path)]
        if index < len(items):
            return items[index]
        index -= len(items)
    raise IndexError(index)


def test_hdf5_pushdataset_index_arithmetic_in_all_three_modes(h5dir, monkeypatch):
    root, content = h5dir
    monkeypatch.setitem(sys.modules, "h5py", _standin())
    jpeg = TL.PushDataset(root, seq_start=1, seq_length=3, raw_jpeg=True)
    u8 = TL.PushDataset(root, seq_start=1, seq_length=3, raw_uint8=True)
    f32 = TL.PushDataset(root, seq_start=1, seq_length=3)
    assert jpeg._bundles is None and jpeg.mode == "jpeg" and not hasattr(u8, "mode")
    assert len(jpeg) == len(u8) == len(f32) == FILES * PER_FILE and sorted(jpeg.files) == sorted(os.path.join(root, n) for n in content)
    for index in range(FILES * PER_FILE):                              # 2 | 3 is the file boundary
        frames, states, actions, goal = _expected(jpeg, content, index)
        got = jpeg[index]
        assert got[0] == list(frames[1:4]) and all(isinstance(s, bytes) for s in got[0])
        assert torch.equal(got[1], torch.from_numpy(states[1:4])) and torch.equal(got[2], torch.from_numpy(actions[1:4]))
        assert torch.equal(got[3], torch.from_numpy(goal))
        decoded = np.stack([_decode(s) for s in frames[1:4]])
        assert np.array_equal(u8[index][0].numpy(), decoded)
        assert torch.equal(f32[index][0], torch.stack([TL.norm_frame(d) for d in decoded]))


def test_convert_and_the_converted_directory_equals_the_source(h5dir, monkeypatch, tmp_path, capsys):
    root, content = h5dir
    monkeypatch.setitem(sys.modules, "h5py", _standin())
    dst = str(tmp_path / "ndpt")
    assert bundle.main(["convert", root, dst]) == 0
    printed = capsys.readouterr().out.split()
    assert [os.path.basename(p) for p in printed] == ["trajectory_bundle_00001.ndpt", "trajectory_bundle_00002.ndpt"]
    source = TL.PushDataset(root, seq_length=STEPS, raw_jpeg=True)
    source_items = [source[i] for i in range(len(source))]
    monkeypatch.setitem(sys.modules, "h5py", None)                     # the converted directory needs none
    converted = bundle.BundleDataset(dst, seq_length=STEPS, raw_jpeg=True)
    assert len(converted) == len(source) == FILES * PER_FILE
    # BundleDataset takes the files in sorted order; the HDF5 loader in the directory's own order
    order = [os.path.basename(f) for f in source.files]
    starts = {name: sum(len(content[n]) for n in order[:order.index(name)]) for name in order}
    at = 0
    for name in sorted(content):
        for ix in range(len(content[name])):
            got, want = converted[at], source_items[starts[name] + ix]
            assert got[0] == want[0]
            assert all(torch.equal(g, w) and g.dtype == w.dtype for g, w in zip(got[1:], want[1:]))
            at += 1
    through_push = TL.PushDataset(dst, seq_length=STEPS, raw_uint8=True)  # and PushDataset reads it with no h5py
    assert np.array_equal(through_push[0][0].numpy(), np.stack([_decode(s) for s in content[sorted(content)[0]][0][0]]))


def test_convert_reports_a_missing_h5py(h5dir, monkeypatch, tmp_path):
    monkeypatch.setitem(sys.modules, "h5py", None)
    with pytest.raises(SystemExit, match="h5py"):
        bundle.main(["convert", h5dir[0], str(tmp_path / "out")])


def test_the_generators_ndpt_writer(monkeypatch, tmp_path, capsys):
    monkeypatch.setitem(sys.modules, "h5py", None)
    assert GT._bundle_format(["--num_files", "2", "--bundle-format", "ndpt"]) == "ndpt"
    assert GT._bundle_format(["--num_files", "2"]) == "h5"
    (tmp_path / "model.pt").write_bytes(b"")
    common = ["--pretrained_model_path", str(tmp_path / "model.pt")]
    (tmp_path / "out").mkdir()
    tmp_path = tmp_path / "out"
    args = GT._parser().parse_args(common + ["--outdir", str(tmp_path), "--bundle-format", "ndpt", "--num_files", "2",
                                    "--num_trajectory_per_file", "3", "--filename_start_idx", "4", "--trajectory-length", "4"])
    assert args.bundle_format == "ndpt" and GT._parser().parse_args(common + ["--outdir", str(tmp_path)]).bundle_format == "h5"
    rng = np.random.RandomState(3)
    made = []

    def make_trajectory():                                             # generate_trajectory's return: float64 tables
        if len(made) == 1 and not make_trajectory.failed:
            make_trajectory.failed = True
            raise RuntimeError("the simulator fell over")
        item = ([bytes(rng.randint(0, 256, rng.randint(1, 50)).astype(np.uint8)) for _ in range(4)], rng.randn(4, 25),
                rng.randn(4, 4), rng.randn(3))
        made.append(item)
        return item
    make_trajectory.failed = False
    GT.write_bundles(args, make_trajectory)                            # no h5py.File given, none needed
    assert "trajectory 00001 of bundle 00004 was not written: the simulator fell over" in capsys.readouterr().out
    assert sorted(os.listdir(str(tmp_path))) == ["trajectory_bundle_00004.ndpt", "trajectory_bundle_00005.ndpt"]
    first, second = (bundle.read_bundle(str(tmp_path / ("trajectory_bundle_%05d.ndpt" % k))) for k in (4, 5))
    assert (first.n, second.n, first.steps) == (2, 3, 4)              # the failed trajectory is left out
    for b, items in ((first, made[:2]), (second, made[2:])):
        for i, (frames, states, actions, goal) in enumerate(items):
            assert [b.stream(i, t).tobytes() for t in range(4)] == frames
            assert np.array_equal(b.states[i], states.astype(np.float32)) and np.array_equal(b.actions[i], actions.astype(np.float32))
            assert np.array_equal(b.goal[i], goal.astype(np.float32))
    # main() with ndpt never asks for h5py: the first thing it misses is gym
    monkeypatch.setitem(sys.modules, "gym", None)
    with pytest.raises(SystemExit, match="`gym` package"):
        GT.main(["--bundle-format", "ndpt", "--outdir", str(tmp_path)])
