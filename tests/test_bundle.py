"""The project's own trajectory bundles (ndivplanning_amd/bundle.py) on the host: the file layout
as documented, write -> read -> BundleDataset round trips in all three image modes, the reference's index arithmetic at the
file boundary, PushDataset's dispatch with h5py absent, every way a file can be corrupt, and the command lines."""
import io
import os
import struct
import sys

import numpy as np
import pytest
import torch

from ndivplanning_amd import bundle
from ndivplanning_amd.utils import trajectory_loader as TL

FILES, PER_FILE, STEPS = 2, 3, 5


def _trajectories():
    """FILES x PER_FILE trajectories of STEPS PIL-encoded synthetic scenes."""
    gen = torch.Generator().manual_seed(21)
    out = []
    for _ in range(FILES * PER_FILE):
        frames = [TL.encode_jpeg(TL.synthetic_scene(gen)) for _ in range(STEPS)]
        out.append((frames, torch.randn(STEPS, 25, generator=gen).numpy(), torch.randn(STEPS, 4, generator=gen).numpy(),
                    torch.randn(3, generator=gen).numpy()))
    return out


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    root = tmp_path_factory.mktemp("bundles")
    items = _trajectories()
    for f in range(FILES):                                             # written out of name order: the reader sorts
        part = items[(FILES - 1 - f) * PER_FILE:(FILES - f) * PER_FILE]
        assert bundle.write_bundle(str(root / ("part_%05d.ndpt" % (FILES - f))), part) == PER_FILE
    return str(root), items


def _decode(stream):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(stream)), dtype=np.uint8)


def test_the_layout_is_the_documented_one(written):
    root, items = written
    path = os.path.join(root, "part_00001.ndpt")
    raw = open(path, "rb").read()
    magic, version, header_bytes, n, steps, sd, ad, gd, z0, blob_bytes, z1 = struct.unpack("<8sIIqqIIIIqq", raw[:64])
    assert (magic, version, header_bytes, n, steps, sd, ad, gd, z0, z1) == (b"NDPTRAJ\0", 1, 64, PER_FILE, STEPS, 25, 4, 3, 0, 0)
    streams = [s for item in items[:PER_FILE] for s in item[0]]
    assert blob_bytes == sum(len(s) for s in streams)
    layout, size = bundle.section_layout(n, steps, blob_bytes)
    assert size == len(raw)
    at = 64
    for name, count in (("offsets", 8 * (n * steps + 1)), ("states", 4 * n * steps * 25), ("actions", 4 * n * steps * 4),
                        ("goal", 4 * n * 3), ("blob", blob_bytes)):
        at = (at + 63) // 64 * 64                                      # every section starts at a multiple of 64
        assert layout[name] == (at, count)
        at += count
    offsets = np.frombuffer(raw, "<i8", n * steps + 1, layout["offsets"][0])
    assert offsets[0] == 0 and offsets[-1] == blob_bytes
    assert np.array_equal(np.diff(offsets), [len(s) for s in streams])
    assert raw[layout["blob"][0]:] == b"".join(streams)
    assert np.array_equal(np.frombuffer(raw, "<f4", n * steps * 25, layout["states"][0]).reshape(n, steps, 25),
                          np.stack([i[1] for i in items[:PER_FILE]]))
    assert np.array_equal(np.frombuffer(raw, "<f4", n * 3, layout["goal"][0]).reshape(n, 3), np.stack([i[3] for i in items[:PER_FILE]]))


def test_read_bundle_returns_views_of_the_file(written):
    root, items = written
    b = bundle.read_bundle(os.path.join(root, "part_00002.ndpt"))
    assert (b.n, b.steps, len(b)) == (PER_FILE, STEPS, PER_FILE)
    assert isinstance(b.blob.base, np.memmap) or isinstance(b.blob, np.memmap)
    for i, item in enumerate(items[PER_FILE:]):
        assert [b.stream(i, t).tobytes() for t in range(STEPS)] == item[0]
        assert np.array_equal(b.states[i], item[1]) and np.array_equal(b.actions[i], item[2]) and np.array_equal(b.goal[i], item[3])
    assert b.max_stream_bytes() == max(len(s) for item in items[PER_FILE:] for s in item[0])


def test_dataset_round_trip_in_all_three_modes(written):
    root, items = written
    jpeg = bundle.BundleDataset(root, seq_length=STEPS, raw_jpeg=True)
    u8 = bundle.BundleDataset(root, seq_length=STEPS, raw_uint8=True)
    f32 = bundle.BundleDataset(root, seq_length=STEPS)
    assert len(jpeg) == len(u8) == len(f32) == FILES * PER_FILE
    assert jpeg.mode == "jpeg" and not hasattr(u8, "mode") and jpeg.seq_length == STEPS
    assert [os.path.basename(f) for f in jpeg.files] == ["part_00001.ndpt", "part_00002.ndpt"]       # sorted
    for index in (0, 2, 3, 5):                                         # both sides of the file boundary, and the last
        streams, states, actions, goal = jpeg[index]
        want = items[index]
        assert streams == want[0] and all(isinstance(s, bytes) for s in streams)
        for got, w in ((states, want[1]), (actions, want[2]), (goal, want[3])):
            assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(w))
        decoded = np.stack([_decode(s) for s in want[0]])
        frames = u8[index][0]
        assert frames.dtype == torch.uint8 and tuple(frames.shape) == (STEPS, 128, 128, 3)
        assert np.array_equal(frames.numpy(), decoded)
        images = f32[index][0]
        assert images.dtype == torch.float32 and tuple(images.shape) == (STEPS, 3, 128, 128)
        assert torch.equal(images, torch.stack([TL.norm_frame(d) for d in decoded]))
    with pytest.raises(IndexError):
        jpeg[FILES * PER_FILE]


def test_seq_start_and_seq_length_slice_the_trajectory(written):
    root, items = written
    ds = bundle.BundleDataset(root, seq_start=1, seq_length=3, raw_jpeg=True, transform=lambda s: list(reversed(s)))
    streams, states, actions, goal = ds[4]
    assert streams == list(reversed(items[4][0][1:4]))                 # (the transform sees the images only)
    assert torch.equal(states, torch.from_numpy(items[4][1][1:4])) and torch.equal(actions, torch.from_numpy(items[4][2][1:4]))
    assert torch.equal(goal, torch.from_numpy(items[4][3]))
    for seq_start, seq_length in ((0, STEPS + 1), (3, 3), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match="part_00001.ndpt"):
            bundle.BundleDataset(root, seq_start=seq_start, seq_length=seq_length, raw_jpeg=True)


def test_pushdataset_dispatches_to_the_bundle_reader_without_h5py(written, monkeypatch, tmp_path):
    root, items = written
    monkeypatch.setitem(sys.modules, "h5py", None)                     # `import h5py` raises ImportError
    with pytest.raises(ImportError):
        import h5py  # noqa: F401
    ds = TL.PushDataset(root, seq_length=4, raw_jpeg=True)
    assert len(ds) == FILES * PER_FILE and ds.mode == "jpeg" and ds.seq_length == 4 and ds.raw_jpeg
    assert ds[3][0] == items[3][0][:4]
    u8 = TL.PushDataset(root, seq_start=2, seq_length=2, raw_uint8=True)
    assert not hasattr(u8, "mode") and np.array_equal(u8[1][0].numpy(), np.stack([_decode(s) for s in items[1][0][2:4]]))
    # the HDF5 path is still what an HDF5 directory gets: without h5py, its error
    other = tmp_path / "h5"
    other.mkdir()
    (other / "trajectory_bundle_00001.h5").write_bytes(b"x")
    with pytest.raises(RuntimeError, match="h5py"):
        TL.PushDataset(str(other))


def test_a_directory_that_mixes_file_types_raises(written, tmp_path):
    root, _ = written
    mixed = tmp_path / "mixed"
    mixed.mkdir()
    (mixed / "a.ndpt").write_bytes(open(os.path.join(root, "part_00001.ndpt"), "rb").read())
    (mixed / "b.h5").write_bytes(b"x")
    with pytest.raises(ValueError, match="mixes"):
        TL.PushDataset(str(mixed))
    with pytest.raises(ValueError, match="mixes"):
        bundle.BundleDataset(str(mixed))
    (mixed / ".hidden").write_bytes(b"x")                              # dot-files are not entries
    os.remove(str(mixed / "b.h5"))
    assert len(bundle.BundleDataset(str(mixed), seq_length=STEPS, raw_jpeg=True)) == PER_FILE


def _corrupt(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(data)
    with pytest.raises(ValueError, match=name):
        bundle.read_bundle(str(path))


def test_corrupt_files_raise_valueerror_naming_the_file(written, tmp_path):
    root, _ = written
    raw = open(os.path.join(root, "part_00001.ndpt"), "rb").read()
    n, steps, blob_bytes = PER_FILE, STEPS, struct.unpack_from("<q", raw, 48)[0]
    layout, size = bundle.section_layout(n, steps, blob_bytes)
    boundaries = {0, 64, size}
    for at, count in layout.values():
        boundaries |= {at, at + count}
    cuts = sorted({b + d for b in boundaries for d in (-1, 0, 1) if 0 <= b + d} - {size})
    assert size - 1 in cuts and size + 1 in cuts and len(cuts) >= 25
    for cut in cuts:                                                   # truncated (or, past the end, padded)
        _corrupt(tmp_path, "cut_%d.ndpt" % cut, raw[:cut] + b"\0" * max(0, cut - size))

    def patched(at, fmt, value):
        data = bytearray(raw)
        struct.pack_into(fmt, data, at, value)
        return bytes(data)

    off = layout["offsets"][0]
    third, fourth = struct.unpack_from("<qq", raw, off + 8 * 3)
    assert fourth > third
    _corrupt(tmp_path, "decreasing.ndpt", patched(off + 8 * 3, "<q", fourth + 1))
    _corrupt(tmp_path, "last_offset.ndpt", patched(off + 8 * n * steps, "<q", blob_bytes - 1))
    _corrupt(tmp_path, "first_offset.ndpt", patched(off, "<q", 1))
    _corrupt(tmp_path, "magic.ndpt", b"NDPTRAJ1" + raw[8:])
    _corrupt(tmp_path, "version.ndpt", patched(8, "<I", 2))
    _corrupt(tmp_path, "blob_bytes.ndpt", patched(48, "<q", blob_bytes + 64))
    _corrupt(tmp_path, "count.ndpt", patched(16, "<q", n + 1))
    _corrupt(tmp_path, "huge.ndpt", patched(16, "<q", 2 ** 62))
    _corrupt(tmp_path, "negative.ndpt", patched(24, "<q", -steps))
    good = tmp_path / "good.ndpt"
    good.write_bytes(raw)
    assert bundle.read_bundle(str(good)).n == n


def test_write_bundle_rejects_inconsistent_trajectories(written, tmp_path):
    _, items = written
    frames, states, actions, goal = items[0]
    for bad in ((frames[:-1], states, actions, goal), (frames, states[:-1], actions, goal), (frames, states, actions[:, :3], goal),
                (frames, states, actions, goal[:2])):
        with pytest.raises(ValueError, match="bad.ndpt"):
            bundle.write_bundle(str(tmp_path / "bad.ndpt"), [items[1], bad])
    with pytest.raises(ValueError, match="no trajectories"):
        bundle.write_bundle(str(tmp_path / "bad.ndpt"), [])
    assert not os.path.exists(str(tmp_path / "bad.ndpt"))
    # float64 tables, as generate_trajectory returns them, are stored as float32
    bundle.write_bundle(str(tmp_path / "f64.ndpt"), [(frames, states.astype(np.float64), actions.astype(np.float64), list(goal))])
    assert np.array_equal(bundle.read_bundle(str(tmp_path / "f64.ndpt")).states[0], states)


def test_synth_and_info_command_lines(tmp_path, capsys):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for dst in (a, b):
        assert bundle.main(["synth", "5", dst, "--steps", "3", "--seed", "7", "--per-file", "2"]) == 0
    names = sorted(os.listdir(a))
    assert names == ["trajectory_bundle_00001.ndpt", "trajectory_bundle_00002.ndpt", "trajectory_bundle_00003.ndpt"]
    assert capsys.readouterr().out.split() == [os.path.join(d, n) for d in (a, b) for n in names]
    for n in names:                                                    # one seed, identical files
        assert open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read()
    assert bundle.main(["synth", "5", str(tmp_path / "c"), "--steps", "3", "--seed", "8", "--per-file", "2"]) == 0
    assert open(os.path.join(a, names[0]), "rb").read() != open(str(tmp_path / "c" / names[0]), "rb").read()
    capsys.readouterr()
    # what synth wrote is SyntheticPushDataset(mode="jpeg") of that seed
    ds, want = bundle.BundleDataset(a, seq_length=3, raw_jpeg=True), TL.SyntheticPushDataset(5, seq_length=3, mode="jpeg", seed=7)
    assert len(ds) == 5
    for i in range(5):
        assert ds[i][0] == want[i][0] and all(torch.equal(g, w) for g, w in zip(ds[i][1:], want[i][1:]))
    assert bundle.main(["info", os.path.join(a, names[2])]) == 0
    out = capsys.readouterr().out
    assert "1 trajectories x 3 steps" in out and names[2] in out
    assert bundle.main(["info", a]) == 0
    out = capsys.readouterr().out
    assert "3 bundles, 5 trajectories" in out and out.count("2 trajectories x 3 steps") == 2
    (tmp_path / "broken.ndpt").write_bytes(b"nothing")
    with pytest.raises(SystemExit, match="broken.ndpt"):
        bundle.main(["info", str(tmp_path / "broken.ndpt")])
