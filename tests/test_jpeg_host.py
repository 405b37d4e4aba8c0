"""CPU tests of the JPEG input path (ndivplanning_amd/jpeg.py, the loader's raw_jpeg / jpeg modes, the C ABI's argument
checks).  The decode itself runs on the GPU: tests/test_gpu_jpeg.py."""
import ctypes
import io
import sys
import types

import numpy as np
import pytest
import torch

from conftest import load_golden


def _streams():
    g = load_golden("jpeg_case")
    o = g["offsets"]
    return g, [g["streams"][o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]


def test_fixture_agrees_with_this_machine_s_pil():
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this PIL is not built on libjpeg-turbo")
    g, streams = _streams()
    frames = np.cumsum(g["frames_dx"], axis=2, dtype=np.uint8)
    assert (g["status"] == 0).sum() >= 8 * 3 + 4 and len(streams) == len(g["names"])
    for i, s in enumerate(streams):
        if g["frame_of"][i] >= 0:
            assert np.array_equal(np.array(Image.open(io.BytesIO(s))), frames[g["frame_of"][i]]), g["names"][i]


def test_pack_jpegs_offsets_and_pinning():
    from ndivplanning_amd.jpeg import pack_jpegs
    streams = [b"\xff\xd8abc", b"", b"xyz\xff\xd9", bytearray(b"12")]
    buf, off = pack_jpegs(streams, pin=False)
    assert off.dtype == torch.int64 and off.tolist() == [0, 5, 5, 10, 12]
    assert buf.dtype == torch.uint8 and bytes(buf.numpy()) == b"".join(bytes(s) for s in streams)
    assert not buf.is_pinned() and not off.is_pinned()
    buf, off = pack_jpegs(streams)                          # pinned where a GPU is present
    assert buf.is_pinned() == torch.cuda.is_available() and off.is_pinned() == torch.cuda.is_available()
    with pytest.raises(ValueError):
        pack_jpegs([])


def test_collate_jpeg_shapes_and_slices():
    from ndivplanning_amd.jpeg import JpegFrames, collate_jpeg
    items = [([bytes([b, t]) * (t + 1) for t in range(3)], torch.full((3, 25), float(b)), torch.zeros(3, 4), torch.zeros(3))
             for b in range(4)]
    frames, states, actions, goal = collate_jpeg(items)
    assert isinstance(frames, JpegFrames) and frames.shape == (4, 3, 128, 128, 3) and len(frames) == 4
    assert frames.offsets.tolist() == [0, 2, 6, 12, 14, 18, 24, 26, 30, 36, 38, 42, 48]
    assert states.shape == (4, 3, 25) and actions.shape == (4, 3, 4) and goal.shape == (4, 3)
    part = frames[1:3]
    assert part.shape[0] == 2 and part.offsets.tolist() == [12, 14, 18, 24, 26, 30, 36]
    assert bytes(part.buffer[part.offsets[0]:part.offsets[1]].numpy()) == bytes([1, 0])
    with pytest.raises(ValueError):
        collate_jpeg([([b"a"], torch.zeros(1)), ([b"a", b"b"], torch.zeros(1))])


def test_synthetic_jpeg_dataset_is_deterministic_per_seed():
    pytest.importorskip("PIL.Image")
    from ndivplanning_amd.utils.trajectory_loader import SyntheticPushDataset
    a = SyntheticPushDataset(3, seq_length=2, mode="jpeg", seed=4)
    b = SyntheticPushDataset(3, seq_length=2, mode="jpeg", seed=4)
    c = SyntheticPushDataset(3, seq_length=2, mode="jpeg", seed=5)
    fa, sa, aa, ga = a[1]
    fb, sb, ab, gb = b[1]
    assert fa == fb and torch.equal(sa, sb) and torch.equal(aa, ab) and torch.equal(ga, gb)
    assert fa != c[1][0] and fa != a[2][0]
    assert len(fa) == 2 and all(f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9" for f in fa)
    from PIL import Image
    img = Image.open(io.BytesIO(fa[0]))
    assert img.size == (128, 128) and img.mode == "RGB"
    assert a.mode == "jpeg" and sa.shape == (2, 25) and aa.shape == (2, 4)


class _StubSeq(dict):
    pass


def _stub_h5py(files):
    mod = types.ModuleType("h5py")

    class File:
        def __init__(self, path, mode="r"):
            self.data = files[path]

        def __enter__(self):
            return self.data

        def __exit__(self, *a):
            return False
    mod.File = File
    return mod


def test_jpeg_datasets_of_the_scripts():
    pytest.importorskip("PIL.Image")
    from ndivplanning_amd import evaluation, train_autoencoder, train_gan
    from ndivplanning_amd.jpeg import is_jpeg, loader_kwargs
    from ndivplanning_amd.utils.file import AttrDict
    ds = evaluation.make_eval_dataset(AttrDict({"evaluation_data_path": "synthetic:3:jpeg", "trajectory_length": 4,
                                                "random_seed": 1}))
    assert is_jpeg(ds) and len(ds[0][0]) == 4 and "collate_fn" in loader_kwargs(ds)
    assert is_jpeg(train_autoencoder.make_dataset("synthetic:2:jpeg"))
    assert is_jpeg(train_gan.make_dataset(AttrDict({"train_data_path": "synthetic:2:jpeg", "trajectory_length": 3,
                                                     "random_seed": 0})))
    assert loader_kwargs(train_autoencoder.make_dataset("synthetic:2:images")) == {}


def test_push_dataset_raw_jpeg_returns_the_stored_bytes_unchanged(tmp_path, monkeypatch):
    from ndivplanning_amd.utils import trajectory_loader as TL
    _, streams = _streams()
    path = str(tmp_path / "a.hdf5")
    open(path, "wb").close()
    seqs = {}
    for k in range(2):
        frames = streams[4 * k:4 * k + 4]
        seqs["trajectory_{:05d}".format(k)] = {
            "images": np.array(frames, dtype=object),
            "states": np.full((4, 25), k, np.float32), "actions": np.zeros((4, 4), np.float32),
            "goal": np.zeros(3, np.float32)}
    monkeypatch.setitem(sys.modules, "h5py", _stub_h5py({path: seqs}))
    monkeypatch.setitem(sys.modules, "PIL", None)           # raw_jpeg must not need PIL
    monkeypatch.setitem(sys.modules, "PIL.Image", None)
    ds = TL.PushDataset(str(tmp_path), seq_length=3, raw_jpeg=True)
    assert len(ds) == 2 and ds.mode == "jpeg"
    images, states, actions, goal = ds[1]
    assert images == streams[4:7] and all(isinstance(b, bytes) for b in images)
    assert states.shape == (3, 25) and float(states[0, 0]) == 1.0
    with pytest.raises(RuntimeError):
        TL.PushDataset(str(tmp_path), seq_length=3)              # the decoding dataset still needs PIL


@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


def test_jpeg_symbols_are_exported(lib):
    from ndivplanning_amd import _capi
    raw = ctypes.CDLL(lib._name)
    for name in ("ndp_jpeg_workspace_bytes", "ndp_jpeg_decode_u8"):
        assert hasattr(raw, name) and name in _capi.SIGNATURES


def test_decode_entry_rejects_bad_arguments_without_a_gpu(lib):
    need = lib.ndp_jpeg_workspace_bytes(4, 40000)
    assert need > 4 * 40000 // 4 and lib.ndp_jpeg_workspace_bytes(4, 80000) > need
    assert lib.ndp_jpeg_workspace_bytes(0, 100) == 0 and lib.ndp_jpeg_workspace_bytes(-1, 100) == 0
    assert lib.ndp_jpeg_workspace_bytes(4, -1) == 0 and lib.ndp_jpeg_workspace_bytes(1 << 20, 100) == 0
    fake = ctypes.c_void_p(1 << 12)                         # never dereferenced: every call fails its checks first
    ws = ctypes.c_void_p(1 << 20)
    assert lib.ndp_jpeg_decode_u8(None, fake, 4, fake, fake, ws, need, None) == 1
    assert b"null" in lib.ndp_last_error()
    assert lib.ndp_jpeg_decode_u8(fake, fake, 4, fake, None, ws, need, None) == 1
    assert lib.ndp_jpeg_decode_u8(fake, fake, 0, fake, fake, ws, need, None) == 1
    assert lib.ndp_jpeg_decode_u8(fake, fake, -3, fake, fake, ws, need, None) == 1
    assert b"count" in lib.ndp_last_error()
    small = lib.ndp_jpeg_workspace_bytes(4, 0) - 1
    assert lib.ndp_jpeg_decode_u8(fake, fake, 4, fake, fake, ws, small, None) == 1
    assert b"workspace" in lib.ndp_last_error()
    assert lib.ndp_jpeg_decode_u8(fake, fake, 4, fake, fake, ctypes.c_void_p((1 << 20) + 16), need, None) == 1
    assert b"aligned" in lib.ndp_last_error()
