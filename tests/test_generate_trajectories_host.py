"""CPU-only: the generate_trajectories drop-in imports and reports without gym / h5py, refuses other image shapes, and
`write_trajectory` writes the reference's HDF5 layout (generate_trajectories.py:275-324) -- checked against a dict-backed
stand-in for h5py that records names, dtypes, attributes and compression options, through which PushDataset(raw_jpeg=True)
reads the same trajectories back.  No GPU involved (the trajectories themselves: tests/test_gpu_generate_trajectories.py)."""
import sys
import types

import numpy as np
import pytest


class _Dataset:
    def __init__(self, name, shape, dtype, data, options):
        self.name, self.options, self.attrs = name, options, {}
        if dtype is None and all(isinstance(b, bytes) for b in data):
            self.data = np.array(list(data), dtype=object)          # h5py: variable-length byte strings
            self.dtype = "bytes"
        else:
            self.data = np.asarray(data, dtype=dtype)
            self.dtype = str(self.data.dtype)
        assert self.data.shape == tuple(shape), (name, self.data.shape, shape)

    def __getitem__(self, key):
        return self.data[key]

    def __array__(self, dtype=None, copy=None):
        return self.data if dtype is None else self.data.astype(dtype)


class _Group(dict):
    def create_group(self, name):
        assert name not in self
        self[name] = _Group()
        return self[name]

    def create_dataset(self, name, shape=None, dtype=None, data=None, **options):
        assert name not in self
        self[name] = _Dataset(name, shape, dtype, data, options)
        return self[name]


def _stub_h5py(files):
    """h5py.File over `files` {path: _Group}: "w" makes the group, "r" returns it."""
    mod = types.ModuleType("h5py")

    class File:
        def __init__(self, path, mode="r"):
            if mode == "w":
                files[path] = _Group()
            self.data = files[path]

        def __enter__(self):
            return self.data

        def __exit__(self, *a):
            return False
    mod.File = File
    return mod


def test_root_module_imports_without_gym_or_h5py(monkeypatch):
    import importlib
    for name in ("gym", "h5py", "hindsight_experience_replay"):
        monkeypatch.setitem(sys.modules, name, None)
    import generate_trajectories as root
    from ndivplanning_amd import generate_trajectories as G
    G = importlib.reload(G)                      # the module's top level runs again, in the same module object
    root = importlib.reload(root)
    assert sorted(n for n in vars(root) if not n.startswith("_")) == ["generate_trajectory", "main", "process_inputs", "render",
                                                                       "write_trajectory"]
    for name in ("process_inputs", "render", "generate_trajectory", "write_trajectory", "main"):
        assert getattr(root, name) is getattr(G, name)
    assert G.o_mean is None and G.o_std is None and G.g_mean is None and G.g_std is None


@pytest.mark.parametrize("missing", ["gym", "h5py"])
def test_main_says_plainly_what_is_missing(monkeypatch, missing):
    from ndivplanning_amd import generate_trajectories as G
    for name in ("gym", "h5py"):
        monkeypatch.setitem(sys.modules, name, None if name == missing else types.ModuleType(name))
    with pytest.raises(SystemExit) as e:
        G.main([])
    assert "needs the `%s` package" % missing in str(e.value) and "generate_trajectory(env" in str(e.value)


def test_other_image_shapes_raise(tmp_path):
    from ndivplanning_amd import generate_trajectories as G
    args = types.SimpleNamespace(image_shape=(500, 500), simplify_task=False, goal_inline=False, trajectory_length=2,
                                 clip_obs=200, clip_range=5, normalizer=(0, 1, 0, 1))
    with pytest.raises(ValueError, match="500"):
        G.generate_trajectory(object(), None, args)           # before the environment is touched
    model = tmp_path / "model.pt"
    model.write_bytes(b"")
    common = ["--pretrained_model_path", str(model), "--outdir", str(tmp_path)]
    parsed = G._parser().parse_args(common)
    assert tuple(parsed.image_shape) == (128, 128) and parsed.trajectory_length == 20 and parsed.simplify_task is False
    G._check_image_shape(parsed)
    parsed = G._parser().parse_args(common + ["--image-shape", "500", "500", "--simplify-task"])
    assert parsed.simplify_task is True
    with pytest.raises(ValueError, match="not supported"):
        G._check_image_shape(parsed)


def test_process_inputs_is_the_reference_s():
    import torch
    from ndivplanning_amd import generate_trajectories as G
    args = types.SimpleNamespace(clip_obs=2.0, clip_range=1.5)
    out = G.process_inputs(np.array([5.0, -5.0, 0.5]), np.array([1.0]), np.array([0.5, 0.0, 0.0]), np.array([1.0, 1.0, 0.25]),
                           np.array([0.0]), np.array([2.0]), args)
    assert out.dtype == torch.float32 and out.tolist() == [1.5, -1.5, 1.5, 0.5]


def test_write_trajectory_writes_the_reference_s_layout_and_push_dataset_reads_it_back(tmp_path, monkeypatch):
    from ndivplanning_amd import generate_trajectories as G
    from ndivplanning_amd.utils import trajectory_loader as TL
    files = {}
    h5py = _stub_h5py(files)
    monkeypatch.setitem(sys.modules, "h5py", h5py)
    monkeypatch.setitem(sys.modules, "PIL", None)                # raw_jpeg needs no PIL
    monkeypatch.setitem(sys.modules, "PIL.Image", None)
    path = str(tmp_path / "trajectory_bundle_00001.h5")
    open(path, "wb").close()
    rng = np.random.RandomState(0)
    T = 5
    trajectories = []
    with h5py.File(path, "w") as f:
        for ix in range(3):
            frames = [b"\xff\xd8" + bytes(rng.randint(0, 256, 30 + 7 * t).astype(np.uint8)) + b"\xff\xd9" for t in range(T)]
            states, actions, goal = rng.randn(T, 25), rng.randn(T, 4), rng.randn(3)
            G.write_trajectory(f, ix, frames, states, actions, goal)
            trajectories.append((frames, states, actions, goal))
    root = files[path]
    assert sorted(root) == ["trajectory_00000", "trajectory_00001", "trajectory_00002"]
    gzip9 = {"compression": "gzip", "compression_opts": 9}
    for ix, (frames, states, actions, goal) in enumerate(trajectories):
        g = root["trajectory_{:05d}".format(ix)]
        assert sorted(g) == ["actions", "goal", "images", "states"]
        assert all(g[k].options == gzip9 for k in g)
        assert g["images"].dtype == "bytes" and g["images"].data.shape == (T,) and list(g["images"].data) == frames
        assert g["images"].attrs["description"] == b"raw_pixels"
        assert g["images"].attrs["shape"].tolist() == [T, 500, 500, 3] and g["images"].attrs["shape"].dtype == np.int32
        assert g["states"].dtype == "float32" and np.array_equal(g["states"].data, states.astype(np.float32))
        assert g["states"].attrs["description"] == b"gripper_and_object_position_velocity_rotation"
        assert g["states"].attrs["shape"].tolist() == [T, 25] and g["states"].attrs["shape"].dtype == np.int32
        assert g["actions"].dtype == "float32" and np.array_equal(g["actions"].data, actions.astype(np.float32))
        assert g["actions"].attrs["description"] == b"action_tensor" and g["actions"].attrs["shape"].tolist() == [T, 4]
        assert g["goal"].dtype == "float32" and g["goal"].data.shape == (3,) and g["goal"].attrs == {}
        assert np.array_equal(g["goal"].data, goal.astype(np.float32))
    ds = TL.PushDataset(str(tmp_path), seq_start=1, seq_length=3, raw_jpeg=True)
    assert len(ds) == 3
    for ix, (frames, states, actions, goal) in enumerate(trajectories):
        images, s, a, gl = ds[ix]
        assert images == frames[1:4]
        assert np.array_equal(s.numpy(), states[1:4].astype(np.float32)) and np.array_equal(a.numpy(), actions[1:4].astype(np.float32))
        assert np.array_equal(gl.numpy(), goal.astype(np.float32))
