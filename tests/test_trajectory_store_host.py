"""`StoreLoader`'s host side (ndivplanning_amd/trajectory_store.py) without a GPU: over a tiny in-memory stand-in for the
store's `gather`, its index batches are a `DataLoader`'s for the same `torch.manual_seed`, the rank / world sharding is
`dp.shard_bounds` of every full batch, and the switches' argument errors are raised before any GPU is touched."""
import pytest
import torch
from torch.utils.data import DataLoader

from ndivplanning_amd import bundle, dp
from ndivplanning_amd.trajectory_store import DeviceTrajectoryStore, StoreLoader


class FakeStore:
    """len() trajectories; gather returns its arguments."""

    def __init__(self, n):
        self.n, self.calls = n, 0

    def __len__(self):
        return self.n

    def gather(self, indices, seq_start, seq_length):
        self.calls += 1
        assert indices.dtype == torch.int64 and not indices.is_cuda
        return indices, seq_start, seq_length


def _dataloader_epochs(n, batch_size, shuffle, seed, epochs=2):
    torch.manual_seed(seed)
    loader = DataLoader(list(range(n)), batch_size=batch_size, shuffle=shuffle)
    return [[b.tolist() for b in loader] for _ in range(epochs)]


@pytest.mark.parametrize("n,batch_size", [(10, 4), (12, 4), (3, 8), (7, 1)])
@pytest.mark.parametrize("shuffle", [True, False])
def test_index_batches_equal_a_dataloaders_over_two_epochs(n, batch_size, shuffle):
    want = _dataloader_epochs(n, batch_size, shuffle, seed=5)
    torch.manual_seed(5)
    loader = StoreLoader(FakeStore(n), batch_size, 1, 3, shuffle=shuffle)
    got = [[(idx.tolist(), s, t) for idx, s, t in loader] for _ in range(2)]
    assert [[b[0] for b in epoch] for epoch in got] == want
    assert all(b[1:] == (1, 3) for epoch in got for b in epoch)
    assert len(loader) == len(want[0]) == -(-n // batch_size)
    if n % batch_size:                                                 # the ragged final batch is there
        assert len(got[0][-1][0]) == n % batch_size
    if shuffle and n > 3:
        assert want[0] != want[1]
    # the global generator is left where a DataLoader leaves it
    state = torch.get_rng_state()
    _dataloader_epochs(n, batch_size, shuffle, seed=5)
    assert torch.equal(torch.get_rng_state(), state)


def test_rank_and_world_take_shard_bounds_of_every_full_batch():
    n, batch_size, world = 14, 4, 2
    want = _dataloader_epochs(n, batch_size, True, seed=9)
    per_rank = []
    for rank in range(world):
        torch.manual_seed(9)
        loader = StoreLoader(FakeStore(n), batch_size, 0, 2, shuffle=True, rank=rank, world=world)
        assert len(loader) == n // batch_size == 3
        per_rank.append([[idx.tolist() for idx, _, _ in loader] for _ in range(2)])
    for epoch in range(2):
        full = [b for b in want[epoch] if len(b) == batch_size]        # the ragged batch of 2 is skipped
        assert len(full) == 3
        for rank in range(world):
            lo, hi = dp.shard_bounds(batch_size, rank, world)
            assert per_rank[rank][epoch] == [b[lo:hi] for b in full]
    with pytest.raises(ValueError):
        StoreLoader(FakeStore(n), 5, 0, 2, rank=0, world=2)            # 5 rows do not split over 2 ranks
    with pytest.raises(ValueError):
        StoreLoader(FakeStore(n), 4, 0, 2, rank=2, world=2)


def test_the_switch_needs_a_bundle_directory(tmp_path):
    from ndivplanning_amd import train_autoencoder, train_forward_model
    from ndivplanning_amd.utils.file import AttrDict

    def config(path):
        return AttrDict({"random_seed": 0, "train_data_path": path, "gpu_id": 0, "trajectory_length": 3,
                         "forward_save_path": str(tmp_path / "fm"),
                         "training": {"forward": {"num_epochs": 1, "learning_rate": 2e-4, "report_feq": 10, "batch_size": 2,
                                                  "epochs_per_stage": 1, "device_store": True}}})
    empty = tmp_path / "empty"
    empty.mkdir()
    h5 = tmp_path / "h5"
    h5.mkdir()
    (h5 / "trajectory_bundle_00001.h5").write_bytes(b"x")
    for path in ("synthetic:4:jpeg", str(empty), str(h5), str(tmp_path / "missing")):
        with pytest.raises(ValueError, match="ndpt"):
            train_forward_model.train(config(path))
        with pytest.raises(ValueError, match="ndpt"):
            train_autoencoder.train(path, batch_size=2, num_epochs=1, device_store=True)
    assert train_autoencoder.make_parser().parse_args(["--device-store"]).device_store is True
    assert train_autoencoder.make_parser().parse_args([]).device_store is False


def test_a_directory_over_max_bytes_is_refused_and_points_to_the_host_loader(tmp_path):
    data = str(tmp_path / "data")
    bundle.synth(2, data, steps=2, seed=1)
    need = sum(b.blob.size for b in bundle.open_dir(data))
    with pytest.raises(ValueError, match="host loader"):
        DeviceTrajectoryStore(data, max_bytes=need)                    # the tables count too
    with pytest.raises(ValueError, match="max_bytes"):
        DeviceTrajectoryStore(data, max_bytes=0)
    mixed = tmp_path / "mixed"
    bundle.synth(1, str(mixed), steps=2, seed=1)
    bundle.write_bundle(str(mixed / "other.ndpt"), [bundle.BundleDataset(data, seq_length=1, raw_jpeg=True)[0]])
    with pytest.raises(ValueError, match="different trajectory lengths"):
        DeviceTrajectoryStore(str(mixed), max_bytes=1 << 30)
