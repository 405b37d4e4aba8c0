"""CPU tests of ndivplanning_amd/_train_io.py, the training scripts' shared front-end.  The expectations are restated by
hand from what the three scripts did each on their own; none is produced by the helpers."""
import logging

import pytest
import torch

from ndivplanning_amd import _train_io as T
from ndivplanning_amd import dp
from ndivplanning_amd.utils.file import AttrDict


# ------------------------------------------------------------------ configuration reads
@pytest.mark.parametrize("node, want", [
    ({}, "D"),                                   # absent
    ({"k": None}, "D"),
    ({"k": {}}, "D"),                            # what a DotMap makes of a missing key
    ({"k": False}, False),                       # values, not absences
    ({"k": 0}, 0),
    ({"k": 0.0}, 0.0),
    ({"k": ""}, ""),
    ({"k": "x"}, "x"),
    ({"k": {"a": 1}}, {"a": 1}),
])
def test_cfg_get(node, want):
    for n in (node, AttrDict(node)):
        got = T.cfg_get(n, "k", "D")
        assert got == want and (isinstance(want, dict) or type(got) is type(want))     # False is not 0
    assert T.cfg_get(AttrDict(node), "other", 7) == 7                 # AttrDict reads the missing key as {}
    assert T.cfg_get(None, "k", "D") == "D" and T.cfg_get(3, "k", "D") == "D"   # a node that is no map has no keys


def test_cfg_require_names_the_missing_key():
    cfg = AttrDict({"seed": 0, "flag": False, "text": "", "none": None, "empty": {},
                    "training": {"forward": {"lr": 2e-4, "epochs": 0, "none": None, "empty": {}}}})
    assert T.cfg_require(cfg, "seed") == 0 and T.cfg_require(cfg, "flag") is False and T.cfg_require(cfg, "text") == ""
    assert T.cfg_require(cfg, "training.forward.lr") == 2e-4 and T.cfg_require(cfg, "training.forward.epochs") == 0
    assert T.cfg_require(cfg, "training.forward") == {"lr": 2e-4, "epochs": 0, "none": None, "empty": {}}
    for dotted in ("missing", "none", "empty", "training.gan", "training.gan.lr", "training.forward.missing",
                   "training.forward.none", "training.forward.empty", "seed.below_a_number", "missing.below.nothing"):
        with pytest.raises(KeyError, match=dotted.replace(".", r"\.") + " is missing from the config"):
            T.cfg_require(cfg, dotted)
        with pytest.raises(KeyError):
            T.cfg_require(cfg.toDict(), dotted)


# ------------------------------------------------------------------ this rank's batches
def _batches():
    g = torch.Generator().manual_seed(0)
    return [(torch.rand(n, 3, 2, generator=g), torch.arange(n), torch.rand(n, 4, generator=g)) for n in (6, 6, 4)]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_batches_takes_this_ranks_rows_and_skips_the_ragged_batch(world):
    batches = _batches()
    for rank in range(world):
        ragged = []
        got = list(T.rank_batches(batches, 6, rank, world, False, on_ragged=ragged.append))
        if world == 1:
            assert len(got) == 3 and ragged == []
            for g, b in zip(got, batches):
                assert all(x is y for x, y in zip(g, b))                  # as they came
            continue
        assert len(got) == 2 and ragged == [4]                            # once, with the rows of the skipped batch
        lo, hi = dp.shard_bounds(6, rank, world)
        assert (lo, hi) == (rank * 6 // world, (rank + 1) * 6 // world)
        for g, b in zip(got, batches):
            assert len(g) == 3 and all(torch.equal(x, y[lo:hi]) for x, y in zip(g, b))
    assert len(list(T.rank_batches(batches, 6, 1, 2, False))) == 2        # on_ragged is optional


def test_rank_batches_leaves_a_presharded_loader_alone():
    batches = _batches()
    for world in (1, 2, 3):
        ragged = []
        got = list(T.rank_batches(batches, 6, world - 1, world, True, on_ragged=ragged.append))
        assert len(got) == 3 and ragged == [] and all(g is b for g, b in zip(got, batches))


# ------------------------------------------------------------------ upload
class _Decoder:
    def __init__(self, events):
        self.events = events

    def decode_frames(self, frames):
        self.events.append(("decode_frames", frames))
        return torch.full((2, 3, 4, 4, 3), 7, dtype=torch.uint8)

    def decode_images(self, frames):
        self.events.append(("decode_images", frames))
        return torch.full((2, 3, 3, 4, 4), 0.5, dtype=torch.float64)


def test_upload_frames_keeps_bytes_and_makes_everything_else_float32(monkeypatch):
    events = []
    real_to = torch.Tensor.to

    def to(self, *a, **kw):
        events.append(("to", self.dtype, a, kw))
        return real_to(self, *a, **kw)
    monkeypatch.setattr(torch.Tensor, "to", to)
    cpu = torch.device("cpu")
    u8 = torch.arange(24, dtype=torch.uint8).view(1, 2, 2, 2, 3)
    out = T.upload_frames(u8, cpu)
    assert out.dtype == torch.uint8 and torch.equal(out, u8)
    assert events == [("to", torch.uint8, (cpu,), {"non_blocking": True})]
    del events[:]
    f64 = torch.linspace(-1, 1, 24, dtype=torch.float64).view(1, 2, 3, 2, 2)
    out = T.upload_frames(f64, cpu, non_blocking=False)
    assert out.dtype == torch.float32 and torch.equal(out, f64.float())
    assert events[-1] == ("to", torch.float32, (cpu,), {"non_blocking": False})      # converted on the host, then uploaded
    del events[:]
    out = T.upload_frames("streams", cpu, _Decoder(events))                          # the decoder runs before the upload
    assert [e[0] for e in events] == ["decode_frames", "to"] and events[0][1] == "streams"
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 3, 4, 4, 3) and bool((out == 7).all())
    del events[:]
    out = T.upload_frames("streams", cpu, _Decoder(events), "decode_images")
    assert events[0] == ("decode_images", "streams") and events[-1][0] == "to"
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 3, 3, 4, 4) and bool((out == 0.5).all())


# ------------------------------------------------------------------ device and process group
@pytest.mark.parametrize("world, local_rank, one_gpu, honour, single, want", [
    (1, 0, None, True, 0, "cuda:0"),             # one process: the script's own device ...
    (1, 0, None, True, 3, "cuda:3"),
    (1, 5, "1", True, 2, "cuda:2"),              # ... whatever the launcher's variables say
    (1, 0, None, True, "cuda:1", "cuda:1"),      # gpu_id as a string (anything torch.device takes)
    (1, 0, None, True, "cpu", "cpu"),
    (2, 0, None, True, 3, "cuda:0"),             # data parallel: the local rank's GPU
    (2, 1, None, True, 3, "cuda:1"),
    (4, 3, "0", True, 0, "cuda:3"),
    (2, 1, "1", True, 3, "cuda:0"),              # the rehearsal: all ranks on one card
    (2, 1, "1", False, 3, "cuda:1"),             # train_gan does not honour it
    (2, 1, None, False, None, "cuda:1"),
])
def test_open_device(monkeypatch, world, local_rank, one_gpu, honour, single, want):
    calls = []
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: calls.append(("set_device", device)))
    monkeypatch.setattr(dp, "init_process_group", lambda device=None, force=False: calls.append(("init_process_group", device)))
    if one_gpu is None:
        monkeypatch.delenv("NDP_BENCH_ONE_GPU", raising=False)
    else:
        monkeypatch.setenv("NDP_BENCH_ONE_GPU", one_gpu)
    device = T.open_device(world, local_rank, single, one_gpu_rehearsal=honour)
    assert isinstance(device, torch.device) and device == torch.device(want)
    assert calls == [("set_device", torch.device(want)), ("init_process_group", torch.device(want))]


# ------------------------------------------------------------------ class paths
def test_bind_reference_class_paths(monkeypatch, caplog):
    import importlib

    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    from ndivplanning_amd.models.gan import Decoder, Discriminator
    classes = (Decoder, Discriminator, ForwardAutoencoder)
    table = {"models.gan": (Decoder, Discriminator), "models.forward_encoder": (ForwardAutoencoder,)}
    saved = [c.__module__ for c in classes]
    try:
        for c in classes:
            c.__module__ = "somewhere.else"
        assert T.bind_reference_class_paths(table) == []                  # (conftest puts the repository root on sys.path)
        assert [c.__module__ for c in classes] == ["models.gan", "models.gan", "models.forward_encoder"]
        for c in classes:
            c.__module__ = "somewhere.else"
        real_import = importlib.import_module

        def no_shims(name, *a, **kw):
            if name.startswith("models"):
                raise ImportError(name)
            return real_import(name, *a, **kw)
        monkeypatch.setattr(importlib, "import_module", no_shims)
        with caplog.at_level(logging.WARNING):
            missing = T.bind_reference_class_paths(table)
        assert missing == ["models.gan.Decoder", "models.gan.Discriminator", "models.forward_encoder.ForwardAutoencoder"]
        assert [c.__module__ for c in classes] == ["somewhere.else"] * 3
        warnings = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
        assert len(warnings) == 1 and "models.gan.Decoder, models.gan.Discriminator" in warnings[0]
        assert "sys.path" in warnings[0]
    finally:
        for c, m in zip(classes, saved):
            c.__module__ = m


def test_the_scripts_bind_their_own_tables():
    from ndivplanning_amd import train_forward_model, train_gan
    from ndivplanning_amd.models import forward_encoder, gan, image_autoencoder
    classes = (gan.Decoder, gan.Discriminator, image_autoencoder.Encoder, forward_encoder.ForwardAutoencoder,
               forward_encoder.Encoder, forward_encoder.Decoder)
    saved = [c.__module__ for c in classes]
    try:
        assert train_gan.bind_reference_class_paths() == [] and train_forward_model.bind_reference_class_paths() == []
        assert [c.__module__ for c in classes] == ["models.gan"] * 2 + ["models.image_autoencoder"] + ["models.forward_encoder"] * 3
    finally:
        for c, m in zip(classes, saved):
            c.__module__ = m


def test_one_definition_of_denorm_and_norm():
    from ndivplanning_amd import (_eval_io, complete_eval, control_evaluation, mpc_eval, mpc_gym_eval, train_autoencoder,
                                  train_forward_model, train_gan)
    for module in (complete_eval, control_evaluation, mpc_eval, mpc_gym_eval, train_autoencoder, train_forward_model, train_gan, T):
        assert module.denorm is _eval_io.denorm and module.norm is _eval_io.norm
    x = torch.tensor([0.0, 51.0, 255.0])
    assert torch.equal(_eval_io.norm(x), torch.tensor([-1.0, (51.0 / 255.0 - 0.5) * 2.0, 1.0]))
    assert torch.equal(_eval_io.denorm(torch.tensor([-1.0, 0.0, 1.0])), torch.tensor([0.0, 127.5, 255.0]))
