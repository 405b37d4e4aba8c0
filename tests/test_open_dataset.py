"""utils.trajectory_loader.open_dataset behind its seven entry points, on the CPU: what each makes of a `synthetic:`
specification (class, mode, seq_length, seed, the first item's bits, the refused modes with the entry's own words, the
specification behind a directory prefix) and which PushDataset arguments each passes for a directory.  The expected
values are written out here, entry by entry; nothing is computed by the code under test."""
import pytest
import torch

from ndivplanning_amd import (evaluation, forward_model_eval, gan_eval, train_autoencoder, train_forward_model,
                              train_gan)
from ndivplanning_amd.utils import trajectory_loader as TL
from ndivplanning_amd.utils.file import AttrDict

T, SEED = 4, 7
IMAGES = ("images", "frames_u8", "jpeg")
ANY = ("codes", "images", "frames_u8", "jpeg")


def _config(path, **extra):
    return AttrDict(dict({"trajectory_length": T, "random_seed": SEED, "train_data_path": path, "evaluation_data_path": path},
                         **extra))


# name: (open(path), default mode, allowed modes, the refusal's words, seq_length, seed)
ENTRIES = {
    "train_gan.make_dataset": (lambda p: train_gan.make_dataset(_config(p)), "codes", ANY, "mode must be", T, SEED),
    "train_gan.make_val_dataset": (lambda p: train_gan.make_val_dataset(_config("unused"), p), "codes", ANY, "mode must be",
                                   T, SEED + 1),
    "train_forward_model.make_val_dataset": (lambda p: train_forward_model.make_val_dataset(_config("unused"), p), "images",
                                             IMAGES, "the forward model is validated on images: use `synthetic:<N>:images`, "
                                             "`:frames_u8` or `:jpeg`", T, SEED + 1),
    "train_autoencoder.make_dataset": (lambda p: train_autoencoder.make_dataset(p, seed=SEED), "images", ("images", "jpeg"),
                                       "the autoencoder trains on images: use synthetic:<N>:images or synthetic:<N>:jpeg",
                                       15, SEED),
    "forward_model_eval.make_dataset": (lambda p: forward_model_eval.make_dataset(p, seq_length=T, seed=SEED), "images", IMAGES,
                                        "the forward model predicts images: use synthetic:<N>:images, :frames_u8 or :jpeg, "
                                        "got 'codes'", T, SEED),
    "gan_eval.make_dataset": (lambda p: gan_eval.make_dataset(p, seq_length=T, seed=SEED), "codes", ANY, "mode must be", T, SEED),
    "evaluation.make_eval_dataset": (lambda p: evaluation.make_eval_dataset(_config(p)), "images", IMAGES,
                                     "evaluation needs images: use synthetic:<N>:images, synthetic:<N>:frames_u8 or "
                                     "synthetic:<N>:jpeg", T, SEED),
}


def _same_item(a, b):
    return len(a) == len(b) == 4 and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_synthetic_specifications(name):
    make, default_mode, modes, words, seq_length, seed = ENTRIES[name]
    ds = make("synthetic:3")
    assert type(ds) is TL.SyntheticPushDataset
    assert (len(ds), ds.mode, ds.seq_length, ds.seed) == (3, default_mode, seq_length, seed)
    assert _same_item(ds[0], TL.SyntheticPushDataset(3, seq_length=seq_length, mode=default_mode, seed=seed)[0])
    for mode in modes:
        if mode != "jpeg":                                           # (that mode needs PIL at construction)
            assert make("synthetic:2:" + mode).mode == mode
    refused = "bogus" if "codes" in modes else "codes"
    with pytest.raises(ValueError) as e:
        make("synthetic:2:" + refused)
    assert words in str(e.value)
    # behind a directory prefix, as make_paths_absolute can leave it
    if "frames_u8" in modes:
        ds = make("/somewhere/synthetic:5:frames_u8")
        assert type(ds) is TL.SyntheticPushDataset and (len(ds), ds.mode, ds.seq_length, ds.seed) == (5, "frames_u8", seq_length, seed)
        assert _same_item(ds[0], TL.SyntheticPushDataset(5, seq_length=seq_length, mode="frames_u8", seed=seed)[0])
    else:                                                            # recognised, and refused in the entry's own words
        with pytest.raises(ValueError) as e:
            make("/somewhere/synthetic:5:frames_u8")
        assert words in str(e.value)
        assert (len(make("/somewhere/synthetic:5:images")), make("/somewhere/synthetic:5:images").mode) == (5, "images")


def test_directories_get_each_entrys_own_pushdataset_arguments(monkeypatch):
    calls = []

    def recorder(*args, **kwargs):
        calls.append((args, kwargs))
        return "the dataset"

    monkeypatch.setattr(TL, "PushDataset", recorder)
    trainer_default = dict(seq_length=T, raw_uint8=True, raw_jpeg=False)
    trainer_jpeg = dict(seq_length=T, raw_uint8=False, raw_jpeg=True)
    flags = dict(raw_uint8=False, raw_jpeg=True)
    table = [
        (lambda: train_gan.make_dataset(_config("/data/dir")), trainer_default),
        (lambda: train_gan.make_dataset(_config("/data/dir", **flags)), trainer_jpeg),
        (lambda: train_gan.make_val_dataset(_config("unused"), "/data/dir"), trainer_default),
        (lambda: train_gan.make_val_dataset(_config("unused", **flags), "/data/dir"), trainer_jpeg),
        (lambda: train_forward_model.make_val_dataset(_config("unused"), "/data/dir"), trainer_default),
        (lambda: train_forward_model.make_val_dataset(_config("unused", **flags), "/data/dir"), trainer_jpeg),
        (lambda: train_autoencoder.make_dataset("/data/dir"), {}),
        (lambda: train_autoencoder.make_dataset("/data/dir", raw_jpeg=True), dict(raw_jpeg=True)),
        (lambda: forward_model_eval.make_dataset("/data/dir", seq_length=T), dict(seq_length=T, raw_uint8=True, raw_jpeg=False)),
        (lambda: forward_model_eval.make_dataset("/data/dir", seq_length=T, raw_jpeg=True), trainer_jpeg),
        (lambda: gan_eval.make_dataset("/data/dir", seq_length=T), dict(seq_length=T, raw_uint8=True, raw_jpeg=False)),
        (lambda: gan_eval.make_dataset("/data/dir", seq_length=T, raw_jpeg=True), trainer_jpeg),
        (lambda: evaluation.make_eval_dataset(_config("/data/dir")), dict(seq_length=T, raw_uint8=True)),
        (lambda: evaluation.make_eval_dataset(_config("/data/dir", raw_uint8=False)), dict(seq_length=T, raw_uint8=False)),
        (lambda: evaluation.make_eval_dataset(_config("/data/dir", raw_jpeg=True)), dict(seq_length=T, raw_jpeg=True)),
    ]
    for i, (make, kwargs) in enumerate(table):
        assert make() == "the dataset", i
        assert calls[-1] == (("/data/dir",), kwargs), (i, calls[-1])
    assert len(calls) == len(table)
