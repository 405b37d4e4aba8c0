"""CPU tests of the image training scripts' loops (train_autoencoder.train, train_forward_model.train): what they ask of
their trainer, in order, read on a recording stand-in, as tests/test_planner_calls.py does for the planner.  Every step's
input tensors are recorded with shape, dtype, device and fp64 sum -- the synthetic frames and actions are multiples of
2^-23, so the sum is exact and pins the shuffling order, the seeds and the frame pairing -- next to the constructor's
arguments, the sync / save / close order, the log lines and the returned history.

The expectations are tests/golden/train_script_calls.json, recorded once by `python tests/test_train_script_calls.py`
from the scripts as they were before their shared plumbing moved into ndivplanning_amd/_train_io.py."""
import json
import logging
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_script_calls.json")


def _tensor(t):
    return [list(t.shape), str(t.dtype), str(t.device), float(t.double().sum())]


def _plain(v):
    if isinstance(v, torch.nn.Module):
        return "%s(training=%s)" % (type(v).__name__, v.training)
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    return v if v is None or isinstance(v, (bool, int, float, str)) else repr(v)


class _Recorder:
    """The part of AutoencoderTrainer / ForwardModelTrainer the scripts use.  Step k returns, or adds to loss_sum, the
    loss 1 / (k + 1): the history then pins the number of steps per epoch."""
    made = []

    def __init__(self, *modules, **kw):
        self.modules, self.calls, self.steps = modules, [], 0
        # (an argument left out and one given its default value, None or one rank's statistics, are the same request)
        self.ctor = {"modules": _plain(modules), "kwargs": {k: _plain(v) for k, v in sorted(kw.items())
                                                            if v is not None and (k, v) != ("sync_batchnorm_world", 1)}}
        self.loss_sum = torch.zeros(1)
        self.device = torch.device("cpu")
        _Recorder.made.append(self)

    def _step(self, name, tensors):
        self.calls.append([name] + [_tensor(t) for t in tensors])
        self.steps += 1
        loss = torch.tensor([1.0 / self.steps], dtype=torch.float32)
        self.loss_sum += loss
        return loss

    def step(self, *tensors):
        return self._step("step", tensors)

    def step_rollout(self, *tensors):
        return self._step("step_rollout", tensors)

    def sync_to_modules(self):
        self.calls.append(["sync_to_modules"])
        return self.modules

    def sync_to_module(self):
        self.calls.append(["sync_to_module"])
        return self.modules[0]

    def close(self):
        self.calls.append(["close"])


class _StubDecoder:
    """ndivplanning_amd.jpeg.JpegDecoder without a GPU: frames of zeros in the shape the real one returns."""
    made = []

    def __init__(self, device=None, check=True):
        self.device, self.check, self.seen, self.finished = torch.device(device), check, [], 0
        _StubDecoder.made.append(self)

    def decode_frames(self, frames, check=None):
        self.seen.append(["decode_frames", frames.batch, frames.steps, int(frames.offsets.numel())])
        return torch.zeros(frames.shape, dtype=torch.uint8)

    def decode_images(self, frames, check=None):
        self.seen.append(["decode_images", frames.batch, frames.steps, int(frames.offsets.numel())])
        return torch.zeros(frames.batch, frames.steps, 3, 128, 128, dtype=torch.float32)

    def finish(self):
        self.finished += 1


def _run(monkeypatch, script, trainer_name, call):
    """call() with the script's trainer and torch.save recorded into one list; returns (record, what call returned)."""
    del _Recorder.made[:], _StubDecoder.made[:]
    monkeypatch.setattr(script, trainer_name, _Recorder)
    saves = []
    real_save = torch.save

    def save(obj, path, *a, **kw):
        saves.append(os.path.basename(path))
        _Recorder.made[-1].calls.append(["save", os.path.basename(path)])
        return real_save(obj, path, *a, **kw)
    monkeypatch.setattr(torch, "save", save)
    out = call()
    assert len(_Recorder.made) == 1
    trainer = _Recorder.made[0]
    record = {"ctor": trainer.ctor, "calls": trainer.calls, "saves": saves}
    if _StubDecoder.made:
        assert len(_StubDecoder.made) == 1
        record["decoder"] = {"check": _StubDecoder.made[0].check, "seen": _StubDecoder.made[0].seen,
                             "finished": _StubDecoder.made[0].finished}
    return record, out


def run_autoencoder(monkeypatch, tmp, data="synthetic:5:images", num_epochs=2, **kw):
    from ndivplanning_amd import jpeg, train_autoencoder as script
    monkeypatch.setattr(jpeg, "JpegDecoder", _StubDecoder)
    log, vals = [], []
    if "val_data" in kw:
        def validate(trainer, val_dataset, batch_size, device, display=None, quality=None):
            trainer.calls.append(["validate", len(val_dataset), batch_size, str(device)])
            vals.append(0.125 * (len(vals) + 1))
            return vals[-1]
        monkeypatch.setattr(script, "validate", validate)
    record, out = _run(monkeypatch, script, "AutoencoderTrainer", lambda: script.train(
        data, batch_size=2, num_epochs=num_epochs, device="cpu", save_dir=str(tmp),
        log=lambda *a: log.append([x if isinstance(x, (int, str, float)) else [float(v) for v in x] for x in a]), **kw))
    encoder, decoder, losses = out
    assert (type(encoder).__name__, type(decoder).__name__) == ("Encoder", "Decoder")
    assert script.train.last_trainer is _Recorder.made[0]
    record.update(log=log, history=losses, files=sorted(os.listdir(str(tmp))), last_val=[list(v) for v in script.train.last_val_losses])
    return record


def run_forward(monkeypatch, caplog, tmp, data="synthetic:5:images", num_epochs=2, **forward):
    from ndivplanning_amd import jpeg, train_forward_model as script
    from ndivplanning_amd.utils.file import AttrDict
    monkeypatch.setattr(jpeg, "JpegDecoder", _StubDecoder)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    if "val_data_path" in forward:
        def validate(trainer, val_dataset, horizon, batch_size, quality=False):
            trainer.calls.append(["validate", len(val_dataset), horizon, batch_size, quality])
            return {"one_step_mse": [0.5]}
        monkeypatch.setattr(script, "validate", validate)
    f = {"num_epochs": num_epochs, "learning_rate": 2e-4, "report_feq": 10, "batch_size": 2, "epochs_per_stage": 2,
         "step_lr_gamma": 0.1}
    f.update(forward)
    config = AttrDict({"random_seed": 0, "train_data_path": data, "gpu_id": "cpu", "trajectory_length": 4,
                       "forward_save_path": str(tmp), "training": {"forward": f}})
    with caplog.at_level(logging.INFO):
        record, history = _run(monkeypatch, script, "ForwardModelTrainer", lambda: script.train(config))
    assert script.train.last_trainer is _Recorder.made[0]
    log = [r.getMessage() for r in caplog.records if r.name == "root" and r.levelno == logging.INFO]
    record.update(log=log, history=history, files=sorted(os.listdir(str(tmp))),
                  last_val=[[e, m] for e, m in script.train.last_val])
    return record


CASES = {
    "autoencoder": lambda mp, cl, tmp: run_autoencoder(mp, tmp),
    "autoencoder_jpeg": lambda mp, cl, tmp: run_autoencoder(mp, tmp, data="synthetic:5:jpeg"),
    "autoencoder_val": lambda mp, cl, tmp: run_autoencoder(mp, tmp, num_epochs=4, val_data="synthetic:3:images", val_every=2),
    "forward": lambda mp, cl, tmp: run_forward(mp, cl, tmp),
    "forward_rollout": lambda mp, cl, tmp: run_forward(mp, cl, tmp, rollout_steps=2),
    "forward_jpeg": lambda mp, cl, tmp: run_forward(mp, cl, tmp, data="synthetic:5:jpeg"),
    "forward_val": lambda mp, cl, tmp: run_forward(mp, cl, tmp, num_epochs=4, val_data_path="synthetic:3:images", val_every=2,
                                                   val_horizon=2),
}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_script_asks_of_its_trainer_what_the_recorded_run_asked(case, monkeypatch, caplog, tmp_path):
    got = json.loads(json.dumps(CASES[case](monkeypatch, caplog, tmp_path)))
    want = _golden()[case]
    assert sorted(got) == sorted(want)
    for key in ("ctor", "saves", "files", "log", "history", "last_val", "decoder"):
        assert got.get(key) == want.get(key), key
    assert len(got["calls"]) == len(want["calls"])
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, (i, g, w)


def _names(record):
    return [c[0] for c in record["calls"]]


def test_the_recorded_runs_are_the_ones_the_scripts_are_known_to_make():
    """The counts the fixture must hold, stated by hand: they guard the fixture itself."""
    g = _golden()
    ae = g["autoencoder"]
    assert ae["ctor"]["kwargs"]["batch"] == 30 and ae["ctor"]["modules"] == ["Encoder(training=True)", "Decoder(training=True)"]
    assert _names(ae) == ["step"] * 6 + ["sync_to_modules", "save", "save", "sync_to_modules", "close"]
    assert [c[1][0] for c in ae["calls"][:6]] == [[30, 3, 128, 128], [30, 3, 128, 128], [15, 3, 128, 128]] * 2
    assert ae["files"] == ["decoder_1.pt", "encoder_1.pt"] and len(ae["history"]) == 6 and len(ae["log"]) == 6
    fm = g["forward"]
    assert _names(fm) == ["step"] * 18 + ["sync_to_module", "save", "sync_to_module", "close"]
    assert fm["files"] == ["forward_autoencoder_1.pt"] and fm["ctor"]["kwargs"]["batch"] == 2
    assert fm["history"] == pytest.approx([sum(1.0 / k for k in range(1, 10)) / 9, sum(1.0 / k for k in range(10, 19)) / 9])
    ro = g["forward_rollout"]
    assert _names(ro)[:12] == ["step_rollout"] * 12 and "step" not in _names(ro)
    assert ro["calls"][0][1][:2] == [[2, 3, 3, 128, 128], "torch.float32"] and ro["calls"][0][2][0] == [2, 2, 4]
    for name, steps, epochs in (("autoencoder_jpeg", 6, 2), ("forward_jpeg", 18, 2)):
        d = g[name]["decoder"]
        assert d["check"] == "deferred" and d["finished"] == epochs and _names(g[name]).count("step") == steps
        assert [s[1] for s in d["seen"]] == [2, 2, 1] * epochs                     # every batch once, ragged one included
    assert [i for i, n in enumerate(_names(g["autoencoder_val"])) if n == "validate"] == [6, 16]
    assert [e for e, _ in g["autoencoder_val"]["last_val"]] == [1, 3]
    assert [e for e, _ in g["forward_val"]["last_val"]] == [1, 3]
    assert [c for c in g["forward_val"]["calls"] if c[0] == "validate"] == [["validate", 3, 2, 2, False]] * 2


if __name__ == "__main__":                                                        # record the fixture
    import tempfile

    class _Caplog:
        """caplog for a run outside pytest."""
        def __init__(self):
            self.records = []

        def at_level(self, level):
            import contextlib
            handler = logging.Handler(level)
            handler.emit = self.records.append
            logging.getLogger().addHandler(handler)
            logging.getLogger().setLevel(level)
            return contextlib.nullcontext()

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    for name in sorted(CASES):
        mp, cl = pytest.MonkeyPatch(), _Caplog()
        with tempfile.TemporaryDirectory() as tmp:
            out[name] = CASES[name](mp, cl, tmp)
        logging.getLogger().handlers = [h for h in logging.getLogger().handlers if h.emit != cl.records.append]
        mp.undo()
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
