"""CPU-only: the host side of ndivplanning_amd/forward_model_eval.py -- the rollout schedule against a brute-force
enumeration, the argument errors of `evaluate` and of the command line, the validation keys of train_forward_model --
and the fp64 restatement that tests/test_gpu_forward_model_eval.py judges the kernels by
(oracle.forward_model_oracle.forward(..., training=False), fed its own predictions) against the committed results of the
reference's own module (tests/golden/fm_eval_case.npz)."""
import numpy as np
import pytest
import torch

import fm_eval_common as C
from conftest import load_golden


def test_rollout_schedule_matches_a_brute_force_enumeration():
    from ndivplanning_amd import forward_model_eval as FME
    for T in range(2, 9):
        for horizon in list(range(1, T)) + [None]:
            H = T - 1 if horizon is None else horizon
            sched = FME.rollout_schedule(T, horizon)
            assert len(sched) == H
            # brute force: walk every start frame forward while a target frame exists
            want = {h: [] for h in range(1, H + 1)}
            for t in range(T):
                for h in range(1, H + 1):
                    if t + h <= T - 1:
                        want[h].append((t, t + h - 1, t + h))
            for h, (starts, action_frames, target_frames) in enumerate(sched, start=1):
                assert list(zip(starts, action_frames, target_frames)) == want[h], (T, horizon, h)
                assert len(starts) == T - h and max(target_frames) == T - 1 and min(action_frames) == h - 1
            # step h + 1's starts are step h's without the last one: the survivors' predictions are a prefix
            for a, b in zip(sched, sched[1:]):
                assert b[0] == a[0][:-1]
    for T, horizon in ((1, None), (0, 1), (4, 0), (4, 4), (4, -1), (2, 2)):
        with pytest.raises(ValueError):
            FME.rollout_schedule(T, horizon)


@pytest.fixture(scope="module")
def golden_and_oracle():
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    g, R = load_golden("fm_eval_case"), C.recipe()
    model = R.build_module(ForwardAutoencoder)                       # the mirror's class, on the CPU (never called here)
    frames_u8, actions = R.inputs()
    order = [tuple(int(v) for v in row) for row in g["order"]]
    preds = C.oracle_rollouts(model.state_dict(), R.norm_frames(frames_u8), actions, order)
    return g, R, model, frames_u8, actions, order, preds


def test_the_recipe_replays_the_golden_inputs_and_parameters(golden_and_oracle):
    g, R, model, frames_u8, actions, order, _ = golden_and_oracle
    assert [int(v) for v in g["shape"]] == [R.B, R.T, R.H] == [2, 4, 3]
    assert np.array_equal(g["frames_u8"], frames_u8.numpy()) and np.array_equal(g["actions"], actions.numpy())
    assert order == R.order() and len(order) == 12
    for k, v in model.state_dict().items():                          # an RNG-stream change shows here, not as a wrong result
        if v.is_floating_point():
            np.testing.assert_allclose(R.sums(v), g["state/" + k], rtol=1e-12, atol=1e-12, err_msg=k)
    # the loader's normalisation is the kernels' table
    assert np.array_equal(R.norm_frames(frames_u8).reshape(-1, 3, 128, 128).numpy(),
                          C.as_float_images(frames_u8.reshape(-1, 128, 128, 3).numpy()))
    # every value of every prediction is inside [-1, 1]: the reference's wrapping cast and the saturating one agree
    assert -1.0 <= g["value_range"][0] and g["value_range"][1] <= 1.0


def test_the_fp64_restatement_reproduces_the_reference_s_rollouts(golden_and_oracle):
    """The reference ran in fp32, the restatement in fp64: they differ by the fp32 path's own rounding, which the GPU suite
    uses as its yardstick.  One eval step is held to 2e-4 there (test_eval_and_no_grad_forward_of_the_module_match_the_
    oracle); step h carries the h - 1 earlier steps' differences through state + residual(state), so h x 2e-4 bounds it as
    long as the residual's sensitivity to its input is small against 1 -- measured (printed): 6e-8, 7e-8 and 1e-7 at h = 1, 2, 3."""
    g, R, _, frames_u8, _, order, preds = golden_and_oracle
    frames = R.norm_frames(frames_u8).double()
    worst = {}
    for i, ((b, t, h), pred) in enumerate(zip(order, preds)):
        d = float((pred[:, ::16, ::16] - torch.from_numpy(g["pred_sample"][i]).double()).abs().max())
        worst[h] = max(worst.get(h, 0.0), d)
        mse = float(((pred - frames[b, t + h]) ** 2).mean())
        base = float(((frames[b, t] - frames[b, t + h]) ** 2).mean())
        assert abs(mse - float(g["pred_mse"][i])) <= 2e-6 * mse, (i, mse, g["pred_mse"][i])
        assert abs(base - float(g["persistence_mse"][i])) <= 2e-6 * base, (i, base, g["persistence_mse"][i])
        # the reference's bytes at the samples, from the fp64 values: equal except where fp32 rounding crosses a boundary
        want = np.trunc(((pred[:, ::16, ::16].numpy() + 1.0) / 2.0) * 255.0)
        assert (np.abs(want - g["pred_u8_sample"][i].astype(np.float64)) <= 1).all()
        assert (want == g["pred_u8_sample"][i]).mean() > 0.99
    print("reference fp32 - oracle fp64, largest |difference| over the samples per h:", worst)
    for h, d in worst.items():
        assert d <= h * 2e-4, (h, d)


class _Set:
    """A dataset of n empty-handed trajectories of T frames: evaluate must refuse before it reads one."""

    def __init__(self, n, T):
        self.n, self.seq_length, self.mode = n, T, "images"

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        raise AssertionError("evaluate read a trajectory before checking its arguments")


def test_evaluate_names_what_is_wrong_with_its_arguments():
    from ndivplanning_amd import _capi, forward_model_eval as FME
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    model = ForwardAutoencoder()
    with pytest.raises(_capi.NdpError, match="training mode"):
        FME.evaluate(model, _Set(3, 4))
    model.eval()
    with pytest.raises(ValueError, match="non-empty dataset"):
        FME.evaluate(model, _Set(0, 4))
    with pytest.raises(ValueError, match="batch_size"):
        FME.evaluate(model, _Set(3, 4), batch_size=0)
    with pytest.raises(ValueError, match=r"horizon 4 is outside 1 \.\. T - 1 = 3"):
        FME.evaluate(model, _Set(3, 4), horizon=4)
    with pytest.raises(_capi.NdpError, match="on cpu"):
        FME.evaluate(model, _Set(3, 4), horizon=3)
    # predict / rollout / score: a CPU tensor has no path, a training-mode module is refused, `out` is checked
    x, a = torch.zeros(1, 3, 128, 128), torch.zeros(1, 4)
    with pytest.raises(_capi.NdpError, match="cpu"):
        FME.predict(model, x, a)
    with pytest.raises(_capi.NdpError, match="cpu"):
        FME.rollout(model, x, a.view(1, 1, 4))
    with pytest.raises(_capi.NdpError, match="cpu"):
        FME.score(x, x)
    with pytest.raises(ValueError, match="out must be"):
        FME.predict(model, x, a, out="png")
    with pytest.raises(_capi.NdpError, match="training mode"):
        FME.rollout(model.train(), x, a.view(1, 1, 4))


def test_command_line_errors_name_the_problem(monkeypatch):
    from ndivplanning_amd import _capi, forward_model_eval as FME
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    model = ForwardAutoencoder()
    monkeypatch.setattr(FME, "load_module", lambda path, device: model.to(device).eval())
    base = ["--model", "unused.pt", "--device", "cpu", "--seq-length", "4"]
    with pytest.raises(_capi.NdpError, match="on cpu"):                               # a CPU module
        FME.main(base + ["--data", "synthetic:3:images"])
    with pytest.raises(ValueError, match="non-empty dataset"):                        # an empty dataset
        FME.main(base + ["--data", "synthetic:0:images"])
    with pytest.raises(ValueError, match="horizon 4 is outside"):                     # a horizon larger than T - 1
        FME.main(base + ["--data", "synthetic:3:frames_u8", "--horizon", "4"])
    with pytest.raises(ValueError, match="synthetic:<N>:images"):
        FME.main(base + ["--data", "synthetic:3:codes"])
    monkeypatch.setattr(FME, "load_module", lambda path, device: model.to(device).train())
    with pytest.raises(_capi.NdpError, match="training mode"):                        # a training-mode module
        FME.main(base + ["--data", "synthetic:3:images"])
    with pytest.raises(SystemExit):
        FME.main(["--data", "synthetic:3:images"])                                    # --model is required


def test_validation_keys_are_optional_and_checked():
    from ndivplanning_amd import train_forward_model as TF
    from ndivplanning_amd.utils.file import AttrDict as DotMap
    f = DotMap({"val_every": 2})
    assert TF.cfg_get(f, "val_data_path", None) is None and TF.cfg_get(f, "val_every", 1) == 2
    assert TF.cfg_get(f, "val_horizon", 1) == 1
    config = DotMap({"trajectory_length": 4, "random_seed": 3})
    ds = TF.make_val_dataset(config, "/somewhere/synthetic:5:frames_u8")
    assert len(ds) == 5 and ds.seq_length == 4 and ds.mode == "frames_u8" and ds.seed == 4     # apart from the training set's seed
    with pytest.raises(ValueError, match="validated on images"):
        TF.make_val_dataset(config, "synthetic:5:codes")
    text = open(TF.__file__.replace("ndivplanning_amd/train_forward_model.py", "config/forward_model.yaml")).read()
    for key in ("# val_data_path:", "# val_every:", "# val_horizon:"):
        assert key in text


def test_score_entry_rejects_bad_arguments_before_launching():
    import ctypes
    from ndivplanning_amd import _build, _capi
    _build.build()
    lib = _capi.load()
    p = ctypes.c_void_p(4096)                                  # never dereferenced: every call fails its checks
    f = lib.ndp_fm_score
    assert f(None, 3, None, p, 3, None, None, None, 0, None, p, None, None, None) == 1 and b"null" in lib.ndp_last_error()
    assert f(p, 0, None, p, 3, None, None, None, 0, None, p, None, None, None) == 1 and b"image count" in lib.ndp_last_error()
    assert f(p, 3, p, p, 3, None, None, None, 0, None, p, None, None, None) == 1 and b"two targets" in lib.ndp_last_error()
    assert f(p, 3, None, None, 3, None, None, None, 0, None, p, None, None, None) == 1 and b"no target" in lib.ndp_last_error()
    assert f(p, 3, p, None, 0, None, None, None, 0, None, p, None, None, None) == 1 and b"n_target" in lib.ndp_last_error()
    assert f(p, 3, p, None, 3, None, p, None, 3, None, p, None, None, None) == 1 and b"without base_err" in lib.ndp_last_error()
    assert f(p, 3, p, None, 3, None, None, None, 0, None, p, p, None, None) == 1 and b"without a base" in lib.ndp_last_error()
    assert f(p, 3, p, None, 3, None, p, p, 3, None, p, p, None, None) == 1 and b"two base" in lib.ndp_last_error()
    assert f(p, 3, p, None, 3, None, None, None, 0, None, None, None, None, None) == 1 and b"no output" in lib.ndp_last_error()
    assert f(ctypes.c_void_p(4100), 3, p, None, 3, None, None, None, 0, None, p, None, None, None) == 1 \
        and b"16-byte" in lib.ndp_last_error()
    assert f(p, 3, None, ctypes.c_void_p(4097), 3, None, None, None, 0, None, p, None, None, None) == 1 \
        and b"4-byte" in lib.ndp_last_error()
