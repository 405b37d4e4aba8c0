"""GPU: the evaluation of the forward (next-frame) model (ndivplanning_amd/forward_model_eval.py).  First the scoring
kernel alone (ndp_fm_score, csrc/ndp_eval.inc) against the plain numpy restatement of its stated definition
(tests/fm_eval_common.py), then predict / rollout / evaluate against the reference's own results
(tests/golden/fm_eval_case.npz) and the fp64 restatement (oracle.forward_model_oracle.forward(training=False) fed its own
predictions), then the trainer's validation switch.

Bounds.  One eval step is held to 2e-4 (max |difference| to the fp64 oracle), the bound of
test_eval_and_no_grad_forward_of_the_module_match_the_oracle.  For h > 1 the kernels' distance to the fp64 rollout is
held to 4 x the reference-fp32 CPU path's own distance to it at the same h (the golden samples against the oracle: the
factor covers a different summation order in each of the h passes) + the h = 1 bound.  An MSE moves by at most
2 sqrt(mse) x (max |difference| of the predictions) + its own fp32 rounding when the prediction moves (Cauchy-Schwarz on
mean((d + e)^2) - mean(d^2), e^2 neglected against it at e <= 3e-4)."""
import ctypes
import os
import time

import numpy as np
import pytest
import torch

import fm_eval_common as C
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_BOUND = 2e-4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ the kernel alone
@pytest.fixture(scope="module")
def FME():
    from ndivplanning_amd import _build, forward_model_eval
    _build.build()
    return forward_model_eval


def _kernel_case(n):
    rng = np.random.RandomState(30 + n)
    pred = C.boundary_images(n, seed=n)
    n_target, n_base = n + 1, n + 2
    tgt = rng.randint(0, 256, (n_target, 128, 128, 3)).astype(np.uint8)
    base = rng.randint(0, 256, (n_base, 128, 128, 3)).astype(np.uint8)
    tidx = rng.randint(0, n_target, n).astype(np.int32)
    bidx = rng.randint(0, n_base, n).astype(np.int32)
    tidx[0] = tidx[-1]                                               # a repeat
    return pred, tgt, base, tidx, bidx


@pytest.mark.parametrize("n", [1, 3, 5])
def test_score_matches_the_stated_definition(FME, n):
    pred, tgt, base, tidx, bidx = _kernel_case(n)
    if n > 1:
        pred[0, 2] = pred[1, 2]                                      # image 0 without its NaN / inf plane: a finite error
    want = C.want_mse(pred, np.arange(n), C.as_float_images(tgt), tidx)
    want_b = C.want_mse(C.as_float_images(base), bidx, C.as_float_images(tgt), tidx)
    results = {}
    for tk in ("u8", "f32"):
        for bk in ("u8", "f32"):
            t = _dev(tgt if tk == "u8" else C.as_float_images(tgt))
            b = _dev(base if bk == "u8" else C.as_float_images(base))
            err, base_err, by = FME.score(_dev(pred), t, _dev(tidx), base=b, base_idx=_dev(bidx), out_bytes=True)
            again = FME.score(_dev(pred), t, _dev(tidx), base=b, base_idx=_dev(bidx), out_bytes=True)
            assert all(_bits(x) == _bits(y) for x, y in zip((err, base_err, by), again))         # two calls, the same bits
            results[(tk, bk)] = (err, base_err)
            # bytes: bit for bit (byte boundaries and one ulp either side, beyond +-1, NaN, inf)
            assert np.array_equal(by.cpu().numpy(), C.want_bytes(pred)), (tk, bk)
            got, got_b = err.cpu().numpy(), base_err.cpu().numpy()
            print("n %d %s/%s ulps: pred_err %s base_err %s" % (n, tk, bk, C.ulps(got, want), C.ulps(got_b, want_b)))
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert (C.ulps(got[ok], want[ok]) <= 1).all() and (C.ulps(got_b, want_b) <= 1).all()
    # byte and float operands of the same bytes: identical bits
    for key in results:
        assert _bits(results[key][0]) == _bits(results[("u8", "u8")][0])
        assert _bits(results[key][1]) == _bits(results[("u8", "u8")][1])
    # each output alone, and without index maps (image i uses row i)
    t, b = _dev(tgt), _dev(base)
    only_err = FME.score(_dev(pred), t, _dev(tidx))
    assert only_err[1] is None and only_err[2] is None and _bits(only_err[0]) == _bits(results[("u8", "u8")][0])
    only_bytes = FME.score(_dev(pred), out_bytes=True)
    assert only_bytes[0] is None and np.array_equal(only_bytes[2].cpu().numpy(), C.want_bytes(pred))
    ident = FME.score(_dev(pred), t, base=b)
    want_i = C.want_mse(C.as_float_images(base), np.arange(n), C.as_float_images(tgt), np.arange(n))
    assert (C.ulps(ident[1].cpu().numpy(), want_i) <= 1).all()


def test_out_of_range_indices_give_nan_for_that_image_only(FME):
    pred, tgt, base, tidx, bidx = _kernel_case(5)
    pred[0, 2] = pred[1, 2]
    good = FME.score(_dev(pred), _dev(tgt), _dev(tidx), base=_dev(base), base_idx=_dev(bidx), out_bytes=True)
    tidx2, bidx2 = tidx.copy(), bidx.copy()
    tidx2[1], tidx2[3], bidx2[0], bidx2[4] = -1, len(tgt), len(base), -1
    bad = FME.score(_dev(pred), _dev(tgt), _dev(tidx2), base=_dev(base), base_idx=_dev(bidx2), out_bytes=True)
    err, base_err = bad[0].cpu().numpy(), bad[1].cpu().numpy()
    assert np.isnan(err[[1, 3]]).all() and np.isnan(base_err[[0, 1, 3, 4]]).all()
    for i in (0, 2, 4):
        assert err[i].tobytes() == good[0].cpu().numpy()[i].tobytes()
    assert base_err[2].tobytes() == good[1].cpu().numpy()[2].tobytes()
    assert _bits(bad[2]) == _bits(good[2])                          # the bytes do not depend on the indices


def test_bad_arguments_launch_nothing(FME):
    from ndivplanning_amd import _capi
    lib = _capi.load()
    n = 3
    pred = torch.zeros(n, 3, 128, 128, device=DEV)
    tf, tu = torch.zeros(n, 3, 128, 128, device=DEV), torch.zeros(n, 128, 128, 3, dtype=torch.uint8, device=DEV)
    err, base_err = torch.full((n,), -7.0, device=DEV), torch.full((n,), -7.0, device=DEV)
    by = torch.full((n, 128, 128, 3), 0xA5, dtype=torch.uint8, device=DEV)
    p, st = _capi.ptr, _capi.stream_ptr(torch.device(DEV))

    def call(pred_=pred, n_=n, tf_=None, tu_=tu, nt=n, bf=None, bu=None, nb=0, bidx=None, e=err, be=None, u8=by):
        return lib.ndp_fm_score(p(pred_), n_, p(tf_), p(tu_), nt, None, p(bf), p(bu), nb, p(bidx), p(e), p(be), p(u8), st)

    idx = torch.zeros(n, dtype=torch.int32, device=DEV)
    for name, run, word in (
            ("two targets", lambda: call(tf_=tf), b"two targets"),
            ("no target", lambda: call(tu_=None), b"no target"),
            ("base without base_err", lambda: call(bf=tf, nb=n), b"without base_err"),
            ("base_err without a base", lambda: call(be=base_err), b"without a base"),
            ("base_idx without a base", lambda: call(bidx=idx), b"without a base"),
            ("two bases", lambda: call(bf=tf, bu=tu, nb=n, be=base_err), b"two base"),
            ("no output", lambda: call(e=None, u8=None), b"no output"),
            ("n = 0", lambda: call(n_=0), b"image count"),
            ("n < 0", lambda: call(n_=-2), b"image count"),
            ("n_target = 0", lambda: call(nt=0), b"n_target"),
            ("n_base = 0", lambda: call(bf=tf, nb=0, be=base_err), b"n_base"),
            ("null pred", lambda: call(pred_=None), b"null"),
            ("misaligned floats", lambda: lib.ndp_fm_score(ctypes.c_void_p(pred.data_ptr() + 4), n, None, p(tu), n, None, None, None, 0,
                                                   None, p(err), None, None, st), b"16-byte"),
            ("misaligned bytes", lambda: lib.ndp_fm_score(p(pred), n, None, ctypes.c_void_p(tu.data_ptr() + 1), n, None, None, None, 0,
                                                  None, p(err), None, None, st), b"4-byte")):
        rc = run()
        assert rc == 1 and word in lib.ndp_last_error(), (name, rc, lib.ndp_last_error())
    torch.cuda.synchronize()
    assert (err == -7).all() and (base_err == -7).all() and (by == 0xA5).all()                   # the sentinels stand
    assert call(bf=tf, nb=n, be=base_err) == 0                                                   # and a good call does run
    torch.cuda.synchronize()
    assert (err == 1.0).all() and (base_err == 1.0).all() and (by == 127).all()                  # 0 against byte 0 = -1; (0+1)/2*255


def test_base_err_is_what_ndp_eval_mse_gives_for_the_same_pairs(FME):
    """ndp_eval_mse takes the difference of the two floats in fp64, ndp_fm_score in fp32 (as ndp_ae_decode's error), and
    the two sum in different fixed orders.  Where every difference is exact in fp32 and every partial sum exact in fp64
    -- values that are multiples of 2^-10 in [-1, 1]: squares are multiples of 2^-20 up to 4, 49,152 of them need 38 bits
    -- neither matters and the bits must be equal.  On the byte table's values the fp32 difference carries a relative
    error of at most 2^-24, its square 2^-23, which is 1 fp32 ulp of the mean at most: held to 1 ulp."""
    from ndivplanning_amd import _capi
    lib = _capi.load()
    n, n_t, n_b = 5, 4, 3
    rng = np.random.RandomState(7)
    tidx, bidx = rng.randint(0, n_t, n).astype(np.int32), rng.randint(0, n_b, n).astype(np.int32)
    pred = torch.zeros(n, 3, 128, 128, device=DEV)
    for kind in ("exact", "bytes"):
        if kind == "exact":
            tgt = (rng.randint(-1024, 1025, (n_t, 3, 128, 128)) / 1024.0).astype(np.float32)
            base = (rng.randint(-1024, 1025, (n_b, 3, 128, 128)) / 1024.0).astype(np.float32)
        else:
            tgt = C.as_float_images(rng.randint(0, 256, (n_t, 128, 128, 3)).astype(np.uint8))
            base = C.as_float_images(rng.randint(0, 256, (n_b, 128, 128, 3)).astype(np.uint8))
        t, b = _dev(tgt), _dev(base)
        _, base_err, _ = FME.score(pred, t, _dev(tidx), base=b, base_idx=_dev(bidx))
        mse = torch.empty(n, device=DEV)
        ws = torch.empty(lib.ndp_eval_mse_ws_floats(n) + 2, device=DEV)
        ws = ws[(-(ws.data_ptr() // 4)) % 2:]                                                    # 8-byte aligned
        p = _capi.ptr
        d_bidx, d_tidx = _dev(bidx), _dev(tidx)                                                  # (kept alive over the call)
        _capi.check(lib.ndp_eval_mse(p(b), n_b, p(t), n_t, p(d_bidx), p(d_tidx), n, C.VALUES, 1, p(mse), None, p(ws),
                                     _capi.stream_ptr(torch.device(DEV))), "ndp_eval_mse")
        got, ref = base_err.cpu().numpy(), mse.cpu().numpy()
        print(kind, "base_err", got, "ndp_eval_mse", ref)
        if kind == "exact":
            assert got.tobytes() == ref.tobytes()
        else:
            assert (C.ulps(got, ref.astype(np.float64)) <= 1).all()


# ------------------------------------------------------------------------------------------------ predict / rollout
@pytest.fixture(scope="module")
def case(FME):
    """The golden recipe replayed: the mirror's module on the GPU in eval mode, the fp64 oracle's rollouts (computed once,
    shared, never changed) and the reference-fp32 path's own distance to them per h."""
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    torch.set_num_threads(8)
    g, R = load_golden("fm_eval_case"), C.recipe()
    cpu_model = R.build_module(ForwardAutoencoder)
    frames_u8, actions = R.inputs()
    assert np.array_equal(g["frames_u8"], frames_u8.numpy())
    order = [tuple(int(v) for v in row) for row in g["order"]]
    oracle = C.oracle_rollouts(cpu_model.state_dict(), R.norm_frames(frames_u8), actions, order)
    ref_dist = {}
    for i, (_, _, h) in enumerate(order):
        d = float((oracle[i][:, ::16, ::16] - torch.from_numpy(g["pred_sample"][i]).double()).abs().max())
        ref_dist[h] = max(ref_dist.get(h, 0.0), d)
    print("reference fp32 to fp64 rollout, max |difference| over the samples per h:", ref_dist)
    model = cpu_model.to(DEV).eval()
    return dict(g=g, R=R, model=model, frames=frames_u8.to(DEV), frames_cpu=frames_u8, actions=actions.to(DEV), order=order,
                oracle=oracle, ref_dist=ref_dist, where={o: i for i, o in enumerate(order)})


def _check_prediction(case, i, pred, err, base_err, pred_u8=None):
    """Prediction `i` of the golden order: pred float32 [3,128,128] (device), its errors (host floats)."""
    g, (b, t, h) = case["g"], case["order"][i]
    oracle = case["oracle"][i]
    full = float((pred.cpu().double() - oracle).abs().max())
    at_samples = float((pred.cpu().double() - oracle)[:, ::16, ::16].abs().max())
    bound = STEP_BOUND if h == 1 else 4.0 * case["ref_dist"][h] + STEP_BOUND
    print("prediction %d (traj %d start %d h %d): kernels to fp64 rollout %.3e (samples %.3e), reference fp32 %.3e, bound %.3e"
          % (i, b, t, h, full, at_samples, case["ref_dist"][h], bound))
    assert full <= bound, (i, h, full, bound)
    # the reference's own numbers
    assert float(np.abs(pred.cpu().numpy()[:, ::16, ::16] - g["pred_sample"][i]).max()) <= bound + case["ref_dist"][h]
    mse = float(g["pred_mse"][i])
    assert abs(err - mse) <= 2.0 * np.sqrt(mse) * (bound + case["ref_dist"][h]) + 2e-6 * mse, (i, err, mse)
    assert abs(base_err - float(g["persistence_mse"][i])) <= 2e-6 * base_err, (i, base_err, g["persistence_mse"][i])
    if pred_u8 is not None:
        got = pred_u8.cpu().numpy().transpose(2, 0, 1)[:, ::16, ::16].astype(np.int64)
        ref = g["pred_u8_sample"][i].astype(np.int64)
        assert (np.abs(got - ref) <= 1).all() and (got == ref).mean() > 0.98, i      # a byte moves where rounding crosses a boundary


def test_predict_three_images_against_the_reference_and_the_oracle(FME, case):
    model, frames, actions = case["model"], case["frames"], case["actions"]
    state, target, act = frames[0, 0:3], frames[0, 1:4], actions[0, 0:3]
    pred, err, base_err, mean = FME.predict(model, state, act, target)
    assert pred.shape == (3, 3, 128, 128) and pred.dtype == torch.float32 and err.shape == base_err.shape == (3,)
    by, err_b, base_b, mean_b = FME.predict(model, state, act, target, out="bytes")
    assert by.shape == (3, 128, 128, 3) and by.dtype == torch.uint8
    assert np.array_equal(by.cpu().numpy(), C.want_bytes(pred.cpu().numpy()))
    assert _bits(err) == _bits(err_b) and _bits(base_err) == _bits(base_b) and _bits(mean) == _bits(mean_b)
    assert float(mean) == float(np.float32(err.cpu().numpy().astype(np.float64).mean()))
    for t in range(3):
        _check_prediction(case, case["where"][(0, t, 1)], pred[t], float(err[t]), float(base_err[t]), by[t])
    # the errors are the stated definition of the kernels' own prediction, to the ulp
    tgt = C.as_float_images(target.cpu().numpy())
    assert (C.ulps(err.cpu().numpy(), C.want_mse(pred.cpu().numpy(), np.arange(3), tgt, np.arange(3))) <= 1).all()
    # float frames of the same bytes (state and target): the same bits; no target: no errors
    f_state, f_target = _dev(C.as_float_images(state.cpu().numpy())), _dev(tgt)
    pred_f, err_f, base_f, _ = FME.predict(model, f_state, act, f_target)
    assert _bits(pred_f) == _bits(pred) and _bits(err_f) == _bits(err) and _bits(base_f) == _bits(base_err)
    alone = FME.predict(model, state, act)
    assert _bits(alone[0]) == _bits(pred) and alone[1:] == (None, None, None)
    assert _bits(FME.predict(model, state, act, out="bytes")[0]) == _bits(by)


def test_rollout_feeds_the_model_its_own_predictions(FME, case):
    model, frames, actions = case["model"], case["frames"], case["actions"]
    preds, err, base = FME.rollout(model, frames[:, 0], actions[:, 0:3], frames[:, 1:4])
    assert preds.shape == (2, 3, 3, 128, 128) and err.shape == base.shape == (2, 3)
    by, err_b, _ = FME.rollout(model, frames[:, 0], actions[:, 0:3], frames[:, 1:4], out="bytes")
    assert by.shape == (2, 3, 128, 128, 3) and _bits(err) == _bits(err_b)
    for b in range(2):
        for h in (1, 2, 3):
            _check_prediction(case, case["where"][(b, 0, h)], preds[b, h - 1], float(err[b, h - 1]), float(base[b, h - 1]),
                              by[b, h - 1])
    assert np.array_equal(by.cpu().numpy().reshape(-1, 128, 128, 3), C.want_bytes(preds.cpu().numpy().reshape(-1, 3, 128, 128)))
    # without targets: the same predictions, no errors
    alone = FME.rollout(model, frames[:, 0], actions[:, 0:3])
    assert _bits(alone[0]) == _bits(preds) and alone[1] is None and alone[2] is None


class _Trajectories(torch.utils.data.Dataset):
    """Byte-frame (or JPEG-stream) trajectories held in memory, with PushDataset's item contract."""

    def __init__(self, frames, actions, mode="frames_u8"):
        self.frames, self.actions, self.mode, self.seq_length = frames, actions, mode, len(frames[0])

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i], torch.zeros(self.seq_length, 25), self.actions[i], torch.zeros(3)


def test_evaluate_the_golden_trajectories_from_every_start_frame(FME, case):
    g = case["g"]
    ds = _Trajectories(case["frames_cpu"], case["actions"].cpu())
    res = FME.evaluate(case["model"], ds, batch_size=2, keep=2)
    index = [tuple(int(v) for v in row) for row in res["index"].cpu().numpy()]
    assert sorted(index) == sorted(case["order"]) and res["counts"].tolist() == [6, 4, 2]
    err, base = res["errors"].cpu().numpy(), res["persistence"].cpu().numpy()
    for j, key in enumerate(index):
        i, h = case["where"][key], key[2]
        bound = (STEP_BOUND if h == 1 else 4.0 * case["ref_dist"][h] + STEP_BOUND) + case["ref_dist"][h]
        mse = float(g["pred_mse"][i])
        assert abs(float(err[j]) - mse) <= 2.0 * np.sqrt(mse) * bound + 2e-6 * mse, (key, err[j], mse)
        assert abs(float(base[j]) - float(g["persistence_mse"][i])) <= 2e-6 * float(base[j])
    for h in (1, 2, 3):
        sel = [j for j, key in enumerate(index) if key[2] == h]
        assert float(res["horizon_mse"][h - 1]) == float(np.float32(err[sel].astype(np.float64).mean()))
        assert float(res["persistence_mse"][h - 1]) == float(np.float32(base[sel].astype(np.float64).mean()))
    # strips: T - H = 1 start per trajectory lives for all 3 steps
    s = res["strips"]
    assert s["start"].shape == (2, 128, 128, 3) and s["targets"].shape == s["predictions"].shape == (2, 3, 128, 128, 3)
    assert torch.equal(s["start"], case["frames"][:, 0]) and torch.equal(s["targets"], case["frames"][:, 1:4])
    by = FME.rollout(case["model"], case["frames"][:, 0], case["actions"][:, 0:3], out="bytes")[0]
    assert torch.equal(s["predictions"], by)


# ------------------------------------------------------------------------------------------------ evaluate
@pytest.fixture(scope="module")
def synthetic_model(case):
    return case["model"]


def test_evaluate_synthetic_trajectories(FME, synthetic_model):
    from ndivplanning_amd.utils.trajectory_loader import SyntheticPushDataset
    model, N, T = synthetic_model, 3, 4
    for mode in ("images", "frames_u8"):
        ds = SyntheticPushDataset(N, seq_length=T, mode=mode, seed=5)
        res = FME.evaluate(model, ds, batch_size=2)                 # batches of 2 and 1 trajectories
        again = FME.evaluate(model, ds, batch_size=2)
        for k in ("one_step_mse", "horizon_mse", "persistence_mse", "counts", "errors", "persistence", "index"):
            assert _bits(res[k]) == _bits(again[k]), (mode, k)       # two runs: bit-identical
        assert res["counts"].tolist() == [N * (T - h) for h in (1, 2, 3)]
        assert _bits(res["horizon_mse"][:1]) == _bits(res["one_step_mse"]) and res["one_step_mse"].shape == (1,)
        assert "strips" not in res and res["errors"].shape == (N * 6,) and res["index"].shape == (N * 6, 3)
        # a shorter horizon is a prefix of the work
        short = FME.evaluate(model, ds, horizon=1, batch_size=3)
        assert short["counts"].tolist() == [N * (T - 1)] and short["horizon_mse"].shape == (1,)
        # against rollout called per trajectory and start
        index = res["index"].cpu().numpy()
        err, base = res["errors"].cpu().numpy(), res["persistence"].cpu().numpy()
        for i in range(N):
            frames, _, actions, _ = ds[i]
            frames, actions = frames.to(DEV), actions.to(DEV)
            for t in range(T - 1):
                H = T - 1 - t
                _, e, p = FME.rollout(model, frames[t:t + 1], actions[None, t:t + H], frames[None, t + 1:t + 1 + H])
                for h in range(1, H + 1):
                    j = int(np.flatnonzero((index == (i, t, h)).all(axis=1))[0])
                    # the same images in another batch: both are within the bound of the exact rollout (the reference
                    # path's own distance, 1e-7 on the golden case, is nothing against it), so within twice it of each other
                    bound = 2.0 * np.sqrt(float(err[j])) * 2 * STEP_BOUND + 2e-6 * float(err[j])
                    assert abs(float(e[0, h - 1]) - float(err[j])) <= bound, (mode, i, t, h, float(e[0, h - 1]), err[j])
                    assert float(p[0, h - 1]) == float(base[j])


def test_evaluate_jpeg_streams_and_their_decoded_frames_give_the_same_bits(FME, synthetic_model):
    import io
    from PIL import Image
    from ndivplanning_amd.utils.trajectory_loader import SyntheticPushDataset
    N, T = 3, 4
    jpeg = SyntheticPushDataset(N, seq_length=T, mode="jpeg", seed=6)
    items = [jpeg[i] for i in range(N)]
    frames = [torch.from_numpy(np.stack([np.array(Image.open(io.BytesIO(s))) for s in it[0]])) for it in items]
    decoded = _Trajectories(frames, [it[2] for it in items])
    streams = _Trajectories([it[0] for it in items], [it[2] for it in items], mode="jpeg")
    a = FME.evaluate(synthetic_model, streams, batch_size=2, keep=1)
    b = FME.evaluate(synthetic_model, decoded, batch_size=2, keep=1)
    c = FME.evaluate(synthetic_model, jpeg, batch_size=2)            # the dataset class itself
    for k in ("one_step_mse", "horizon_mse", "persistence_mse", "counts", "errors", "persistence", "index"):
        assert _bits(a[k]) == _bits(b[k]) == _bits(c[k]), k
    for k in ("start", "targets", "predictions"):
        assert torch.equal(a["strips"][k], b["strips"][k])
    assert torch.equal(a["strips"]["start"][0].cpu(), frames[0][0])
    # smooth scenes: "the frame does not change" is a finite, positive error
    assert bool((a["persistence_mse"] > 0).all()) and bool(torch.isfinite(a["horizon_mse"]).all())


def test_command_line_prints_every_horizon_and_writes_strips(FME, synthetic_model, tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setattr(FME, "load_module", lambda path, device: synthetic_model)
    lines = []
    one_step = FME.main(["--model", "unused.pt", "--data", "synthetic:3:frames_u8", "--seq-length", "4", "--batch-size", "2",
                         "--device", DEV, "--save-dir", str(tmp_path / "strips"), "--num-save", "2"],
                        log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    assert lines[0].startswith("val_pred_loss: %s" % one_step) and len([ln for ln in lines if ln.startswith("horizon ")]) == 3
    assert "count 9" in lines[1] and "count 6" in lines[2] and "count 3" in lines[3] and "persistence_mse" in lines[1]
    png = Image.open(str(tmp_path / "strips" / "strip_001.png"))
    assert png.size == (128 * 4, 256) and sorted(os.listdir(str(tmp_path / "strips"))) == ["strip_000.png", "strip_001.png"]


# ------------------------------------------------------------------------------------------------ the trainer's switch
def _train_config(tmp_path, name, val):
    from ndivplanning_amd.utils.file import AttrDict
    forward = {"num_epochs": 2, "learning_rate": 2e-4, "report_feq": 10, "batch_size": 2, "epochs_per_stage": 10,
               "step_lr_gamma": 0.1}
    if val:
        forward.update(val_data_path="synthetic:2:frames_u8", val_every=1, val_horizon=2)
    return AttrDict({"random_seed": 0, "train_data_path": "synthetic:4:images", "gpu_id": 0, "trajectory_length": 3,
                     "forward_save_path": str(tmp_path / name), "training": {"forward": forward}})


def test_validation_changes_no_bit_of_training(tmp_path, caplog):
    import logging
    from ndivplanning_amd import train_forward_model as script
    real_step = script.ForwardModelTrainer.step
    runs = {}
    for name, val in (("with", True), ("without", False)):
        losses = []

        def spy(self, *a, _losses=losses, **kw):
            _losses.append(real_step(self, *a, **kw).clone())
            return self.loss
        script.ForwardModelTrainer.step = spy
        caplog.clear()
        try:
            with caplog.at_level(logging.INFO):
                hist = script.train(_train_config(tmp_path, name, val))
        finally:
            script.ForwardModelTrainer.step = real_step
        tr = script.train.last_trainer
        model_stats = torch.cat([b.detach().float().reshape(-1).cpu() for b in tr.model.buffers()])
        runs[name] = dict(hist=hist, losses=torch.cat(losses).cpu(), params=tr.params.cpu(), stats=tr.stats.cpu(),
                          buffers=model_stats, val=script.train.last_val, log=caplog.text, training=tr.model.training)
    a, b = runs["with"], runs["without"]
    assert a["losses"].numel() == 2 * 2 * 2 and _bits(a["losses"]) == _bits(b["losses"])          # every step's loss
    assert a["hist"] == b["hist"] and _bits(a["params"]) == _bits(b["params"]) and _bits(a["stats"]) == _bits(b["stats"])
    assert _bits(a["buffers"]) == _bits(b["buffers"]) and a["training"] and b["training"]
    assert "val_pred_loss" in a["log"] and "val_persistence_loss" in a["log"] and "val horizon 2" in a["log"]
    assert "val_pred_loss" not in b["log"] and b["val"] == []
    assert [e for e, _ in a["val"]] == [0, 1] and a["val"][0][1]["counts"] == [4, 2]
    v0, v1 = a["val"][0][1], a["val"][1][1]
    assert v0["one_step_mse"][0] == v0["horizon_mse"][0] and np.isfinite(v0["horizon_mse"]).all()
    assert v0["horizon_mse"] != v1["horizon_mse"]                    # the parameters moved in between: the trainer's were used
    assert v0["persistence_mse"] == v1["persistence_mse"]            # ... and the baseline does not depend on them


def _val_rank_main(rank, world, port, cfg_dict, out_dir):
    import logging
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", NDP_DIST_BACKEND="gloo", NDP_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    logging.basicConfig(filename=os.path.join(out_dir, "rank%d.log" % rank), level=logging.INFO, force=True)
    import torch.distributed as dist
    from ndivplanning_amd import train_forward_model as script
    from ndivplanning_amd.utils.file import AttrDict
    hist = script.train(AttrDict(cfg_dict))
    tr = script.train.last_trainer
    torch.save({"params": tr.params.cpu(), "stats": tr.stats.cpu(), "hist": hist, "val": script.train.last_val},
               os.path.join(out_dir, "rank%d.pt" % rank))
    logging.shutdown()
    dist.destroy_process_group()


def test_two_ranks_validate_on_rank_zero_alone(tmp_path):
    """train_forward_model.train under two processes (both on cuda:0, gloo), cross-rank BatchNorm on (the default), with
    val_data_path set: rank 0 evaluates alone -- no collective, the statistics hook is not invoked in eval mode, or this
    run would not end -- and the replicas stay bit-identical.  One attempt under its own time limit."""
    import socket
    import torch.multiprocessing as mp
    cfg = _train_config(tmp_path, "fm", True)
    cfg["train_data_path"] = "synthetic:4:images"
    cfg["training"]["forward"]["batch_size"] = 4
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in cfg.items()}
    cfg["training"] = {"forward": dict(cfg["training"]["forward"])}
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.start_processes(_val_rank_main, args=(2, port, cfg, str(tmp_path)), nprocs=2, join=False, start_method="spawn")
    deadline = time.monotonic() + 240
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail("the two-rank run with validation did not end within 240 s")
    res = [torch.load(str(tmp_path / ("rank%d.pt" % r))) for r in range(2)]
    assert torch.equal(res[0]["params"], res[1]["params"]) and torch.equal(res[0]["stats"], res[1]["stats"])
    assert res[0]["hist"] == res[1]["hist"] and len(res[0]["hist"]) == 2
    logs = [open(str(tmp_path / ("rank%d.log" % r))).read() for r in range(2)]
    assert logs[0].count("val_pred_loss") == 2 and "val_persistence_loss" in logs[0]
    assert "val_" not in logs[1] and "reconstruction loss per epoch" in logs[1]
    assert len(res[0]["val"]) == 2 and res[1]["val"] == []
