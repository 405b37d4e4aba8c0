"""ndp_image_quality on the GPU (csrc/ndp_eval.inc, ndivplanning_amd/image_quality.py): the golden pairs
(tests/golden/image_quality_case.npz -- SSIM by scipy's gaussian_filter in fp64, a route that is not the kernel's, and the
fp64 evaluation of the stated PSNR) through both operand kinds on both sides, with and without index maps; the exact-1, the
bit-equality and the NaN properties; the raw entry's argument errors; and the opt-in `quality` of the two evaluations, their
command lines and the forward trainer's validation switch.  The SSIM allowance is 4 * d32, read from the golden file
(tests/test_image_quality_host.py has the reasoning); each test prints the distances it measured before it asserts.
n <= 5 pairs except where the entry switches from 16-row to 32-row bands (12 pairs through an index map)."""
import logging

import numpy as np
import pytest
import torch

import quality_common as Q
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def IQ():
    from ndivplanning_amd import _build, image_quality
    _build.build()
    return image_quality


@pytest.fixture(scope="module")
def rec():
    return load_golden("image_quality_case")


@pytest.fixture(scope="module")
def pairs(rec):
    return Q.golden_pairs(rec)


def _check(names, ssim, psnr, rec, what):
    """The results of the golden pairs `names` (None: not a golden pair) against the file."""
    allow = 4.0 * float(rec["d32"])
    ssim, psnr = ssim.cpu().numpy(), psnr.cpu().numpy()
    for p, name in enumerate(names):
        if name is None:
            continue
        k = Q.NAMES.index(name)
        want_s, want_p = float(rec["ssim64"][k]), float(rec["psnr64"][k])
        print("%s %-12s ssim %.9f (fp64 %.9f, off by %.3e, allowance %.3e)  psnr %.7g (fp64 %.7g)"
              % (what, name, ssim[p], want_s, abs(float(ssim[p]) - want_s), allow, psnr[p], want_p))
        if np.isnan(want_s):
            assert np.isnan(ssim[p]) and np.isnan(psnr[p]), (what, name)
            continue
        assert abs(float(ssim[p]) - want_s) <= allow, (what, name, ssim[p], want_s)
        if np.isinf(want_p):
            assert psnr[p] == np.inf, (what, name)
        else:
            assert Q.ulps(psnr[p], want_p) <= 1, (what, name, psnr[p], want_p)


def test_golden_pairs_every_operand_kind(IQ, rec, pairs):
    byte_pairs = [p for p in pairs if p[0] not in Q.FLOAT_ONLY]
    float_pairs = [p for p in pairs if p[0] in Q.FLOAT_ONLY]
    results = {}
    for lo in (0, 4):                                            # 4 and 3 pairs per call
        part = byte_pairs[lo:lo + 4]
        names = [p[0] for p in part]
        a_u8, b_u8 = np.stack([p[1] for p in part]), np.stack([p[2] for p in part])
        kinds = {"u8": (a_u8, b_u8), "f32": (Q.as_float_images(a_u8), Q.as_float_images(b_u8))}
        for ka in ("u8", "f32"):
            for kb in ("u8", "f32"):
                ssim, psnr = IQ.image_quality(_dev(kinds[ka][0]), _dev(kinds[kb][1]))
                assert ssim.shape == psnr.shape == (len(part),) and ssim.dtype == psnr.dtype == torch.float32 and ssim.is_cuda
                _check(names, ssim, psnr, rec, "a %s b %s" % (ka, kb))
                results[(lo, ka, kb)] = _bits(ssim) + _bits(psnr)
        # bytes and the floats of the same bytes: identical bits, on either side
        assert len({results[(lo, ka, kb)] for ka in ("u8", "f32") for kb in ("u8", "f32")}) == 1
    names = [p[0] for p in float_pairs]
    ssim, psnr = IQ.image_quality(_dev(np.stack([p[1] for p in float_pairs])), _dev(np.stack([p[2] for p in float_pairs])))
    _check(names, ssim, psnr, rec, "floats")
    # the NaN pair alone is NaN; its neighbours are not
    assert np.isnan(ssim.cpu().numpy()).tolist() == [n == "one_nan" for n in names]


def test_identical_images_give_exactly_one(IQ, rec, pairs):
    img = rec["images_u8"][:5]
    for a in (_dev(img), _dev(Q.as_float_images(img))):
        ssim, psnr = IQ.image_quality(a, a.clone())
        assert (ssim.cpu().numpy() == np.float32(1.0)).all() and (psnr.cpu().numpy() == np.inf).all()
    out = _dev(np.stack([p[1] for p in pairs if p[0] in ("outside_1", "outside_2")]))       # clamped values too
    ssim, psnr = IQ.image_quality(out, out.clone())
    assert (ssim.cpu().numpy() == np.float32(1.0)).all() and (psnr.cpu().numpy() == np.inf).all()


def test_index_maps_repeats_and_out_of_range(IQ, rec):
    pool = rec["images_u8"]
    names = [str(n) for n in rec["image_names"]]
    at, n_pool = names.index, len(names)
    a_idx = torch.tensor([at("scene0"), at("scene0"), -1, at("noise0"), n_pool], dtype=torch.int32)
    b_idx = torch.tensor([at("scene1"), n_pool, at("noise1"), at("noise1"), at("scene0")], dtype=torch.int32)
    golden_names = ["unrelated", None, None, "byte_noise", None]
    got = {}
    for kind, images in (("u8", _dev(pool)), ("f32", _dev(Q.as_float_images(pool)))):
        ssim, psnr = IQ.image_quality(images, images, a_idx=a_idx, b_idx=b_idx.to(DEV))
        _check(golden_names, ssim, psnr, rec, "mapped " + kind)
        s, p = ssim.cpu().numpy(), psnr.cpu().numpy()
        assert np.isnan(s[[1, 2, 4]]).all() and np.isnan(p[[1, 2, 4]]).all() and np.isfinite(s[[0, 3]]).all()
        got[kind] = _bits(ssim) + _bits(psnr)
        # the mapped pairs are the gathered ones, bit for bit; one side mapped, int64 indices
        ga, gb = images[[at("scene0"), at("noise0")]], images[[at("scene1"), at("noise1")]]
        s2, p2 = IQ.image_quality(ga, gb)
        assert _bits(s2) == _bits(ssim[[0, 3]]) and _bits(p2) == _bits(psnr[[0, 3]])
        s3, p3 = IQ.image_quality(ga, images, b_idx=torch.tensor([at("scene1"), at("noise1")]))
        assert _bits(s3) == _bits(s2) and _bits(p3) == _bits(p2)
    assert got["u8"] == got["f32"]
    with pytest.raises(Exception, match="number of pairs"):
        IQ.image_quality(_dev(pool[:2]), _dev(pool[:3]))
    with pytest.raises(Exception, match="number of pairs"):
        IQ.image_quality(_dev(pool[:2]), _dev(pool[:3]), a_idx=torch.tensor([0, 1, 0, 1]))


def test_one_output_alone_a_second_call_and_the_band_split(IQ, rec):
    pool = _dev(rec["images_u8"])
    fl = _dev(Q.as_float_images(rec["images_u8"]))
    a_idx = torch.tensor([0, 0, 0, 7, 0], dtype=torch.int32)
    b_idx = torch.tensor([1, 2, 3, 8, 4], dtype=torch.int32)
    ssim, psnr = IQ.image_quality(pool, fl, a_idx=a_idx, b_idx=b_idx)
    s_only, none = IQ.image_quality(pool, fl, a_idx=a_idx, b_idx=b_idx, psnr=False)
    assert none is None and _bits(s_only) == _bits(ssim)
    none, p_only = IQ.image_quality(pool, fl, a_idx=a_idx, b_idx=b_idx, ssim=False)
    assert none is None and _bits(p_only) == _bits(psnr)
    again = IQ.image_quality(pool, fl, a_idx=a_idx, b_idx=b_idx)
    assert _bits(again[0]) == _bits(ssim) and _bits(again[1]) == _bits(psnr)
    # 12 pairs take the 32-row bands, 5 the 16-row bands (image_quality_band_rows): the same pairs, the same bits
    many_a, many_b = torch.cat([a_idx, a_idx, a_idx[:2]]), torch.cat([b_idx, b_idx, b_idx[:2]])
    s12, p12 = IQ.image_quality(pool, fl, a_idx=many_a, b_idx=many_b)
    assert s12.shape == (12,)
    assert _bits(s12[:5]) == _bits(ssim) and _bits(s12[5:10]) == _bits(ssim) and _bits(s12[10:]) == _bits(ssim[:2])
    assert _bits(p12[:5]) == _bits(psnr) and _bits(p12[5:10]) == _bits(psnr) and _bits(p12[10:]) == _bits(psnr[:2])
    # +-Inf clamp to the ends: the bits of finite values beyond the ends
    inf, big = fl[:1].clone(), fl[:1].clone()
    inf[0, 0, 3, 3], inf[0, 2, 100, 100] = float("inf"), float("-inf")
    big[0, 0, 3, 3], big[0, 2, 100, 100] = 5.0, -5.0
    ri, rb = IQ.image_quality(inf, pool[1:2]), IQ.image_quality(big, pool[1:2])
    assert bool(torch.isfinite(ri[0]).all()) and _bits(ri[0]) == _bits(rb[0]) and _bits(ri[1]) == _bits(rb[1])


def test_raw_entry_argument_errors_launch_nothing(IQ):
    from ndivplanning_amd import _capi
    lib = _capi.load()
    n = 2
    f = torch.full((n, 3, 128, 128), -1.0, device=DEV)            # the floats of the zero bytes
    u = torch.zeros(n, 128, 128, 3, dtype=torch.uint8, device=DEV)
    ws_bytes = int(lib.ndp_image_quality_ws_bytes(n))
    assert ws_bytes == n * (3 * 118 + 3 * 128) * 8 and lib.ndp_image_quality_ws_bytes(0) == 0
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=DEV)
    ssim = torch.full((n,), -7.0, device=DEV)
    psnr = torch.full((n,), -7.0, device=DEV)
    p, st = _capi.ptr, _capi.stream_ptr(torch.device(DEV))

    def call(a_f=f, a_u=None, n_a=n, b_f=None, b_u=u, n_b=n, pairs=n, s=ssim, q=psnr, w=ws, wb=ws_bytes):
        return lib.ndp_image_quality(p(a_f), p(a_u), n_a, None, p(b_f), p(b_u), n_b, None, pairs, p(s), p(q), p(w), wb, st)
    bad = [dict(a_u=u), dict(a_f=None), dict(b_f=f), dict(b_u=None), dict(s=None, q=None), dict(pairs=0), dict(n_a=0),
           dict(n_b=0), dict(wb=ws_bytes - 8), dict(w=None)]
    for kw in bad:
        assert call(**kw) == 1, kw                                # NDP_E_ARG
        assert lib.ndp_last_error(), kw
    torch.cuda.synchronize()
    assert (ssim == -7).all() and (psnr == -7).all()              # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert (ssim == 1).all() and (psnr == float("inf")).all()     # black against black


# ------------------------------------------------------------------------------------------------ the evaluations
@pytest.fixture(scope="module")
def fwd_model():
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    torch.manual_seed(3)
    model = ForwardAutoencoder()
    model.decoder.weight_init(mean=0.0, std=0.03)                # a residual that matters (tests/golden/make_golden_fm_eval.py)
    model.encoder.weight_init(mean=0.0, std=0.03)
    return model.to(DEV).eval()


PRESENT = ("one_step_mse", "horizon_mse", "persistence_mse", "counts", "errors", "persistence", "index")


def test_forward_model_evaluate_with_quality(IQ, fwd_model):
    from ndivplanning_amd import forward_model_eval as FME
    ds = FME.make_dataset("synthetic:3:frames_u8", seq_length=4)
    plain = FME.evaluate(fwd_model, ds, batch_size=2)
    res = FME.evaluate(fwd_model, ds, batch_size=2, quality=True)
    assert set(res) == set(plain) | {"horizon_ssim", "horizon_psnr", "persistence_ssim", "persistence_psnr", "quality"}
    for k in PRESENT:
        assert _bits(res[k]) == _bits(plain[k]), k                # nothing that existed moves
    q = res["quality"]
    P = int(res["errors"].numel())
    assert set(q) == {"ssim", "psnr", "persistence_ssim", "persistence_psnr"} and all(v.shape == (P,) for v in q.values())
    index = res["index"].cpu().numpy()
    # per-pair calls: the start frame against its target, and the prediction of a rollout of its own
    for j in range(0, P, 3):
        i, t, h = (int(v) for v in index[j])
        frames, _, actions, _ = ds[i]
        frames, actions = frames.to(DEV), actions.to(DEV)
        s, p = IQ.image_quality(frames[t:t + 1], frames[t + h:t + h + 1])
        assert _bits(s) == _bits(q["persistence_ssim"][j:j + 1]) and _bits(p) == _bits(q["persistence_psnr"][j:j + 1])
        out = FME.rollout(fwd_model, frames[t:t + 1], actions[None, t:t + h], frames[None, t + 1:t + 1 + h], quality=True)
        assert len(out) == 7 and all(v.shape == (1, h) for v in out[3:])
        s, p = IQ.image_quality(out[0][0, h - 1:h], frames[t + h:t + h + 1])
        assert _bits(s) == _bits(out[3][0, h - 1:h]) and _bits(p) == _bits(out[4][0, h - 1:h])
        assert _bits(out[5][0, h - 1:h]) == _bits(q["persistence_ssim"][j:j + 1])
    # the predictions' values: the first batch's passes replayed (the same forward calls, so the same bits), every pair
    # scored by a call of its own
    T, b = 4, 2
    frames = torch.cat([ds[i][0] for i in range(b)]).to(DEV)
    flat_actions = torch.cat([ds[i][2] for i in range(b)]).to(DEV).float()
    state = None
    for h in (1, 2, 3):
        alive = T - h
        rows = (torch.arange(b)[:, None] * T + torch.arange(alive)[None, :]).reshape(-1).to(DEV)
        state = frames[rows] if h == 1 else state.view(b, alive + 1, 3, 128, 128)[:, :alive].reshape(b * alive, 3, 128, 128)
        state = FME._forward(fwd_model, state, flat_actions[rows + h - 1])
        for k, row in enumerate(rows.tolist()):
            j = int(np.flatnonzero((index == (row // T, row % T, h)).all(axis=1))[0])
            s, p = IQ.image_quality(state[k:k + 1], frames[row + h:row + h + 1])
            assert _bits(s) == _bits(q["ssim"][j:j + 1]) and _bits(p) == _bits(q["psnr"][j:j + 1]), (row, h)
    for h in range(3):
        sel = torch.from_numpy(np.flatnonzero(index[:, 2] == h + 1)).to(DEV)
        for name, key in (("horizon_ssim", "ssim"), ("horizon_psnr", "psnr"), ("persistence_ssim", "persistence_ssim"),
                          ("persistence_psnr", "persistence_psnr")):
            want = np.float32(q[key][sel].cpu().numpy().astype(np.float64).mean())
            assert float(res[name][h]) == float(want), (name, h)
    assert bool(((q["ssim"] > -1) & (q["ssim"] <= 1)).all()) and bool(torch.isfinite(q["psnr"]).all())
    # predict: four more results; without a target they are None
    frames, _, actions, _ = ds[0]
    frames, actions = frames.to(DEV), actions.to(DEV)
    out = FME.predict(fwd_model, frames[:3], actions[:3], frames[1:4], quality=True)
    base = FME.predict(fwd_model, frames[:3], actions[:3], frames[1:4])
    assert len(out) == 8 and all(_bits(x) == _bits(y) for x, y in zip(out[:4], base))
    s, p = IQ.image_quality(out[0], frames[1:4])
    assert _bits(s) == _bits(out[4]) and _bits(p) == _bits(out[5])
    s, p = IQ.image_quality(frames[:3], frames[1:4])
    assert _bits(s) == _bits(out[6]) and _bits(p) == _bits(out[7])
    assert FME.predict(fwd_model, frames[:3], actions[:3], quality=True)[1:] == (None,) * 7


def test_forward_model_command_line_quality(fwd_model, monkeypatch):
    from ndivplanning_amd import forward_model_eval as FME
    monkeypatch.setattr(FME, "load_module", lambda path, device: fwd_model)
    args = ["--model", "unused.pt", "--data", "synthetic:3:frames_u8", "--seq-length", "4", "--batch-size", "2", "--device", DEV]
    plain, lines = [], []
    FME.main(args, log=lambda *a: plain.append(" ".join(str(x) for x in a)))
    FME.main(args + ["--quality"], log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    assert lines[:len(plain)] == plain and len(lines) == len(plain) + 3         # the present output, then three more lines
    for h, line in enumerate(lines[len(plain):], start=1):
        assert line.startswith("horizon %d: model_ssim " % h) and "persistence_ssim" in line and "model_psnr" in line


@pytest.fixture(scope="module")
def autoencoder():
    from ndivplanning_amd import train_autoencoder as T
    torch.manual_seed(4)
    enc, dec = T.build_models(torch.device(DEV))
    return enc.eval(), dec.eval()


def test_autoencoder_evaluate_with_quality_and_its_command_line(IQ, autoencoder, monkeypatch):
    from ndivplanning_amd import autoencoder_eval as AE
    from ndivplanning_amd.utils.trajectory_loader import SyntheticPushDataset
    enc, dec = autoencoder
    ds = SyntheticPushDataset(2, seq_length=3, mode="images", seed=4)
    mean, per_image = AE.evaluate(enc, dec, ds, batch_size=1)
    out = AE.evaluate(enc, dec, ds, batch_size=1, quality=True)
    assert len(out) == 3 and _bits(out[0]) == _bits(mean) and _bits(out[1]) == _bits(per_image)
    q = out[2]
    assert set(q) == {"ssim", "psnr", "mean_ssim", "mean_psnr"} and q["ssim"].shape == q["psnr"].shape == (6,)
    frames = torch.cat([ds[i][0] for i in range(2)]).to(DEV)
    recon = AE.reconstruct(enc, dec, frames[:3])[0]              # the first batch: trajectory 0
    s, p = IQ.image_quality(recon, frames[:3])
    assert _bits(s) == _bits(q["ssim"][:3]) and _bits(p) == _bits(q["psnr"][:3])
    assert float(q["mean_ssim"]) == float(np.float32(q["ssim"].cpu().numpy().astype(np.float64).mean()))
    assert float(q["mean_psnr"]) == float(np.float32(q["psnr"].cpu().numpy().astype(np.float64).mean()))
    # with kept pairs: the third result stays what it is, the dict comes last
    kept = AE.evaluate(enc, dec, ds, batch_size=1, keep=2)
    both = AE.evaluate(enc, dec, ds, batch_size=1, keep=2, quality=True)
    assert len(both) == 4 and torch.equal(both[2][0], kept[2][0]) and torch.equal(both[2][1], kept[2][1])
    assert _bits(both[3]["ssim"]) == _bits(q["ssim"])
    # the command line
    monkeypatch.setattr(AE, "load_module", lambda path, device: enc if "encoder" in path else dec)
    args = ["--encoder", "encoder.pt", "--decoder", "decoder.pt", "--data", "synthetic:1:images", "--batch-size", "1", "--device", DEV]
    plain, lines = [], []
    AE.main(args, log=lambda *a: plain.append(a))
    AE.main(args + ["--quality"], log=lambda *a: lines.append(a))
    assert lines[:len(plain)] == plain and len(lines) == len(plain) + 1
    assert lines[-1][0] == "val_recon_ssim:" and lines[-1][2] == "val_recon_psnr:" and -1 < lines[-1][1] <= 1


def test_forward_training_is_bit_identical_with_val_quality(tmp_path, caplog):
    from ndivplanning_amd import train_forward_model as script
    from ndivplanning_amd.utils.file import AttrDict
    real_step = script.ForwardModelTrainer.step
    runs = {}
    for name, quality in (("with", True), ("without", False)):
        forward = {"num_epochs": 1, "learning_rate": 2e-4, "report_feq": 10, "batch_size": 2, "epochs_per_stage": 10,
                   "step_lr_gamma": 0.1, "val_data_path": "synthetic:2:frames_u8", "val_every": 1, "val_horizon": 2}
        if quality:
            forward["val_quality"] = True
        cfg = AttrDict({"random_seed": 0, "train_data_path": "synthetic:4:images", "gpu_id": 0, "trajectory_length": 3,
                        "forward_save_path": str(tmp_path / name), "training": {"forward": forward}})
        losses = []

        def spy(self, *a, _losses=losses, **kw):
            _losses.append(real_step(self, *a, **kw).clone())
            return self.loss
        script.ForwardModelTrainer.step = spy
        caplog.clear()
        try:
            with caplog.at_level(logging.INFO):
                hist = script.train(cfg)
        finally:
            script.ForwardModelTrainer.step = real_step
        tr = script.train.last_trainer
        runs[name] = dict(hist=hist, losses=torch.cat(losses).cpu(), params=tr.params.cpu(), stats=tr.stats.cpu(),
                          val=script.train.last_val, log=caplog.text)
    a, b = runs["with"], runs["without"]
    assert a["losses"].numel() == 4 and _bits(a["losses"]) == _bits(b["losses"]) and a["hist"] == b["hist"]
    assert _bits(a["params"]) == _bits(b["params"]) and _bits(a["stats"]) == _bits(b["stats"])
    assert "val_ssim" in a["log"] and "val_psnr" in a["log"] and "val_ssim" not in b["log"]
    va, vb = a["val"][0][1], b["val"][0][1]
    assert all(va[k] == vb[k] for k in vb) and len(va["horizon_ssim"]) == len(va["persistence_psnr"]) == 2
    assert "horizon_ssim" not in vb and all(-1 < v <= 1 for v in va["horizon_ssim"])
