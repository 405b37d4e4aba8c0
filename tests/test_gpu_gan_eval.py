"""GPU: the evaluation of the action generator (ndivplanning_amd/gan_eval.py).  First the scoring kernel alone
(ndp_gan_score, csrc/ndp_eval.inc) on the host driver's cases against the plain numpy restatement of its stated
definition (tests/gan_eval_common.py) and against ndp_ndiv_fwd_bwd, then sample / score / evaluate against the reference's
own results (tests/golden/gan_eval_case.npz, fp64), then the command line and the trainer's validation switch.

Bounds of the golden case.  action_hat is held to the project's 1e-4 of the fp64 reference (DELTA).  A sample's error
e = mean of 4 squares then moves by at most 2 sqrt(e) DELTA + 1e-8 (Cauchy-Schwarz, as test_gpu_forward_model_eval.py
propagates its step bound); a distance between two samples by at most the two samples' errors, 2e-4 for the spread as the
issue states it.  For ndiv the noise is an input and only x~_ij = dx_ij / s_i (s_i = sum_j dx_ij) moves: with every
component within DELTA a sample moves by at most 2 DELTA in norm, a distance by eps = 4 DELTA, s_i by (K - 1) eps, so
|x~'_ij - x~_ij| <= eps / s'_i + dx_ij (K - 1) eps / (s_i s'_i) with s'_i = s_i - (K - 1) eps, which sums over j to
2 (K - 1) eps / s'_i; relu is 1-Lipschitz, so the row's ndiv moves by at most sum_i 8 (K - 1) DELTA / s'_i (DESIGN.md
section 5k).  On top of that come the kernel's own bounds: 4 x the distance of the reference's fp32 result from its fp64
one, and the floors of tests/gan_eval_common.py."""
import ctypes
import logging
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch

import gan_eval_common as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTA = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def GE():
    from ndivplanning_amd import _build, gan_eval
    _build.build()
    return gan_eval


def _score(GE, case, wanted=None):
    got = GE.score(_dev(case["x"]), _dev(case["action"]), _dev(case["noise"]), _dev(case["logits"]), outputs=wanted)
    return {o: v.cpu().numpy() for o, v in got.items()}


# ------------------------------------------------------------------------------------------------ the kernel alone
def test_kernel_matches_the_stated_definition_on_the_host_drivers_cases(GE):
    worst = {}
    for case, wanted in C.cases():
        wanted = C.available(case) if wanted is None else wanted
        got, again = _score(GE, case, wanted), _score(GE, case, wanted)
        assert sorted(got) == sorted(wanted)
        for o in wanted:
            assert got[o].tobytes() == again[o].tobytes(), (case["name"], o)          # two launches, the same bits
        for o, m in C.check_scores(case, got, wanted).items():
            worst[o] = tuple(max(a, b) for a, b in zip(worst.get(o, (0, 0, 0)), m))
    for o, (dist, ref, tol) in sorted(worst.items()):
        print("%s: kernel to fp64 %.3g, torch fp32 to fp64 %.3g, bound %.3g" % (o, dist, ref, tol))


def test_absent_outputs_leave_the_others_bits_alone(GE):
    base = C.random_case(11, 6, 2, seed=102)
    full = _score(GE, base)
    for o in C.OUTPUTS:
        got = _score(GE, base, tuple(w for w in C.OUTPUTS if w != o))
        assert o not in got and all(got[w].tobytes() == full[w].tobytes() for w in got), o
    alone = _score(GE, C.without(base, "action", "noise", "logits"))
    assert list(alone) == ["spread"] and alone["spread"].tobytes() == full["spread"].tobytes()


@pytest.mark.parametrize("shape", [(11, 6, 2), (3, 7, 5)])
def test_row_shares_sum_to_the_training_kernels_loss(GE, shape):
    from ndivplanning_amd import diversity
    n, k, nz = shape
    case = C.random_case(n, k, nz, seed=200 + k)
    got = _score(GE, case, ("ndiv",))["ndiv"]
    loss = float(diversity.compute_pairwise_divergence(_dev(case["x"]), _dev(case["noise"])).item())
    want64 = C.want_scores(case["x"], None, case["noise"])["ndiv"].sum()
    t32 = torch.from_numpy(C.torch_fp32(case["x"], case["noise"])["ndiv"]).float().sum().item()
    bound = max(4.0 * abs(t32 - want64), n * 8 * k * C.EPS)
    total = got.astype(np.float64).sum()
    print("ndiv total: rows %.9g, ndp_ndiv_fwd_bwd %.9g, fp64 %.9g, torch fp32 %.9g, bound %.3g" % (total, loss, want64, t32, bound))
    assert want64 > 0.01 and abs(total - loss) <= bound and abs(total - want64) <= bound


def test_bad_arguments_launch_nothing(GE):
    from ndivplanning_amd import _capi
    lib = _capi.load()
    n, k, nz = 3, 6, 2
    c = C.random_case(n, k, nz, seed=5)
    x, action, noise, logits = (_dev(c[i]) for i in ("x", "action", "noise", "logits"))
    poison = {o: torch.full(C.out_shape(o, n, k), -12345, dtype=torch.int32 if o in C.INT_OUTPUTS else torch.float32, device=DEV)
              for o in C.OUTPUTS}
    before = {o: _bits(v) for o, v in poison.items()}
    p = _capi.ptr

    def call(outs, x_=x, n_=n, k_=k, action_=action, noise_=noise, nz_=nz, logits_=logits):
        rc = lib.ndp_gan_score(p(x_), n_, k_, p(action_), p(noise_), nz_, p(logits_),
                               *[p(poison[o]) if o in outs else None for o in C.OUTPUTS], _capi.stream_ptr(DEV))
        torch.cuda.synchronize()
        return rc

    bad = []
    for o in C.NEED_ACTION:
        bad.append(("%s without action" % o, call((o,), action_=None)))
    bad.append(("ndiv without noise", call(("ndiv",), noise_=None)))
    for o in C.NEED_LOGITS:
        bad.append(("%s without logits" % o, call((o,), logits_=None)))
    bad.append(("no output", call(())))
    bad.append(("no action_hat", call(C.OUTPUTS, x_=None)))
    for k_bad in (0, -1, 257):
        bad.append(("K = %d" % k_bad, call(C.OUTPUTS, k_=k_bad)))
    for nz_bad in (0, 17):
        bad.append(("nz = %d" % nz_bad, call(C.OUTPUTS, nz_=nz_bad)))
    bad.append(("n = 0", call(C.OUTPUTS, n_=0)))
    bad.append(("n K = 2^31", call(C.OUTPUTS, n_=(1 << 31) // k + 1)))
    for what, rc in bad:
        assert rc == 1, what                                         # NDP_E_ARG
    assert b"ndp_gan_score" in lib.ndp_last_error()
    assert all(_bits(poison[o]) == before[o] for o in C.OUTPUTS)      # nothing was written: nothing was launched
    assert call(C.OUTPUTS) == 0 and all(_bits(poison[o]) != before[o] for o in C.OUTPUTS)
    with pytest.raises(ValueError, match="needs noise"):
        GE.score(x, action, None, logits, outputs=("ndiv",))
    with pytest.raises(ValueError, match="needs fake_logits"):
        GE.score(x, action, noise, None, outputs=("d_pick_k",))
    with pytest.raises(ValueError, match="no output"):
        GE.score(x, action, noise, logits, outputs=())


# ------------------------------------------------------------------------------------------------ the golden case
@pytest.fixture(scope="module")
def golden():
    return np.load(C.GOLDEN)


def _golden_modules(golden, name):
    from ndivplanning_amd.models.gan import Decoder, Discriminator
    nz = int(golden[name + "/shape"][2])
    state = torch.get_rng_state()
    g, d = Decoder(noise_dim=nz), Discriminator()
    torch.set_rng_state(state)
    for net, m in (("g", g), ("d", d)):
        m.load_state_dict({key: torch.from_numpy(golden["%s/%s/%s" % (name, net, key)]) for key in m.state_dict()})
    return g.to(DEV).eval(), d.to(DEV).eval()


@pytest.mark.parametrize("name", ["a", "b"])
def test_golden_case_end_to_end(GE, golden, name):
    w = lambda key, tag="64": golden["%s/%s/%s" % (name, key, tag)]                       # noqa: E731
    n, k, nz = (int(v) for v in golden[name + "/shape"][:3])
    g, d = _golden_modules(golden, name)
    codes, actions, noise = (_dev(golden["%s/%s" % (name, i)]) for i in ("codes", "actions", "noise"))
    hat, used = GE.sample(g, codes, k, noise=noise)
    assert used.data_ptr() == noise.data_ptr() and tuple(hat.shape) == (n, k, 4)
    err_hat = np.abs(hat.cpu().numpy() - w("action_hat")).max()
    logits = GE.discriminate(d, hat, codes, code_rep=k).view(n, k)
    err_logit = np.abs(logits.cpu().numpy() - w("fake_logits")).max()
    print("%s: action_hat to fp64 %.3g, logits to fp64 %.3g (bound %.0e)" % (name, err_hat, err_logit, DELTA))
    assert err_hat <= DELTA and err_logit <= DELTA
    got = {o: v.cpu().numpy() for o, v in GE.score(hat, actions, noise, logits).items()}
    assert np.array_equal(got["best_k"], w("best_k")) and np.array_equal(got["d_pick_k"], w("d_pick_k"))      # all rows
    for o in ("sample_err", "mean_err", "best_err", "best_curve", "d_pick_err"):
        dist, bound = np.abs(got[o] - w(o)), 2.0 * np.sqrt(w(o)) * DELTA + 1e-8
        print("%s %s: to fp64 %.3g (bound %.3g)" % (name, o, dist.max(), bound.min()))
        assert (dist <= bound).all(), o
    kernel = {o: C.tolerance(o, w(o), w(o, "32").astype(np.float64), k) for o in ("spread", "ndiv", "d_fake_prob")}
    assert (np.abs(got["spread"] - w("spread")) <= 2 * DELTA + kernel["spread"]).all()
    assert (np.abs(got["d_fake_prob"] - w("d_fake_prob")) <= 0.25 * DELTA + kernel["d_fake_prob"]).all()
    dx = C.pair_distances(w("action_hat"))
    s = dx.sum(2) - (k - 1) * 4 * DELTA
    moved = (8.0 * (k - 1) * DELTA / s).sum(1)
    dist = np.abs(got["ndiv"] - w("ndiv"))
    print("%s ndiv: to fp64 %s, reference fp32 to fp64 %s, propagated term %s" % (name, dist, np.abs(w("ndiv", "32") - w("ndiv")), moved))
    assert (dist <= kernel["ndiv"] + moved).all()
    # the reference's reductions
    assert abs(got["mean_err"].astype(np.float64).mean() - float(w("action_mse"))) <= 2 * np.sqrt(float(w("action_mse"))) * DELTA + 1e-8
    real = torch.sigmoid(GE.discriminate(d, actions, codes)).cpu().numpy()
    assert (np.abs(real - w("d_real_prob")) <= 0.25 * DELTA + 1e-6).all()


# ------------------------------------------------------------------------------------------------ sample / evaluate
@pytest.fixture(scope="module")
def modules(golden):
    from ndivplanning_amd.models.image_autoencoder import Encoder
    g, d = _golden_modules(golden, "a")
    state = torch.get_rng_state()
    torch.manual_seed(3)
    enc = Encoder().to(DEV).eval()
    torch.set_rng_state(state)
    return g, d, enc


@pytest.mark.parametrize("num_sample", [1, 6])
def test_sample_gives_the_bits_of_the_materialised_input(GE, modules, num_sample):
    """The materialised input is built from the noise the DEVICE drew in the same call: this holds the layout
    cat(codes[r], noise[r, k]) and repeatability, not the stream.  tests/test_gpu_noise.py holds the drawn noise to the
    host restatement of the stream (tests/philox_ref.py)."""
    g = modules[0]
    codes = torch.randn(7, 256, generator=torch.Generator().manual_seed(1)).to(DEV)
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(0)
    hat, noise = GE.sample(g, codes, num_sample, seed=11)
    again, noise2 = GE.sample(g, codes, num_sample, seed=11)
    other = GE.sample(g, codes, num_sample, seed=12)[1]
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(0), gpu_state)
    assert tuple(noise.shape) == (7, num_sample, 2) and 0 <= float(noise.min()) and float(noise.max()) < 1
    assert _bits(noise) == _bits(noise2) and _bits(hat) == _bits(again) and _bits(noise) != _bits(other)
    z = torch.cat([torch.repeat_interleave(codes, num_sample, dim=0), noise.view(-1, 2)], dim=1)
    with torch.no_grad():
        assert _bits(g(z)) == _bits(hat)


@pytest.mark.parametrize("mode", ["codes", "frames_u8"])
def test_evaluate_synthetic_trajectories(GE, modules, mode):
    from ndivplanning_amd.train_gan import encode_batch
    g, d, enc = modules
    data = GE.make_dataset("synthetic:3:%s" % mode, seq_length=4)
    encoder = None if mode == "codes" else enc
    runs = {b: GE.evaluate(g, data, encoder=encoder, discriminator=d, num_sample=6, batch_size=b, seed=4) for b in (2, 3)}
    again = GE.evaluate(g, data, encoder=encoder, discriminator=d, num_sample=6, batch_size=2, seed=4)
    res = runs[2]
    for key in ("action_mse", "best_action_mse", "best_of_k_curve", "spread", "ndiv_per_row", "d_fake_prob", "d_real_prob", "d_pick_mse"):
        assert _bits(res[key]) == _bits(again[key]) and bool(torch.isfinite(res[key]).all()), key
    assert all(_bits(res["rows"][o]) == _bits(again["rows"][o]) for o in res["rows"])
    assert _bits(runs[2]["rows"]["noise"]) == _bits(runs[3]["rows"]["noise"])              # the noise does not depend on batch_size
    assert res["count"] == 9 and tuple(res["rows"]["noise"].shape) == (9, 6, 2)
    assert res["index"].tolist() == [[i, t] for i in range(3) for t in range(3)]
    curve = res["best_of_k_curve"]
    assert tuple(curve.shape) == (6,) and bool((curve[1:] <= curve[:-1]).all())
    assert _bits(curve[-1:]) == _bits(res["best_action_mse"])
    assert _bits(curve[:1]) == _bits(res["rows"]["sample_err"][:, 0].double().mean().float().view(1))
    # every batch's rows are what `score` gives for that batch's own action_hat
    for bsz, run in runs.items():
        row0 = 0
        for frames, actions, b in GE._batches(data, data[0], bsz, torch.device(DEV), None):
            codes = encode_batch(frames, encoder, 4)
            acts = actions[:, :-1].reshape(-1, 4).contiguous()
            rows = slice(row0, row0 + 3 * b)
            hat, noise = run["rows"]["action_hat"][rows], run["rows"]["noise"][rows]
            logits = GE.discriminate(d, hat.contiguous(), codes, code_rep=6).view(-1, 6)
            want = GE.score(hat, acts, noise, logits)
            assert all(_bits(want[o]) == _bits(run["rows"][o][rows]) for o in C.OUTPUTS), bsz
            assert _bits(GE.sample(g, codes, 6, noise=noise)[0]) == _bits(hat)
            row0 += 3 * b
        assert row0 == 9
    with pytest.raises(ValueError, match="needs the image encoder"):
        GE.evaluate(g, GE.make_dataset("synthetic:3:frames_u8", seq_length=4))
    no_d = GE.evaluate(g, data, encoder=encoder, num_sample=6, batch_size=2, seed=4)
    assert "d_fake_prob" not in no_d and _bits(no_d["best_of_k_curve"]) == _bits(curve)


def test_command_line_prints_the_means_and_the_curve(GE, modules, monkeypatch):
    g, d, _ = modules
    monkeypatch.setattr(GE, "load_module", lambda path, device: g if "decoder" in path else d)
    lines = []
    log = lambda *a: lines.append(" ".join(str(x) for x in a))                             # noqa: E731
    args = ["--generator", "gan_decoder_0.pt", "--data", "synthetic:3:codes", "--num-sample", "4", "--seq-length", "4",
            "--batch-size", "2", "--seed", "3", "--device", DEV]
    best = GE.main(args, log=log)
    assert [ln.split(":")[0] for ln in lines[:4]] == ["val_action_loss", "val_best_action_loss", "val_div_loss", "val_spread"]
    assert lines[0].endswith("rows: 9") and lines[1] == "val_best_action_loss: %s" % best
    assert [ln.split(":")[0] for ln in lines[4:]] == ["best of %d" % k for k in range(1, 5)]
    assert float(lines[7].split()[-1]) == pytest.approx(best, rel=1e-6)
    del lines[:]
    assert GE.main(args + ["--discriminator", "gan_discriminator_0.pt"], log=log) == best
    assert [ln.split(":")[0] for ln in lines[8:]] == ["val_d_fake_prob", "val_d_real_prob", "val_d_pick_loss"] and len(lines) == 11


# ------------------------------------------------------------------------------------------------ the trainer's switch
def _train_config(tmp_path, name, val, noise_source, batch=2):
    from ndivplanning_amd.utils.file import AttrDict
    gan = {"num_epochs": 2, "num_sample": 6, "noise_dim": 2, "learning_rate": 2e-4, "report_feq": 10, "batch_size": batch,
           "discrim_steps_per_gen": 1, "epochs_per_stage": 10, "pairwise_div_factor": 0.1, "noise_source": noise_source,
           "use_graph": True}
    if val:
        gan.update(val_data_path="synthetic:2:codes", val_every=1, val_num_sample=4)
    return AttrDict({"random_seed": 0, "train_data_path": "synthetic:4:codes", "gpu_id": 0, "trajectory_length": 3,
                     "gan_save_path": str(tmp_path / name), "image_encoder_model_path": str(tmp_path / "no_encoder.pt"),
                     "training": {"gan": gan}})


@pytest.mark.parametrize("noise_source", ["device", "cpu"])
def test_validation_changes_no_bit_of_training(tmp_path, caplog, noise_source):
    from ndivplanning_amd import train_gan as script
    real_trainer = script.GanTrainer
    runs = {}
    for name, val in (("with", True), ("without", False)):
        captured = {}

        def spy(*a, _c=captured, **kw):
            _c["t"] = real_trainer(*a, **kw)
            return _c["t"]
        script.GanTrainer = spy
        caplog.clear()
        try:
            with caplog.at_level(logging.INFO):
                hist = script.train(_train_config(tmp_path, name, val, noise_source))
        finally:
            script.GanTrainer = real_trainer
        t = captured["t"]
        g_flat, d_flat = script.train.last_params
        assert g_flat.data_ptr() == t.g_flat.data_ptr() == t.decoder.flat_parameters().data_ptr()
        runs[name] = dict(hist=hist, g=g_flat.cpu(), d=d_flat.cpu(), val=script.train.last_val,
                          log=[r.getMessage() for r in caplog.records], training=t.decoder.training and t.discriminator.training)
    a, b = runs["with"], runs["without"]
    assert a["hist"] == b["hist"] and len(a["hist"]) == 2
    assert _bits(a["g"]) == _bits(b["g"]) and _bits(a["d"]) == _bits(b["d"])
    assert a["training"] and b["training"]
    assert not any("val_" in ln for ln in b["log"]) and b["val"] == []
    # the val_ line comes right after each epoch's line
    marks = [("epoch" if ", D: " in ln else "val") for ln in a["log"] if ", D: " in ln or ln.startswith("val_action_loss")]
    assert marks == ["epoch", "val", "epoch", "val"]
    line = next(ln for ln in a["log"] if ln.startswith("val_action_loss"))
    assert all(key in line for key in ("val_action_loss:", "val_best_action_loss:", "val_div_loss:", "val_spread:"))
    assert [e for e, _ in a["val"]] == [0, 1]
    v0, v1 = a["val"][0][1], a["val"][1][1]
    assert len(v0["best_of_k_curve"]) == 4 and np.isfinite(list(v0.values())[:7]).all()
    assert v0["best_action_mse"] <= v0["action_mse"] and v0["action_mse"] != v1["action_mse"]   # the live parameters were used


def _val_rank_main(rank, world, port, cfg_dict, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", NDP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", NDP_DP_EXCHANGE="p2p")
    logging.basicConfig(filename=os.path.join(out_dir, "rank%d.log" % rank), level=logging.INFO, force=True)
    import torch.distributed as dist
    from ndivplanning_amd import train_gan
    from ndivplanning_amd.utils.file import AttrDict
    hist = train_gan.train(AttrDict(cfg_dict))
    g_flat, d_flat = train_gan.train.last_params
    torch.save({"g": g_flat.cpu(), "d": d_flat.cpu(), "hist": hist, "val": train_gan.train.last_val},
               os.path.join(out_dir, "rank%d.pt" % rank))
    logging.shutdown()
    dist.destroy_process_group()


def _two_ranks(tmp_path, name, val):
    import torch.multiprocessing as mp
    out = tmp_path / name
    out.mkdir()
    cfg = _train_config(tmp_path, name + "_ckpt", val, "device", batch=4).toDict()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.start_processes(_val_rank_main, args=(2, port, cfg, str(out)), nprocs=2, join=False, start_method="spawn")
    deadline = time.monotonic() + 240
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail("the two-rank run (%s validation) did not end within 240 s" % name)
    res = [torch.load(str(out / ("rank%d.pt" % r))) for r in range(2)]
    logs = [open(str(out / ("rank%d.log" % r))).read() for r in range(2)]
    return res, logs


def test_two_ranks_validate_on_rank_zero_alone(tmp_path):
    """train_gan.train under two processes (both on cuda:0, gloo for the handle exchange, the in-kernel gradient exchange
    with its 10 s time-out) with val_data_path set: rank 0 evaluates alone, the ranks meet at the barrier, the run ends,
    and every rank's parameters are those of the same run without the key.  One attempt per run under its own limit."""
    with_val, logs = _two_ranks(tmp_path, "with", True)
    without, logs_without = _two_ranks(tmp_path, "without", False)
    assert logs[0].count("val_action_loss") == 2 and "val_" not in logs[1] and "val_" not in logs_without[0]
    assert len(with_val[0]["val"]) == 2 and with_val[1]["val"] == []
    for r in range(2):
        assert torch.equal(with_val[r]["g"], without[r]["g"]) and torch.equal(with_val[r]["d"], without[r]["d"])
        assert with_val[r]["hist"] == without[r]["hist"] and len(with_val[r]["hist"]) == 2
    assert torch.equal(with_val[0]["g"], with_val[1]["g"]) and torch.equal(with_val[0]["d"], with_val[1]["d"])
