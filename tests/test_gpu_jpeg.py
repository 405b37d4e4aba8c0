"""GPU tests of the device JPEG decoder (ndp_jpeg_decode_u8, ndivplanning_amd/jpeg.py) against PIL's bytes stored in
tests/golden/jpeg_case.npz (made by tests/golden/make_golden_jpeg.py; PIL is not needed here)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case():
    g = load_golden("jpeg_case")
    g["frames"] = np.cumsum(g["frames_dx"], axis=2, dtype=np.uint8)
    o = g["offsets"]
    g["list"] = [g["streams"][o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]
    return g


def _decoder(check=False):
    from ndivplanning_amd.jpeg import JpegDecoder
    return JpegDecoder(DEV, check=check)


def _want(g, i):
    fo = int(g["frame_of"][i])
    return torch.from_numpy(g["frames"][fo]) if fo >= 0 else torch.zeros(128, 128, 3, dtype=torch.uint8)


def _run(dec, streams, pad=None, lead=0):
    """Pack `streams` behind `lead` junk bytes, frame i spanning stream i plus `pad[i]` junk bytes after it (never 0xFF:
    no marker), and decode.  Returns the frames and statuses on the host."""
    rng = np.random.RandomState(5)
    parts, offsets, pos = [rng.randint(0, 255, lead).astype(np.uint8)], [], lead
    for i, s in enumerate(streams):
        offsets.append(pos)
        gap = 0 if pad is None else int(pad[i])
        parts += [np.frombuffer(s, np.uint8), rng.randint(0, 255, gap).astype(np.uint8)]
        pos += len(s) + gap
    buf = torch.from_numpy(np.concatenate(parts))
    frames = dec.decode(buf, torch.tensor(offsets + [pos], dtype=torch.int64))
    return frames.cpu(), dec.status.cpu()


def test_every_fixture_stream_alone_and_all_together():
    g = _case()
    dec = _decoder()
    n = len(g["list"])
    for i in range(n):
        frames, st = _run(dec, [g["list"][i]])
        assert int(st[0]) == int(g["status"][i]), (g["names"][i], int(st[0]))
        assert torch.equal(frames[0], _want(g, i)), g["names"][i]
    frames, st = _run(dec, g["list"])
    assert st.tolist() == g["status"].tolist()
    for i in range(n):
        assert torch.equal(frames[i], _want(g, i)), g["names"][i]
    # the frames of a few streams interleaved with rejected ones, in another order
    order = [40, 0, 36, 5, 43, 27, 33, 12, 41]
    frames, st = _run(dec, [g["list"][i] for i in order])
    for j, i in enumerate(order):
        assert int(st[j]) == int(g["status"][i]) and torch.equal(frames[j], _want(g, i)), g["names"][i]


def test_a_batch_of_1024_shuffled_at_unaligned_offsets_is_exact_and_reproducible():
    g = _case()
    dec = _decoder()
    rng = np.random.RandomState(0)
    pick = rng.randint(0, len(g["list"]), 1024)
    streams = [g["list"][i] for i in pick]
    pad = rng.randint(0, 7, 1024)
    f1, s1 = _run(dec, streams, pad=pad, lead=3)
    f2, s2 = _run(dec, streams, pad=pad, lead=3)
    assert torch.equal(f1, f2) and torch.equal(s1, s2)
    want_st = g["status"][pick]
    for j, i in enumerate(pick):
        st = int(s1[j])
        if want_st[j] == 0:
            assert st == 0 and torch.equal(f1[j], _want(g, i)), (j, g["names"][i])
        else:
            assert st != 0 and not f1[j].any(), (j, g["names"][i], st)


def test_flipped_entropy_bytes_give_ok_or_corrupt_and_leave_neighbours_exact():
    g = _case()
    dec = _decoder()
    rng = np.random.RandomState(7)
    ok = [i for i in range(len(g["list"])) if g["status"][i] == 0]
    streams, kinds = [], []
    for t in range(48):
        i = ok[t % len(ok)]
        s = bytearray(g["list"][i])
        if t % 2:
            sos = bytes(s).index(b"\xff\xda")
            lo = sos + 14
            for _ in range(1 + t % 5):
                p = rng.randint(lo, len(s) - 2)
                s[p] ^= 1 << rng.randint(0, 8)
            kinds.append(("flipped", i))
        else:
            kinds.append(("clean", i))
        streams.append(bytes(s))
    frames, st = _run(dec, streams)
    for j, (kind, i) in enumerate(kinds):
        if kind == "clean":
            assert int(st[j]) == 0 and torch.equal(frames[j], _want(g, i))
        else:
            assert int(st[j]) in (0, 3)
            if int(st[j]) == 3:
                assert not frames[j].any()


def test_check_modes_raise_and_name_the_frame():
    from ndivplanning_amd.jpeg import JpegDecodeError, pack_jpegs
    g = _case()
    good = [g["list"][i] for i in range(3)]
    bad_index = [i for i in range(len(g["list"])) if g["status"][i] == 2][0]
    streams = good[:2] + [g["list"][bad_index]] + good[2:]
    buf, off = pack_jpegs(streams)
    with pytest.raises(JpegDecodeError) as e:
        _decoder(check=True).decode(buf, off)
    assert e.value.index == 2 and e.value.status == 2 and "frame 2" in str(e.value)
    dec = _decoder(check="deferred")
    frames = dec.decode(buf, off)                         # no raise yet
    assert torch.equal(frames[0].cpu(), _want(g, 0))
    gbuf, goff = pack_jpegs(good)
    with pytest.raises(JpegDecodeError) as e:
        dec.decode(gbuf, goff)
    assert e.value.index == 2
    dec.decode(gbuf, goff)
    dec.finish()                                          # the good batch: nothing outstanding
    dec.decode(buf, off)
    with pytest.raises(JpegDecodeError):
        dec.finish()


def test_frames_case_decodes_to_its_bytes_and_the_reference_codes():
    from ndivplanning_amd.jpeg import pack_jpegs
    from ndivplanning_amd.models.image_autoencoder import Encoder
    from oracle import encoder_oracle as EO
    g = load_golden("frames_case")
    buf, off = pack_jpegs([g["jpeg0"].tobytes(), g["jpeg1"].tobytes()])
    frames = _decoder(check=True).decode(buf, off)
    assert torch.equal(frames.cpu(), torch.from_numpy(g["frames_u8"]))
    seed, bn_seed = (int(v) for v in g["seeds"])
    enc = Encoder()
    enc.load_state_dict(EO.init_encoder_state(seed, bn_seed=bn_seed), strict=False)
    enc = enc.to(DEV).eval()
    with torch.no_grad():
        codes = enc(frames).reshape(2, 128).cpu().numpy()
    assert np.abs(codes - g["codes"]).max() <= 1e-4 * np.abs(g["codes"]).max()


def _fixture_trajectories(g, n_traj, steps):
    ok = [i for i in range(len(g["list"])) if g["status"][i] == 0]
    return [[ok[(t * steps + j) * 5 % len(ok)] for j in range(steps)] for t in range(n_traj)]


def test_forward_model_steps_from_jpeg_batches_equal_the_steps_from_pil_bytes():
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    from ndivplanning_amd.jpeg import collate_jpeg
    from ndivplanning_amd.models import forward_encoder as FE
    from oracle import forward_model_oracle as FO
    g = _case()
    trajs = _fixture_trajectories(g, 8, 4)
    gen = torch.Generator().manual_seed(3)
    actions = torch.rand(8, 4, 4, generator=gen) * 2 - 1
    items = [([g["list"][i] for i in tr], torch.zeros(4, 25), actions[k], torch.zeros(3)) for k, tr in enumerate(trajs)]
    jpeg_batch = collate_jpeg(items)[0]
    pil_bytes = torch.from_numpy(np.stack([g["frames"][g["frame_of"][tr]] for tr in trajs]))
    state = FO.init_forward_model_state(4)
    runs = []
    for source in ("jpeg", "pil"):
        model = FE.ForwardAutoencoder()
        model.load_state_dict(state)
        tr = ForwardModelTrainer(model.to(DEV).train(), batch=8, lr=2e-4)
        images = _decoder(check=True).decode_frames(jpeg_batch) if source == "jpeg" else pil_bytes.to(DEV)
        assert images.shape == (8, 4, 128, 128, 3) and images.dtype == torch.uint8
        acts = actions.to(DEV)
        losses = []
        for s in range(3):
            losses.append(tr.step(images[:, s].contiguous(), images[:, s + 1].contiguous(),
                                  acts[:, s].contiguous()).clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), tr.params.clone().cpu(), tr.stats.clone().cpu()))
        tr.close()
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


class _FixtureDataset(torch.utils.data.Dataset):
    """Trajectories of fixture frames: JPEG streams (mode 'jpeg'), PIL's bytes of them (mode 'frames_u8') or the
    loader's floats of those bytes (mode 'images')."""

    def __init__(self, g, mode, n_traj=4, steps=4):
        self.g, self.mode, self.seq_length = g, mode, steps
        self.trajs = _fixture_trajectories(g, n_traj, steps)
        gen = torch.Generator().manual_seed(11)
        self.actions = torch.rand(n_traj, steps, 4, generator=gen) * 2 - 1

    def __len__(self):
        return len(self.trajs)

    def __getitem__(self, i):
        tr = self.trajs[i]
        if self.mode == "jpeg":
            frames = [self.g["list"][k] for k in tr]
        else:
            frames = torch.from_numpy(self.g["frames"][self.g["frame_of"][tr]])
            if self.mode == "images":                      # the reference loader's floats (utils/hdf5_load.py:9-11)
                frames = (frames.permute(0, 3, 1, 2).float().div(255) - 0.5) * 2.0
        return frames, torch.zeros(self.seq_length, 25), self.actions[i], torch.zeros(3)


def test_gan_image_epochs_with_the_code_cache_equal_from_jpeg_and_from_pil_bytes(tmp_path, monkeypatch):
    from ndivplanning_amd import train_gan
    from ndivplanning_amd.utils.file import AttrDict
    g = _case()
    runs = []
    real_trainer = train_gan.GanTrainer
    for mode in ("jpeg", "frames_u8"):
        ds = _FixtureDataset(g, mode)
        monkeypatch.setattr(train_gan, "make_dataset", lambda config, ds=ds: ds)
        captured = {}

        def spy(*a, **kw):
            captured["t"] = real_trainer(*a, **kw)
            return captured["t"]
        monkeypatch.setattr(train_gan, "GanTrainer", spy)
        cfg = AttrDict({
            "random_seed": 0, "train_data_path": "unused", "gpu_id": 0, "gan_save_path": str(tmp_path / mode),
            "trajectory_length": 4, "image_encoder_model_path": str(tmp_path / "no_encoder.pt"),
            "training": {"gan": {"num_epochs": 2, "num_sample": 3, "noise_dim": 2, "learning_rate": 2e-4,
                                 "report_feq": 10, "batch_size": 2, "discrim_steps_per_gen": 1, "epochs_per_stage": 100,
                                 "pairwise_div_factor": 0.1, "noise_source": "cpu", "use_graph": True,
                                 "cache_codes": True}}})
        hist = train_gan.train(cfg)
        t = captured["t"]
        torch.cuda.synchronize()
        runs.append((hist, t.g_flat.cpu().clone(), t.d_flat.cpu().clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_a_workspace_sized_for_smaller_streams_gives_the_workspace_status():
    from ndivplanning_amd import _capi
    g = _case()
    lib = _capi.load()
    ok = [i for i in range(len(g["list"])) if g["status"][i] == 0][:6]
    streams = [g["list"][i] for i in ok]
    from ndivplanning_amd.jpeg import pack_jpegs
    buf, off = pack_jpegs(streams)
    n = len(streams)
    half = int(off[3])                                   # room for the first three streams only
    need = int(lib.ndp_jpeg_workspace_bytes(n, half))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    frames = torch.empty(n, 128, 128, 3, dtype=torch.uint8, device=DEV)
    status = torch.empty(n, dtype=torch.int32, device=DEV)
    b, o = buf.to(DEV), off.to(DEV)
    _capi.check(lib.ndp_jpeg_decode_u8(_capi.ptr(b), _capi.ptr(o), n, _capi.ptr(frames), _capi.ptr(status), _capi.ptr(ws),
                                       need, _capi.stream_ptr()), "ndp_jpeg_decode_u8")
    st = status.cpu().tolist()
    assert st[:3] == [0, 0, 0] and all(s == 4 for s in st[3:]), st
    frames = frames.cpu()
    for j in range(3):
        assert torch.equal(frames[j], _want(g, ok[j]))
    assert not frames[3:].any()


def test_host_offsets_outside_the_buffer_are_refused():
    from ndivplanning_amd import _capi
    g = _case()
    dec = _decoder()
    buf = torch.from_numpy(np.frombuffer(g["list"][0], np.uint8).copy())
    with pytest.raises(_capi.NdpError):
        dec.decode(buf, torch.tensor([0, buf.numel() + 1], dtype=torch.int64))
    with pytest.raises(_capi.NdpError):
        dec.decode(buf, torch.tensor([5, 3], dtype=torch.int64))


def test_decode_images_is_the_loader_s_normalisation_of_pil_s_bytes():
    from ndivplanning_amd.jpeg import collate_jpeg
    g = _case()
    trajs = _fixture_trajectories(g, 3, 5)
    jf = collate_jpeg([([g["list"][i] for i in tr], torch.zeros(5, 25), torch.zeros(5, 4), torch.zeros(3))
                       for tr in trajs])[0]
    got = _decoder(check=True).decode_images(jf)
    pil = torch.from_numpy(np.stack([g["frames"][g["frame_of"][tr]] for tr in trajs]))
    want = (pil.permute(0, 1, 4, 2, 3).float().div(255) - 0.5) * 2.0      # utils/hdf5_load.py:9-11
    assert got.shape == (3, 5, 3, 128, 128) and torch.equal(got.cpu(), want)


def test_autoencoder_raw_jpeg_epoch_equals_the_epoch_on_pil_s_floats(tmp_path, monkeypatch):
    from ndivplanning_amd import train_autoencoder as TA
    g = _case()
    runs = []
    for mode in ("jpeg", "images"):
        ds = _FixtureDataset(g, mode, n_traj=4, steps=15)
        seen = {}

        def make(path, seed=1, raw_jpeg=False, ds=ds, seen=seen):
            seen["raw_jpeg"] = raw_jpeg
            return ds
        monkeypatch.setattr(TA, "make_dataset", make)
        argv = ["--data", "unused", "--batch-size", "2", "--epochs", "1", "--save-dir", str(tmp_path / mode)]
        _, _, losses = TA.main(argv + (["--raw-jpeg"] if mode == "jpeg" else []))
        assert seen["raw_jpeg"] == (mode == "jpeg")
        runs.append((losses, TA.train.last_trainer.params.detach().cpu().clone()))
    assert len(runs[0][0]) == 2 and runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])


def test_evaluation_loops_take_jpeg_frames():
    from ndivplanning_amd import evaluation as E
    from ndivplanning_amd.jpeg import collate_jpeg
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    from ndivplanning_amd.models.gan import Decoder
    from ndivplanning_amd.models.image_autoencoder import Encoder
    g = _case()
    torch.manual_seed(0)
    enc, fm, gen = Encoder(), ForwardAutoencoder(), Decoder(2)
    enc.weight_init(0.0, 0.02)
    fm.decoder.weight_init(0.0, 0.02)
    fm.encoder.weight_init(0.0, 0.02)
    models = E.EvalModels(enc.to(DEV), fm.to(DEV), gen.to(DEV), DEV)
    trajs = _fixture_trajectories(g, 2, 5)
    actions = (torch.rand(2, 5, 4, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(DEV)
    jf = collate_jpeg([([g["list"][i] for i in tr], torch.zeros(5, 25), torch.zeros(5, 4), torch.zeros(3))
                       for tr in trajs])[0]
    pil = torch.from_numpy(np.stack([g["frames"][g["frame_of"][tr]] for tr in trajs])).to(DEV)
    noise = torch.rand(2 * 4 * 3 * 2, device=DEV)
    a = E.open_loop(models, jf, actions, 3, noise)
    b = E.open_loop(models, pil, actions, 3, noise)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    models.finish_jpeg()
