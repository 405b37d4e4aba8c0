"""CPU-only tests of the generator evaluation (ndivplanning_amd/gan_eval.py): the numpy restatement of ndp_gan_score's
definition (tests/gan_eval_common.py) against the golden file made from the reference's own Decoder, Discriminator and
diversity module (tests/golden/make_golden_gan_eval.py), the argument errors of evaluate / sample / score -- raised before
anything is launched -- and that sampling and evaluating leave torch's CPU generator alone (the C calls mocked).  The
kernels themselves: tests/test_gan_score_host.py (CPU, sanitized) and tests/test_gpu_gan_eval.py."""
import contextlib

import numpy as np
import pytest
import torch

import gan_eval_common as C


@pytest.fixture(scope="module")
def golden():
    return np.load(C.GOLDEN)


def err_bound(e, delta):
    """What an error of `delta` in every component of a sample can move its mean squared error e by."""
    return 2.0 * np.sqrt(e) * delta + delta * delta


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_matches_the_reference(golden, name):
    g = lambda key, tag="32": golden["%s/%s/%s" % (name, key, tag)]                       # noqa: E731
    n, k, nz = golden[name + "/shape"][:3]
    hat, actions, noise, logits = g("action_hat"), golden[name + "/actions"], golden[name + "/noise"], g("fake_logits")
    assert hat.shape == (n, k, 4) and noise.shape == (n, k, nz) and hat.dtype == np.float32
    want = C.want_scores(hat, actions, noise, logits)
    # the reference's own fp32 results on the same fp32 samples: a few fp32 roundings apart
    for key in ("sample_err", "mean_err", "best_err", "best_curve", "d_pick_err", "spread", "d_fake_prob"):
        np.testing.assert_allclose(want[key], g(key), rtol=4e-6, atol=0, err_msg=key)
    np.testing.assert_allclose(want["ndiv"], g("ndiv"), rtol=0, atol=8 * k * C.EPS)
    # the selections: every row (the fixture's recipe asserts that no row is a near-tie)
    for key in ("best_k", "d_pick_k"):
        assert np.array_equal(want[key], g(key)) and np.array_equal(want[key], g(key, "64")), key
    # the fp64 run of the same modules: the samples differ by the fp32 forward pass's error
    delta = np.abs(hat - g("action_hat", "64")).max()
    assert delta < 1e-4
    for key in ("sample_err", "mean_err", "best_err", "best_curve", "d_pick_err"):
        w64 = g(key, "64")
        assert (np.abs(want[key] - w64) <= err_bound(w64, delta) + 1e-7 * w64).all(), key
    assert (np.abs(want["spread"] - g("spread", "64")) <= 2 * 2 * delta + 1e-6).all()
    # the reference's reductions of the per-row values
    np.testing.assert_allclose(g("mean_err").mean(), g("action_mse"), rtol=1e-6)
    np.testing.assert_allclose(g("ndiv", "64").sum(), g("ndiv_total", "64"), rtol=1e-12)
    np.testing.assert_allclose(want["ndiv"].sum(), g("ndiv_total"), rtol=0, atol=n * 8 * k * C.EPS)


def test_fixture_rows_are_no_near_ties(golden):
    for name in ("a", "b"):
        e = np.sort(golden[name + "/sample_err/64"], axis=1)
        lg = np.sort(golden[name + "/fake_logits/64"], axis=1)
        assert (e[:, 1] - e[:, 0] >= 100 * (2 * np.sqrt(e[:, 1]) * 1e-4 + 1e-8)).all()
        assert (lg[:, -1] - lg[:, -2] >= 100 * 1e-4).all()
        for arr in golden.files:
            if arr.startswith(name + "/g/") or arr.startswith(name + "/d/"):
                assert np.array_equal(np.round(golden[arr] * 256) / 256, golden[arr]), arr


def test_restatement_rules():
    nan = np.nan
    assert C._first_best(np.array([nan, 3, 1, 1, nan], np.float32), larger=False)[0] == 2
    assert C._first_best(np.array([nan, nan], np.float32), larger=False)[0] == 0
    assert C._first_best(np.array([2, nan, 5, 5], np.float32), larger=True)[0] == 2
    run = C._first_best(np.array([nan, 3, 4, 1], np.float32), larger=False)[1]
    assert np.isnan(run[0]) and list(run[1:]) == [3, 3, 1]
    one = C.want_scores(np.zeros((2, 1, 4), np.float32), np.ones((2, 4), np.float32), np.zeros((2, 1, 2), np.float32))
    assert np.isnan(one["spread"]).all() and np.isnan(one["ndiv"]).all() and (one["mean_err"] == 1).all()


# ------------------------------------------------------------------------------------------ argument errors
class _Data:
    def __init__(self, n, T, frames):
        self.n, self.seq_length, self.frames = n, T, frames

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        T = self.seq_length
        return self.frames(T), torch.zeros(T, 25), torch.zeros(T, 4), torch.zeros(3)


def _modules(nz=2):
    from ndivplanning_amd.models.gan import Decoder, Discriminator
    state = torch.get_rng_state()                                   # the modules' initialisation draws: put the state back
    g, d = Decoder(noise_dim=nz), Discriminator()
    torch.set_rng_state(state)
    return g.eval(), d.eval()


def test_evaluate_argument_errors():
    from ndivplanning_amd import gan_eval as GE
    g, d = _modules()
    codes = _Data(2, 3, lambda T: torch.zeros(T, 128))
    images = _Data(2, 3, lambda T: torch.zeros(T, 3, 128, 128))
    with pytest.raises(ValueError, match="num_sample"):
        GE.evaluate(g, codes, num_sample=0)
    with pytest.raises(ValueError, match="num_sample"):
        GE.evaluate(g, codes, num_sample=257)
    with pytest.raises(ValueError, match="non-empty"):
        GE.evaluate(g, _Data(0, 3, None))
    with pytest.raises(ValueError, match="batch_size"):
        GE.evaluate(g, codes, batch_size=0)
    with pytest.raises(ValueError, match="T must be >= 2"):
        GE.evaluate(g, _Data(2, 1, lambda T: torch.zeros(T, 128)))
    with pytest.raises(ValueError, match="training mode"):
        GE.evaluate(g.train(), codes)
    g.eval()
    with pytest.raises(ValueError, match="training mode"):
        GE.evaluate(g, codes, discriminator=d.train())
    d.eval()
    with pytest.raises(ValueError, match="needs the image encoder"):
        GE.evaluate(g, images)
    with pytest.raises(ValueError, match="no CPU fallback"):        # a generator on the CPU, a CPU device
        GE.evaluate(g, codes)
    with pytest.raises(ValueError, match="no CPU fallback"):
        GE.evaluate(g, codes, device="cpu")


def test_sample_and_score_argument_errors():
    from ndivplanning_amd import gan_eval as GE
    g, _ = _modules()
    with pytest.raises(ValueError, match="num_sample"):
        GE.sample(g, torch.zeros(3, 256), 0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        GE.sample(g, torch.zeros(3, 256), 6)
    with pytest.raises(ValueError, match="training mode"):
        GE.sample(g.train(), torch.zeros(3, 256), 6)
    with pytest.raises(ValueError, match="torch.Tensor"):
        GE.score(np.zeros((3, 6, 4)))
    with pytest.raises(ValueError, match="no CPU fallback"):
        GE.score(torch.zeros(3, 6, 4))


# ------------------------------------------------------------------------------------------ torch's generators
class _FakeLib:
    """Every C entry returns 0 and records its name."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


@pytest.fixture()
def mocked(monkeypatch):
    from ndivplanning_amd import _capi, gan_eval as GE
    lib = _FakeLib()
    monkeypatch.setattr(_capi, "load", lambda: lib)
    monkeypatch.setattr(_capi, "on_device", lambda t: contextlib.nullcontext())
    monkeypatch.setattr(_capi, "stream_ptr", lambda device=None: None)
    monkeypatch.setattr(GE, "_device_f32", lambda t, name, shape_text, ok: t.detach().contiguous())
    monkeypatch.setattr(GE, "_check_devices", lambda device, **modules: torch.device("cpu"))
    return lib


def test_sample_and_evaluate_leave_torchs_generator_alone(mocked):
    from ndivplanning_amd import gan_eval as GE
    g, d = _modules()
    torch.manual_seed(1234)
    before = torch.get_rng_state()
    hat, noise = GE.sample(g, torch.zeros(3, 256), 6, seed=5)
    assert hat.shape == (3, 6, 4) and noise.shape == (3, 6, 2)
    assert mocked.calls == ["ndp_uniform_noise", "ndp_g_forward"]
    del mocked.calls[:]
    data = _Data(3, 4, lambda T: torch.zeros(T, 128))
    res = GE.evaluate(g, data, discriminator=d, num_sample=6, batch_size=2)
    assert res["count"] == 9 and res["best_of_k_curve"].shape == (6,) and tuple(res["index"].shape) == (9, 2)
    # ONE noise call for the whole dataset, then per batch (2 of them): G, D on the samples, D on the true actions, score
    assert mocked.calls == ["ndp_uniform_noise"] + ["ndp_g_forward", "ndp_d_forward", "ndp_d_forward", "ndp_gan_score"] * 2
    assert torch.equal(torch.get_rng_state(), before)
