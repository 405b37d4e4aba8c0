"""GPU: the device noise held to the host restatement of its stream (tests/philox_ref.py, pinned on the CPU by the
published Philox known answers in tests/test_philox_ref_host.py; the stream is defined in DESIGN.md section 3).

`ndp_uniform_noise` and the draws `k_phase_a` makes inside the GAN step are compared bit for bit, so there is no
tolerance to choose.  A trainer that draws on the device (noise=None, the default of train_gan and of every throughput
figure) must leave the reference's floats in its noise buffers -- element row * nz + t of the stream (noise_seed, number
of completed G updates) -- and end with the bits of a second trainer that is handed those floats, made on the host, as
explicit noise.  The explicit path is the one tests/test_gpu_parity.py, test_gpu_step_gradients.py and
test_gpu_step_handoff.py hold to fp64, so after these tests the device-noise path inherits what they prove.
`ndp_normal_noise` is held to 1e-5 of the fp64 Box-Muller (plan_common.box_muller) of the REFERENCE's uniforms, the bound
tests/test_gpu_plan_cem.py derives and DESIGN 5p records."""
import numpy as np
import pytest
import torch

import philox_ref as P
import plan_common as PC
import test_gpu_step_gradients as G
from oracle import gan_oracle as O
from test_gpu_parity import _close, _ndiv_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 5003                                   # the trainers' noise_seed
SENTINEL = -7.0


def _lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


def _bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t).tobytes()


def _assert_bits(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if _bits(got) != _bits(want):
        bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))
        raise AssertionError("%s: %d of %d values differ, the first at %d: %r against %r"
                             % (what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


def _call(lib, fn, out, n, seed, offset):
    from ndivplanning_amd import _capi
    off = None if offset is None else torch.tensor([offset], dtype=torch.int32, device=DEV)
    _capi.check(getattr(lib, fn)(_capi.ptr(out), n, seed, _capi.ptr(off), _capi.stream_ptr()), fn)
    torch.cuda.synchronize()


def _draw(lib, fn, n, seed, offset=None):
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device=DEV)
    _call(lib, fn, out, n, seed, offset)
    return out.cpu().numpy()


def _draw_off_alignment(lib, fn, n, seed, offset=None):
    """The same call into a view that starts one float past a 16-byte boundary; the floats around it keep a sentinel."""
    buf = torch.full((n + 9,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    _call(lib, fn, buf[1:1 + n], n, seed, offset)
    host = buf.cpu().numpy()
    assert host[0] == SENTINEL and (host[1 + n:] == SENTINEL).all(), "%s wrote outside out[0 .. n)" % fn
    return host[1:1 + n]


# ------------------------------------------------------------------------------------------------ a. ndp_uniform_noise
# every n (the tails around a Philox block and around a workgroup of 256, more than one workgroup), every seed (the
# key's high word set, all bits set) and every offset word at least once
UNIFORM_CASES = [(1, 0, None), (3, 123, 0), (4, (1 << 32) + 5, 1), (5, (1 << 64) - 1, 3), (255, 0, (1 << 31) - 1),
                 (256, 123, -1), (257, (1 << 32) + 5, None), ((1 << 20) + 3, (1 << 64) - 1, 1), (257, 123, (1 << 31) - 1),
                 (5, (1 << 32) + 5, -1)]


@pytest.mark.parametrize("n,seed,offset", UNIFORM_CASES)
def test_uniform_noise_is_the_reference_stream(n, seed, offset):
    got = _draw(_lib(), "ndp_uniform_noise", n, seed, offset)
    _assert_bits(got, P.uniform(seed, offset, n), "ndp_uniform_noise(n %d, seed %d, offset %s)" % (n, seed, offset))


def test_uniform_noise_offset_word_and_key_words():
    lib = _lib()
    n = 257
    absent, zero = _draw(lib, "ndp_uniform_noise", n, 123, None), _draw(lib, "ndp_uniform_noise", n, 123, 0)
    _assert_bits(absent, zero, "no offset word against an offset word of 0")
    minus = _draw(lib, "ndp_uniform_noise", n, 123, -1)
    _assert_bits(minus, P.uniform(123, 0xFFFFFFFF, n), "offset word -1 read as 0xFFFFFFFF")
    assert _bits(minus) != _bits(zero)
    low, high = _draw(lib, "ndp_uniform_noise", n, 5, 1), _draw(lib, "ndp_uniform_noise", n, (1 << 32) + 5, 1)
    assert _bits(low) != _bits(high), "the key's high word does not matter"
    _assert_bits(high, P.uniform((1 << 32) + 5, 1, n), "seed 2^32 + 5")


def test_uniform_noise_into_an_output_off_alignment():
    lib = _lib()
    n = 261
    got = _draw_off_alignment(lib, "ndp_uniform_noise", n, 123, 3)
    _assert_bits(got, P.uniform(123, 3, n), "ndp_uniform_noise into a view one float off a 16-byte boundary")


# ------------------------------------------------------------------------------------------------ b. ndp_normal_noise
def _reference_normals(seed, offset, n):
    return PC.box_muller(P.uniform(seed, offset, (n + 1) // 2 * 2))[:n]


@pytest.mark.parametrize("offset", [None, 3])
def test_normal_noise_against_box_muller_of_the_reference_uniforms(offset):
    """|device - fp64 Box-Muller of the reference's uniforms| <= 1e-5 over 2^20 draws (the derivation is in
    tests/test_gpu_plan_cem.py; DESIGN 5p records the measured error)."""
    n, seed = 1 << 20, 0x5EED1234
    z = _draw(_lib(), "ndp_normal_noise", n, seed, offset)
    worst = np.abs(z.astype(np.float64) - _reference_normals(seed, offset, n)).max()
    print("offset %s: max |device - fp64 Box-Muller of the reference's uniforms| = %.3g" % (offset, worst))
    assert np.isfinite(z).all()
    assert worst <= 1e-5


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_normal_noise_tails(n):
    lib = _lib()
    seed = 0x5EED1234
    for offset in (None, 3):
        z = _draw(lib, "ndp_normal_noise", n, seed, offset)
        worst = np.abs(z.astype(np.float64) - _reference_normals(seed, offset, n)).max()
        assert np.isfinite(z).all() and worst <= 1e-5, (n, offset, worst)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_normal_noise_off_alignment_gives_the_bits_of_the_aligned_call(n):
    """An output that is not 16-byte aligned takes the scalar stores; the values are the aligned call's."""
    lib = _lib()
    aligned = _draw(lib, "ndp_normal_noise", n, 77, 1)
    _assert_bits(_draw_off_alignment(lib, "ndp_normal_noise", n, 77, 1), aligned, "ndp_normal_noise off alignment, n %d" % n)
    assert np.abs(aligned.astype(np.float64) - _reference_normals(77, 1, n)).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ the GAN step
def _reference_noise(offset, flat, k, nz, seed=SEED):
    """[flat, K, nz] made on the host: element row * nz + t of the stream (seed, offset), row = flat row * K + sample."""
    return torch.from_numpy(P.uniform(seed, offset, flat * k * nz).reshape(flat, k, nz))


def _assert_noise(buf, offset, what, seed=SEED):
    _assert_bits(buf.reshape(-1), P.uniform(seed, offset, buf.numel()), "%s: noise buffer against stream offset %d" % (what, offset))


def _pair(batch, k, nz, seed=SEED, **kw):
    """Two trainers from the same parameters: A draws on the device, B is handed noise.  B's noise_seed is another one:
    nothing it computes may depend on it."""
    from ndivplanning_amd.trainer import GanTrainer
    g0, d0, codes, actions, _ = G._case_inputs(batch, k, nz)
    out = []
    for s in (seed, seed + 1):
        dec, dis = G._load_modules(g0, d0, nz)
        out.append(GanTrainer(dec, dis, flat=codes.shape[0], num_sample=k, noise_seed=s, **kw))
    return out[0], out[1], codes.to(DEV), actions.to(DEV)


def _assert_same_state(a, b, what, action_hat=True):
    torch.cuda.synchronize()
    _assert_bits(a.g_flat, b.g_flat, what + ": g_flat")
    _assert_bits(a.d_flat, b.d_flat, what + ": d_flat")
    assert a.losses() == b.losses(), (what, a.losses(), b.losses())
    if action_hat:
        _assert_bits(a.action_hat[:a.m], b.action_hat[:b.m], what + ": action_hat")


# (B, K, nz) of test_gpu_step_gradients.SHAPES: every way k_phase_a lays out its tiles, see the comments there
STEP_SHAPES = [(5, 7, 2), (25, 6, 2), (64, 6, 2), (52, 6, 2), (72, 6, 2), (98, 6, 2), (200, 3, 2), (24, 32, 2), (40, 5, 5),
               (40, 6, 1)]


# ------------------------------------------------------------------------------------------------ c. every tile layout
@pytest.mark.parametrize("batch,k,nz", STEP_SHAPES)
def test_device_noise_step_is_the_explicit_noise_step_on_the_reference_noise(batch, k, nz):
    """Three graph-replayed steps.  After step i A's buffer holds the stream at offset i -- the element index row * nz + t,
    the offset being the count of completed G updates, every row of every tile written -- and A has B's bits."""
    assert (batch, k, nz) in G.SHAPES
    a, b, codes, actions = _pair(batch, k, nz, use_graph=True)
    what = "B %d K %d nz %d" % (batch, k, nz)
    for i in range(3):
        a.step(codes, actions, None)
        b.step(codes, actions, _reference_noise(i, a.flat, k, nz).to(DEV))
        torch.cuda.synchronize()
        _assert_noise(a.noise, i, "%s step %d" % (what, i))
        _assert_same_state(a, b, "%s step %d" % (what, i))
    assert int(a.g_step[0].item()) == 3


# ------------------------------------------------------------------------------------------------ d. the host paths
CFG1 = (16, 6, 2)                             # config 1: FLAT 112, M 672


def test_eager_steps():
    batch, k, nz = CFG1
    a, b, codes, actions = _pair(batch, k, nz, use_graph=False)
    for i in range(3):
        a.step(codes, actions, None)
        b.step(codes, actions, _reference_noise(i, a.flat, k, nz).to(DEV))
        _assert_noise(a.noise, i, "eager step %d" % i)
        _assert_same_state(a, b, "eager step %d" % i)


def test_multi_step_graph_slot_s_of_launch_l_holds_offset_3l_plus_s():
    batch, k, nz = CFG1
    a, b, codes, actions = _pair(batch, k, nz, steps_per_launch=3)
    codes3, actions3 = codes.expand(3, -1, -1).contiguous(), actions.expand(3, -1, -1).contiguous()
    done = 0
    for launch, count in enumerate((None, None, 2)):
        n = 3 if count is None else count
        a.step_many(codes3[:n], actions3[:n], None, count=count)
        b.step_many(codes3[:n], actions3[:n], torch.stack([_reference_noise(done + s, a.flat, k, nz) for s in range(n)]).to(DEV),
                    count=count)
        torch.cuda.synchronize()
        for s in range(n):
            _assert_noise(a.noise_slots[s], done + s, "launch %d slot %d" % (launch, s))
        done += n
        _assert_same_state(a, b, "launch %d" % launch)
    _assert_noise(a.noise_slots[2], 5, "the slot the count = 2 launch left alone")
    assert done == 8 and int(a.g_step[0].item()) == 8
    assert a.pop_loss_sums() == b.pop_loss_sums()


def test_pinned_host_uploads_draw_into_both_slot_sets():
    batch, k, nz = CFG1
    a, b, codes, actions = _pair(batch, k, nz, steps_per_launch=3)
    launches = [[O.synthetic_batch(60 + 3 * j + s, batch, k, steps=1) for s in range(3)] for j in range(3)]
    for j, batches in enumerate(launches):
        c3, a3 = torch.stack([x[0] for x in batches]), torch.stack([x[1] for x in batches])
        a.step_many_from_host(c3.pin_memory(), a3.pin_memory())
        b.step_many(c3.to(DEV), a3.to(DEV), torch.stack([_reference_noise(3 * j + s, a.flat, k, nz) for s in range(3)]).to(DEV))
        torch.cuda.synchronize()
        slots = a.noise_slots if j % 2 == 0 else a._alt_slots[2]
        for s in range(3):
            _assert_noise(slots[s], 3 * j + s, "upload launch %d slot %d" % (j, s))
        _assert_same_state(a, b, "upload launch %d" % j)
    for s in range(3):                          # what each set holds in the end: launches 2 and 1
        _assert_noise(a.noise_slots[s], 6 + s, "first slot set, slot %d" % s)
        _assert_noise(a._alt_slots[2][s], 3 + s, "second slot set, slot %d" % s)
    assert a.pop_loss_sums() == b.pop_loss_sums()


def test_repeat_d_step_draws_once_per_iteration():
    """discrim_steps = 2, fused and graph-replayed: the D state word counts 2 per iteration, the noise offset 1."""
    batch, k, nz = CFG1
    a, b, codes, actions = _pair(batch, k, nz, discrim_steps=2, use_graph=True)
    for i in range(3):
        a.step(codes, actions, None)
        b.step(codes, actions, _reference_noise(i, a.flat, k, nz).to(DEV))
        _assert_noise(a.noise, i, "discrim_steps 2, iteration %d" % i)
        _assert_same_state(a, b, "discrim_steps 2, iteration %d" % i)
    assert int(a.d_step[0].item()) == 6 and int(a.g_step[0].item()) == 3


def test_repeat_d_step_leaves_the_first_d_steps_buffer():
    """Segment by segment (non-fused, eager, as test_repeat_d_step_gradient runs them): the first D step writes the
    buffer; the repeat D step and the G step only read it.  A redraw at the same offset would write the same bits, so
    in the second iteration the buffer is replaced by another stream after the first D step: it must survive the rest."""
    batch, k, nz = CFG1
    a, _, codes, actions = _pair(batch, k, nz, discrim_steps=2, use_graph=False, reduce_fn=lambda grad: None)
    a.codes.copy_(codes)
    a.actions.copy_(actions)
    for i in range(2):
        a.noise.fill_(SENTINEL)
        segs = [fn for fn, _ in a._segments(True)]      # d_grads, D Adam, d_grads (repeat), D Adam, g_grads, G Adam
        assert len(segs) == 6
        with torch.cuda.device(a.device):
            segs[0]()
            torch.cuda.synchronize()
            _assert_noise(a.noise, i, "iteration %d after the first D step" % i)
            if i == 1:
                a.noise.copy_(_reference_noise(0, a.flat, k, nz, seed=SEED + 99))
            for fn in segs[1:]:
                fn()
            torch.cuda.synchronize()
        if i == 0:
            _assert_noise(a.noise, 0, "iteration 0 after the repeat D step and the G step")
        else:
            _assert_noise(a.noise, 0, "iteration 1: the marker stream after the repeat D step and the G step", seed=SEED + 99)
    assert int(a.d_step[0].item()) == 4 and int(a.g_step[0].item()) == 2


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("discrim_steps", [1, 2])
def test_non_fused_segments(use_graph, discrim_steps):
    """reduce_fn given (the data-parallel form, here without a collective): phases and Adam launches apart."""
    batch, k, nz = CFG1
    a, b, codes, actions = _pair(batch, k, nz, use_graph=use_graph, discrim_steps=discrim_steps, reduce_fn=lambda grad: None)
    for i in range(3):
        a.step(codes, actions, None)
        b.step(codes, actions, _reference_noise(i, a.flat, k, nz).to(DEV))
        _assert_noise(a.noise, i, "non-fused step %d" % i)
        _assert_same_state(a, b, "non-fused step %d" % i)


@pytest.mark.parametrize("use_graph", [True, False])
def test_restored_adam_state_continues_the_stream(use_graph):
    """After load_adam_state with 7 G updates (and 11 D updates) the next draw has offset 7, then 8."""
    batch, k, nz = CFG1
    a, b, codes, actions = _pair(batch, k, nz, use_graph=use_graph)
    a.step(codes, actions, None)                       # a graph captured before the restore must follow it too
    b.step(codes, actions, _reference_noise(0, a.flat, k, nz).to(DEV))
    gen = torch.Generator().manual_seed(3)

    def moments(flat, count):
        return {"m": (1e-3 * torch.randn(flat.numel(), generator=gen)).to(DEV),
                "v": (1e-6 * torch.rand(flat.numel(), generator=gen)).to(DEV), "t": count}
    g_state, d_state = moments(a.g_flat, 7), moments(a.d_flat, 11)
    for t in (a, b):
        t.load_adam_state(g_state, d_state)
    for i in (7, 8):
        a.step(codes, actions, None)
        b.step(codes, actions, _reference_noise(i, a.flat, k, nz).to(DEV))
        _assert_noise(a.noise, i, "after the restore, G update %d" % i)
        _assert_same_state(a, b, "after the restore, G update %d" % i)
    assert int(a.g_step[0].item()) == 9 and int(a.d_step[0].item()) == 13


# ------------------------------------------------------------------------------------------------ e. the oracle
def test_free_running_device_noise_steps_against_the_oracle_on_host_made_noise():
    """No device-produced number enters the reference: gan_oracle.StepMath is fed philox_ref's tensors.  The bounds are
    test_gpu_parity.test_free_running_vs_oracle's."""
    from ndivplanning_amd.trainer import GanTrainer
    batch, k, nz = CFG1
    g0, d0, codes, actions, _ = G._case_inputs(batch, k, nz)
    sm = O.StepMath({n: v.clone() for n, v in g0.items()}, {n: v.clone() for n, v in d0.items()})
    dec, dis = G._load_modules(g0, d0, nz)
    tr = GanTrainer(dec, dis, flat=codes.shape[0], num_sample=k, noise_seed=SEED)
    for s in range(3):
        ref = sm.step(codes, actions, _reference_noise(s, codes.shape[0], k, nz))
        tr.step(codes.to(DEV), actions.to(DEV), None)
        d_loss, g_loss, pd = tr.losses()
        print("step %d: D %.3e, G %.3e from the oracle; NDiv %.6f against %.6f"
              % (s, abs(d_loss - ref["d_loss"].item()), abs(g_loss - ref["g_loss"].item()), pd, ref["pair_div"].item()))
        _close(d_loss, ref["d_loss"], 1e-4, "D_loss step %d" % s)
        _close(g_loss, ref["g_loss"], 1e-4, "G_loss step %d" % s)
        if s == 0:
            _ndiv_close(pd, ref["pair_div"].item(), "pair_div")
            _close(tr.action_hat[:codes.shape[0] * k], ref["action_hat"], 1e-4, "action_hat")
        else:
            rtol = 2e-2 if codes.shape[0] >= 100 else 1e-1
            assert abs(pd - ref["pair_div"].item()) <= rtol * abs(ref["pair_div"].item())


# ------------------------------------------------------------------------------------------------ f. the consumers
def test_eval_models_uniform_and_normal():
    from ndivplanning_amd import evaluation as E
    from test_gpu_eval import _modules
    models = E.EvalModels(*_modules(), DEV)
    n = 4096
    for seed in (77, (1 << 32) + 77):
        _assert_bits(models.uniform(n, seed), P.uniform(seed, 0, n), "EvalModels.uniform(seed %d)" % seed)
        z = models.normal(n, seed).cpu().numpy().astype(np.float64)
        worst = np.abs(z - _reference_normals(seed, 1, n)).max()
        assert worst <= 1e-5, (seed, worst)


@pytest.mark.parametrize("num_sample", [1, 6])
def test_gan_eval_sample_without_noise_is_the_call_with_the_reference_noise(num_sample):
    from ndivplanning_amd import gan_eval as GE
    _lib()
    g0, d0, _, _, _ = G._case_inputs(*CFG1)
    g = G._load_modules(g0, d0, 2)[0].eval()
    codes = torch.randn(7, 256, generator=torch.Generator().manual_seed(1)).to(DEV)
    hat, noise = GE.sample(g, codes, num_sample, seed=11)
    want = torch.from_numpy(P.uniform(11, 0, 7 * num_sample * 2).reshape(7, num_sample, 2))
    _assert_bits(noise, want, "gan_eval.sample's noise")
    hat_explicit, used = GE.sample(g, codes, num_sample, noise=want.to(DEV))
    _assert_bits(hat, hat_explicit, "gan_eval.sample's action_hat")
    _assert_bits(used, want, "the explicit noise comes back unchanged")


def test_train_gan_with_device_noise_is_a_trainer_driven_by_hand_on_the_reference_noise(tmp_path):
    """One single-process epoch of train_gan.train with `noise_source: device` (three batches of 8: one two-step graph
    launch and one single step) against a GanTrainer stepped by hand on the same batches with the reference's noise at
    key random_seed * 1000 + rank 0: the same history and the same parameters, bit for bit."""
    from ndivplanning_amd import train_gan
    from ndivplanning_amd.trainer import GanTrainer
    from test_gpu_train_gan import _config
    random_seed = 5

    def config():
        cfg = _config(tmp_path, 24, "codes", 8, noise_source="device", stage=100)
        cfg.random_seed = random_seed
        cfg.training.gan.steps_per_launch = 2
        return cfg
    hist = train_gan.train(config())
    g_run, d_run = (t.detach().clone() for t in train_gan.train.last_params)

    cfg = config()
    g_cfg = cfg.training.gan
    g0, d0 = O.init_params(random_seed, g_cfg.noise_dim)
    ds = train_gan.make_dataset(cfg)
    batches = train_gan.epoch_batches(len(ds), g_cfg.batch_size, torch.Generator().manual_seed(random_seed))
    assert len(batches) == 3
    loader = torch.utils.data.DataLoader(ds, batch_sampler=[x.tolist() for x in batches])
    dec, dis = G._load_modules(g0, d0, g_cfg.noise_dim)
    flat = g_cfg.batch_size * (ds.seq_length - 1)
    tr = GanTrainer(dec, dis, flat=flat, num_sample=g_cfg.num_sample, lr=g_cfg.learning_rate,
                    pairwise_div_factor=g_cfg.pairwise_div_factor, noise_seed=1)
    for i, (frames, _s, actions, _g) in enumerate(loader):
        codes = train_gan.encode_batch(frames.float(), None, ds.seq_length)
        acts = actions.float()[:, :-1].reshape(-1, 4)
        noise = _reference_noise(i, flat, g_cfg.num_sample, g_cfg.noise_dim, seed=random_seed * 1000)
        tr.step(codes.to(DEV), acts.to(DEV), noise.to(DEV))
    want = tuple(v / len(batches) for v in tr.pop_loss_sums())
    assert len(hist) == 1 and tuple(hist[0]) == want, (hist, want)
    _assert_bits(g_run, tr.g_flat, "train(): g_flat")
    _assert_bits(d_run, tr.d_flat, "train(): d_flat")
