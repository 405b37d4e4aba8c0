"""GPU: the autoencoder trained data-parallel -- ndp_ae_train_grads_dp (cross-rank BatchNorm statistics through a per-call
callback, one event per gradient bucket), AutoencoderTrainer(sync_batchnorm_world=..., bucket_reduce=...), and
train_autoencoder.train under two ranks.  The ranks are processes spawned here, both on cuda:0, over gloo.

Two ranks that each trained the whole batch with the same seeds would match one process bit for bit, so "2 ranks equal 1
process" alone shows nothing: the shard sizes, the ranks' different losses and per-rank statistics are what show that
the batch was split."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_BIASES = tuple("encoder.conv%d.bias" % i for i in (1, 2, 3)) + tuple("decoder.deconv%d.bias" % i for i in range(1, 6))
DEV = "cuda:0"
LR = 2e-4

pytestmark = pytest.mark.gpu


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(fn, *args):
    import torch.multiprocessing as mp
    mp.spawn(fn, args=(2, _port()) + args, nprocs=2, join=True)


def _rank_env(rank, world, port):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", NDP_DIST_BACKEND="gloo", NDP_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")


def _models(seed):
    from ndivplanning_amd.models.image_autoencoder import Decoder, Encoder
    torch.manual_seed(seed)
    enc, dec = Encoder(), Decoder()
    dec.weight_init(0.0, 0.02)
    enc.weight_init(0.0, 0.02)
    return enc.to(DEV).train(), dec.to(DEV).train()


def _images(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, 128, 128, generator=gen) * 2 - 1


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def test_bucket_events_order_a_side_stream_behind_each_range():
    """After one ndp_ae_train_grads_dp call, a stream that waits on bucket b's event reads the final values of its range;
    at world 1 without a statistics callback the gradient has the bits of ndp_ae_train_grads."""
    from ndivplanning_amd import _capi
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    lib = _capi.load()
    buckets = _capi.ae_grad_buckets()
    n = 16
    tr = AutoencoderTrainer(*_models(3), batch=n)
    x = _images(n, 4).to(DEV)
    p = _capi.ptr
    with torch.cuda.device(DEV):
        _capi.check(lib.ndp_ae_train_grads_dp(p(tr.params), p(tr.stats), p(x), n, p(tr.grad), p(tr.loss), None, None,
                                              p(tr.workspace), _capi.stream_ptr(DEV), None, None, 1),
                    "ndp_ae_train_grads_dp")
        side = torch.cuda.Stream(DEV)
        sums = []
        with torch.cuda.stream(side):
            for b, (o, c) in enumerate(buckets):
                _capi.check(lib.ndp_ae_bucket_wait(b, _capi.stream_ptr(DEV)), "ndp_ae_bucket_wait")
                sums.append(tr.grad[o:o + c].double().abs().sum())
    torch.cuda.synchronize(DEV)
    want = [tr.grad[o:o + c].double().abs().sum().item() for o, c in buckets]
    assert [s.item() for s in sums] == want and all(w > 0 for w in want)
    g_dp, loss_dp = tr.grad.clone(), tr.loss.item()
    tr.grad.zero_()
    tr.grads(x)                                                        # ndp_ae_train_grads: one slab-sum launch
    assert torch.equal(tr.grad, g_dp) and tr.loss.item() == loss_dp


def _grads_rank(rank, world, port, n, out_dir):
    _rank_env(rank, world, port)
    import torch.distributed as dist
    from ndivplanning_amd import dp
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    dp.init_process_group(DEV)
    tr = AutoencoderTrainer(*_models(11), batch=n, sync_batchnorm_world=world)
    x = _images(world * n, 12)[rank * n:(rank + 1) * n].contiguous().to(DEV)
    tr.grads(x)
    g = tr.grad.clone()
    dp.mean_all_reduce(world)(g)
    torch.save({"grad": g.cpu(), "loss": tr.loss.item(), "stats": tr.stats.cpu(), "calls": tr.stat_sync.calls},
               os.path.join(out_dir, "ae_grads%d.pt" % rank))
    tr.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("n", [3, 16])
def test_cross_rank_statistics_give_the_global_batch_gradient(tmp_path, n):
    """2 ranks x n images, BatchNorm statistics summed over the ranks through the per-call callback (8 forward + 8 backward
    calls), gradients averaged, against ONE process on the 2n images: same loss, same running statistics, every gradient
    tensor close to its norm (below; the conv biases in front of a BatchNorm are rounding noise)."""
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    _spawn(_grads_rank, n, str(tmp_path))
    res = [torch.load(str(tmp_path / ("ae_grads%d.pt" % r))) for r in range(2)]
    assert res[0]["calls"] == res[1]["calls"] == 16
    assert abs(res[0]["loss"] - res[1]["loss"]) > 1e-4                   # (the ranks saw different images)
    assert torch.equal(res[0]["stats"], res[1]["stats"])
    tr = AutoencoderTrainer(*_models(11), batch=2 * n)
    tr.grads(_images(2 * n, 12).to(DEV))
    assert abs(tr.loss.item() - (res[0]["loss"] + res[1]["loss"]) / 2) <= 1e-6
    stats = tr.stats.cpu()
    assert float((stats - res[0]["stats"]).abs().max()) <= 1e-5 * float(stats.abs().max())
    want = tr.named_gradients()
    got = _capi_unpack(res[0]["grad"].to(DEV), tr)
    rel = {name: _rel(got[name], want[name]) for name in want if name not in NOISE_BIASES}
    # A tile's fp32 column sums group the rows differently when the tile holds one rank's images or both ranks', so the
    # statistics differ by ~1e-7 of sum x^2, up to 3e-5 of a variance (as in the forward model).  At 3 images per rank
    # every gradient stays within 1e-4.  At 16, pre-activations that close to zero decide their ReLU the other way
    # often enough to move the gradients at the end of the backward chain (conv1..3 and their BatchNorms) by a few 1e-3
    # (measured at most 3.4e-3).
    bound = 1e-4 if n <= 3 else 1e-2
    assert all(v <= bound for v in rel.values()), sorted(rel.items(), key=lambda kv: -kv[1])[:6]


def _capi_unpack(vec, tr):
    from ndivplanning_amd.models import image_autoencoder as IA
    return IA.unpack_autoencoder_vector(vec, tr.encoder, tr.decoder)


def _script_rank(rank, world, port, kw, out_dir):
    _rank_env(rank, world, port)
    import models.image_autoencoder  # noqa: F401  (the reference's class paths in the checkpoints)
    from ndivplanning_amd import train_autoencoder as script
    initial, saves = {}, []
    real_trainer, real_save = script.AutoencoderTrainer, torch.save

    def spy(encoder, decoder, **k):
        for prefix, m in (("encoder.", encoder), ("decoder.", decoder)):
            initial.update({prefix + a: v.detach().cpu().clone() for a, v in m.state_dict().items()})
        return real_trainer(encoder, decoder, **k)

    def counting_save(obj, f, *a, **k):
        saves.append(os.path.basename(str(f)))
        return real_save(obj, f, *a, **k)
    script.AutoencoderTrainer, torch.save = spy, counting_save
    try:
        _, _, losses = script.train(log=lambda *a: None, **kw)
    finally:
        script.AutoencoderTrainer, torch.save = real_trainer, real_save
    tr = script.train.last_trainer
    torch.save({"params": tr.params.cpu(), "stats": tr.stats.cpu(), "losses": losses, "initial": initial,
                "batch": tr.batch, "saves": saves, "named": {k: v.cpu() for k, v in tr.named_parameters().items()}},
               os.path.join(out_dir, "ae_script%d.pt" % rank))


def _script_kw(save_dir, **extra):
    return dict(dict(data_path="synthetic:2:images", batch_size=2, num_epochs=2, save_dir=str(save_dir)), **extra)


def _run_script(tmp_path, name, **extra):
    out = tmp_path / name
    out.mkdir()
    _spawn(_script_rank, _script_kw(out / "models", **extra), str(out))
    return [torch.load(str(out / ("ae_script%d.pt" % r))) for r in range(2)]


def test_per_rank_statistics_replay_bit_exact(tmp_path):
    """train(sync_batchnorm=False) on 2 ranks, replayed in one process: each rank's trajectory of every batch through
    ndp_ae_train_grads with that rank's own running statistics, the mean of the two gradients, Adam -- the same bits."""
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    from ndivplanning_amd.models.image_autoencoder import Decoder, Encoder
    from ndivplanning_amd.train_autoencoder import build_models, make_dataset
    res = _run_script(tmp_path, "per_rank", sync_batchnorm=False)
    assert res[0]["batch"] == res[1]["batch"] == 15                   # one trajectory of 15 frames per rank, not 30
    assert torch.equal(res[0]["params"], res[1]["params"]) and res[0]["losses"] == res[1]["losses"]
    assert not torch.equal(res[0]["stats"], res[1]["stats"])           # each rank normalised over its own images
    # the run's loader order: seeds, dataset, loader, the modules' construction (CPU stream), as train() does
    torch.manual_seed(1)
    np.random.seed(1)
    loader = torch.utils.data.DataLoader(make_dataset("synthetic:2:images"), batch_size=2, shuffle=True)
    build_models(DEV)
    batches = [images for _ in range(2) for images, _, _, _ in loader]
    assert len(batches) == 2 and all(b.shape[0] == 2 for b in batches)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict({k[8:]: v for k, v in res[0]["initial"].items() if k.startswith("encoder.")})
    dec.load_state_dict({k[8:]: v for k, v in res[0]["initial"].items() if k.startswith("decoder.")})
    tr = AutoencoderTrainer(enc.to(DEV).train(), dec.to(DEV).train(), batch=15)
    stats = [tr.stats.clone(), tr.stats.clone()]
    losses = []
    for images in batches:
        grads, loss = [], 0.0
        for r in range(2):
            tr.stats = stats[r]
            tr.grads(images[r:r + 1].reshape(-1, 3, 128, 128).contiguous().to(DEV))
            grads.append(tr.grad.clone())
            loss += tr.loss.item() / 2
        tr.grad.copy_(grads[0] + grads[1]).mul_(0.5)                  # dp.mean_all_reduce of two ranks
        tr.apply()
        losses.append(float(np.float32(loss)))
    assert torch.equal(tr.params.cpu(), res[0]["params"])
    assert torch.equal(stats[0].cpu(), res[0]["stats"]) and torch.equal(stats[1].cpu(), res[1]["stats"])
    assert losses == res[0]["losses"]


def test_script_defaults_train_the_single_process_step(tmp_path):
    """train() under two ranks with its defaults (cross-rank statistics, bucketed exchange on its own communicator)
    against train() in one process on the whole batch: the same losses, the same running statistics, parameters within
    Adam's sign tolerance; checkpoints written once, by rank 0; grad_exchange="single" gives the same bits."""
    import models.image_autoencoder as shim
    from ndivplanning_amd import train_autoencoder as script
    res = _run_script(tmp_path, "bucketed")
    assert res[0]["batch"] == res[1]["batch"] == 15
    assert torch.equal(res[0]["params"], res[1]["params"]) and torch.equal(res[0]["stats"], res[1]["stats"])
    assert res[0]["losses"] == res[1]["losses"] and len(res[0]["losses"]) == 2
    assert sorted(res[0]["saves"]) == ["decoder_1.pt", "encoder_1.pt"] and res[1]["saves"] == []
    saved = tmp_path / "bucketed" / "models"
    assert sorted(os.listdir(str(saved))) == ["decoder_1.pt", "encoder_1.pt"]
    enc = torch.load(str(saved / "encoder_1.pt"), map_location=DEV, weights_only=False)
    dec = torch.load(str(saved / "decoder_1.pt"), map_location=DEV, weights_only=False)
    assert isinstance(enc, shim.Encoder) and isinstance(dec, shim.Decoder)
    assert type(enc).__module__ == type(dec).__module__ == "models.image_autoencoder"
    # one process, the whole batch of 2 trajectories
    _, _, losses = script.train(log=lambda *a: None, **_script_kw(tmp_path / "single_process"))
    tr = script.train.last_trainer
    assert tr.batch == 30
    # the first step's loss: the same up to the statistics' summation order; later ones after Adam steps whose signs
    # differ where a gradient is noise (below)
    assert abs(losses[0] - res[0]["losses"][0]) <= 2e-6 * abs(losses[0]), (losses, res[0]["losses"])
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(losses, res[0]["losses"])), (losses, res[0]["losses"])
    # (the running statistics also carry the parameters' sign-step differences)
    stats = tr.stats.cpu()
    assert float((stats - res[0]["stats"]).abs().max()) <= 1e-2 * float(stats.abs().max())
    worst, off, total = 0.0, 0, 0
    for name, want in tr.named_parameters().items():
        if name in NOISE_BIASES:
            continue
        diff = (res[0]["named"][name] - want.cpu()).abs()
        worst = max(worst, float(diff.max()))
        off += int((diff > 2e-5).sum())
        total += diff.numel()
    # Adam's first steps are lr * sign(g) whatever |g| is: an element whose gradient lies inside the summation-order noise
    # may step the other way, 2 lr per step (as in test_gpu_forward_model's cross-rank test)
    assert worst <= 2.5 * len(losses) * LR and off <= 0.05 * total, (worst, off, total)
    # ONE collective between backward and Adam: two ranks, one addition per element -- the same bits as per bucket
    single = _run_script(tmp_path, "single", grad_exchange="single")
    assert torch.equal(single[0]["params"], res[0]["params"]) and single[0]["losses"] == res[0]["losses"]
    assert torch.equal(single[0]["stats"], res[0]["stats"])
