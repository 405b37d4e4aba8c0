"""The data that crosses the kernel boundaries of the fused GAN step (activations, weight-gradient slabs, Adam
outputs, packed weight copies): however it is stored, every consumer must see exactly what it saw before.

(i)   one fused step (k_reduce_adam applies Adam itself) equals the split path (gradients out of the grad-only
      k_reduce_adam, then ndp_step_apply_adam) bit for bit: both run adam_update on the same fp32 sum of the same
      slabs in the same order, and they were bitwise equal before the hand-off stores changed (measured with the
      previous build of the library on an MI355X: 0 differing words in parameters and moments of D and G at all six
      shapes below), so nothing weaker than equality is asserted;
(ii)  the packed weight copies the fused Adam refreshes equal a rebuild from the canonical parameters;
(iii) graph replay equals eager launches at a large-M shape (k_wgrad_wide, several workgroups per CU).

Shapes: config 2 (B = 64, K = 6), B = 2 / K = 3 and B = 128 / K = 32 with noise_dim 2 and 5 -- D's 58,305
parameters (one past a multiple of 4), G vectors of two lengths, and both slab plans (64 x 64 jobs only; k_wgrad_wide
with its own slab count per region).
"""
import pytest
import torch

from oracle import gan_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(64, 6), (2, 3), (128, 32)]


def _trainer(nz, flat, k, **kw):
    from ndivplanning_amd.models.gan import Decoder, Discriminator
    from ndivplanning_amd.trainer import GanTrainer
    g, d = O.init_params(0, nz)
    dec, dis = Decoder(nz), Discriminator()
    dec.load_state_dict(g)
    dis.load_state_dict(d)
    return GanTrainer(dec.to(DEV), dis.to(DEV), flat=flat, num_sample=k, **kw)


def _state(tr):
    torch.cuda.synchronize()
    return {"g_params": tr.g_flat.clone(), "g_exp_avg": tr.g_m.clone(), "g_exp_avg_sq": tr.g_v.clone(),
            "d_params": tr.d_flat.clone(), "d_exp_avg": tr.d_m.clone(), "d_exp_avg_sq": tr.d_v.clone()}


def _differing(a, b):
    return int((a.view(torch.int32) != b.view(torch.int32)).sum().item())


@pytest.mark.parametrize("nz", [2, 5])
@pytest.mark.parametrize("batch,k", SHAPES)
def test_fused_adam_equals_split_path_bitwise(batch, k, nz):
    codes, actions, noise = O.synthetic_batch(11, batch, k, nz, steps=1)
    states = []
    for reduce_fn in (None, lambda grad: None):
        tr = _trainer(nz, codes.shape[0], k, use_graph=False, reduce_fn=reduce_fn)
        assert tr.cfg.fuse_adam == (1 if reduce_fn is None else 0)
        tr.step(codes.to(DEV), actions.to(DEV), noise[0].to(DEV))
        states.append(_state(tr))
    assert states[0]["d_params"].numel() == 58305
    for name in states[0]:
        n = _differing(states[0][name], states[1][name])
        err = (states[0][name] - states[1][name]).abs().max().item()
        print("B=%d K=%d nz=%d %s: %d differing words of %d, max |diff| %.3e"
              % (batch, k, nz, name, n, states[0][name].numel(), err))
    for name in states[0]:
        assert torch.equal(states[0][name], states[1][name]), name


@pytest.mark.parametrize("batch,k,nz", [(64, 6, 2), (2, 3, 5), (128, 32, 2)])
def test_packed_copies_refreshed_by_fused_adam_equal_a_rebuild(batch, k, nz):
    codes, actions, noise = O.synthetic_batch(12, batch, k, nz, steps=4)
    outs = []
    for repack in (False, True):
        tr = _trainer(nz, codes.shape[0], k)
        for s in range(3):
            tr.step(codes.to(DEV), actions.to(DEV), noise[s].to(DEV))
        if repack:
            tr._repack()                      # ndp_step_pack_params: the packed copies rebuilt from the parameters
        tr.step(codes.to(DEV), actions.to(DEV), noise[3].to(DEV))
        torch.cuda.synchronize()
        outs.append((tr.action_hat.clone(), tr.g_flat.clone(), tr.d_flat.clone()))
    for x, y, name in zip(outs[0], outs[1], ("action_hat", "g_params", "d_params")):
        print("B=%d K=%d nz=%d %s: %d differing words" % (batch, k, nz, name, _differing(x, y)))
        assert torch.equal(x, y), name


def test_graph_replay_is_bitwise_eager_at_large_m():
    batch, k = 128, 32
    codes, actions, noise = O.synthetic_batch(13, batch, k, 2, steps=4)
    outs = []
    for use_graph in (False, True):
        tr = _trainer(2, codes.shape[0], k, use_graph=use_graph)
        for s in range(4):
            tr.step(codes.to(DEV), actions.to(DEV), noise[s].to(DEV))
        torch.cuda.synchronize()
        outs.append((tr.action_hat.clone(), tr.g_flat.clone(), tr.d_flat.clone(), tr.g_m.clone(), tr.d_v.clone(),
                     tr.losses()))
    for i, name in enumerate(("action_hat", "g_params", "d_params", "g_exp_avg", "d_exp_avg_sq")):
        print("%s: %d differing words" % (name, _differing(outs[0][i], outs[1][i])))
        assert torch.equal(outs[0][i], outs[1][i]), name
    assert outs[0][5] == outs[1][5]
