"""k_wgrad's block -> (job, chunk) map (csrc/ndp_kernels.hip: wgrad_slot) and the slab sums behind it, at the smallest
shape of every dispatch branch of the launch plan; checks of coverage, parity and bit-equality.

 * the map itself, on the host (no GPU): ndp_step_wgrad_blocks enumerates, through the function the kernel calls, the pair
   of every block of both launches at every shape of the gradient suite, first and repeat D step: each (job, chunk <
   the job's count) exactly once, no pair outside the job table, the WIDE jobs' blocks first, chunk % 8 == block % 8
   behind them, NDiv blocks exactly past the slots;
 * D and G gradients against the fp64 oracle (test_gpu_step_gradients' run, rule and bounds, by import) at (5, 7, 2)
   uniform small chunks, (40, 6, 1) G heavy 24 / light 12 -- the only branch with slots that have nothing to do, and NDiv
   blocks behind the D jobs --, (40, 5, 5) NDiv as a launch of its own;
 * at (40, 6, 1) with both slab areas filled with NaN before the step: a slab element that no workgroup wrote would leave
   a NaN in the gradient k_reduce_adam sums;
 * parameters after 3 steps at (5, 7, 2) and (40, 6, 1), bit for bit: eager launches == graph replay, run 1 == run 2
   (k_reduce_adam adds the slabs in chunk order whatever order the workgroups ran in).
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_step_gradients as G

DEV = G.DEV
BRANCHES = [(5, 7, 2), (40, 6, 1), (40, 5, 5)]
MAX_JOBS = 28


def _config(batch, k, nz):
    from ndivplanning_amd import _capi
    return _capi.StepConfig(noise_dim=nz, num_sample=k, flat=7 * batch)


def _blocks(lib, cfg, which, first):
    """Of a step's weight-gradient launch: grid, pairs [grid, 2], the chunk count of every job [28], (njobs, nwide,
    wide_chunks, nchunks), and the slab area (offset, floats)."""
    table = np.zeros(MAX_JOBS + 4, dtype=np.int32)
    area = np.zeros(2, dtype=np.int64)
    probe = np.zeros(2, dtype=np.int32)
    grid = lib.ndp_step_wgrad_blocks(ctypes.byref(cfg), which, first, probe.ctypes.data, 0, table.ctypes.data, area.ctypes.data)
    assert grid > 0
    pairs = np.full((grid, 2), -7, dtype=np.int32)
    assert lib.ndp_step_wgrad_blocks(ctypes.byref(cfg), which, first, pairs.ctypes.data, grid, table.ctypes.data,
                                     area.ctypes.data) == grid
    return grid, pairs, table[:MAX_JOBS].copy(), tuple(int(v) for v in table[MAX_JOBS:]), (int(area[0]), int(area[1]))


@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


@pytest.mark.parametrize("first", [1, 0])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("batch,k,nz", G.SHAPES)
def test_every_pair_runs_exactly_once(lib, batch, k, nz, which, first):
    grid, pairs, chunks, (njobs, nwide, wide_chunks, nchunks), _ = _blocks(lib, _config(batch, k, nz), which, first)
    job, chunk = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    assert 1 <= njobs and njobs + nwide <= MAX_JOBS and (chunks[:njobs + nwide] >= 1).all() and (chunks[njobs + nwide:] == 0).all()
    assert nchunks == chunks[:njobs].max() and (chunks[njobs:njobs + nwide] == wide_chunks).all()
    assert ((job >= -2) & (job < njobs + nwide)).all()                      # no pair outside the job table
    slots = nwide * wide_chunks + 8 * ((nchunks + 7) // 8) * njobs
    b = np.arange(grid)
    ndiv = job == -2
    assert (ndiv == (b >= slots)).all()                                    # NDiv blocks ride behind the slots
    live = ~ndiv
    assert (job[live] >= 0).all() and (chunk[live] >= 0).all() and (chunk[ndiv] == -2).all()
    work = live & (chunk < chunks[np.where(live, job, 0)])                 # k_wgrad: chunk >= the job's count returns
    seen = np.zeros((MAX_JOBS, int(chunks.max())), dtype=np.int32)
    np.add.at(seen, (job[work], chunk[work]), 1)
    want = (np.arange(seen.shape[1])[None, :] < chunks[:, None]).astype(np.int32)
    assert (seen == want).all()                                            # every (job, chunk) once, none twice
    # WIDE blocks first; behind them one XCD per row chunk
    wide = b < nwide * wide_chunks
    assert (job[wide] >= njobs).all() and (job[live & ~wide] < njobs).all() and work[wide].all()
    rest = live & ~wide
    assert ((chunk[rest] & 7) == ((b[rest] - nwide * wide_chunks) & 7)).all()
    if (which, first, (batch, k, nz)) == (1, 1, (40, 6, 1)):               # the branch with slots that have nothing to do
        assert grid == 624 and int((live & ~work).sum()) == 168 and int(work.sum()) == 12 * 24 + 14 * 12 == grid - 168


@pytest.mark.gpu
@pytest.mark.parametrize("batch,k,nz", BRANCHES)
def test_gradients_at_each_dispatch_branch(batch, k, nz):
    G._run_and_adjudicate("dispatch B %d K %d nz %d" % (batch, k, nz), batch, k, nz, G.FACTORS[0])


@pytest.mark.gpu
def test_every_slab_element_is_written(lib):
    """(40, 6, 1): G 24 / 12 chunks with idle slots, D with NDiv blocks behind its jobs.  The slab areas hold NaN when the
    step starts; the gradients are finite and within the suite's bounds of the fp64 oracle."""
    from ndivplanning_amd.trainer import GanTrainer
    batch, k, nz = 40, 6, 1
    factor = G.FACTORS[0]
    g0, d0, codes, actions, noise = G._case_inputs(batch, k, nz)
    flat = codes.shape[0]
    dec, dis = G._load_modules(g0, d0, nz)
    tr = GanTrainer(dec, dis, flat=flat, num_sample=k, pairwise_div_factor=factor, use_graph=True)
    for which in (0, 1):
        _, _, chunks, _, (off, floats) = _blocks(lib, tr.cfg, which, 1)
        assert floats > 0 and off + floats <= tr.workspace.numel()
        tr.workspace[off:off + floats].fill_(float("nan"))
        if which == 1:
            assert sorted(set(int(c) for c in chunks if c)) == [12, 24]   # the branch this test is about
    torch.cuda.synchronize()
    tr.step(codes.to(DEV), actions.to(DEV), noise.to(DEV))
    run = G._exposed(tr)
    assert torch.isfinite(run["d_grad"]).all() and torch.isfinite(run["g_grad"]).all()
    assert torch.isfinite(run["d_post"]).all() and torch.isfinite(tr.g_flat.detach()).all()
    rep = G.C.adjudicate("NaN slabs B 40 K 6 nz 1", run, g0, d0, codes, actions, noise, factor, 1.0 / (flat * k))
    print(rep.line())
    rep.assert_ok()


def _params_after(batch, k, nz, steps, use_graph):
    from ndivplanning_amd.trainer import GanTrainer
    g0, d0, codes, actions, noise = G._case_inputs(batch, k, nz)
    dec, dis = G._load_modules(g0, d0, nz)
    tr = GanTrainer(dec, dis, flat=codes.shape[0], num_sample=k, pairwise_div_factor=G.FACTORS[0], use_graph=use_graph)
    for _ in range(steps):
        tr.step(codes.to(DEV), actions.to(DEV), noise.to(DEV))
    torch.cuda.synchronize()
    return tr.g_flat.detach().cpu().clone(), tr.d_flat.detach().cpu().clone()


@pytest.mark.gpu
@pytest.mark.parametrize("batch,k,nz", [(5, 7, 2), (40, 6, 1)])
def test_parameters_are_bitwise_reproducible(batch, k, nz):
    start = _params_after(batch, k, nz, 0, use_graph=False)
    eager = _params_after(batch, k, nz, 3, use_graph=False)
    graph1 = _params_after(batch, k, nz, 3, use_graph=True)
    graph2 = _params_after(batch, k, nz, 3, use_graph=True)
    for name, a, b, c in zip("GD", eager, graph1, graph2):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), "%s: eager launches differ from graph replay" % name
        assert torch.equal(b, c), "%s: run 1 differs from run 2" % name
    assert not torch.equal(eager[0], start[0]) and not torch.equal(eager[1], start[1])   # the steps did update both
