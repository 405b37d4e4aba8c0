"""k_wgrad's main loop (csrc/ndp_kernels.hip: wgrad_loop): the operand ring of PF = 8 steps at every step count at which it
takes another path, every B-row map and every job kind; gradients against the fp64 oracle under the suite's rule and
bounds (test_gpu_step_gradients' run, by import) and parameters bit for bit.

A chunk of s steps runs s // 8 passes of the loop and s % 8 steps of the remainder.  Steps per chunk of a job over R rows
in n chunks: ((ceil(R / n) + 15) & ~15) / 16, the last chunk what is left.  Rows are padded to 32 (NDP_ROW_PAD), so the
fused D launch runs pad32(7 B) + pad32(7 B K) rows, its fc1 code jobs seg_entries + pad32(7 B) entries, G pad32(7 B K)
rows and seg_entries entries; test_step_counts_reach_every_path computes the counts below from the chunk counts
ndp_step_wgrad_blocks reports and asserts them (it needs no GPU).  Steps per chunk, "a/b" = all chunks but the last /
the last:

  shape        D fused: fc2, fc3, tail, fc4   fc1 codes   G: fc2 .. fc4   fc5, tail   fc1 codes
  (5, 7, 2)    4                              2 / 0       4               4           1
  (16, 8, 2)   8      (exactly PF)            3 / 1 / 0   4               4           1 / 0
  (18, 8, 2)   9      (PF + 1)                3 / 2 / 0   4               4           1 / 0
  (19, 7, 2)   9 / 7  (below PF)              4 / 1 / 0   4               4           1
  (32, 8, 2)   16 / 14 (2 PF)                 5 / 0       5 / 2 / 0       10 / 2      2 / 1 / 0
  (34, 8, 2)   17     (2 PF + 1)              5 / 4       5               10          2 / 1
  (72, 6, 2)   28 / 26                        10          8 / 6           16 / 14     4
  repeat D step at (64, 6, 2), 32 / 8 chunks: fc2, fc3 11 / 6 / 0; fc1 codes (by b_rowdiv / b_rowmod), tail, fc4 42

so the loop runs 0 passes + 1 .. 7 steps, 1 pass + 0 / 1 / 2 / 3 / 6 steps, 2 passes + 0 / 1 steps, 3 passes + 2 / 4 steps
and 5 passes + 2 steps, with last chunks shorter than the others, one-step chunks and chunks with no step at all.  G's
heavy jobs enter the loop at (72, 6, 2) (8 steps = 128 rows per chunk).

B-row maps and kinds, and where each runs on the GPU:
  WB_PLAIN    fc2 .. fc4 of D and fc2 .. fc5 of G (every shape); G's fc1 code columns in Decoder's backward
              (code_rep = 1, b_rowmod unset: test_decoder_backward_with_unaligned_codes)
  WB_SEGWRAP  D's fc1 code columns in the fused step: segment-sum entries followed by the real rows (every shape)
  WB_SEG      G's fc1 code columns in the fused step (every shape)
  WB_DIV      D's fc1 code columns whenever they are not segment sums: build_d_jobs always sets b_rowmod = the pass' rows,
              so a repeat D step (b_rowdiv = K, 42 steps) and EVERY Discriminator backward (b_rowdiv = code_rep, 1 from
              the module) take this loop.  Held to the oracles by test_repeat_d_step_gradient (test_gpu_step_gradients) and
              test_discriminator_forward_backward (test_gpu_parity), not by this file;
              test_module_backward_with_repeated_codes below only compares two divisors inside the same loop.
  WG_SKINNY_B the fc1 tails (D's action columns, G's noise columns), WG_SKINNY_A G.fc5 and D.fc4 (every shape)
  b_vec == 0  B rows that are not 16-byte aligned: only fc1's codes are the caller's tensor.  The step passes a contiguous
              [FLAT, 256] tensor; Decoder's backward passes its input z = [M, 256 + nz] with ld = 256 + nz (257, 258), so
              G's fc1 code jobs read unaligned rows in every Decoder backward.  wgrad_loop reads B as four floats of
              4-byte alignment in every job (one global_load_dwordx4 with this compiler), so this is the same loop as the
              aligned case: test_decoder_backward_with_unaligned_codes runs it over 9 / 5 steps per chunk at odd and
              even nz against the fp64 oracle and from run to run.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_step_gradients as G
from oracle import gan_oracle as O

DEV = G.DEV
PF = 8
LOOP_SHAPES = [(16, 8, 2), (18, 8, 2), (19, 7, 2), (32, 8, 2), (34, 8, 2), (72, 6, 2)]   # (5, 7, 2): test_gpu_wgrad_dispatch
MAX_JOBS = 28
CODE_BLOCKS = 4                                                     # fc1's 256 code columns as 64-column jobs


def _pad(n, to):
    return (n + to - 1) // to * to


def _seg_entries(mpad, k):
    return _pad(mpad // 16 * min(15 // k + 2, 16), 16)


def _job_steps(lib, batch, k, nz, which, first=1):
    """{job: [steps of chunk 0, 1, ...]} of a step's weight-gradient launch (which: 0 D, 1 G), as wgrad_body cuts them."""
    from ndivplanning_amd import _capi
    cfg = _capi.StepConfig(noise_dim=nz, num_sample=k, flat=7 * batch)
    table = np.zeros(MAX_JOBS + 4, dtype=np.int32)
    area = np.zeros(2, dtype=np.int64)
    probe = np.zeros(2, dtype=np.int32)
    assert lib.ndp_step_wgrad_blocks(ctypes.byref(cfg), which, first, probe.ctypes.data, 0, table.ctypes.data, area.ctypes.data) > 0
    njobs = int(table[MAX_JOBS])
    rpad, mpad = _pad(7 * batch, 32), _pad(7 * batch * k, 32)
    assert rpad == lib.ndp_pad_rows(7 * batch) and mpad == lib.ndp_pad_rows(7 * batch * k)
    if which == 0:
        rows, seg_rows = (rpad + mpad, _seg_entries(mpad, k) + rpad) if first else (2 * mpad, 2 * mpad)
        code_jobs = set(range(CODE_BLOCKS))
    else:
        rows, seg_rows = mpad, _seg_entries(mpad, k)
        code_jobs = set(range(CODE_BLOCKS)) | set(range(CODE_BLOCKS + 1, 2 * CODE_BLOCKS + 1))
    out = {}
    for j in range(njobs):
        r, n = (seg_rows if j in code_jobs else rows), int(table[j])
        per = (-(-r // n) + 15) & ~15
        out[j] = [max(0, min(r, (c + 1) * per) - c * per) // 16 for c in range(n)]
    return out


@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


def _counts(steps, jobs):
    return sorted(set(s for j in jobs for s in steps[j]))


def test_step_counts_reach_every_path(lib):
    """The table of the module docstring, from the host's own launch plan (no GPU)."""
    d_heavy, d_codes = range(5, 15), range(0, 4)          # D: fc1 codes 0..3, tail 4, fc2 5..6, fc3 7..14, fc4 15..18
    g_heavy, g_codes = range(10, 22), (0, 1, 2, 3, 5, 6, 7, 8)   # G: fc1 (codes, tail) x 2, fc2, fc3, fc4 10..21, fc5 22..25
    want_d = {(5, 7, 2): ([4], [0, 2]), (16, 8, 2): ([8], [0, 1, 3]), (18, 8, 2): ([9], [0, 2, 3]),
              (19, 7, 2): ([7, 9], [0, 1, 4]), (32, 8, 2): ([14, 16], [0, 5]), (34, 8, 2): ([17], [4, 5]),
              (72, 6, 2): ([26, 28], [10])}
    want_g = {(5, 7, 2): ([4], [1]), (16, 8, 2): ([4], [0, 1]), (18, 8, 2): ([4], [0, 1]), (19, 7, 2): ([4], [1]),
              (32, 8, 2): ([0, 2, 5], [0, 1, 2]), (34, 8, 2): ([5], [1, 2]), (72, 6, 2): ([6, 8], [4])}
    reached = set()
    for shape in want_d:
        d, g = _job_steps(lib, *shape, which=0), _job_steps(lib, *shape, which=1)
        print(shape, "steps reached: D heavy", _counts(d, d_heavy), "codes", _counts(d, d_codes), "tail / fc4", _counts(d, (4, 15)),
              "| G heavy", _counts(g, g_heavy), "codes", _counts(g, g_codes), "tail / fc5", _counts(g, (4, 22)))
        assert (_counts(d, d_heavy), _counts(d, d_codes)) == want_d[shape], shape
        assert d[4] == d[5] == d[15]                                     # tail and fc4: the launch's rows, D's chunk count
        assert (_counts(g, g_heavy), _counts(g, g_codes)) == want_g[shape], shape
        reached |= set(s for steps in (d, g) for per_job in steps.values() for s in per_job)
    rep = _job_steps(lib, 64, 6, 2, which=0, first=0)
    print("repeat D step (64, 6, 2): heavy", _counts(rep, d_heavy), "codes", _counts(rep, d_codes), "tail / fc4", _counts(rep, (4, 15)))
    assert _counts(rep, d_heavy) == [0, 6, 11] and _counts(rep, d_codes) == [42] and rep[4] == rep[15] == [42] * 8
    reached |= set(s for per_job in rep.values() for s in per_job)
    # below PF, PF, PF + 1, 2 PF, 2 PF + 1; a one-step chunk; and a remainder behind more than one pass
    assert {1, PF - 1, PF, PF + 1, 2 * PF, 2 * PF + 1}.issubset(reached) and any(s > 2 * PF and s % PF for s in reached)
    big = _job_steps(lib, 72, 6, 2, which=1)
    assert all(max(big[j]) >= PF for j in g_heavy)                       # G's heavy jobs inside the loop


@pytest.mark.gpu
@pytest.mark.parametrize("batch,k,nz", LOOP_SHAPES)
def test_gradients_at_each_step_count(batch, k, nz):
    G._run_and_adjudicate("loop B %d K %d nz %d" % (batch, k, nz), batch, k, nz, G.FACTORS[0])


@pytest.mark.gpu
def test_module_backward_with_repeated_codes(lib):
    """ndp_d_backward, the call behind Discriminator's backward, with every code row shared by K = 8 rows (code_rep = 8)
    against the call the module itself makes on the K times repeated codes (code_rep = 1).  Both run fc1's code jobs in
    the WB_DIV loop (b_rowmod = 1,120 either way), with b_rowdiv = 8 and 1, over 9 / 7 steps per chunk: this checks the
    division by a reciprocal against the trivial one, not the loop against something independent of it (the module
    docstring says which tests do that).  The same rows, chunks and terms in the same order: bit-equal, and equal from
    run to run."""
    from ndivplanning_amd import _capi
    batch, k, nz = 20, 8, 2
    g0, d0, codes, actions, noise = G._case_inputs(batch, k, nz)
    _, dis = G._load_modules(g0, d0, nz)
    flat = dis.flat_parameters()
    m = codes.shape[0] * k
    mpad = lib.ndp_pad_rows(m)                 # one pass over 1,120 rows, D's 8 chunks: 7 of PF + 1 steps and one of 7
    assert mpad == 1120 and ((-(-mpad // 8) + 15) & ~15) // 16 == PF + 1 and (mpad - 7 * 144) // 16 == PF - 1
    gen = torch.Generator().manual_seed(3)
    a = (torch.rand(m, 4, generator=gen) * 2 - 1).to(DEV)
    d_logits = torch.randn(m, generator=gen).to(DEV)
    c_flat = codes.to(DEV).contiguous()
    c_rep = torch.repeat_interleave(c_flat, k, dim=0).contiguous()
    grads = []
    for code, rep in ((c_flat, k), (c_rep, 1), (c_flat, k)):
        grad = torch.full_like(flat, float("nan"))
        ws = _capi.empty(lib.ndp_d_bwd_ws_floats(m), a)
        with _capi.on_device(a):
            _capi.check(lib.ndp_d_backward(_capi.ptr(flat), _capi.ptr(a), 1, _capi.ptr(code), code.stride(0), rep, m,
                                           _capi.ptr(d_logits), _capi.ptr(grad), None, _capi.ptr(ws), _capi.stream_ptr()),
                        "ndp_d_backward")
        torch.cuda.synchronize()
        grads.append(grad.cpu())
    assert torch.isfinite(grads[0]).all() and float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1]), "code_rep = K differs from the repeated codes"
    assert torch.equal(grads[0], grads[2]), "run 1 differs from run 2"


@pytest.mark.gpu
@pytest.mark.parametrize("nz", [1, 2])
def test_decoder_backward_with_unaligned_codes(lib, nz):
    """Decoder's backward at M = 1,650 rows (1,664 padded; G's 24 / 12 chunks): fc1's code jobs read z's rows with
    ld = 256 + nz floats (257: no row but every fourth 16-byte aligned; 258: every other 8-byte aligned) over 9 steps in
    eleven chunks and 5 in the last, the plain 64 x 64 jobs 5 / 4 steps, fc5 and the noise tail 9 / 5.
    Parameter gradients per tensor against the fp64 oracle: max |run - fp64| <= max(4 x max |fp32 oracle - fp64 oracle|,
    1e-5 x S), S = the largest fp64 gradient entry of the network -- the fp32 oracle sums the same 1,650 terms in fp32
    and takes its own ReLU decisions, so four times its error covers a different summation order and a unit deciding
    differently; the floor is the suite's (test_gpu_parity.test_decoder_forward_backward).  Then run 1 == run 2, bit
    for bit."""
    m = 1650
    mpad = lib.ndp_pad_rows(m)
    per = (-(-mpad // 12) + 15) & ~15
    assert mpad == 1664 and mpad // 64 >= 24 and per // 16 == PF + 1 and (mpad - 11 * per) // 16 == 5
    g, d = O.init_params(1, nz)
    dec, _ = G._load_modules(g, d, nz)
    gen = torch.Generator().manual_seed(100 + nz)
    z = torch.cat([torch.randn(m, 256, generator=gen), torch.rand(m, nz, generator=gen)], dim=1)
    up = torch.randn(m, 4, generator=gen)
    refs = []
    for dtype in (torch.float64, torch.float32):
        gr = {k: v.clone().to(dtype).requires_grad_(True) for k, v in g.items()}
        (O.g_forward(gr, z.to(dtype)) * up.to(dtype)).sum().backward()
        refs.append({k: v.grad.double() for k, v in gr.items()})
    ref64, ref32 = refs
    scale = max(v.abs().max().item() for v in ref64.values())
    zd = z.to(DEV)
    assert zd.stride(0) == 256 + nz and zd.stride(0) % 4 != 0
    runs = []
    for _ in range(2):
        dec.zero_grad()
        (dec(zd) * up.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        runs.append({n: p.grad.detach().cpu().clone() for n, p in dec.named_parameters()})
    worst = []
    for name, got in runs[0].items():
        err = (got.double() - ref64[name]).abs().max().item()
        bound = max(4 * (ref32[name] - ref64[name]).abs().max().item(), 1e-5 * scale)
        worst.append((name, err / bound))
    print("Decoder backward, nz %d, |run - fp64| / bound per tensor: %s" % (nz, ", ".join("%s %.3f" % w for w in worst)))
    assert all(r <= 1.0 for _, r in worst), worst
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), "%s: run 1 differs from run 2" % name


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
@pytest.mark.parametrize("batch,k,nz", [(18, 8, 2), (34, 8, 2)])
def test_parameters_are_bitwise_reproducible(batch, k, nz):
    """Parameters after 3 steps, bit for bit: eager launches == graph replay, run 1 == run 2."""
    start = _params_after(batch, k, nz, 0, use_graph=False)
    eager = _params_after(batch, k, nz, 3, use_graph=False)
    graph1 = _params_after(batch, k, nz, 3, use_graph=True)
    graph2 = _params_after(batch, k, nz, 3, use_graph=True)
    for name, a, b, c in zip("GD", eager, graph1, graph2):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), "%s: eager launches differ from graph replay" % name
        assert torch.equal(b, c), "%s: run 1 differs from run 2" % name
    assert not torch.equal(eager[0], start[0]) and not torch.equal(eager[1], start[1])   # the steps did update both
