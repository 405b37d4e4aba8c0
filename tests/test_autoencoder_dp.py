"""CPU: the autoencoder's data-parallel ABI and script plumbing (no GPU needed).  ndp_ae_grad_buckets tiles the flat
vector in the order the backward pass completes it; the new entry points reject bad arguments with an error code;
ndp_ae_bucket_wait refuses before any data-parallel call has recorded the events; the script's new options parse and a
world size that does not divide the global batch is refused before any process group or GPU is touched."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


def _weight_offset(lib, what, index):
    off, dims = ctypes.c_int64(), (ctypes.c_int64 * 6)()
    assert lib.ndp_ae_layout(what, index, ctypes.byref(off), dims) == 0
    return off.value


def test_buckets_tile_the_flat_vector_once(lib):
    from ndivplanning_amd import _capi
    buckets = _capi.ae_grad_buckets()
    total = lib.ndp_ae_param_floats()
    assert len(buckets) == 6 and all(c > 0 for _, c in buckets)
    covered = sorted(buckets)
    assert covered[0][0] == 0 and covered[-1][0] + covered[-1][1] == total
    assert all(a[0] + a[1] == b[0] for a, b in zip(covered, covered[1:]))


def test_buckets_come_in_completion_order_at_layer_boundaries(lib):
    from ndivplanning_amd import _capi
    buckets = _capi.ae_grad_buckets()
    layer = [_weight_offset(lib, 0, i) for i in range(12)]            # weights of conv1..6, deconv1..6
    bn0 = _weight_offset(lib, 2, 0)                                    # conv1_bn.weight: the first BatchNorm parameter
    # {deconv3..6}, {deconv2}, {deconv1, conv6}, {conv5}, {conv1..4}, {BatchNorm weights and biases}
    assert [o for o, _ in buckets] == [layer[8], layer[7], layer[5], layer[4], layer[0], bn0]
    assert buckets[0][0] + buckets[0][1] == bn0                        # the decoder tail ends where BatchNorm starts
    assert buckets[1][1] == layer[8] - layer[7] == 1024 * 16 * 512 + 512   # deconv2 alone: 8.4 M floats
    assert buckets[-1][0] + buckets[-1][1] == lib.ndp_ae_param_floats()


def test_bad_arguments_return_error_codes(lib):
    off, cnt = (ctypes.c_int64 * 16)(), (ctypes.c_int64 * 16)()
    n = ctypes.c_int(-1)
    assert lib.ndp_ae_grad_buckets(off, cnt, 5, ctypes.byref(n)) != 0 and n.value == -1     # capacity too small
    assert b"6 buckets" in lib.ndp_last_error()
    assert lib.ndp_ae_grad_buckets(None, cnt, 16, ctypes.byref(n)) != 0
    assert lib.ndp_ae_grad_buckets(off, None, 16, ctypes.byref(n)) != 0
    assert lib.ndp_ae_grad_buckets(off, cnt, 16, None) != 0
    assert lib.ndp_ae_grad_buckets(off, cnt, 16, ctypes.byref(n)) == 0 and n.value == 6
    buf = (ctypes.c_float * 64)()                                       # host memory: every check comes before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(params=p, running=p, images=p, n=1, grad=p, loss=p, loss_sum=None, recon=None, ws=p, stream=None,
                fn=None, ctx=None, world=1)

    def call(**bad):
        a = dict(good, **bad)
        return lib.ndp_ae_train_grads_dp(a["params"], a["running"], a["images"], a["n"], a["grad"], a["loss"],
                                         a["loss_sum"], a["recon"], a["ws"], a["stream"], a["fn"], a["ctx"], a["world"])
    for bad in (dict(params=None), dict(images=None), dict(grad=None), dict(loss=None), dict(ws=None), dict(world=0),
                dict(world=-1), dict(world=4097), dict(n=0), dict(n=-3), dict(n=8193)):
        assert call(**bad) != 0, bad
        assert b"ndp_ae_train_grads_dp" in lib.ndp_last_error(), bad
    for b in (-1, 6, 7):
        assert lib.ndp_ae_bucket_wait(b, None) != 0
        assert b"out of range" in lib.ndp_last_error()


def test_bucket_wait_before_any_data_parallel_call_is_an_error(lib):
    """A fresh process: no ndp_ae_train_grads_dp call has recorded the events, so there is nothing to wait for."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from ndivplanning_amd import _capi\n"
            "lib = _capi.load()\n"
            "rc = [lib.ndp_ae_bucket_wait(b, None) for b in range(6)]\n"
            "assert all(r != 0 for r in rc), rc\n"
            "assert b'ndp_ae_bucket_wait' in lib.ndp_last_error()\n"
            "print('refused', rc)\n") % ROOT
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "refused" in res.stdout, res.stdout[-1500:] + res.stderr[-1500:]


def test_cli_flags_parse():
    from ndivplanning_amd.train_autoencoder import make_parser
    p = make_parser()
    args = p.parse_args([])
    assert args.sync_batchnorm is True and args.grad_exchange == "bucketed"
    args = p.parse_args(["--no-sync-batchnorm", "--grad-exchange", "single", "--batch-size", "8"])
    assert args.sync_batchnorm is False and args.grad_exchange == "single" and args.batch_size == 8
    with pytest.raises(SystemExit):
        p.parse_args(["--grad-exchange", "ring"])


def test_world_size_that_does_not_divide_the_batch_is_refused_without_a_gpu(monkeypatch, tmp_path):
    import torch
    import torch.distributed as dist
    from ndivplanning_amd import train_autoencoder as script

    def no_gpu(*a, **k):
        raise AssertionError("touched the GPU before checking the batch")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "3")
    monkeypatch.setenv("LOCAL_RANK", "0")
    with pytest.raises(ValueError, match="multiple of the 3 ranks"):
        script.train("synthetic:4:images", batch_size=4, num_epochs=1, save_dir=str(tmp_path))
    with pytest.raises(ValueError, match="grad_exchange"):
        script.train("synthetic:4:images", batch_size=3, num_epochs=1, save_dir=str(tmp_path), grad_exchange="ring")
    assert not dist.is_initialized() and not os.listdir(str(tmp_path))
