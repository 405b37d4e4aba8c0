"""The driver's multi-GPU invocation, `python3 bench.py --gpus N --steps 20 --warmup 5 --full` with no torch.distributed.run
environment, rehearsed with two ranks on the one GPU of the test box (NDP_BENCH_ONE_GPU=1: every rank uses cuda:0;
gloo for the rendezvous / collectives because RCCL refuses two ranks on one device).  The figures it prints are not
measurements (the ranks time-slice one GPU); what is tested is that the parent starts the ranks, relays ONE JSON line,
exits 0, and that the data-parallel workloads all ran with replicas that stayed bit-identical."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("exchange", ["auto", "p2p"])
def test_bench_gpus_2_starts_its_own_ranks(exchange):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(NDP_BENCH_ONE_GPU="1", NDP_DIST_BACKEND="gloo", NDP_DP_EXCHANGE=exchange, NDP_BENCH_LAUNCH_TIMEOUT_S="500")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5",
                        "--full"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]                            # ONE JSON line on stdout, nothing else
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 20 and out["warmup"] == 5 and out["scaling"] == "weak"
    assert out["metric"] == "gan_train_steps_per_sec_traj8_batch64" and out["value"] > 0
    cfg = out["config"]
    assert cfg["global_batch"] == 128 and cfg["parallelism"] == "dp2"
    assert cfg["replicas_bit_identical"] is True
    # shared GPU: "auto" must have chosen the collective (the in-kernel hand-shake needs a GPU per rank), "p2p" forces it
    assert cfg["gradient_exchange"].startswith("rccl" if exchange == "auto" else ("p2p", "rccl (p2p"))
    assert "extras_failed" not in out, out.get("extras_failed")
    for name in ("strong_config3", "config5_shard", "forward_model_dp"):
        assert name in out, sorted(out)
        assert out[name]["replicas_bit_identical"] is True, (name, out[name])
    assert out["strong_config3"]["global_batch"] == 256 and out["strong_config3"]["scaling"] == "strong"
    assert "roofline" in out and out["roofline"]["kernel"].startswith("k_")


def test_plain_run_times_exactly_k_steps_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one bracket of K steps, nothing of --full, and the
    outputs of the last timed step as float32 .npy files that agree with the losses of the JSON line."""
    import numpy as np
    out_dir = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "gan_train_steps_per_sec_traj8_batch64" and out["unit"] == "steps/s" and out["dtype"] == "f32"
    assert out["steps"] == 20 and out["warmup"] == 5 and out["higher_is_better"] is True
    assert out["config"]["repeats"] == 1 and out["ms_per_step"] == out["config"]["repeat_ms_per_step"][0]
    assert abs(out["value"] * out["ms_per_step"] - 1e3) <= 1e-2 * 1e3
    for name in ("roofline", "parity_step0", "cpu_baseline", "forward_model", "config4", "large_m", "h2d_per_launch"):
        assert name not in out, name
    m = out["config"]["rows_per_gpu"]
    want = {"action_hat": (m, 4), "losses": (3,), "g_params": (83780,), "d_params": (58305,)}
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in want)
    arrays = {n: np.load(out_dir / (n + ".npy")) for n in want}
    for n, shape in want.items():
        assert arrays[n].dtype == np.float32 and arrays[n].shape == shape and np.isfinite(arrays[n]).all(), n
    last = out["config"]["last_losses"]
    assert np.array_equal(arrays["losses"], np.array([last["D"], last["G"], last["ndiv"]], dtype=np.float32))
