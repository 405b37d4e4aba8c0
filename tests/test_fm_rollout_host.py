"""The rollout link kernels and the gradient sum (csrc/ndp_forward_model.inc, namespace ndp::fm_rollout) on the CPU, under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/host_drivers/fm_rollout.inc follows the library's source in main.hip and runs
the kernels' cores by their schedule, every buffer (inputs with their image stride, outputs, each LDS array) in an
allocation of exactly its size.  The expected values are the plain numpy restatement in tests/rollout_common.py: every
addition is in a fixed order, so sums and adds must agree to the bit.  The sanitizers are on the host half of the
stand-alone driver only; it runs as an ordinary child process.  No GPU involved (the same kernels on the GPU:
tests/test_gpu_forward_rollout.py)."""
import numpy as np
import pytest

import host_driver
import rollout_common as C

F32 = np.float32


@pytest.fixture(scope="module")
def driver():
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    return host_driver.build()


def _images(rng, n):
    return (rng.rand(n, 3, 128, 128).astype(F32) * F32(2.0) - F32(1.0))


def _cases():
    rng = np.random.RandomState(5)
    cases = []
    for n in (1, 3):
        floats = _images(rng, n)
        frames8 = rng.randint(0, 256, (n, 128, 128, 3)).astype(np.uint8)
        frames8[0, 0, 0], frames8[-1, -1, -1] = (0, 255, 128), (255, 0, 1)
        # image strides: the images of a window tensor lie (H + 1) frames apart, and further inside a longer trajectory
        for tgt, name in ((floats, "f32"), (frames8, "u8")):
            cases.append(dict(kind="begin", frames=tgt, stride=4 * C.VALUES, name=(n, name)))
        state, resid = _images(rng, n), (_images(rng, n) * F32(0.25))
        for tgt, name in ((floats, "f32"), (frames8, "u8"), (C.as_float_frames(frames8), "u8 as f32")):
            # steps 3: the first step resets the running loss, the middle one adds, the last one also adds to loss_sum
            for step, steps in ((0, 3), (1, 3), (2, 3), (0, 1)):
                cases.append(dict(kind="advance", state=state, resid=resid, target=tgt, stride=C.VALUES if steps == 1 else 5 * C.VALUES,
                                  step=step, steps=steps, loss=F32(0.625), loss_sum=F32(3.5), name=(n, name, step, steps)))
        cases.append(dict(kind="chain", local=_images(rng, n) * F32(1e-5), g_next=_images(rng, n) * F32(1e-5),
                          d_cur=_images(rng, n) * F32(1e-5), name=(n,)))
    # gradient vectors: not a multiple of 4 x the block (and not of 4), one exact block, shorter than one float4
    for count, floats, stride in ((3, 4 * 256 * 2 + 4 * 77 + 3, 4 * 256 * 3), (2, 1024, 1024), (1, 5, 8), (4, 3, 4), (3, 1031, 1032)):
        cases.append(dict(kind="sum", grads=rng.randn(count, floats).astype(F32), stride=stride, name=(count, floats)))
    return cases


@pytest.fixture(scope="module")
def report(driver, tmp_path_factory):
    cases = _cases()
    return cases, C.run_driver(driver, cases, tmp_path_factory.mktemp("fm_rollout_cases"))


def test_begin_gathers_the_first_frame_as_the_floats_the_loader_would_upload(report):
    cases, results = report
    seen = 0
    for c, got in zip(cases, results):
        if c["kind"] != "begin":
            continue
        seen += 1
        assert got.tobytes() == C.as_float_frames(c["frames"]).tobytes(), c["name"]
    assert seen == 4


def test_advance_states_local_gradients_and_losses_are_bit_equal_to_the_fixed_order_restatement(report):
    cases, results = report
    seen = 0
    for c, got in zip(cases, results):
        if c["kind"] != "advance":
            continue
        seen += 1
        sn, local, partial, lk, loss, loss_sum = C.want_advance(c["state"], c["resid"], c["target"], c["step"], c["steps"],
                                                                c["loss"], c["loss_sum"])
        assert got[0].tobytes() == sn.tobytes() and got[1].tobytes() == local.tobytes(), c["name"]
        assert got[2].tobytes() == partial.tobytes(), c["name"]
        want_losses = np.full(c["steps"], -7.0, F32)
        want_losses[c["step"]] = lk
        assert got[3].tobytes() == want_losses.tobytes(), (c["name"], got[3], want_losses)
        assert F32(got[4]).tobytes() == F32(loss).tobytes() and F32(got[5]).tobytes() == F32(loss_sum).tobytes(), c["name"]
        # and the numbers mean what the definition says
        x = C.as_float_frames(c["target"]).astype(np.float64)
        exact = (((c["state"].astype(np.float64) + c["resid"]) - x) ** 2).mean()
        assert abs(float(lk) - exact) <= 1e-6 * exact, c["name"]
    assert seen == 2 * 3 * 4


def test_byte_targets_and_the_floats_of_the_same_bytes_give_identical_bits(report):
    cases, results = report
    by_name = {c["name"]: r for c, r in zip(cases, results) if c["kind"] == "advance"}
    for n in (1, 3):
        for step, steps in ((0, 3), (2, 3), (0, 1)):
            a, b = by_name[(n, "u8", step, steps)], by_name[(n, "u8 as f32", step, steps)]
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def test_chain_and_gradient_sum_add_in_the_stated_order(report):
    cases, results = report
    for c, got in zip(cases, results):
        if c["kind"] == "chain":
            want = ((c["local"] + c["g_next"]).astype(F32) + c["d_cur"]).astype(F32)
            assert got.tobytes() == want.tobytes(), c["name"]
        elif c["kind"] == "sum":
            want = c["grads"][0].copy()
            for h in range(1, c["grads"].shape[0]):
                want = (want + c["grads"][h]).astype(F32)
            assert got.tobytes() == want.tobytes(), c["name"]
