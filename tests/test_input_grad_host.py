"""The input-gradient switch (ndivplanning_amd.input_grad) on the host: state handling only, no GPU."""
import threading

from ndivplanning_amd import _capi
from ndivplanning_amd.input_grad import enabled, input_gradients


def test_off_by_default_and_restored_on_exit():
    assert not enabled()
    with input_gradients():
        assert enabled()
    assert not enabled()
    try:
        with input_gradients():
            raise KeyError("x")
    except KeyError:
        pass
    assert not enabled()


def test_nests_and_restores_the_previous_state():
    with input_gradients():
        with input_gradients(False):
            assert not enabled()
            with input_gradients(True):
                assert enabled()
            assert not enabled()
        assert enabled()
    assert not enabled()


def test_one_object_is_reentrant_and_works_as_a_decorator():
    ctx = input_gradients()
    with ctx:
        with ctx:
            assert enabled()
        assert enabled()
    assert not enabled()

    @input_gradients()
    def inside():
        return enabled()
    assert inside() and inside() and not enabled()


def test_the_switch_is_per_thread():
    seen = {}
    entered, release = threading.Event(), threading.Event()

    def other():
        seen["before"] = enabled()
        with input_gradients():
            seen["inside"] = enabled()
            entered.set()
            release.wait(10)
        seen["after"] = enabled()
    with input_gradients():
        t = threading.Thread(target=other)
        t.start()
        assert entered.wait(10)
    assert not enabled()                     # the other thread is still inside its own switch
    release.set()
    t.join(10)
    assert seen == {"before": False, "inside": True, "after": False}


def test_new_entry_points_are_declared():
    for name in ("ndp_g_input_grad", "ndp_d_input_grad", "ndp_fm_input_grads"):
        assert name in _capi.SIGNATURES
