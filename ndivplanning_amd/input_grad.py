"""The switch for gradients with respect to the INPUTS of `models.gan.Decoder`, `models.gan.Discriminator` and the
eval-mode `models.forward_encoder.ForwardAutoencoder`.

The reference's classes are plain `nn.Module`s, so autograd differentiates them in every input; the reference itself
never asks for such a gradient (it detaches the codes, train_gan.py:152-153), and outside this switch the three modules
raise `NotImplementedError` when one is requested -- that behaviour is pinned by the test suite and stays the default.

    from ndivplanning_amd.input_grad import input_gradients

    with input_gradients():
        loss = ((fwd_model(state, actions) - goal) ** 2).mean()
        loss.backward()                      # actions.grad, state.grad

Inside it the modules' outputs are differentiable in their tensor inputs as well (ndp_g_input_grad, ndp_d_input_grad,
ndp_fm_input_grads); everything else is as outside.  The switch is thread-local and re-entrant; `input_gradients(False)`
switches it off again for a region.  Only the FORWARD call has to run inside the switch: its backward may run anywhere.
"""
import contextlib
import threading

_state = threading.local()


def enabled():
    """Whether input gradients are switched on in the calling thread."""
    return getattr(_state, "on", False)


class input_gradients(contextlib.ContextDecorator):
    """Context manager / decorator: input gradients on (or, with enabled=False, off) in the calling thread; the previous
    state comes back on exit.  One object may be entered again while it is active."""

    def __init__(self, enabled=True):
        self._want = bool(enabled)
        self._saved = threading.local()

    def __enter__(self):
        stack = self._saved.__dict__.setdefault("stack", [])
        stack.append(enabled())
        _state.on = self._want
        return self

    def __exit__(self, *exc):
        _state.on = self._saved.stack.pop()
        return False
