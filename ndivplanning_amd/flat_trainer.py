"""What ForwardModelTrainer (forward_trainer.py) and AutoencoderTrainer (autoencoder_trainer.py) share: one flat parameter
vector that the kernels read, its gradient, Adam moments and running BatchNorm statistics on one GPU, the checks of what
a step is given, the cross-rank BatchNorm statistics of a data-parallel driver (`sync_batchnorm_world` > 1: a callback
passed with every *_train_grads_dp call, never installed anywhere), and the reduce-then-apply tail of a step."""
import ctypes

import torch

from . import _capi


class FlatTrainer:
    """A subclass names its entry points, packs its modules, and calls its own `grads()`."""
    _WORKSPACE_FN = _APPLY_FN = _PACK_FN = None          # "ndp_fm_workspace_floats", "ndp_fm_apply_adam", "ndp_fm_pack_params"
    _grad_buckets = None                                 # _capi.fm_grad_buckets

    def _place(self, modules, where, batch, reduce_fn, bucket_reduce):
        """The library, the one GPU all `modules` are on (`where` words the refusal), the largest batch and the gradient
        exchange of a data-parallel driver (at most one of the two)."""
        self.lib = _capi.load()
        devices = [next(m.parameters()).device for m in modules]
        if devices[0].type != "cuda" or any(d != devices[0] for d in devices):
            raise _capi.NdpError("%s needs %s ROCm GPU (got %s); there is no CPU path"
                                 % (type(self).__name__, where, ", ".join(str(d) for d in devices)))
        self.device, self.batch = devices[0], int(batch)
        if reduce_fn is not None and bucket_reduce is not None:
            raise ValueError("give either reduce_fn (one collective) or bucket_reduce (per-bucket, overlapped)")
        self.reduce_fn, self.bucket_reduce = reduce_fn, bucket_reduce

    def _allocate(self, packed, lr, betas, eps, sync_batchnorm_world=1, stat_group=None):
        """Buffers of a trainer on self.device for at most self.batch images; packed: (params, running_stats).
        sync_batchnorm_world > 1: BatchNorm statistics summed over that many ranks (`stat_group`: their process group)."""
        self.sync_world = int(sync_batchnorm_world)
        if self.sync_world < 1:
            raise ValueError("sync_batchnorm_world must be >= 1, got %r" % (sync_batchnorm_world,))
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params, self.stats = packed
        self.grad = torch.zeros_like(self.params)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.step_word = torch.zeros(4, dtype=torch.int32, device=self.device)      # Adam state word (include/ndp.h)
        self.loss = torch.zeros(1, **f32)
        self.loss_sum = torch.zeros(1, **f32)
        self.workspace = torch.empty(getattr(self.lib, self._WORKSPACE_FN)(self.batch), **f32)
        self.steps = 0                                                               # Adam steps
        # cross-rank statistics: the callback and the ctypes thunk the library calls, alive until close()
        self.stat_sync, self._stat_cb = None, None
        if self.sync_world > 1:
            from . import dp
            self.stat_sync = dp.StatAllReduce(self.workspace, group=stat_group)
            self._stat_cb = _capi.STAT_SYNC_FN(self.stat_sync)

    def _stat_args(self):
        """(stat_sync, stat_ctx, world): the last three arguments of this trainer's *_train_grads_dp call."""
        if self.sync_world > 1 and self._stat_cb is None:
            raise _capi.NdpError("%s: closed (its cross-rank statistics callback is released)" % type(self).__name__)
        return ctypes.cast(self._stat_cb, ctypes.c_void_p) if self._stat_cb is not None else None, None, self.sync_world

    def _stat_check(self):
        """After a pass: re-raise what a statistics callback raised inside it."""
        if self.stat_sync is not None:
            self.stat_sync.check()

    def close(self):
        """Release the cross-rank statistics callback (if any); a closed data-parallel trainer refuses grads()."""
        self.stat_sync, self._stat_cb = None, None

    def _pack(self, workspace=None):
        """The second weight order the kernels read, rebuilt from .params in the head of a workspace (.workspace)."""
        workspace = self.workspace if workspace is None else workspace
        with torch.cuda.device(self.device):
            _capi.check(getattr(self.lib, self._PACK_FN)(_capi.ptr(self.params), _capi.ptr(workspace),
                                                         _capi.stream_ptr(self.device)), self._PACK_FN)

    def _check_batch(self, n, of="images"):
        if not 1 <= n <= self.batch:
            raise _capi.NdpError("batch of %d %s with a trainer built for at most %d" % (n, of, self.batch))

    def _check(self, t, shape, what, dtype=torch.float32):
        if t.device != self.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise _capi.NdpError("%s: expected a contiguous %s %s tensor on %s, got %s %s on %s"
                                 % (what, dtype, list(shape), self.device, t.dtype, list(t.shape), t.device))

    def apply(self):
        """optimizer.step()"""
        p = _capi.ptr
        with torch.cuda.device(self.device):
            _capi.check(getattr(self.lib, self._APPLY_FN)(p(self.params), p(self.grad), p(self.exp_avg), p(self.exp_avg_sq),
                                                          p(self.step_word), self.lr, self.betas[0], self.betas[1], self.eps,
                                                          p(self.workspace), _capi.stream_ptr(self.device)), self._APPLY_FN)
        self.steps += 1

    def _reduce_and_apply(self):
        """The rest of a step after grads(): the data-parallel reduction of the gradient (if any), then Adam."""
        if self.bucket_reduce is not None:
            self.bucket_reduce(self.grad, self.device)
        elif self.reduce_fn is not None:
            self.reduce_fn(self.grad)
        self.apply()
        return self.loss

    def gradient_buckets(self):
        """[(offset, count)] of the flat gradient, in the order the backward pass completes them."""
        return self._grad_buckets()

    def named_gradients(self):
        """'encoder.conv1.weight' ... -> gradient in the modules' own tensor shapes (tests, inspection)."""
        return self._unpack(self.grad)

    def named_parameters(self):
        return self._unpack(self.params)
