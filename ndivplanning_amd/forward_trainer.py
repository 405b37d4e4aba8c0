"""One iteration of the reference's forward-model training loop (train_forward_model.py:98-112) as gfx950 kernels:

    state_fut_resid_hat = forward_autoencoder(state_cur, action)      ->  ndp_fm_train_grads_dp (forward, training-mode
    loss = mse(state_fut_resid_hat, state_fut - state_cur)                BatchNorm, MSE, backward: every gradient)
    optimizer.zero_grad(); loss.backward()
    optimizer.step()                                                   ->  ndp_fm_apply_adam

The trainer owns the flat parameter vector the kernels read (include/ndp.h: forward model), its gradient, Adam moments
and the running BatchNorm statistics; `sync_to_module()` writes them back into the `ForwardAutoencoder` (the reference
saves the whole module: train_forward_model.py:157-163).  `reduce_fn(grad)` -- when given, called between the two
library calls -- is where a data-parallel driver all-reduces the gradient ("same DP recipe";
the loss is a mean over the local batch, so the driver averages).  `bucket_reduce` (dp.BucketedMeanAllReduce) does the
same per gradient bucket on a communication stream, each bucket as soon as the backward pass has completed it
(ndp_fm_grad_buckets / ndp_fm_bucket_wait): the all-reduce runs beside the rest of the backward pass.
`sync_batchnorm_world` > 1 sums the BatchNorm statistics over the ranks (`stat_group`: their process group) through a
callback passed with every ndp_fm_train_grads_dp call (FlatTrainer), so that W ranks with B / W images each train the
step of one process with B images; `close()` releases the callback.

`rollout_steps=H` > 1 adds `grads_rollout` / `step_rollout`: the model is unrolled H steps on its
own predictions over a window of H + 1 frames and trained on the mean of the H step losses through every path
(backpropagation through time), one Adam step per window.  Each pass keeps its activations in a workspace of its own."""
import torch

from . import _capi
from .flat_trainer import FlatTrainer
from .models import forward_encoder as FE


class ForwardModelTrainer(FlatTrainer):
    _WORKSPACE_FN, _APPLY_FN, _PACK_FN = "ndp_fm_workspace_floats", "ndp_fm_apply_adam", "ndp_fm_pack_params"
    _grad_buckets = staticmethod(_capi.fm_grad_buckets)

    def __init__(self, model: FE.ForwardAutoencoder, batch: int, lr: float = 2e-4, betas=(0.5, 0.999), eps: float = 1e-8,
                 reduce_fn=None, keep_residual: bool = False, bucket_reduce=None, sync_batchnorm_world: int = 1,
                 rollout_steps: int = 1, stat_group=None):
        self.rollout_steps = int(rollout_steps)
        if self.rollout_steps < 1:
            raise ValueError("rollout_steps must be >= 1, got %r" % (rollout_steps,))
        if self.rollout_steps > 1 and (bucket_reduce is not None or int(sync_batchnorm_world) > 1):
            # the bucket events are those of the most recent backward pass (one pass per iteration), and the entry points
            # a rollout is made of (ndp_fm_forward, ndp_fm_backward_inputs) take no statistics function
            raise ValueError("rollout_steps > 1 works with reduce_fn only: not with bucket_reduce or cross-rank BatchNorm")
        self.model = model
        self._place([model], "the model on a", batch, reduce_fn, bucket_reduce)
        self._allocate(FE.pack_module(model, self.device), lr, betas, eps, sync_batchnorm_world, stat_group)
        self.resid = torch.zeros(self.batch, 3, 128, 128, dtype=torch.float32, device=self.device) if keep_residual else None
        self.forwards = 0                                            # training-mode forwards (num_batches_tracked)
        self._batches0 = int(model.encoder.conv1_bn.num_batches_tracked.item())
        self._pack()
        self._workspaces = [self.workspace]                          # pass k of a rollout keeps its activations in [k]
        self._extra_stale = False                                    # the extra workspaces' second weight order is behind
        self.rollout_losses = None
        if self.rollout_steps > 1:
            self._allocate_rollout()

    def _allocate_rollout(self):
        """What H > 1 passes alive at once need, allocated once: a workspace, a gradient vector and a state per pass."""
        H, f32 = self.rollout_steps, dict(dtype=torch.float32, device=self.device)
        values = self.batch * 3 * 128 * 128
        self._workspaces += [torch.empty(self.workspace.numel(), **f32) for _ in range(H - 1)]
        self._grad_stride = (self.params.numel() + 3) // 4 * 4
        self._step_grads = torch.zeros(H, self._grad_stride, **f32)  # grad_k of pass k; their sum in pass order is .grad
        self._states = torch.zeros(H + 1, values, **f32)             # s_0 .. s_H
        self._locals = torch.zeros(H, values, **f32)                 # [j - 1]: local_j, then G_j in place
        self._resid = torch.zeros(values, **f32)
        self._dcur = torch.zeros(values, **f32)
        self.rollout_losses = torch.zeros(H, **f32)                  # loss_0 .. loss_{H-1} of the last window
        self._pack_extra_workspaces()

    def _pack_extra_workspaces(self):
        """The second weight order lives in each workspace's head; ndp_fm_apply_adam rebuilds it in .workspace only.  The
        others are rebuilt here, by the next grads_rollout after the parameters changed: one-pair steps pay nothing."""
        self._extra_stale = False
        for ws in self._workspaces[1:]:
            self._pack(ws)

    def apply(self):
        """optimizer.step()"""
        super().apply()
        self._extra_stale = True

    def grads(self, state_cur, state_fut, actions):
        """forward + loss + backward: fills .grad, .loss (device scalar, the reference's `loss`), adds it to .loss_sum.
        Frames: the reference's float tensors [n,3,128,128] in [-1,1], or decoded camera frames as bytes [n,128,128,3]
        (normalised by the kernels as they read them: utils/hdf5_load.py:9-11's formula, a quarter of the upload)."""
        n = int(state_cur.shape[0])
        self._check_batch(n)
        u8 = state_cur.dtype == torch.uint8
        shape = (n, 128, 128, 3) if u8 else (n, 3, 128, 128)
        self._check(state_cur, shape, "state_cur", state_cur.dtype if u8 else torch.float32)
        self._check(state_fut, shape, "state_fut", torch.uint8 if u8 else torch.float32)
        self._check(actions, (n, 4), "actions")
        p = _capi.ptr
        with torch.cuda.device(self.device):
            _capi.check(self.lib.ndp_fm_train_grads_dp(
                p(self.params), p(self.stats), p(state_cur), p(state_fut), int(u8), p(actions), n, p(self.grad), p(self.loss),
                p(self.loss_sum), p(self.resid) if self.resid is not None else None, p(self.workspace),
                _capi.stream_ptr(self.device), *self._stat_args()), "ndp_fm_train_grads_dp")
        self._stat_check()
        self.forwards += 1
        return self.loss

    def step(self, state_cur, state_fut, actions):
        """The loop body of train_forward_model.py:98-112 for one frame pair; returns the loss (device scalar)."""
        self.grads(state_cur, state_fut, actions)
        return self._reduce_and_apply()

    def grads_rollout(self, frames, actions):
        """forward + loss + backward over a window: frames [n,H+1,3,128,128] float (or [n,H+1,128,128,3] bytes), actions
        [n,H,4]; n <= batch.  Fills .grad (d L / d params through every path), .loss (L, the mean of the H step losses),
        .rollout_losses [H]; adds L to .loss_sum.  The windows of a longer trajectory tensor may be passed as slices along
        the time axis (frames[:, i:i + H + 1]): only the image stride differs.  No host synchronisation."""
        H = self.rollout_steps
        if H == 1:
            return self.grads(frames[:, 0].contiguous(), frames[:, 1].contiguous(), actions[:, 0].contiguous())
        n = int(frames.shape[0])
        self._check_batch(n, "trajectories")
        u8 = frames.dtype == torch.uint8
        shape = (n, H + 1, 128, 128, 3) if u8 else (n, H + 1, 3, 128, 128)
        inner = torch.empty(shape[1:], device="meta").stride()
        if frames.device != self.device or (not u8 and frames.dtype != torch.float32) or tuple(frames.shape) != shape:
            raise _capi.NdpError("frames: expected a float32 %s (or uint8 [n,%d,128,128,3]) tensor on %s, got %s %s on %s"
                                 % (list(shape), H + 1, self.device, frames.dtype, list(frames.shape), frames.device))
        if tuple(frames.stride()[1:]) != tuple(inner):
            raise _capi.NdpError("frames: the %d frames of a trajectory must be contiguous (strides %s), got strides %s"
                                 % (H + 1, list(inner), list(frames.stride()[1:])))
        if n > 1 and (frames.stride(0) < inner[0] * (H + 1) or frames.stride(0) % 4 != 0):
            raise _capi.NdpError("frames: the stride along the batch axis must be at least one window (%d elements, no "
                                 "overlap) and a multiple of 4, got %d" % (inner[0] * (H + 1), frames.stride(0)))
        if actions.device != self.device or actions.dtype != torch.float32 or tuple(actions.shape) != (n, H, 4):
            raise _capi.NdpError("actions: expected a float32 %s tensor on %s, got %s %s on %s"
                                 % ([n, H, 4], self.device, actions.dtype, list(actions.shape), actions.device))
        if self._extra_stale:
            self._pack_extra_workspaces()
        acts = actions.transpose(0, 1).contiguous()                  # [H,n,4]: pass k reads its actions as one block
        stride, image = int(frames.stride(0)) if n > 1 else inner[0] * (H + 1), 3 * 128 * 128 * frames.element_size()
        p, lib, c = _capi.ptr, self.lib, _capi.check
        frame = lambda k: _capi.c_void_p(frames.data_ptr() + k * image)      # noqa: E731  (frame k of every trajectory)
        with torch.cuda.device(self.device):
            st = _capi.stream_ptr(self.device)
            c(lib.ndp_fm_rollout_begin(frame(0), int(u8), stride, n, p(self._states[0]), st), "ndp_fm_rollout_begin")
            for k in range(H):
                c(lib.ndp_fm_forward(p(self.params), p(self.stats), p(self._states[k]), p(acts[k]), n, 1, p(self._resid),
                                     p(self._workspaces[k]), st), "ndp_fm_forward")
                c(lib.ndp_fm_rollout_advance(p(self._states[k]), p(self._resid), frame(k + 1), int(u8), stride, n, k, H,
                                             p(self._states[k + 1]), p(self._locals[k]), p(self.rollout_losses), p(self.loss),
                                             p(self.loss_sum), p(self._workspaces[k]), st), "ndp_fm_rollout_advance")
            for k in range(H - 1, -1, -1):                           # _locals[k] holds G_{k+1} = d L / d r_k
                c(lib.ndp_fm_backward_inputs(p(self.params), p(self._locals[k]), n, p(self._step_grads[k]),
                                             p(self._dcur) if k >= 1 else None, None, p(self._workspaces[k]), st),
                  "ndp_fm_backward_inputs")
                if k >= 1:                                           # G_k = (local_k + G_{k+1}) + dcur_k, in local_k's place
                    c(lib.ndp_fm_rollout_chain(p(self._locals[k - 1]), p(self._locals[k]), p(self._dcur), n,
                                               p(self._locals[k - 1]), st), "ndp_fm_rollout_chain")
            c(lib.ndp_fm_grad_sum(p(self._step_grads), self._grad_stride, H, self.params.numel(), p(self.grad), st),
              "ndp_fm_grad_sum")
        self.forwards += H                                           # every pass of the window moved the statistics
        return self.loss

    def step_rollout(self, frames, actions):
        """One optimiser step on a window (grads_rollout, the reduction if any, Adam); returns L (device scalar)."""
        if self.rollout_steps == 1:
            return self.step(frames[:, 0].contiguous(), frames[:, 1].contiguous(), actions[:, 0].contiguous())
        self.grads_rollout(frames, actions)
        return self._reduce_and_apply()

    # intermediate maps of the last grads() call (tests, inspection): name -> (workspace tensor index, side, channels kept)
    _MAPS = {"feat1": (1, 64, 128, 64, 128), "up5": (1, 64, 128, 0, 64), "feat2": (2, 32, 256, 128, 256), "up4": (2, 32, 256, 0, 128),
             "feat3": (3, 16, 512, 256, 512), "up3": (3, 16, 512, 0, 256), "feat4": (4, 8, 1024, 512, 1024),
             "up2": (4, 8, 1024, 0, 512), "feat5": (5, 4, 2048, 1024, 2048), "up1": (5, 4, 2048, 0, 1024),
             "up6": (16, 128, 32, 0, 32), "r1": (18, 128, 16, 0, 16)}

    def activation(self, name, n, step=0):
        """Post-ReLU map `name` (feat1..5, up1..6, r1) of the last call on n images, NCHW; step: the pass of a rollout."""
        idx, side, ld, c0, c1 = self._MAPS[name]
        off = self.lib.ndp_fm_workspace_offset(n, idx)
        view = self._workspaces[step][off:off + n * side * side * ld].view(n, side, side, ld)
        return view[..., c0:c1].permute(0, 3, 1, 2).contiguous()

    def load_from_module(self):
        """Take parameters and running statistics from the module again (after they were changed from outside)."""
        self.params, self.stats = FE.pack_module(self.model, self.device)
        self._batches0 = int(self.model.encoder.conv1_bn.num_batches_tracked.item())
        self.forwards = 0
        self._pack()
        self._extra_stale = True

    def sync_to_module(self):
        """num_batches_tracked counts training-mode forwards as torch's BatchNorm does (a window of H passes counts H, a
        grads() without apply() counts), on top of what the module held when it was packed; .steps counts Adam steps."""
        FE.unpack_into_module(self.model, self.params, self.stats, batches_tracked=self._batches0 + self.forwards)
        return self.model

    def _unpack(self, vec):
        return FE.unpack_vector(vec, self.model)
