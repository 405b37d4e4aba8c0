"""One iteration of the reference's autoencoder training loop (train_autoencoder.py:79-90) as gfx950 kernels:

    z = encoder(state_cur); state_cur_hat = decoder(z)              ->  ndp_ae_train_grads   (forward, training-mode
    recon_loss = mse(state_cur_hat, state_cur)                            BatchNorm, MSE, backward: every gradient)
    optimizer.zero_grad(); recon_loss.backward()
    optimizer.step()                                                 ->  ndp_ae_apply_adam

The trainer owns the flat parameter vector the kernels read (include/ndp.h: image autoencoder), its gradient, the Adam
moments (one Adam over both modules, as the reference's two parameter groups with the same settings) and the running
BatchNorm statistics; `sync_to_modules()` writes them back into the `Encoder` and `Decoder` (the reference saves the whole
modules: train_autoencoder.py:92-97).  There is no CPU path.

Data parallel (one rank's share of a global batch), as ForwardModelTrainer: `reduce_fn(grad)` all-reduces the gradient
between the two library calls, or `bucket_reduce` (dp.BucketedMeanAllReduce over ndp_ae_grad_buckets /
ndp_ae_bucket_wait) does it per gradient bucket beside the rest of the backward pass; `sync_batchnorm_world` > 1 sums
the BatchNorm statistics over the ranks (`stat_group`: their process group) through a callback passed with every
ndp_ae_train_grads_dp call (FlatTrainer owns it), so that W ranks with B / W images each train the step of one process
with B images."""
import torch

from . import _capi
from .flat_trainer import FlatTrainer
from .models import image_autoencoder as IA


class AutoencoderTrainer(FlatTrainer):
    _WORKSPACE_FN, _APPLY_FN, _PACK_FN = "ndp_ae_workspace_floats", "ndp_ae_apply_adam", "ndp_ae_pack_params"
    _grad_buckets = staticmethod(_capi.ae_grad_buckets)

    def __init__(self, encoder: IA.Encoder, decoder: IA.Decoder, batch: int, lr: float = 2e-4, betas=(0.5, 0.999),
                 eps: float = 1e-8, keep_reconstruction: bool = False, reduce_fn=None, bucket_reduce=None,
                 sync_batchnorm_world: int = 1, stat_group=None):
        self.encoder, self.decoder = encoder, decoder
        self._place([encoder, decoder], "both modules on one", batch, reduce_fn, bucket_reduce)
        dev = self.device
        if self.batch < 1 or self.lib.ndp_ae_workspace_floats(self.batch) <= 0:
            raise _capi.NdpError("AutoencoderTrainer: unsupported batch of %d images" % self.batch)
        self._allocate(IA.pack_autoencoder(encoder, decoder, dev), lr, betas, eps, sync_batchnorm_world, stat_group)
        self.recon = torch.zeros(self.batch, 3, 128, 128, dtype=torch.float32, device=dev) if keep_reconstruction else None
        self.forwards = 0                                                    # training-mode forwards (num_batches_tracked)
        self._batches0 = int(encoder.conv1_bn.num_batches_tracked.item())
        self._pack()

    def grads(self, images):
        """forward + loss + backward on images [n,3,128,128] (n <= batch): fills .grad, .loss (device scalar, the
        reference's `recon_loss`), adds it to .loss_sum, moves the running statistics."""
        n = int(images.shape[0]) if images.dim() == 4 else 0
        self._check_batch(n)
        self._check(images, (n, 3, 128, 128), "images")
        p = _capi.ptr
        recon = p(self.recon) if self.recon is not None else None
        with torch.cuda.device(self.device):
            if self.sync_world == 1 and self.bucket_reduce is None:
                _capi.check(self.lib.ndp_ae_train_grads(p(self.params), p(self.stats), p(images), n, p(self.grad),
                                                        p(self.loss), p(self.loss_sum), recon, p(self.workspace),
                                                        _capi.stream_ptr(self.device)), "ndp_ae_train_grads")
            else:
                _capi.check(self.lib.ndp_ae_train_grads_dp(p(self.params), p(self.stats), p(images), n, p(self.grad),
                                                           p(self.loss), p(self.loss_sum), recon, p(self.workspace),
                                                           _capi.stream_ptr(self.device), *self._stat_args()),
                            "ndp_ae_train_grads_dp")
        self._stat_check()
        self.forwards += 1
        return self.loss

    def step(self, images):
        """The loop body of train_autoencoder.py:79-90 for one image batch; returns the loss (device scalar: this rank's,
        the mean over its own images)."""
        self.grads(images)
        return self._reduce_and_apply()

    def load_from_modules(self):
        """Take parameters and running statistics from the modules again (after they were changed from outside)."""
        self.params, self.stats = IA.pack_autoencoder(self.encoder, self.decoder, self.device)
        self._batches0 = int(self.encoder.conv1_bn.num_batches_tracked.item())
        self.forwards = 0
        self._pack()

    def sync_to_modules(self):
        IA.unpack_into_autoencoder(self.encoder, self.decoder, self.params, self.stats,
                                   batches_tracked=self._batches0 + self.forwards)
        return self.encoder, self.decoder

    # post-ReLU maps of the last grads() call (tests, inspection): name -> (workspace tensor index, side, channels)
    _MAPS = {"feat1": (2, 64, 64), "feat2": (4, 32, 128), "feat3": (6, 16, 256), "feat4": (7, 8, 512), "feat5": (8, 4, 1024),
             "up1": (11, 4, 1024), "up2": (13, 8, 512), "up3": (15, 16, 256), "up4": (17, 32, 128), "up5": (19, 64, 64)}

    def activation(self, name, n):
        """Post-ReLU map `name` (feat1..5, up1..5) of the last call on n images, NCHW."""
        idx, side, ch = self._MAPS[name]
        off = self.lib.ndp_ae_workspace_offset(n, idx)
        return self.workspace[off:off + n * side * side * ch].view(n, side, side, ch).permute(0, 3, 1, 2).contiguous()

    def _unpack(self, vec):
        return IA.unpack_autoencoder_vector(vec, self.encoder, self.decoder)
