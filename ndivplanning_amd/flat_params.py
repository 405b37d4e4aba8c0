"""The flat vectors of a network of the forward-model family (include/ndp.h: forward model, image autoencoder) <->
its nn.Modules: one packer, described by the network's layout entry point, its two size entry points and the ordered
names of its layers and BatchNorms.  `resolve(name)` returns the module for a dotted name ("encoder.conv1")."""
import ctypes

import torch

from . import _capi


def to_kernel_layout(weight, rows, cols):
    """Conv2d [co][ci][kh][kw] / ConvTranspose2d [ci][co][kh][kw] -> [dim0 padded to rows][kh][kw][dim1 padded to cols]
    (include/ndp.h)."""
    w = weight.detach().float().permute(0, 2, 3, 1)
    out = torch.zeros(rows, w.shape[1], w.shape[2], cols, dtype=torch.float32, device=w.device)
    out[: w.shape[0], :, :, : w.shape[3]] = w
    return out


def from_kernel_layout(flat_w, rows, taps, cols, shape):
    """Inverse of to_kernel_layout: back to the module's weight shape."""
    k = int(round(taps ** 0.5))
    w = flat_w.view(rows, k, k, cols)[: shape[0], :, :, : shape[1]]
    return w.permute(0, 3, 1, 2).contiguous()


class FlatParams:
    def __init__(self, layout_fn, param_floats_fn, stat_floats_fn, layer_names, bn_names):
        self.layout_fn, self.param_floats_fn, self.stat_floats_fn = layout_fn, param_floats_fn, stat_floats_fn
        self.layer_names, self.bn_names = tuple(layer_names), tuple(bn_names)

    def layout(self, what, index):
        """(offset, dims[6]) of ndp_*_layout(what, index)."""
        lib = _capi.load()
        off, dims = ctypes.c_int64(), (ctypes.c_int64 * 6)()
        _capi.check(getattr(lib, self.layout_fn)(what, index, ctypes.byref(off), dims), self.layout_fn)
        return off.value, list(dims)

    def pack(self, resolve, device):
        """(params, running_stats): the flat vectors the kernels read."""
        lib = _capi.load()
        params = torch.zeros(getattr(lib, self.param_floats_fn)(), dtype=torch.float32, device=device)
        stats = torch.zeros(getattr(lib, self.stat_floats_fn)(), dtype=torch.float32, device=device)
        with torch.no_grad():
            for i, name in enumerate(self.layer_names):
                mod = resolve(name)
                off, d = self.layout(0, i)
                params[off:off + d[0] * d[1] * d[2]] = to_kernel_layout(mod.weight, d[0], d[2]).to(device).reshape(-1)
                boff, _ = self.layout(1, i)
                params[boff:boff + mod.bias.numel()] = mod.bias.detach().float().to(device)
            for i, name in enumerate(self.bn_names):
                bn = resolve(name)
                c = bn.weight.numel()
                params[self.layout(2, i)[0]:][:c] = bn.weight.detach().float().to(device)
                params[self.layout(3, i)[0]:][:c] = bn.bias.detach().float().to(device)
                stats[self.layout(4, i)[0]:][:c] = bn.running_mean.detach().float().to(device)
                stats[self.layout(5, i)[0]:][:c] = bn.running_var.detach().float().to(device)
        return params, stats

    def unpack_vector(self, vec, resolve):
        """'encoder.conv1.weight' ... -> tensor in the modules' own shapes, from a flat vector in the parameters' layout
        (parameters, gradients or Adam moments)."""
        out = {}
        for i, name in enumerate(self.layer_names):
            shape = tuple(resolve(name).weight.shape)
            off, d = self.layout(0, i)
            out[name + ".weight"] = from_kernel_layout(vec[off:off + d[0] * d[1] * d[2]], d[0], d[1], d[2], shape)
            boff, _ = self.layout(1, i)
            out[name + ".bias"] = vec[boff:boff + d[5]].clone()
        for i, name in enumerate(self.bn_names):
            off, d = self.layout(2, i)
            out[name + ".weight"] = vec[off:off + d[0]].clone()
            off, d = self.layout(3, i)
            out[name + ".bias"] = vec[off:off + d[0]].clone()
        return out

    def unpack_into(self, resolve, params, stats=None, batches_tracked=None):
        """Write the flat vectors back into the modules' parameters and buffers (after HIP training).  Only the listed
        layers and BatchNorms are touched."""
        with torch.no_grad():
            for key, value in self.unpack_vector(params, resolve).items():
                name, attr = key.rsplit(".", 1)
                getattr(resolve(name), attr).copy_(value)
            if stats is not None:
                for i, name in enumerate(self.bn_names):
                    bn = resolve(name)
                    c = bn.weight.numel()
                    bn.running_mean.copy_(stats[self.layout(4, i)[0]:][:c])
                    bn.running_var.copy_(stats[self.layout(5, i)[0]:][:c])
                    if batches_tracked is not None:
                        bn.num_batches_tracked.fill_(int(batches_tracked))


def module_at(root, dotted):
    """'encoder.conv1' -> root.encoder.conv1 (functools.partial(module_at, root) is a `resolve`)."""
    obj = root
    for part in dotted.split("."):
        obj = getattr(obj, part)
    return obj
