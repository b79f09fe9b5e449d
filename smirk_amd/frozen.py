"""The host-side frame of a frozen reference network on the HIP path: VGGPerceptualLoss, ExpressionLoss and MICA (and the next frozen term to be ported).

A frozen network is an nn.Module tree in the reference's layout (so the reference's state dicts load) whose layers hold the parameters and are never called;
the arithmetic is libsmirk_hip.so's, on operands derived from the parameters once: packed split16 weight images, BatchNorm folded into scales and shifts.
FrozenNetwork owns the rules around that; a network supplies `_build_operands(dev)` and its schedule of launches.

The operand cache.  The operands are cached under (device, (data_ptr, _version) of every parameter and buffer the arithmetic reads): a re-allocation moves
data_ptr, an in-place update moves torch's version counter, and .to() / load_state_dict drop the cache outright.  A hit costs that key and nothing else (no
device query, no host wait).  A miss checks that every tensor read is a contiguous fp32 tensor on the images' device, so images on another device than the
parameters are refused on every call, and then builds ALL operands again (a build may read the parameters on the host: it is the only step that may wait).
"""
import os

import torch
import torch.nn as nn

from . import _lib as L


class Holder(nn.Module):
    """A container of parameters in the reference's layout.  It is never called: the arithmetic is libsmirk_hip.so's.  `owner`: the public module to call."""
    owner = "FrozenNetwork"

    def forward(self, *a, **k):
        raise L.SmirkHipError(f"{type(self).__name__} holds the parameters of smirk_amd.{self.owner} and has no forward of its own (no eager fallback exists): "
                              f"call {self.owner}")


# ---- host-side folding (plain torch, float64: runs without a device) ---------------------------------------------------------------------------------------
def host64(t):
    return t.detach().cpu().double()


def bn_affine(bn):
    """BatchNorm in eval mode as y = x * s + t, float64 on the host."""
    s = host64(bn.weight) / torch.sqrt(host64(bn.running_var) + bn.eps)
    return s, host64(bn.bias) - host64(bn.running_mean) * s


def read_checkpoint(checkpoint, default, who, hint, **load_kwargs):
    """-> the checkpoint dict: `checkpoint` itself if it is one, else torch.load of that path on the host; None reads `default`, relative to the working
    directory like the reference.  `hint`: the entries a dict must have, for the error text."""
    if checkpoint is None:
        checkpoint = default
    if isinstance(checkpoint, dict):
        return checkpoint
    path = os.fspath(checkpoint)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{who}: `checkpoint` = {path!r} does not exist (the default is {default!r} relative to the working directory, as in the "
                                f"reference; pass a path or a dict with {hint})")
    return torch.load(path, map_location="cpu", **load_kwargs)


def pack_conv(w, cin_pad, fwd=True, dgrad=False, dgrad_from=None):
    """-> (forward image [Cout][(ky, kx, c)] or None, data-gradient image [cin_pad][(ky, kx, co)] or None): the split16 operand images of the convolution
    weight `w` [Cout, Cin, k, k] on its device, c padded to `cin_pad`.  `dgrad_from` (a copy of `w` with the scale behind the convolution folded in) asks for the
    data-gradient image as well and is what it is packed from, in a launch of its own."""
    lib, st, (cout, cin, k) = L.lib(), L.stream_ptr(), w.shape[:3]
    f = torch.empty(cout, k * k * cin_pad, device=w.device) if fwd else None
    d = torch.empty(cin_pad, k * k * cout, device=w.device) if dgrad or dgrad_from is not None else None
    if dgrad_from is None:
        L.check(lib.smirk_pack_conv_weights_split16(L.ptr(w), cout, cin, 0, cin, k, cin_pad, L.ptr(f, allow_none=True), L.ptr(d, allow_none=True), st))
    else:
        if fwd:
            L.check(lib.smirk_pack_conv_weights_split16(L.ptr(w), cout, cin, 0, cin, k, cin_pad, L.ptr(f), None, st))
        L.check(lib.smirk_pack_conv_weights_split16(L.ptr(dgrad_from), cout, cin, 0, cin, k, cin_pad, None, L.ptr(d), st))
    return f, d


# ---- input conditioning ------------------------------------------------------------------------------------------------------------------------------------
def _refuse_image(who, name, t):
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3:
        raise L.SmirkHipError(f"{who}: {name} must be a [B, 3, H, W] tensor")
    if not t.is_cuda:
        raise L.SmirkHipError(f"smirk_amd runs on the MI355X HIP device only: {who}: {name} is a CPU tensor (no CPU fallback exists)")


def device_image(who, name, t):
    """The one image of a forward-only network: refused unless a [B, 3, H, W] tensor on the device; -> it detached, fp32, contiguous, 16-byte aligned."""
    _refuse_image(who, name, t)
    return L.aligned16(t.detach())


def image_pair(who, names, a, b):
    """The two images of a loss, differentiable with respect to the first: both as in device_image, of one shape on one device, the second a constant.
    -> (a, b detached), both fp32, contiguous, 16-byte aligned."""
    for name, t in zip(names, (a, b)):
        _refuse_image(who, name, t)
    if tuple(a.shape) != tuple(b.shape) or a.device != b.device:
        raise L.SmirkHipError(f"{who}: {names[0]} {tuple(a.shape)} and {names[1]} {tuple(b.shape)} must have one shape and one device")
    if b.requires_grad:
        raise L.SmirkHipError(f"{who}: {names[1]} requires grad; the second image is the constant of the loss (the trainer passes the input image there)")
    return L.aligned16(a), L.aligned16(b.detach())


class FrozenNetwork(nn.Module):
    """Base of a frozen network (the module docstring).  A subclass builds its layers, calls freeze() and defines `_build_operands(dev)`; its forward takes
    `self._operands(device of the images)`."""
    pin_eval = False                                                   # True: train() is pinned to eval (a network with BatchNorm: ALWAYS the running statistics)

    def __init__(self):
        super().__init__()
        self._tensors = None                                           # every parameter and buffer the arithmetic reads (listed again after .to() / load_state_dict)
        self._packed = None                                            # (key, operands)

    def freeze(self):
        for p in self.parameters():
            p.requires_grad = False
        return self.train(False) if self.pin_eval else self

    def train(self, mode=True):
        return super().train(mode and not self.pin_eval)

    def _apply(self, fn, *a, **k):
        self._tensors = self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._tensors = self._packed = None
        return super().load_state_dict(*a, **k)

    def _reads(self, name):
        """whether the arithmetic reads the parameter or buffer `name`"""
        return not name.endswith("num_batches_tracked")

    def _operands(self, dev):
        if self._tensors is None:
            self._tensors = [t for n, t in list(self.named_parameters()) + list(self.named_buffers()) if self._reads(n)]
        key = (dev, L.version_key(self._tensors))
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        for t in self._tensors:
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise L.SmirkHipError(f"{type(self).__name__}: the parameters and buffers must be contiguous fp32 tensors on the images' device (call .to(device))")
        # A rebuild always allocates fresh buffers and never writes into the old images, because an earlier forward's tape may still hold them.
        ops = self._build_operands(dev)
        self._packed = (key, ops)
        return ops
