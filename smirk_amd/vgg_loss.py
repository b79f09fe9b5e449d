"""The perceptual term of the reference trainer's first path (smirk_trainer.py:104 `self.vgg_loss(reconstructed_img, img)`;
src/losses/VGGPerceptualLoss.py) on the MI355X.

    vgg = VGGPerceptualLoss(features).to(device)                       # features: torchvision's vgg16().features, or ten (weight, bias) pairs
    loss, terms, out = first_path(..., extra=lambda out: {'perceptual_vgg_loss': vgg(out['reconstructed_img'], batch['img'])})

loss(x, y), x and y [B, 3, H, W] in [-1, 1]: both go through v -> (0.5 v + 0.5 - mean) / std, a bilinear resize to 224 x 224 and the first ten
convolutions of VGG-16 (3 x 3, pad 1, bias, ReLU; 2 x 2 max-pools before the third, fifth and eighth); after convolutions 2, 4, 7 and 10 the mean of
|fx - fy| over the feature tensor is added.  The result is the unweighted sum of the four means.

The module keeps the reference's structure (`blocks`: four nn.Sequential holding Conv2d / ReLU / MaxPool2d under torchvision's indices, buffers `mean`
and `std`), so the reference's state dicts load; the layers themselves are never called.  The forward is ONE torch.autograd.Function: x and y are packed
into one split16 NHWC tensor [2B, H, W, 8] (csrc/vgg_loss.hip), the ten convolutions run on smirk_conv_igemm_f16x3 (shift = bias, fused ReLU) over the 2B
rows, each tap leaves float64 partial sums, and one finalise launch turns them into the four terms and their total.  The weights are frozen, so the
backward is data gradients only, over the x rows alone: tap / ReLU kernel, the same convolution entry with the rotated weights, the pool backward, and the
backward of the packing.  No launch waits for the host.  The packed weight images are the operands that frozen.FrozenNetwork caches (the rule is stated
there).  Arithmetic: f16x3 (fp32-class).
"""
import ctypes as C
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from .frozen import FrozenNetwork, image_pair, pack_conv
from .smirk_generator import split16_to_float

CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512)           # output channels of the ten convolutions
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)                      # their positions in torchvision's vgg16().features
BLOCK_SLICES = ((0, 4), (4, 9), (9, 16), (16, 23))                     # VGGPerceptualLoss.py:11-14
TAPS = (1, 3, 6, 9)                                                    # the convolutions (0-based) whose ReLU output enters the loss: the ends of the blocks
POOL_BEFORE = (2, 4, 7)                                                # the convolutions preceded by a 2 x 2 / 2 max-pool
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LIMIT_BYTES = 1 << 31                                                  # the convolution entries address an activation through 32-bit byte offsets


def _check_conv(m, cin, cout, where):
    if not isinstance(m, nn.Conv2d) or (m.in_channels, m.out_channels) != (cin, cout) or m.kernel_size != (3, 3) or m.stride != (1, 1) or \
            m.padding != (1, 1) or m.dilation != (1, 1) or m.groups != 1 or m.bias is None or m.padding_mode != "zeros":
        raise L.SmirkHipError(f"VGGPerceptualLoss: {where} must be Conv2d({cin}, {cout}, 3, padding=1) with a bias, got {m}")


def _blocks_from_pairs(pairs):
    pairs = list(pairs)
    if len(pairs) != len(CHANNELS):
        raise L.SmirkHipError(f"VGGPerceptualLoss: expected {len(CHANNELS)} (weight, bias) pairs, got {len(pairs)}")
    layers, cin = OrderedDict(), 3
    for k, ((w, b), cout) in enumerate(zip(pairs, CHANNELS)):
        if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
            raise L.SmirkHipError(f"VGGPerceptualLoss: pair {k}: expected weight {(cout, cin, 3, 3)} and bias {(cout,)}, got {tuple(w.shape)} and {tuple(b.shape)}")
        if k in POOL_BEFORE:
            layers[str(CONV_INDEX[k] - 1)] = nn.MaxPool2d(2, 2)
        conv = nn.Conv2d(cin, cout, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        layers[str(CONV_INDEX[k])] = conv
        layers[str(CONV_INDEX[k] + 1)] = nn.ReLU(inplace=True)
        cin = cout
    return [nn.Sequential(OrderedDict((k, m) for k, m in layers.items() if lo <= int(k) < hi)) for lo, hi in BLOCK_SLICES]


class _VGGLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, y, keep, trace):
        lib, st, dev = L.lib(), L.stream_ptr(), x.device
        B, _, H, W = x.shape
        P = L.ptr
        wf, wd, bias = module._operands(dev)
        xin = torch.empty(2 * B, H, W, 8, device=dev)
        L.check(lib.smirk_vgg_prepare_split16(P(x), P(y), P(module.mean), P(module.std), P(xin), B, H, W, st))
        sizes, h, w = [], H, W
        for k in TAPS:
            h, w = (h, w) if k == TAPS[0] else (h // 2, w // 2)
            sizes.append(B * h * w * CHANNELS[k])
        half = (C.c_longlong * len(TAPS))(*sizes)
        ws = module._ws.get(lib.smirk_vgg_l1_workspace_bytes(half, len(TAPS)), dev)
        wsp = C.c_void_p(ws.data_ptr())
        relu_x, tap_full, cur, h, w = [], [], xin, H, W
        if trace is not None:
            trace["relu_x"], trace["tap_y"] = [], []
        for k, cout in enumerate(CHANNELS):
            if k in POOL_BEFORE:
                pooled = torch.empty(2 * B, h // 2, w // 2, cur.shape[-1], device=dev)
                L.check(lib.smirk_maxpool2x2_split16(P(cur), P(pooled), 2 * B, h, w, cur.shape[-1], st))
                cur, h, w = pooled, h // 2, w // 2
            out = L.conv_launch(lib.smirk_conv_igemm_f16x3, L.conv_desc(2 * B, h, w, cur.shape[-1], cout, 3, relu=True), st, cur, wf[k], shift=bias[k])
            if k in TAPS:
                L.check(lib.smirk_vgg_l1_partials_split16(P(out), cout, TAPS.index(k), half, len(TAPS), wsp, ws.numel(), st))
            if keep:                                                     # the x rows of every ReLU output; of the y rows the four tap features only
                relu_x.append(out[:B] if k in TAPS else out[:B].clone())
                if k in TAPS:
                    tap_full.append(out)
            if trace is not None:
                trace["relu_x"].append(split16_to_float(out[:B]).permute(0, 3, 1, 2).contiguous())
                if k in TAPS:
                    trace["tap_y"].append(split16_to_float(out[B:]).permute(0, 3, 1, 2).contiguous())
            cur = out
        terms, total = torch.empty(len(TAPS), device=dev), torch.empty((), device=dev)
        L.check(lib.smirk_vgg_l1_finalise(half, len(TAPS), wsp, ws.numel(), P(terms), P(total), st))
        if trace is not None:
            trace["terms"] = terms
        # the backward is linear in the upstream gradient and 1 / numel(tap) is deep in fp16's subnormal range: the injected terms are lifted by a power of two
        # (the largest of them to [1, 2) times the upstream gradient) and the packing's backward divides it out again, both exactly
        scale = float(1 << (min(sizes) - 1).bit_length())
        ctx.tape = (module, relu_x, tap_full, wd, (B, H, W), scale) if keep else None
        ctx.kept = bool(keep)
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        if not ctx.kept:
            return None, None, None, None, None
        if ctx.tape is None:
            raise L.second_backward("VGGPerceptualLoss", "saved activations")
        module, relu_x, tap_full, wd, (B, H, W), scale = ctx.tape
        ctx.tape = None
        lib, st, dev = L.lib(), L.stream_ptr(), relu_x[0].device
        P = L.ptr
        g = L.as_f32c(g_total.detach())
        grad = None
        for k in range(len(CHANNELS) - 1, -1, -1):
            fx = relu_x[k]
            _, h, w, c = fx.shape
            fy = tap_full[TAPS.index(k)][B:] if k in TAPS else None
            dz = torch.empty_like(fx)
            L.check(lib.smirk_vgg_relu_tap_backward_split16(P(fx), P(fy, allow_none=True), P(grad, allow_none=True), P(g), P(dz), fx.numel(), c, scale, st))
            cin = wd[k].shape[0]
            grad = L.conv_launch(lib.smirk_conv_igemm_f16x3, L.conv_desc(B, h, w, c, cin, 3), st, dz, wd[k])
            if k in POOL_BEFORE:
                up = torch.empty_like(relu_x[k - 1])
                L.check(lib.smirk_maxpool2x2_backward_split16(P(relu_x[k - 1]), P(grad), None, P(up), B, 2 * h, 2 * w, cin, st))
                grad = up
        dx = torch.empty(B, 3, H, W, device=dev)
        L.check(lib.smirk_vgg_prepare_backward_split16(P(grad), P(module.std), P(dx), B, H, W, 1.0 / scale, st))
        return None, dx, None, None, None


class VGGPerceptualLoss(FrozenNetwork):
    """src/losses/VGGPerceptualLoss.py.  `features`: None (torchvision's pretrained vgg16, imported lazily, as the reference does), an nn.Sequential with
    torchvision's layout, or a list of ten (weight, bias) pairs.  `resize_to`: the size both images are resized to (the reference: 224 x 224); None runs the
    network at the input's own size.  The parameters are frozen like the reference's (:15-17)."""

    def __init__(self, features=None, resize_to=(224, 224)):
        super().__init__()
        if features is None:
            try:
                import torchvision
            except ImportError as e:
                raise ImportError("VGGPerceptualLoss(features=None) takes torchvision's pretrained vgg16 (src/losses/VGGPerceptualLoss.py:11-14) and torchvision "
                                  "is not installed; pass `features` (an nn.Sequential or ten (weight, bias) pairs) instead") from e
            features = torchvision.models.vgg16(weights="DEFAULT").features
        if isinstance(features, nn.Sequential):
            if len(features) < BLOCK_SLICES[-1][1]:
                raise L.SmirkHipError(f"VGGPerceptualLoss: `features` has {len(features)} layers, the loss reads the first {BLOCK_SLICES[-1][1]}")
            blocks = [features[lo:hi] for lo, hi in BLOCK_SLICES]       # (a slice of an nn.Sequential keeps the layers' names: torchvision's indices)
        else:
            blocks = _blocks_from_pairs(features)
        self.blocks = nn.ModuleList(blocks)
        cin = 3
        for idx, cout in zip(CONV_INDEX, CHANNELS):
            _check_conv(self._layer(idx), cin, cout, f"features[{idx}]")
            cin = cout
        for idx in (4, 9, 16):
            if not isinstance(self._layer(idx), nn.MaxPool2d):
                raise L.SmirkHipError(f"VGGPerceptualLoss: features[{idx}] must be MaxPool2d(2, 2), got {self._layer(idx)}")
        self.freeze()
        self.register_buffer("mean", torch.tensor(MEAN).view(1, 3, 1, 1))
        self.register_buffer("std", torch.tensor(STD).view(1, 3, 1, 1))
        self.resize_to = None if resize_to is None else (int(resize_to[0]), int(resize_to[1]))
        self._ws = L.Workspace()

    def _layer(self, idx):
        for (lo, hi), b in zip(BLOCK_SLICES, self.blocks):
            if lo <= idx < hi:
                return dict(b.named_children())[str(idx)]
        raise KeyError(idx)

    def convs(self):
        return [self._layer(i) for i in CONV_INDEX]

    def _build_operands(self, dev):
        """-> (wf, wd, bias): the split16 operand images of the ten weights, forward [Cout][(ky,kx,c)] and data-gradient [cin_pad][(ky,kx,co)], and the biases
        (live views of the parameters)"""
        packed = [pack_conv(c.weight.detach(), max(c.in_channels, 8), dgrad=True) for c in self.convs()]
        return [f for f, _ in packed], [d for _, d in packed], [c.bias.detach() for c in self.convs()]

    def forward(self, x, y, *, _trace=None):
        """x, y: [B, 3, H, W] fp32 on the HIP device -> the 0-dim fp32 loss, differentiable with respect to x.  `_trace` (a dict) receives the decoded fp32
        NCHW activations 'relu_x' (the ten ReLU outputs of the x rows) and 'tap_y' (the four tap features of the y rows), and the four 'terms'."""
        x, y = image_pair("VGGPerceptualLoss", ("x", "y"), x, y)
        if self.resize_to is not None and tuple(x.shape[2:]) != self.resize_to:
            # off the hot path (the trainer's images are 224 x 224): eager torch, differentiable.  The resize is a convex combination per pixel, so it commutes
            # with the per-channel affine map that the packing kernel applies afterwards.  Its outputs are fresh fp32 contiguous tensors: still conditioned.
            x = F.interpolate(x, mode="bilinear", size=self.resize_to, align_corners=False)
            y = F.interpolate(y, mode="bilinear", size=self.resize_to, align_corners=False)
        B, _, H, W = x.shape
        if B < 1 or H % 8 or W % 8 or H < 16 or W < 16:
            raise L.SmirkHipError(f"VGGPerceptualLoss: the network needs H and W to be multiples of 8 and at least 16 (three 2 x 2 pools), got {H} x {W}")
        if 2 * B * H * W * CHANNELS[0] * 4 >= LIMIT_BYTES:              # refused here, before the first launch
            raise L.SmirkHipError(f"VGGPerceptualLoss: the largest activation [2 x {B}, {H}, {W}, {CHANNELS[0]}] reaches 2 GiB, the limit of the convolution entries; "
                                  "split the batch")
        L.raise_if_range_tripped("VGGPerceptualLoss")
        keep = torch.is_grad_enabled() and x.requires_grad
        return _VGGLoss.apply(self, x, y, keep, _trace)[0]
