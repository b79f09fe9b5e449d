"""The perceptual loss of the trainer's first path (src/losses/VGGPerceptualLoss.py:23-47) in plain torch, in any dtype, with seeded synthetic weights, and
the FORCED law: the same computation with every discrete decision (ReLU on / off, pool winner, sign of fx - fy) taken from a trace instead of from its own
values.  The decisions of this network sit within fp32 rounding of their thresholds at every shape and seed (min |pre-activation| about 1e-6 .. 1e-5), so two
correct evaluations in different arithmetic flip a handful of them and their gradients differ by 1e-3 in relative L2 at 224 x 224.  With the decisions forced the
law is a linear map of the image, and a gradient is checked against it at rounding level: the adjoint of the very decisions the evaluation under test took."""
import math

import torch
import torch.nn.functional as F

CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512)
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)                      # torchvision vgg16().features
BLOCK_OF = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3)                              # VGGPerceptualLoss.py:11-14: features[:4], [4:9], [9:16], [16:23]
TAPS = (1, 3, 6, 9)
POOL_BEFORE = (2, 4, 7)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def state_dict_shapes():
    """the keys and shapes of the reference module's state dict"""
    out, cin = {"mean": (1, 3, 1, 1), "std": (1, 3, 1, 1)}, 3
    for idx, blk, c in zip(CONV_INDEX, BLOCK_OF, CHANNELS):
        out[f"blocks.{blk}.{idx}.weight"], out[f"blocks.{blk}.{idx}.bias"] = (c, cin, 3, 3), (c,)
        cin = c
    return out


def synth_weights(seed=0, device="cpu"):
    """He-initialised weights, biases 0.05 N(0, 1): every activation stays below 30 at the tested sizes"""
    g = torch.Generator().manual_seed(seed)
    pairs, cin = [], 3
    for c in CHANNELS:
        pairs.append(((torch.randn(c, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))).to(device), (0.05 * torch.randn(c, generator=g)).to(device)))
        cin = c
    return pairs


def synth_images(B, H, W, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(1000 + seed)
    return ((torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(device), (torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(device))


def _front(v, resize_to):
    mean, std = v.new_tensor(MEAN).view(1, 3, 1, 1), v.new_tensor(STD).view(1, 3, 1, 1)
    v = (v * 0.5 + 0.5 - mean) / std
    if resize_to is not None:
        v = F.interpolate(v, mode="bilinear", size=tuple(resize_to), align_corners=False)
    return v


def vgg_law(x, y, weights, resize_to=None, trace=None):
    """-> (total, [terms]) in x's dtype.  `trace` (a dict) receives 'relu_x' (ten) and 'tap_y' (four), detached."""
    dt = x.dtype
    fx, fy = _front(x, resize_to), _front(y.to(dt), resize_to)
    terms, rx, ty = [], [], []
    for k, (w, b) in enumerate(weights):
        if k in POOL_BEFORE:
            fx, fy = F.max_pool2d(fx, 2, 2), F.max_pool2d(fy, 2, 2)
        fx, fy = F.relu(F.conv2d(fx, w.to(dt), b.to(dt), padding=1)), F.relu(F.conv2d(fy, w.to(dt), b.to(dt), padding=1))
        rx.append(fx.detach())
        if k in TAPS:
            ty.append(fy.detach())
            terms.append((fx - fy).abs().mean())
    if trace is not None:
        trace["relu_x"], trace["tap_y"] = rx, ty
    return sum(terms), terms


def vgg_forced_law(x, weights, trace, resize_to=None):
    """The law with its decisions taken from `trace` (relu_x, tap_y: NCHW, any float dtype): ReLU = z * [trace.relu_x > 0]; a pool = a gather at the arg-max
    indices of max_pool2d(trace's pool input); a tap term = sum sign(trace.relu_x - trace.tap_y) * (fx - trace.tap_y) / numel.  Linear in x."""
    dt = x.dtype
    fx = _front(x, resize_to)
    total, t = 0.0, 0
    for k, (w, b) in enumerate(weights):
        if k in POOL_BEFORE:
            idx = F.max_pool2d(trace["relu_x"][k - 1], 2, 2, return_indices=True)[1]
            fx = fx.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
        fx = F.conv2d(fx, w.to(dt), b.to(dt), padding=1) * (trace["relu_x"][k] > 0).to(dt)
        if k in TAPS:
            ty = trace["tap_y"][t]
            total = total + (torch.sign(trace["relu_x"][k] - ty).to(dt) * (fx - ty.to(dt))).sum() / fx.numel()
            t += 1
    return total


def grad_of(fn, x):
    """-> (value, d value / d x) with x a fresh leaf"""
    x = x.detach().clone().requires_grad_(True)
    v = fn(x)
    v.backward()
    return v.detach(), x.grad
