"""The law of the emotion term for the tests of smirk_amd.expression_loss: a float64 restatement of src/losses/ExpressionLoss.py and src/losses/resnet.py
(resnet50(num_classes=100, include_top=False, emoca_specific=True)) written from the architecture, sharing no code with the reference and none with
smirk_amd/expression_loss.py, evaluated functionally on a checkpoint in the reference's format; the gradient is torch's autograd over it.

    x = maxpool(relu(bn1(conv1(img))))                                    7 x 7, stride 2, pad 3, no bias; BatchNorm in eval mode, eps 1e-5; 3 x 3, stride 2, pad 1
    per block:  y = relu(bn1(conv1(x)))                                   1 x 1
                y = relu(bn2(conv2(y)))                                   3 x 3, pad 1, stride 2 on the first block of layers 2 - 4
                x = relu(bn3(conv3(y)) + (x, or downsample.1(downsample.0(x)) on the first block of a layer))      downsample.0: 1 x 1 of conv2's stride
    f = avgpool7(x) as [B, 2048]
    loss_b = mean_c (g - t)^2 ('l2'), mean_c |g - t| ('l1'), 1 - F.cosine_similarity(g, t, dim=1) ('cos'); with use_mean its mean over the batch

`trace` receives (name, max |activation|) per layer.  `variant` makes one deliberate mistake (tests/test_expression_loss_cpu.py shows that the GPU bounds see each):
'stride_on_conv1' (the switch emoca_specific turns off), 'pool_ceil' (MaxPool2d(3, 2, padding 0, ceil_mode), the other side of that switch),
'drop_downsample_bn' (layer2.0's shortcut without its BatchNorm) and 'no_last_relu_mask' (the last ReLU passes every gradient; the forward is unchanged).

synth_checkpoint(layers, seed): convolutions N(0, 2 / fan_in); BatchNorm weight U(0.5, 1.5) (times r for every bn3 and downsample.1), bias and running mean
0.1 N(0, 1), running variance U(0.5, 1.5); `backbone.fc.*` and `linear.*` as the reference's file has them.  r = 0.5: with it max |activation| stays below 50
for (1, 1, 1, 1) and for the full (3, 4, 6, 3) at B = 2 (test_conditions_on_the_gpu_tests_inputs prints the figures), three orders of magnitude inside the
split-fp16 limit of 65504.  synth_images: a random 14 x 14 image enlarged bilinearly plus 10 % noise, in [0, 1] like the trainer's.
"""
import functools
import math

import torch
import torch.nn.functional as F

FULL = (3, 4, 6, 3)
PLANES = (64, 128, 256, 512)
METRICS = ("l2", "l1", "cos")
RESIDUAL_GAIN = 0.5
# (layers, seed, B, H, W) of the whole-module GPU tests: at 199 x 213 every level has one odd and one even side (100 x 107, 50 x 54, 25 x 27, 13 x 14, 7 x 7)
NET_CASES = (((1, 1, 1, 1), 1, 2, 224, 224), ((1, 1, 1, 1), 1, 2, 199, 213), (FULL, 2, 2, 224, 224))


def _bn(g, c, gain=1.0):
    return {"weight": (0.5 + torch.rand(c, generator=g)) * gain, "bias": 0.1 * torch.randn(c, generator=g), "running_mean": 0.1 * torch.randn(c, generator=g),
            "running_var": 0.5 + torch.rand(c, generator=g), "num_batches_tracked": torch.tensor(0, dtype=torch.long)}


def _conv(g, cout, cin, k):
    return torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))


@functools.lru_cache(maxsize=None)
def synth_checkpoint(layers, seed):
    """-> {'state_dict': {'backbone.conv1.weight': ..., 'backbone.fc.*', 'linear.*'}, 'epoch': 1} (fp32 CPU tensors; do not modify)"""
    g = torch.Generator().manual_seed(3000 + seed)
    sd = {}

    def put(prefix, d):
        for k, v in d.items():
            sd[f"backbone.{prefix}.{k}"] = v

    sd["backbone.conv1.weight"] = _conv(g, 64, 3, 7)
    put("bn1", _bn(g, 64))
    cin = 64
    for li, (planes, n) in enumerate(zip(PLANES, layers)):
        for i in range(n):
            p = f"layer{li + 1}.{i}"
            sd[f"backbone.{p}.conv1.weight"] = _conv(g, planes, cin, 1)
            sd[f"backbone.{p}.conv2.weight"] = _conv(g, planes, planes, 3)
            put(p + ".bn1", _bn(g, planes))
            put(p + ".bn2", _bn(g, planes))
            sd[f"backbone.{p}.conv3.weight"] = _conv(g, planes * 4, planes, 1)
            put(p + ".bn3", _bn(g, planes * 4, RESIDUAL_GAIN))
            if i == 0:
                sd[f"backbone.{p}.downsample.0.weight"] = _conv(g, planes * 4, cin, 1)
                put(p + ".downsample.1", _bn(g, planes * 4, RESIDUAL_GAIN))
            cin = planes * 4
    sd["backbone.fc.weight"] = torch.randn(100, 2048, generator=g) / math.sqrt(2048)
    sd["backbone.fc.bias"] = torch.zeros(100)
    sd["linear.weight"] = torch.randn(10, 2048, generator=g) / math.sqrt(2048)      # EMOCA's head on the features, which the reference deletes
    sd["linear.bias"] = torch.zeros(10)
    return {"state_dict": sd, "epoch": 1}


def synth_images(B, H, W, seed):
    g = torch.Generator().manual_seed(4000 + seed)
    base = F.interpolate(torch.rand(B, 3, 14, 14, generator=g), size=(H, W), mode="bilinear", align_corners=False)
    return (0.9 * base + 0.1 * torch.rand(B, 3, H, W, generator=g)).clamp(0.0, 1.0)


def _norm(sd, p, x, dtype):
    get = lambda k: sd[f"backbone.{p}.{k}"].to(dtype).view(1, -1, 1, 1)
    return (x - get("running_mean")) / torch.sqrt(get("running_var") + 1e-5) * get("weight") + get("bias")


def features_law(ckpt, images, layers, dtype=torch.float64, trace=None, variant=None):
    """images [N, 3, H, W] -> features [N, 2048] in `dtype` on the CPU (differentiable with respect to images)"""
    sd = ckpt["state_dict"]
    note = (lambda name, t: trace.append((name, float(t.detach().abs().max())))) if trace is not None else (lambda name, t: None)
    conv = lambda x, key, stride, pad: F.conv2d(x, sd[f"backbone.{key}"].to(dtype), None, stride, pad)
    x = torch.relu(_norm(sd, "bn1", conv(images.to(dtype), "conv1.weight", 2, 3), dtype))
    note("stem", x)
    x = F.max_pool2d(x, 3, 2, 0, ceil_mode=True) if variant == "pool_ceil" else F.max_pool2d(x, 3, 2, 1)
    last = (len(layers) - 1, layers[-1] - 1)
    for li, n in enumerate(layers):
        for i in range(n):
            p = f"layer{li + 1}.{i}"
            stride = 2 if (i == 0 and li > 0) else 1
            s1, s2 = (stride, 1) if variant == "stride_on_conv1" else (1, stride)
            y = torch.relu(_norm(sd, p + ".bn1", conv(x, p + ".conv1.weight", s1, 0), dtype))
            y = torch.relu(_norm(sd, p + ".bn2", conv(y, p + ".conv2.weight", s2, 1), dtype))
            y = _norm(sd, p + ".bn3", conv(y, p + ".conv3.weight", 1, 0), dtype)
            if i == 0:
                r = conv(x, p + ".downsample.0.weight", stride, 0)
                if not (variant == "drop_downsample_bn" and li == 1):
                    r = _norm(sd, p + ".downsample.1", r, dtype)
            else:
                r = x
            z = y + r
            x = torch.relu(z)
            if variant == "no_last_relu_mask" and (li, i) == last:
                x = z + (x - z).detach()                                   # the ReLU's value, the identity's gradient
            note(p, x)
    return F.avg_pool2d(x, 7).flatten(1)


def loss_law(g, t, metric, use_mean):
    """ExpressionLoss.py:53-65 on feature rows g, t [B, C]"""
    if metric == "l2":
        loss = ((g - t) ** 2).mean(dim=1)
    elif metric == "l1":
        loss = (g - t).abs().mean(dim=1)
    elif metric == "cos":
        loss = 1.0 - F.cosine_similarity(g, t, dim=1)
    else:
        raise ValueError(metric)
    return loss.mean() if use_mean else loss


def emotion_law(ckpt, gen, tar, layers, dtype=torch.float64, metric="l2", use_mean=True, upstream=None, trace=None, variant=None):
    """-> dict(features [2B, 2048] (gen rows first), loss, grad = d (loss * upstream).sum() / d gen) in `dtype` on the CPU"""
    B = gen.shape[0]
    x = gen.to(dtype).clone().requires_grad_(True)
    f = features_law(ckpt, torch.cat([x, tar.to(dtype)]), layers, dtype, trace, variant)
    loss = loss_law(f[:B], f[B:], metric, use_mean)
    up = torch.ones_like(loss) if upstream is None else upstream.to(dtype)
    (grad,) = torch.autograd.grad((loss * up).sum(), x)
    return {"features": f.detach(), "loss": loss.detach(), "grad": grad}


@functools.lru_cache(maxsize=None)
def case_reference(layers, seed, B, H, W):
    """The shared, unchanged reference of one whole-module case: the images, the float64 law with its trace, and eager fp32 torch on the same law and inputs
    ('l2', use_mean=True)."""
    ckpt, gen, tar = synth_checkpoint(layers, seed), synth_images(B, H, W, seed), synth_images(B, H, W, seed + 100)
    trace = []
    f64 = emotion_law(ckpt, gen, tar, layers, torch.float64, trace=trace)
    f32 = emotion_law(ckpt, gen, tar, layers, torch.float32)
    return {"ckpt": ckpt, "gen": gen, "tar": tar, "f64": f64, "f32": f32, "trace": trace}


def bound_of(ref, name, floor=2.0 ** -20):
    """The whole-module bound on `name` ('features', 'loss' or 'grad'): 4 times the distance of eager fp32 torch from float64 on the same law and inputs (the
    convention of tests/enc_tolerances.py), with a floor of 2^-20 max |ref| — four roundings of the 22-bit storage format, below which the comparison with one
    fp32 run's luck would decide."""
    want = ref["f64"][name]
    e32 = float((ref["f32"][name].double() - want).abs().max())
    return max(4 * e32, floor * float(want.abs().max())), e32


def bound_l2_of(ref, name="grad", floor=2.0 ** -20):
    """The same bound in the Euclidean norm.  One ReLU or max-pool that float64 and a 32-bit evaluation decide differently moves the image gradient by several
    per cent of its maximum in a small region (eager fp32 torch shows such switches on two of the three cases), so the maximum-norm bound on the gradient is
    loose; the Euclidean distance is not dominated by one region and is held to 4 times eager fp32's as well."""
    want = ref["f64"][name]
    e32 = float((ref["f32"][name].double() - want).norm())
    return max(4 * e32, floor * float(want.norm())), e32
