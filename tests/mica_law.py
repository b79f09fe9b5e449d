"""The law of the MICA network for the tests of smirk_amd.mica: a float64 restatement of src/models/MICA/mica.py and arcface.py written from the architecture,
sharing no code with the reference and none with smirk_amd/mica.py, evaluated functionally on a checkpoint in the reference's format.

    v = (img - 0.5) / 0.5, channels [2, 1, 0]
    x = prelu(bn1(conv1(v)))                                              3 x 3, pad 1, no bias; BatchNorm in eval mode, eps 1e-5; PReLU per channel
    per block:  x = bn3(conv2(prelu(bn2(conv1(bn1(x)))))) + (x, or downsample.1(downsample.0(x)) on the first block of a layer)
                conv2 and downsample.0 (1 x 1, no pad) have stride 2 on the first block of a layer
    f = features(fc(flatten_nchw(bn2(x))))                                Linear(512 * 7 * 7, 512), BatchNorm1d in eval mode
    z = f / max(|f|_2, 1e-12);  four times z = leaky_relu(W z + b, 0.2);  shape = W z + b

`trace` receives (name, max |activation|) per layer.  `variant` makes one deliberate mistake (tests/test_mica_cpu.py shows that the GPU bounds see each).

synth_checkpoint(layers, seed): convolutions N(0, 2 / fan_in); BatchNorm weight U(0.5, 1.5) (times r for every bn3), bias and running mean 0.1 N(0, 1), running
variance U(0.5, 1.5); PReLU slopes U(-0.25, 0.5) with one slope exactly 0 and one exactly 1 per layer; Linear weights N(0, 1 / in_features); the regressor at the
reference's own initialisation (mica.py:8-32).  r = 0.3 for networks of at most 8 blocks and 0.1 for the full [3, 13, 30, 3]: with the reference's classes at
B = 2, r = 0.3 keeps max |activation| at 45 - 80 for (1,1,1,1), (1,2,1,1) and (2,2,2,2) and r = 0.1 keeps it at 98 for the full network (feature norm about 245),
while r = 0.3 on the full network reaches 2.5e4, too close to the split-fp16 limit of 65504.
"""
import functools
import math

import torch
import torch.nn.functional as F

FULL = (3, 13, 30, 3)
PLANES = (64, 128, 256, 512)
SIZE = 112
# (layers, seed, B) of the whole-network GPU tests
NET_CASES = (((1, 1, 1, 1), 1, 3), ((1, 2, 1, 1), 2, 2), (FULL, 3, 2))


def bn3_gain(layers):
    return 0.3 if sum(layers) <= 8 else 0.1


def _bn(g, c, gain=1.0):
    return {"weight": (0.5 + torch.rand(c, generator=g)) * gain, "bias": 0.1 * torch.randn(c, generator=g), "running_mean": 0.1 * torch.randn(c, generator=g),
            "running_var": 0.5 + torch.rand(c, generator=g), "num_batches_tracked": torch.tensor(0, dtype=torch.long)}


def _conv(g, cout, cin, k):
    return torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))


def _prelu(g, c):
    a = torch.rand(c, generator=g) * 0.75 - 0.25
    a[1], a[c // 2] = 0.0, 1.0
    return a


@functools.lru_cache(maxsize=None)
def synth_checkpoint(layers, seed):
    """-> {'arcface': state dict, 'flameModel': {'regressor.network.0.weight': ..., other keys the loader must ignore}} (fp32 CPU tensors; do not modify)"""
    g = torch.Generator().manual_seed(1000 + seed)
    r = bn3_gain(layers)
    sd = {}

    def put(prefix, d):
        for k, v in d.items():
            sd[f"{prefix}.{k}"] = v

    sd["conv1.weight"] = _conv(g, 64, 3, 3)
    put("bn1", _bn(g, 64))
    sd["prelu.weight"] = _prelu(g, 64)
    cin = 64
    for li, (planes, n) in enumerate(zip(PLANES, layers)):
        for i in range(n):
            p = f"layer{li + 1}.{i}"
            put(p + ".bn1", _bn(g, cin))
            sd[p + ".conv1.weight"] = _conv(g, planes, cin, 3)
            put(p + ".bn2", _bn(g, planes))
            sd[p + ".prelu.weight"] = _prelu(g, planes)
            sd[p + ".conv2.weight"] = _conv(g, planes, planes, 3)
            put(p + ".bn3", _bn(g, planes, r))
            if i == 0:
                sd[p + ".downsample.0.weight"] = _conv(g, planes, cin, 1)
                put(p + ".downsample.1", _bn(g, planes))
            cin = planes
    put("bn2", _bn(g, 512))
    k = 512 * 49
    sd["fc.weight"] = torch.randn(512, k, generator=g) / math.sqrt(k)
    sd["fc.bias"] = 0.1 * torch.randn(512, generator=g)
    put("features", _bn(g, 512))
    flame = {"flame.shapedirs": torch.zeros(3)}                          # a key of the real file's flameModel that is not the regressor's
    gain = math.sqrt(2.0 / (1.0 + 0.2 ** 2))
    dims = [(512, 300), (300, 300), (300, 300), (300, 300)]
    for j, (fi, fo) in enumerate(dims):                                  # kaiming_normal_(a=0.2, fan_in); nn.Linear's default bias
        flame[f"regressor.network.{j}.weight"] = torch.randn(fo, fi, generator=g) * (gain / math.sqrt(fi))
        flame[f"regressor.network.{j}.bias"] = (torch.rand(fo, generator=g) * 2 - 1) / math.sqrt(fi)
    flame["regressor.output.weight"] = 0.25 * (torch.rand(300, 300, generator=g) * 2 - 1) / math.sqrt(300)
    flame["regressor.output.bias"] = (torch.rand(300, generator=g) * 2 - 1) / math.sqrt(300)
    return {"arcface": sd, "flameModel": flame}


def synth_images(B, seed):
    return torch.rand(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(2000 + seed))


def _norm(sd, p, x, dtype):
    shape = (1, -1) + (1,) * (x.dim() - 2)
    get = lambda k: sd[f"{p}.{k}"].to(dtype).view(shape)
    return (x - get("running_mean")) / torch.sqrt(get("running_var") + 1e-5) * get("weight") + get("bias")


def _prelu_fn(sd, p, x, dtype):
    return torch.where(x > 0, x, sd[p + ".weight"].to(dtype).view(1, -1, 1, 1) * x)


def mica_law(ckpt, images, layers, dtype=torch.float64, trace=None, variant=None):
    """-> dict(features [B, 512], shape_params [B, 300]) in `dtype` on the CPU.  variant: None, 'no_reorder', 'nhwc_flatten' or ('drop_bn1', block ordinal)."""
    sd = ckpt["arcface"]
    note = (lambda name, t: trace.append((name, float(t.abs().max())))) if trace is not None else (lambda name, t: None)
    conv = lambda x, key, stride, pad: F.conv2d(x, sd[key].to(dtype), None, stride, pad)
    with torch.no_grad():
        v = (images.to(dtype) - 0.5) / 0.5
        if variant != "no_reorder":
            v = v[:, [2, 1, 0]]
        x = _prelu_fn(sd, "prelu", _norm(sd, "bn1", conv(v, "conv1.weight", 1, 1), dtype), dtype)
        note("stem", x)
        ordinal = 0
        for li, n in enumerate(layers):
            for i in range(n):
                p = f"layer{li + 1}.{i}"
                stride = 2 if i == 0 else 1
                u = x if variant == ("drop_bn1", ordinal) else _norm(sd, p + ".bn1", x, dtype)
                y = _prelu_fn(sd, p + ".prelu", _norm(sd, p + ".bn2", conv(u, p + ".conv1.weight", 1, 1), dtype), dtype)
                note(p + ".prelu", y)
                y = _norm(sd, p + ".bn3", conv(y, p + ".conv2.weight", stride, 1), dtype)
                x = y + (_norm(sd, p + ".downsample.1", conv(x, p + ".downsample.0.weight", stride, 0), dtype) if i == 0 else x)
                note(p, x)
                ordinal += 1
        x = _norm(sd, "bn2", x, dtype)
        flat = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1) if variant == "nhwc_flatten" else x.reshape(x.shape[0], -1)
        f = _norm(sd, "features", F.linear(flat, sd["fc.weight"].to(dtype), sd["fc.bias"].to(dtype)), dtype)
        note("features", f)
        shape = head_law(ckpt, f, dtype)
        note("shape_params", shape)
    return {"features": f, "shape_params": shape}


def head_law(ckpt, feat, dtype=torch.float64, linears=None):
    """F.normalize (eps 1e-12) and the mapping network on features [B, n]; `linears`: five (weight, bias) pairs instead of the checkpoint's regressor."""
    if linears is None:
        fm = ckpt["flameModel"]
        linears = [(fm[f"regressor.network.{j}.weight"], fm[f"regressor.network.{j}.bias"]) for j in range(4)] + [(fm["regressor.output.weight"], fm["regressor.output.bias"])]
    z = feat.to(dtype)
    z = z / z.norm(dim=1, keepdim=True).clamp_min(1e-12)
    for j, (w, b) in enumerate(linears):
        z = z @ w.to(dtype).t() + b.to(dtype)
        if j < len(linears) - 1:
            z = torch.where(z > 0, z, 0.2 * z)
    return z


@functools.lru_cache(maxsize=None)
def case_reference(layers, seed, B):
    """The shared, unchanged reference of one (layers, seed, B): the images, the float64 law with its trace, and eager fp32 torch on the same law and inputs."""
    ckpt, img = synth_checkpoint(layers, seed), synth_images(B, seed)
    trace = []
    f64 = mica_law(ckpt, img, layers, torch.float64, trace)
    f32 = mica_law(ckpt, img, layers, torch.float32)
    return {"ckpt": ckpt, "images": img, "f64": f64, "f32": f32, "trace": trace}
