"""The MICA shape term of the reference's pre-training stage (src/models/MICA/mica.py, arcface.py; smirk_trainer.py:128-131, base_trainer.py:93-100, 196-211;
weight 10 in configs/config_pretrain.yaml) on the MI355X.

    mica = MICA().to(device)                                            # assets/mica.tar, or MICA(checkpoint=<path or dict>)
    loss = mica.calculate_mica_shape_loss(encoder_output['shape_params'], batch['img_mica'])
    shape = mica(batch['img_mica'])['shape_params']                     # [B, 300]

forward(images), images [B, 3, 112, 112] in [0, 1]: v = (images - 0.5) / 0.5 with the channels reordered [2, 1, 0]; ArcFace (an iresnet with blocks
[3, 13, 30, 3]: 3 x 3 stem, BatchNorm, PReLU; blocks bn1 -> conv 3 x 3 -> bn2 -> PReLU -> conv 3 x 3 (stride 2 on the first block of a layer) -> bn3, plus
the input or, on a layer's first block, a 1 x 1 stride-2 convolution and BatchNorm of it; then BatchNorm, flatten, Linear(25088, 512), BatchNorm1d);
F.normalize; the mapping network (four Linear + leaky_relu(0.2), one Linear).

The module keeps the reference's structure (`arcface`, `regressor`), so the reference's state dicts load and state_dict() has the reference's keys; the nn
layers hold the parameters and are never called.  Every parameter is frozen and the network ALWAYS computes with the running statistics, whatever train() is
called with: the reference calls .eval() on it once (base_trainer.py:93-100) and BaseTrainer.train() never touches self.mica, so no caller of the reference
ever sees batch statistics.  It is forward-only, as in the reference (calculate_mica_shape_loss runs it under no_grad): an input that requires grad raises.

One forward (all launches on the caller's stream, nothing waits for the host):
  prepare [1]           smirk_mica_prepare_split16: the affine map, the channel reorder, NCHW fp32 -> split16 NHWC [B, 112, 112, 8]
  stem [2]              conv1 on smirk_conv_igemm_f16x3 with bn1 as the epilogue's scale / shift; PReLU by smirk_mica_affine_prelu_split16
  each block [4 or 5]   u = bn1(x) by the streaming kernel (under zero padding the border taps would see a folded shift); conv1(u) with bn2 in the epilogue;
                        PReLU in place; [the downsample convolution of x with its BatchNorm in the epilogue;] conv2 with bn3 in the epilogue and the residual
  fc [2]                bn2, the flatten order and `features` folded into the matrix and the bias (fold_fc, float64 on the host); smirk_mica_fc_split16
  head [1]              smirk_mica_head: F.normalize and the five Linear layers
Packed weights, folded scales / shifts, the folded FC matrix and the head blob are the operands that frozen.FrozenNetwork caches (the rule is stated there).
Batches above 64 run in chunks of at most 64.  Arithmetic: f16x3 convolutions (fp32-class), fp32 elsewhere.
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from . import _lib as L
from .frozen import FrozenNetwork, Holder, bn_affine, device_image, host64, pack_conv, read_checkpoint
from .losses import Term, weighted_loss

LAYERS = (3, 13, 30, 3)                                               # arcface.py:166
PLANES = (64, 128, 256, 512)
MAX_CHUNK = L.MICA_FC_MAX_B
DEFAULT_CHECKPOINT = "assets/mica.tar"                                # mica.py:56


def kaiming_leaky_init(m):
    if m.__class__.__name__.find("Linear") != -1:
        torch.nn.init.kaiming_normal_(m.weight, a=0.2, mode="fan_in", nonlinearity="leaky_relu")


class MappingNetwork(Holder):
    """mica.py:14-43: `network` (1 + hidden Linear layers, leaky_relu(0.2) after each) and `output`.  MICA runs it inside its fused head kernel."""
    owner = "MICA"

    def __init__(self, z_dim, map_hidden_dim, map_output_dim, hidden=2):
        super().__init__()
        self.skips = [int(hidden / 2)] if hidden > 5 else []
        self.network = nn.ModuleList([nn.Linear(z_dim, map_hidden_dim)] +
                                     [nn.Linear(map_hidden_dim + (z_dim if i in self.skips else 0), map_hidden_dim) for i in range(hidden)])
        self.output = nn.Linear(map_hidden_dim, map_output_dim)
        self.network.apply(kaiming_leaky_init)
        with torch.no_grad():
            self.output.weight *= 0.25

    def linears(self):
        return list(self.network) + [self.output]


class IBasicBlock(Holder):
    owner = "MICA"

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(inplanes, eps=1e-05)
        self.conv1 = nn.Conv2d(inplanes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes, eps=1e-05)
        self.prelu = nn.PReLU(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes, eps=1e-05)
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes, eps=1e-05)) if downsample else None
        self.stride = stride


class Arcface(Holder):
    """arcface.py:65-198 with `layers` blocks per stage (the reference: [3, 13, 30, 3])."""
    owner = "MICA"

    def __init__(self, layers=LAYERS):
        super().__init__()
        layers = tuple(int(n) for n in layers)
        if len(layers) != 4 or min(layers) < 1:
            raise L.SmirkHipError(f"MICA: `layers` must be four positive block counts, got {layers}")
        self.conv1 = nn.Conv2d(3, 64, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(64, eps=1e-05)
        self.prelu = nn.PReLU(64)
        inplanes = 64
        for k, (planes, n) in enumerate(zip(PLANES, layers)):
            setattr(self, f"layer{k + 1}", nn.Sequential(*[IBasicBlock(inplanes if i == 0 else planes, planes, 2 if i == 0 else 1, i == 0) for i in range(n)]))
            inplanes = planes
        self.bn2 = nn.BatchNorm2d(512, eps=1e-05)
        self.fc = nn.Linear(512 * 7 * 7, 512)
        self.features = nn.BatchNorm1d(512, eps=1e-05)
        nn.init.constant_(self.features.weight, 1.0)

    def blocks(self):
        return [b for k in range(4) for b in getattr(self, f"layer{k + 1}")]


def fold_fc(fc, bn2, features, hw):
    """features(fc(flatten_nchw(bn2(x)))) as x_nhwc_flat @ w'.T + b' (float64): w'[n][k'] = g[n] w[n][k] s[c], b'[n] = g[n] (b[n] + sum_k w[n][k] t[c]) + h[n]
    with k = c * hw + p the reference's flatten index and k' = p * C + c its NHWC position."""
    s, t = bn_affine(bn2)
    g, h = bn_affine(features)
    n, c = fc.out_features, s.numel()
    w = host64(fc.weight).view(n, c, hw)
    bias = g * (host64(fc.bias) + (w * t.view(1, c, 1)).sum((1, 2))) + h
    w = (g.view(n, 1, 1) * w * s.view(1, c, 1)).permute(0, 2, 1).reshape(n, hw * c)
    return w.contiguous(), bias


def load_reference_checkpoint(module, checkpoint):
    """mica.py:56-65: checkpoint['arcface'] strictly; of checkpoint['flameModel'] the keys containing `network` or `output`, `regressor.` stripped, strictly."""
    for key in ("arcface", "flameModel"):
        if key not in checkpoint:
            raise L.SmirkHipError(f"MICA: `checkpoint` has no {key!r} entry (expected the format of assets/mica.tar)")
    module.arcface.load_state_dict(checkpoint["arcface"], strict=True)
    module.regressor.load_state_dict({k.replace("regressor.", ""): v for k, v in checkpoint["flameModel"].items() if "network" in k or "output" in k}, strict=True)


class MICA(FrozenNetwork):
    """src/models/MICA/mica.py:48-94.  `checkpoint`: a path or a dict in the reference's format; None reads assets/mica.tar like the reference.  `layers`: the
    blocks per stage (the reference always uses (3, 13, 30, 3); shallower networks are for tests)."""
    pin_eval = True                                                    # the running statistics whatever train() is called with (see the module docstring)

    def __init__(self, checkpoint=None, layers=LAYERS):
        super().__init__()
        self.arcface = Arcface(layers)
        self.regressor = MappingNetwork(512, 300, 300, hidden=3)
        load_reference_checkpoint(self, read_checkpoint(checkpoint, DEFAULT_CHECKPOINT, "MICA", "'arcface' and 'flameModel'"))
        self.freeze()
        self._ws = L.Workspace()

    @property
    def image_size(self):
        """The input size fc.in_features implies: four stride-2 stages in front of a [512, s / 16, s / 16] feature map."""
        return 16 * math.isqrt(self.arcface.fc.in_features // 512)

    # ---- operands ----------------------------------------------------------------------------------------------------------------------------------------
    def _build_operands(self, dev):
        f32 = lambda v: v.float().to(dev)

        def conv(m, bn):                                               # (packed split16 weight, epilogue scale, epilogue shift) of a convolution and the BatchNorm behind it
            s, t = bn_affine(bn)
            return pack_conv(m.weight.detach(), max(m.in_channels, 8))[0], f32(s), f32(t)

        a = self.arcface
        ops = {"stem": conv(a.conv1, a.bn1) + (a.prelu.weight.detach(),), "blocks": []}
        for b in a.blocks():
            s1, t1 = bn_affine(b.bn1)
            ops["blocks"].append(dict(bn1=(f32(s1), f32(t1)), conv1=conv(b.conv1, b.bn2), slope=b.prelu.weight.detach(), conv2=conv(b.conv2, b.bn3), stride=b.stride,
                                      planes=b.conv1.out_channels, down=None if b.downsample is None else conv(b.downsample[0], b.downsample[1])))
        hw = a.fc.in_features // 512
        w, bias = fold_fc(a.fc, a.bn2, a.features, hw)
        ops["fc"] = (f32(w), f32(bias))
        lin = self.regressor.linears()
        if self.regressor.skips or len(lin) != L.MICA_HEAD_LAYERS:
            raise L.SmirkHipError(f"MICA: the head kernel runs {L.MICA_HEAD_LAYERS} plain Linear layers (MappingNetwork(512, 300, 300, hidden=3))")
        pad4 = lambda n: (n + 3) // 4 * 4                              # every matrix and bias starts on a 16-byte boundary of the blob
        blob = torch.zeros(sum(pad4(m.weight.numel()) + pad4(m.bias.numel()) for m in lin), device=dev)
        head, off = L.SmirkMicaHead(), 0
        for k, m in enumerate(lin):
            for name, t in (("w", m.weight), ("b", m.bias)):
                blob[off:off + t.numel()] = t.detach().reshape(-1)
                setattr(head.layer[k], name, blob.data_ptr() + 4 * off)
                off += pad4(t.numel())
            head.layer[k].n_in, head.layer[k].n_out = m.in_features, m.out_features
        ops["head"], ops["head_blob"], ops["n_out"] = head, blob, lin[-1].out_features
        return ops

    # ---- the schedule --------------------------------------------------------------------------------------------------------------------------------------
    def _chunk(self, img, ops):
        """img [b <= 64, 3, S, S] fp32 contiguous -> (features [b, 512], shape_params [b, n_out]), both fp32"""
        lib, st, dev, P = L.lib(), L.stream_ptr(), img.device, L.ptr
        B, _, H, W = img.shape
        x = torch.empty(B, H, W, 8, device=dev)
        L.check(lib.smirk_mica_prepare_split16(P(img), P(x), B, H, W, st))

        def conv(src, op, k, stride, residual=None):
            _, h, w, c = src.shape
            return L.conv_launch(lib.smirk_conv_igemm_f16x3, L.conv_desc(B, h, w, c, op[1].numel(), k, stride=stride), st, src, op[0], None, op[1], op[2], residual)

        def stream(src, scale, shift, slope, dst):
            L.check(lib.smirk_mica_affine_prelu_split16(P(src), P(scale, allow_none=True), P(shift, allow_none=True), P(slope, allow_none=True), P(dst),
                                                        src.numel() // src.shape[-1], src.shape[-1], st))

        x = conv(x, ops["stem"], 3, 1)
        stream(x, None, None, ops["stem"][3], x)
        for b in ops["blocks"]:
            u = torch.empty_like(x)
            stream(x, b["bn1"][0], b["bn1"][1], None, u)
            y = conv(u, b["conv1"], 3, 1)
            stream(y, None, None, b["slope"], y)
            r = x if b["down"] is None else conv(x, b["down"], 1, b["stride"])
            x = conv(y, b["conv2"], 3, b["stride"], residual=r)
        w, bias = ops["fc"]
        n, k = w.shape
        feat = torch.empty(B, n, device=dev)
        ws = self._ws.get(lib.smirk_mica_fc_workspace_bytes(B, k, n), dev)
        L.check(lib.smirk_mica_fc_split16(P(x), P(w), P(bias), P(feat), C.c_void_p(ws.data_ptr()), ws.numel(), B, k, n, st))
        out = torch.empty(B, ops["n_out"], device=dev)
        L.check(lib.smirk_mica_head(P(feat), C.byref(ops["head"]), P(out), B, st))
        return feat, out

    def _run(self, images):
        img = device_image("MICA", "images", images)
        s = self.image_size
        if images.shape[0] < 1 or tuple(images.shape[2:]) != (s, s):
            raise L.SmirkHipError(f"MICA: images must be [B >= 1, 3, {s}, {s}] (the size fc.in_features = {self.arcface.fc.in_features} implies), got {tuple(images.shape)}")
        if images.requires_grad:
            raise L.SmirkHipError("MICA: images requires grad; the network is forward-only (the reference never differentiates through MICA: mica.py:84-86)")
        L.raise_if_range_tripped("MICA")
        ops = self._operands(img.device)
        parts = [self._chunk(img[i:i + MAX_CHUNK], ops) for i in range(0, img.shape[0], MAX_CHUNK)]
        return parts[0] if len(parts) == 1 else tuple(torch.cat(p) for p in zip(*parts))

    def arcface_features(self, images):
        """The [B, 512] output of the ArcFace network (before F.normalize): `self.arcface(transformed_images)` of mica.py:74."""
        return self._run(images)[0]

    def forward(self, images):
        """images [B, 3, 112, 112] fp32 in [0, 1] on the HIP device -> {'shape_params': [B, 300]} (mica.py:68-78)."""
        return {"shape_params": self._run(images)[1]}

    def calculate_mica_shape_loss(self, shape_params, img):
        """mica.py:80-94: F.mse_loss(shape_params, MICA(img)['shape_params'][..., :D]), differentiable with respect to shape_params; the MICA output is a constant."""
        if not torch.is_tensor(shape_params) or shape_params.dim() != 2:
            raise L.SmirkHipError("MICA: shape_params must be a [B, D] tensor")
        D = shape_params.shape[1]
        s = self.image_size
        with torch.no_grad():
            mica_shape = self.forward(img.reshape(-1, 3, s, s))["shape_params"]
        if mica_shape.shape[-1] > D:                                   # the reference prints a warning on every call and truncates
            mica_shape = mica_shape[..., :D]
        return weighted_loss([Term(shape_params, mica_shape)])[0]
