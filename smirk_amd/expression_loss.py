"""The emotion term of the reference trainer's first path (smirk_trainer.py:108-119; src/losses/ExpressionLoss.py, src/losses/resnet.py) on the MI355X.

    emotion = ExpressionLoss().to(device)                               # the reference's checkpoint, or ExpressionLoss(checkpoint=<path or dict>)
    loss = emotion(gen, tar, metric='l2', use_mean=False).mean()        # smirk_trainer.py:117; or first_path.emotion_term(generator, emotion, ...)

forward(gen, tar), both [B, 3, H, W]: each goes through EMOCA's frozen ResNet-50 — Conv2d(3, 64, 7, stride 2, pad 3), BatchNorm, ReLU, MaxPool2d(3, 2, 1), the
Bottleneck stages [3, 4, 6, 3] (1 x 1, 3 x 3, 1 x 1 with a BatchNorm behind each and a ReLU behind the first two; the stride of a stage's first block sits on
its 3 x 3 convolution, `emoca_specific`; that block's shortcut is a 1 x 1 convolution of the same stride and a BatchNorm; ReLU after the sum), AvgPool2d(7) —
and the loss is, per sample, the mean squared ('l2') or absolute ('l1') difference of the two [2048] feature rows or one minus their cosine ('cos'); with
`use_mean` the mean of that over the batch.

The module keeps the reference's structure (`backbone` with `fc`), so the reference's checkpoint loads and state_dict() has the reference's keys; the nn layers
hold the parameters and are never called.  Every parameter is frozen and the network ALWAYS computes with the running statistics, whatever train() is called
with (the reference calls .eval() once in ExpressionLoss.py:30 and BaseTrainer.train() never touches self.emotion_loss).

One forward is ONE torch.autograd.Function with a gradient for `gen` alone.  gen and tar run as one batch of 2B rows (all launches on the caller's stream,
nothing waits for the host):
  stem [1]              smirk_emotion_stem_split16: the 7 x 7 convolution on the fp16 matrix pipe, bn1 folded into the weights and the shift, ReLU
  pool [1]              smirk_emotion_maxpool_split16
  each block [3 or 4]   conv1, conv2, [downsample,] conv3 on smirk_conv_igemm_f16x3: BatchNorm as the epilogue's scale / shift, the ReLU and, in conv3, the
                        shortcut as the epilogue's residual
  head [2]              smirk_emotion_head_forward_split16: the average pool; the per-sample loss and its mean
which is 4 + 3 * blocks + (blocks with a downsample) launches: 56 for [3, 4, 6, 3].  The backward runs over the gen rows only; the weights are frozen, so it is
data gradients alone, with every BatchNorm scale folded into the data-gradient image of the convolution in front of it (float64 on the host):
  head [1]              smirk_emotion_head_backward_split16: the seed, lifted by a power of two into fp16's normal range, under the last ReLU's mask
  each block            [mask of the block's output ReLU, except in the last block] conv3's data gradient; the mask of relu2 (stride 1) or the adjoint helper
                        smirk_emotion_dilate2_split16 with that mask fused in (stride 2: the 3 x 3 stride-2 data gradient is then a stride-1 convolution of the
                        zero-dilated gradient); conv2's data gradient; the mask of relu1; conv1's data gradient with the shortcut's gradient as the residual.
                        A block with a downsample adds that convolution's data gradient and, at stride 2, the helper that scatters it onto the even positions
                        and adds it: 6 launches for a plain block, 7 for layer1.0, 8 for the first blocks of layers 2 - 4, one less in the last block
  pool, stem [2]        smirk_emotion_maxpool_backward_split16 with the stem's ReLU mask; smirk_emotion_stem_dgrad_split16, which also applies the upstream
                        gradient (per sample) and divides the lift out
which is 2 + 6 * blocks + (blocks with a downsample) + (stride-2 blocks): 105 for [3, 4, 6, 3].  `launches(layers)` states both numbers.
The packed and folded weight images are the operands that frozen.FrozenNetwork caches (the rule is stated there).  Arithmetic: f16x3 convolutions (fp32-class), fp32 elsewhere.
"""
import torch
import torch.nn as nn

from . import _lib as L
from .frozen import FrozenNetwork, Holder, bn_affine, host64, image_pair, pack_conv, read_checkpoint
from .smirk_generator import split16_to_float

LAYERS = (3, 4, 6, 3)                                                  # resnet.py:160
PLANES = (64, 128, 256, 512)
EXPANSION = 4
DEFAULT_CHECKPOINT = "assets/ResNet50/checkpoints/deca-epoch=01-val_loss_total/dataloader_idx_0=1.27607644.ckpt"      # ExpressionLoss.py:32
MIN_SIZE, MAX_SIZE = 193, 224                                          # the sizes whose final map is 7 x 7: AvgPool2d(7) then yields [B, 2048]
FINAL = 7
LIMIT_BYTES = 1 << 31


class Bottleneck(Holder):
    """resnet.py:43-63 with emoca_specific=True on a stage's first block (the stride on conv2); the later blocks have stride 1, where the switch changes nothing."""
    owner = "ExpressionLoss"

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * EXPANSION, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * EXPANSION)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


class ResNet(Holder):
    """resnet.py:88-135 with Bottleneck blocks, num_classes=100, include_top=False (`fc` exists and is unused, as in the reference), emoca_specific=True."""
    owner = "ExpressionLoss"

    def __init__(self, layers=LAYERS, num_classes=100):
        super().__init__()
        layers = tuple(int(n) for n in layers)
        if len(layers) != 4 or min(layers) < 1:
            raise L.SmirkHipError(f"ExpressionLoss: `layers` must be four positive block counts, got {layers}")
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for k, (planes, n) in enumerate(zip(PLANES, layers)):
            stride = 1 if k == 0 else 2
            down = nn.Sequential(nn.Conv2d(inplanes, planes * EXPANSION, 1, stride, bias=False), nn.BatchNorm2d(planes * EXPANSION))
            blocks = [Bottleneck(inplanes, planes, stride, down)] + [Bottleneck(planes * EXPANSION, planes, 1, None) for _ in range(1, n)]
            setattr(self, f"layer{k + 1}", nn.Sequential(*blocks))
            inplanes = planes * EXPANSION
        self.avgpool = nn.AvgPool2d(FINAL, stride=1)
        self.fc = nn.Linear(512 * EXPANSION, num_classes)

    def blocks(self):
        return [b for k in range(4) for b in getattr(self, f"layer{k + 1}")]


def launches(layers=LAYERS):
    """-> (forward, backward) kernel launches of one call, the numbers of the module docstring"""
    blocks = sum(layers)
    return 4 + 3 * blocks + 4, 2 + 6 * blocks + 4 + 3


def lift_of(metric, channels, hw=FINAL * FINAL):
    """The power of two the seed gradient is lifted by: d loss / d feature is about (g - t) / (channels * hw) for 'l2' and 'l1' and about
    1 / (|g| hw) with |g| of the order sqrt(channels) for 'cos', far below fp16's normal range at 2048 channels; the lift brings it to the order of (g - t)
    and 1.  It depends on the shapes alone, and the stem's data gradient divides it out exactly."""
    n = channels * hw if metric != "cos" else hw * max(1, int(channels ** 0.5))
    return float(1 << (n - 1).bit_length())


def fold_stem(conv, bn):
    """-> (forward image [64, 160]: k = (ky * 7 + kx) * 3 + c, zeros from 147 on; shift [64]; data-gradient image [7, 7, 3, 64]), float64, the BatchNorm scale
    folded into both images"""
    s, t = bn_affine(bn)
    w = host64(conv.weight) * s.view(-1, 1, 1, 1)                     # [co][c][ky][kx]
    fwd = torch.zeros(w.shape[0], L.EMOTION_STEM_KPAD, dtype=torch.float64)
    fwd[:, :L.EMOTION_STEM_K] = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    return fwd, t, w.permute(2, 3, 1, 0).contiguous()


def load_reference_checkpoint(module, checkpoint):
    """ExpressionLoss.py:32-43: checkpoint['state_dict'] without `backbone.fc.*` and `linear.*`, then load_state_dict(strict=False)."""
    if "state_dict" not in checkpoint:
        raise L.SmirkHipError("ExpressionLoss: `checkpoint` has no 'state_dict' entry (expected the format of EMOCA's ResNet50 checkpoint)")
    sd = dict(checkpoint["state_dict"])
    for key in ("backbone.fc.weight", "backbone.fc.bias", "linear.weight", "linear.bias"):
        if key not in sd:
            raise KeyError(f"ExpressionLoss: the checkpoint's state_dict has no {key!r} (ExpressionLoss.py:34-41 deletes it)")
        del sd[key]
    return module.load_state_dict(sd, strict=False)


class _Emotion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, gen, tar, metric, use_mean, keep, trace):
        lib, st, dev, P = L.lib(), L.stream_ptr(), gen.device, L.ptr
        B, _, H, W = gen.shape
        ops = module._operands(dev)
        n2 = 2 * B
        h, w = (H + 1) // 2, (W + 1) // 2
        stem = torch.empty(n2, h, w, L.EMOTION_STEM_COUT, device=dev)
        L.check(lib.smirk_emotion_stem_split16(P(gen), P(tar), P(ops["stem"][0]), P(ops["stem"][1]), P(stem), B, H, W, st))
        x = torch.empty(n2, (h + 1) // 2, (w + 1) // 2, L.EMOTION_STEM_COUT, device=dev)
        L.check(lib.smirk_emotion_maxpool_split16(P(stem), P(x), n2, h, w, L.EMOTION_STEM_COUT, st))

        def conv(src, op, k, stride, relu, residual=None):
            _, sh, sw, c = src.shape
            return L.conv_launch(lib.smirk_conv_igemm_f16x3, L.conv_desc(n2, sh, sw, c, op[1].numel(), k, stride=stride, relu=relu), st, src, op[0], None, op[1],
                                 op[2], residual)

        tape = []
        for b in ops["blocks"]:
            a1 = conv(x, b["conv1"], 1, 1, True)
            a2 = conv(a1, b["conv2"], 3, b["stride"], True)
            r = x if b["down"] is None else conv(x, b["down"], 1, b["stride"], False)
            out = conv(a2, b["conv3"], 1, 1, True, residual=r)
            if keep:                                                     # the gen rows: leading halves, contiguous views
                tape.append((a1[:B], a2[:B], out[:B]))
            x = out
        _, fh, fw, c = x.shape
        pooled, aux, loss = torch.empty(n2, c, device=dev), torch.empty(B, 4, device=dev), torch.empty(B, device=dev)
        mean = torch.empty((), device=dev) if use_mean else None
        code = L.EMOTION_METRICS[metric]
        L.check(lib.smirk_emotion_head_forward_split16(P(x), P(pooled), P(aux), P(loss), P(mean, allow_none=True), B, fh * fw, c, code, st))
        if trace is not None:
            trace["features"] = pooled
            trace["stem"] = split16_to_float(stem)
        ctx.tape = (module, ops, stem[:B], tape, pooled, aux, (B, H, W, fh * fw, c), code, lift_of(metric, c, fh * fw), use_mean) if keep else None
        ctx.kept = bool(keep)
        return mean if use_mean else loss

    @staticmethod
    def backward(ctx, g_loss):
        if not ctx.kept:
            return (None,) * 7
        if ctx.tape is None:
            raise L.second_backward("ExpressionLoss", "saved activations")
        module, ops, stem, tape, pooled, aux, (B, H, W, hw, c), code, lift, use_mean = ctx.tape
        ctx.tape = None
        lib, st, dev, P = L.lib(), L.stream_ptr(), stem.device, L.ptr
        gup = L.as_f32c(g_loss.detach())
        gup = (gup / B).expand(B).contiguous() if use_mean else gup.reshape(B)

        def conv(src, wd, k, residual=None):                              # a data gradient: the stride-1 convolution with the rotated, scale-folded weights
            _, sh, sw, ci = src.shape
            return L.conv_launch(lib.smirk_conv_igemm_f16x3, L.conv_desc(B, sh, sw, ci, wd.shape[0], k), st, src, wd, residual=residual)

        def mask(dy, y):
            dz = torch.empty_like(dy)
            L.check(lib.smirk_relu_scale_backward_split16(P(dy), P(y), P(ops["ones"]), P(dz), dy.numel() // dy.shape[-1], dy.shape[-1], st))
            return dz

        def dilate(dz, y, add, size):
            out = torch.empty(B, size[0], size[1], dz.shape[-1], device=dev)
            L.check(lib.smirk_emotion_dilate2_split16(P(dz), P(y, allow_none=True), None, P(add, allow_none=True), P(out), B, dz.shape[1], dz.shape[2], size[0],
                                                      size[1], dz.shape[-1], st))
            return out

        g = torch.empty(B, tape[-1][2].shape[1], tape[-1][2].shape[2], c, device=dev)
        L.check(lib.smirk_emotion_head_backward_split16(P(tape[-1][2]), P(pooled), P(aux), P(g), B, hw, c, code, lift, st))
        for k in range(len(tape) - 1, -1, -1):
            b, (a1, a2, out) = ops["blocks"][k], tape[k]
            if k != len(tape) - 1:
                g = mask(g, out)                                         # at the input of the block's last ReLU
            d2 = conv(g, b["conv3_d"], 1)
            size = a1.shape[1:3]
            d2 = mask(d2, a2) if b["stride"] == 1 else dilate(d2, a2, None, size)
            d1 = mask(conv(d2, b["conv2_d"], 3), a1)
            if b["down"] is None:
                g = conv(d1, b["conv1_d"], 1, residual=g)
            elif b["stride"] == 1:
                g = conv(d1, b["conv1_d"], 1, residual=conv(g, b["down_d"], 1))
            else:
                g = dilate(conv(g, b["down_d"], 1), None, conv(d1, b["conv1_d"], 1), size)
        ds = torch.empty_like(stem)
        L.check(lib.smirk_emotion_maxpool_backward_split16(P(stem), P(g), P(ds), B, stem.shape[1], stem.shape[2], stem.shape[3], 1, st))
        dimg = torch.empty(B, 3, H, W, device=dev)
        L.check(lib.smirk_emotion_stem_dgrad_split16(P(ds), P(ops["stem"][2]), P(gup), 1.0 / lift, P(dimg), B, H, W, st))
        return None, dimg, None, None, None, None, None


class ExpressionLoss(FrozenNetwork):
    """src/losses/ExpressionLoss.py.  `checkpoint`: a path or a dict in the reference's format ({'state_dict': {'backbone.*', 'linear.*'}}); None reads the
    reference's path (ExpressionLoss.py:32), relative to the working directory like there.  `layers`: the blocks per stage (the reference always uses
    (3, 4, 6, 3); shallower networks are for tests)."""
    pin_eval = True                                                    # the running statistics whatever train() is called with (see the module docstring)

    def __init__(self, checkpoint=None, layers=LAYERS):
        super().__init__()
        self.backbone = ResNet(layers)
        load_reference_checkpoint(self, read_checkpoint(checkpoint, DEFAULT_CHECKPOINT, "ExpressionLoss", "'state_dict'", weights_only=False))
        self.freeze()

    def _reads(self, name):
        return super()._reads(name) and not name.startswith("backbone.fc.")

    def _build_operands(self, dev):
        f32 = lambda v: v.float().contiguous().to(dev)

        def conv(m, bn):
            """-> ((forward image, epilogue scale, epilogue shift), data-gradient image of the convolution with the BatchNorm scale folded in)"""
            w = m.weight.detach()
            s, t = bn_affine(bn)
            fwd, dgrad = pack_conv(w, m.in_channels, dgrad_from=f32(host64(w) * s.view(-1, 1, 1, 1)))
            return (fwd, f32(s), f32(t)), dgrad

        net = self.backbone
        fwd, shift, dgrad = fold_stem(net.conv1, net.bn1)
        ops = {"stem": (f32(fwd), f32(shift), f32(dgrad)), "blocks": [], "ones": torch.ones(512 * EXPANSION, device=dev)}
        for b in net.blocks():
            d = dict(stride=b.stride, down=None, down_d=None)
            for name, bn in (("conv1", b.bn1), ("conv2", b.bn2), ("conv3", b.bn3)):
                d[name], d[name + "_d"] = conv(getattr(b, name), bn)
            if b.downsample is not None:
                d["down"], d["down_d"] = conv(b.downsample[0], b.downsample[1])
            ops["blocks"].append(d)
        return ops

    def forward(self, gen, tar, use_mean=True, metric="l2", *, _trace=None):
        """gen, tar: [B, 3, H, W] fp32 on the HIP device, H and W in 193 .. 224 -> the loss, 0-dim with `use_mean` and [B] without, differentiable with respect
        to gen.  `_trace` (a dict) receives 'features' (fp32 [2B, 2048], gen rows first) and the decoded 'stem' output."""
        gc, tc = image_pair("ExpressionLoss", ("gen", "tar"), gen, tar)
        if metric not in L.EMOTION_METRICS:
            raise ValueError("Unknown metric {}".format(metric))      # ExpressionLoss.py:60
        B, _, H, W = gen.shape
        if B < 1 or not (MIN_SIZE <= H <= MAX_SIZE and MIN_SIZE <= W <= MAX_SIZE):
            raise L.SmirkHipError(f"ExpressionLoss: H and W must be {MIN_SIZE} .. {MAX_SIZE}, the sizes whose final map is {FINAL} x {FINAL} (the reference's "
                                  f"AvgPool2d({FINAL}) yields [B, 2048] only then), and B >= 1; got {tuple(gen.shape)}")
        if 2 * B * ((H + 1) // 2) * ((W + 1) // 2) * L.EMOTION_STEM_COUT * 4 >= LIMIT_BYTES:       # refused here, before the first launch
            raise L.SmirkHipError(f"ExpressionLoss: the largest activation [2 x {B}, {(H + 1) // 2}, {(W + 1) // 2}, 64] reaches 2 GiB, the limit of the "
                                  "convolution entries; split the batch")
        L.raise_if_range_tripped("ExpressionLoss")
        keep = torch.is_grad_enabled() and gen.requires_grad
        return _Emotion.apply(self, gc, tc, metric, bool(use_mean), keep, _trace)
