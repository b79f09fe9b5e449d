"""The law of SmirkGenerator.precision = "f16x1" (a plain module shared by tests/test_generator_x1_cpu.py and tests/test_generator_x1_gpu.py).

forward() is a float64 torch-CPU eval-mode forward over a state dict with the keys of oracle.generator_ref, driven by the per-level arithmetic that
smirk_generator_arith reports (arith(), below): a layer the query calls F16X1 sees its activations and its weights through `.float().half().double()` — the hi
half of the split-fp16 pair, which is all the one-MFMA product reads — and every other layer sees them unrounded.  Accumulation, the BatchNorm scale / shift, the
bias, the residual sum, the pooling and the sigmoid are float64 (the library accumulates in fp32 and stores (hi, lo) pairs of ~22 bits: both are far below the
11-bit operand rounding this law is about).  ConvTranspose2d and the convolution after it are two layers, each with its own rounding.

compose=True is a SECOND emulation, of what the library does where it composes a level's ConvTranspose2d into the convolution that follows: the
product of the two weights is formed first (in fp32, from unrounded weights), then rounded once; the transposed convolution's bias goes through the unrounded
convolution weights.  The library rounds once, forward() by default twice; the two are samples of the same rounding process and the tests hold them to the
same bound.
"""
import ctypes as C

import torch
import torch.nn.functional as F

ARITH = ("F32", "F16X3", "F16X1")                                     # SMIRK_PRECISION_*, by code (include/smirk_hip.h)


def arith(weights):
    """smirk_generator_arith for a SmirkGeneratorWeights -> dict(x1_from, levels=[4 names], deep=name), or the error code"""
    from smirk_amd import _lib as L
    x1_from, deep, levels = C.c_int32(-1), C.c_int32(-1), (C.c_int32 * 4)(-1, -1, -1, -1)
    rc = L.lib().smirk_generator_arith(weights, C.byref(x1_from), levels, C.byref(deep))
    if rc:
        return rc
    return dict(x1_from=x1_from.value, levels=[ARITH[v] for v in levels], deep=ARITH[deep.value])


def _r(t, x1):
    return t.float().half().double() if x1 else t


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], training=False, eps=1e-5)


def _block(x, sd, mod, nm, x1):
    x = F.relu(_bn(F.conv2d(_r(x, x1), _r(sd[f"{mod}.{nm}conv1.weight"], x1), padding=1), sd, f"{mod}.{nm}norm1"))
    return F.relu(_bn(F.conv2d(_r(x, x1), _r(sd[f"{mod}.{nm}conv2.weight"], x1), padding=1), sd, f"{mod}.{nm}norm2"))


def _composed_first_conv(d, skip, wup, bup, w3, x1):
    """conv3x3(cat(ConvTranspose2d(d), skip); w3) with the ConvTranspose2d composed into the convolution: per output parity class (dy, dx) a 2 x 2 convolution of the
    coarse tensor with Weff[class] = sum over the fine taps of w3[:, :c, tap] . wup[:, :, sub], rounded ONCE."""
    c = w3.shape[0]
    w3a, w3b = w3[:, :c], w3[:, c:]
    B, _, h, w = d.shape
    out = F.conv2d(_r(skip, x1), _r(w3b, x1), padding=1)
    out = out + F.conv2d(bup.view(1, c, 1, 1).expand(B, c, 2 * h, 2 * w), w3a, padding=1)      # the bias image through the zero-padded convolution
    dp = F.pad(_r(d, x1), (1, 1, 1, 1))
    for dy in (0, 1):
        for dx in (0, 1):
            weff = torch.zeros(c, d.shape[1], 2, 2, dtype=torch.float32)
            for fy in (-1, 0, 1):
                for fx in (-1, 0, 1):
                    ta, tb = ((dy + fy) >> 1) - (dy - 1), ((dx + fx) >> 1) - (dx - 1)
                    sub = wup[:, :, (dy + fy) & 1, (dx + fx) & 1]                             # [ci, cu]
                    weff[:, :, ta, tb] += w3a[:, :, fy + 1, fx + 1].float() @ sub.float().t()
            full = F.conv2d(dp, _r(weff.double(), x1))                                          # [B, c, h + 1, w + 1]: entry (i, j) covers coarse rows i - 1, i
            out[:, :, dy::2, dx::2] += full[:, :, dy:dy + h, dx:dx + w]
    return out


def forward(sd, x, res_blocks, ar, compose=False, taps=None):
    """sd: float64 state dict; x [B, C, H, W] float64; ar: arith(); -> the sigmoid image, float64"""
    t = taps if taps is not None else {}
    lv = [a == "F16X1" for a in ar["levels"]]
    deep = ar["deep"] == "F16X1"
    skips, cur = [], x
    for l in range(4):
        e = _block(cur, sd, f"encoder{l + 1}", f"enc{l + 1}", lv[l])
        t[f"enc{l + 1}"] = e
        skips.append(e)
        cur = F.max_pool2d(e, 2, 2)
    b = _block(cur, sd, "bottleneck", "bottleneck", deep)
    t["bottleneck"] = b
    for k in range(res_blocks):
        p = f"resnet_blocks.{k}.conv_block"
        y = F.conv2d(F.pad(_r(b, deep), (1, 1, 1, 1), mode="reflect"), _r(sd[p + ".1.weight"], deep))
        y = F.relu(_bn(y, sd, p + ".2"))
        y = F.conv2d(F.pad(_r(y, deep), (1, 1, 1, 1), mode="reflect"), _r(sd[p + ".5.weight"], deep))
        b = b + _bn(y, sd, p + ".6")
    t["res"] = b
    d = b
    for l in (3, 2, 1, 0):
        lvl, x1 = l + 1, lv[l]
        mod, nm = f"decoder{lvl}", f"dec{lvl}"
        wup, bup, w3 = sd[f"upconv{lvl}.weight"], sd[f"upconv{lvl}.bias"], sd[f"{mod}.{nm}conv1.weight"]
        if compose and x1:
            z = _composed_first_conv(d, skips[l], wup, bup, w3, x1)
        else:
            up = F.conv_transpose2d(_r(d, x1), _r(wup, x1), bup, stride=2)
            z = F.conv2d(_r(torch.cat((up, skips[l]), 1), x1), _r(w3, x1), padding=1)
        z = F.relu(_bn(z, sd, f"{mod}.{nm}norm1"))
        d = F.relu(_bn(F.conv2d(_r(z, x1), _r(sd[f"{mod}.{nm}conv2.weight"], x1), padding=1), sd, f"{mod}.{nm}norm2"))
        t[nm] = d
    return torch.sigmoid(F.conv2d(d, sd["conv.weight"], sd["conv.bias"]))


def double_state_dict(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
