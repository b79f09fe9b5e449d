"""Image gradient through one FROZEN SmirkEncoder backbone (+ its Linear head) in .eval() on the HIP path: the even steps of the reference's training run.

`base_trainer.py:258-268` sets `freeze_encoder_in_second_path = (batch_idx % 2 == 0)`; on those steps `smirk_trainer.py:367-368` calls `utils.freeze_module`
(src/utils/utils.py:46-51: `requires_grad_(False)` on every parameter AND `module.eval()`) on the three sub-encoders, `step2` runs
`self.smirk_encoder(reconstructed_img_2nd_path)` (:300) on an image that requires grad and back-propagates the cycle loss through the frozen encoder into the
generator (:375).  BatchNorm works from the running statistics, which do not move; no parameter gets a gradient.

`MobileNetV3Features.run` comes here when the backbone is in .eval(), autograd is on, the image requires grad, no parameter of the backbone or of its head
requires grad, the precision is "f16x3" and the call carries the head.  One torch.autograd.Function per backbone.

Forward — one launch per conv + BatchNorm(eval) + ReLU unit, with the folded (scale, shift) of `MobileNetV3Features._pack()`: `smirk_stem_conv_s2_split16`,
`smirk_dwconv3x3_split16`, `smirk_conv_igemm_f16x3` / `_f16x1` (act, residual), `smirk_gap_linear_split16`, `smirk_expression_clamps`, all through the op
wrappers and the head / clamp frame of encoder_train.py (the train-mode schedule runs the same entries bare, without scale, shift and ReLU).  The tape holds the
post-activation outputs of the ReLU units only (a ReLU mask is `y > 0`); no pre-BatchNorm tensor exists.  A frozen head has no weight gradient, so no pooled
vectors are kept: heads of at most 64 outputs (pose, expression) pass no workspace and run pool + Linear as one launch.

Backward — data gradients only.  Every BatchNorm is the factor s[c] = gamma / sqrt(running_var + eps).  A unit without ReLU (bn3 of an inverted-residual
block, bn2 of the depthwise-separable block) has it folded into the packed transposed weight of its pointwise data gradient; a unit with ReLU has factor and
mask applied by the kernel that produces its gradient (`smirk_dwconv3x3_eval_backward_split16`, `smirk_relu_scale_backward_split16`,
csrc/encoder_eval_grad.hip):
    "ir"  3 launches: pointwise data gradient of conv_pwl -> fused depthwise kernel -> pointwise data gradient of conv_pw (+ skip gradient as residual)
    "ds"  2 launches: pointwise data gradient of conv_pw -> fused depthwise kernel (+ skip gradient as `add`; the stem's mask and factor ride in its store)
    "cn"  2 launches: mask kernel -> pointwise data gradient
    stem `smirk_stem_conv_s2_dgrad_split16`; head `smirk_gap_linear_backward_split16` with NULL dw / db.
The transposed / folded weights are cached on the backbone per parameter and buffer version (`_wcache`, dropped on every train() <-> eval() transition like
the forward's folded weights).  `train_arith` selects the arithmetic of the pointwise convolutions, forward and data gradient, as in BackboneTrainFunction.

Not built: recomputing the expand / depthwise activations inside a fused MBConv backward (the tape keeps them), and HIP-graph capture of the even step
(`cycle.graph_cycle_modules` captures the train-mode path only).
"""
import torch

from . import _lib as L
from .encoder_train import _EncOps, _pw_t, backbone_image, clamp_grad, head_forward


class _EvalOps(_EncOps):
    """the shared op wrappers plus the two backward kernels that only the frozen schedule runs"""

    def depthwise_backward(self, dy, y_out, s_out, w9c, add, y_in, s_in, shape, stride):
        B, H, W, C = shape
        dx = torch.empty(B, H, W, C, device=self.dev)
        P = L.ptr
        L.check(self.lib.smirk_dwconv3x3_eval_backward_split16(P(dy), P(y_out), P(s_out), P(w9c), P(add, allow_none=True), P(y_in, allow_none=True),
                                                               P(s_in, allow_none=True), P(dx), B, H, W, C, stride, self.st))
        return dx

    def relu_scale_backward(self, dy, y, s):
        C = y.shape[-1]
        dz = torch.empty_like(y)
        L.check(self.lib.smirk_relu_scale_backward_split16(L.ptr(dy), L.ptr(y), L.ptr(s), L.ptr(dz), y.numel() // C, C, self.st))
        return dz


def _backward_weights(backbone, P):
    """{(stage, block): transposed pointwise weights, folded where the unit has no ReLU}, cached per parameter / buffer version (backbone._packed_key)"""
    hit = backbone._wcache.get("eval_grad")
    if hit is not None and hit[0] == backbone._packed_key:
        return hit[1]
    T = {}
    for si, st in enumerate(backbone.blocks):
        for bi, blk in enumerate(st):
            pk = P[(si, bi)]
            if blk.kind == "ds":
                T[(si, bi)] = dict(pw=_pw_t(blk.conv_pw, pk["pw"][1]))
            elif blk.kind == "ir":
                T[(si, bi)] = dict(pw=_pw_t(blk.conv_pw), pwl=_pw_t(blk.conv_pwl, pk["pwl"][1]))
            else:
                T[(si, bi)] = dict(pw=_pw_t(blk.conv))
    backbone._wcache["eval_grad"] = (backbone._packed_key, T)
    return T


class BackboneEvalGradFunction(torch.autograd.Function):
    """(backbone in .eval() with every parameter frozen, head Linear, clamp_n_exp, img) -> head output [B, n_out] (ExpressionEncoder clamps applied when
    clamp_n_exp >= 0); backward returns dL/d img only."""

    @staticmethod
    def forward(ctx, backbone, head, clamp_n_exp, img):
        img = backbone_image(img)
        B, _, H, W = img.shape
        ctx.arith = getattr(backbone, "train_arith", "f16x3")
        ops = _EvalOps(img.device, ctx.arith)
        lib, st = ops.lib, ops.st
        P = backbone._pack()
        if not backbone._split:
            raise L.SmirkHipError("the eval-mode image gradient runs in the split-fp16 precision only")
        T = _backward_weights(backbone, P)
        trace = getattr(backbone, "_trace", None)               # tests: the post-activation outputs of the ReLU units, in unit order
        keep = (lambda y: y) if trace is None else (lambda y: (trace.append(y), y)[1])
        wst, s0, b0 = P["stem"]
        c0 = wst.shape[0]
        x = torch.empty(B, (H + 1) // 2, (W + 1) // 2, c0, device=img.device)
        L.check(lib.smirk_stem_conv_s2_split16(L.ptr(img), L.ptr(wst), L.ptr(s0), L.ptr(b0), L.ptr(x), B, H, W, c0, st))
        keep(x)
        tape, relu_in = [("stem", wst)], (x, s0)              # the stem's (output, factor): its mask and factor are applied by the FIRST block's backward
        for si, stage in enumerate(backbone.blocks):
            for bi, blk in enumerate(stage):
                pk, tk = P[(si, bi)], T[(si, bi)]
                if blk.kind == "ds":
                    wdw, s1, b1 = pk["dw"]
                    y1 = keep(ops.depthwise(x, wdw, blk.stride, s1, b1, relu=True))
                    w2, s2, b2 = pk["pw"]
                    out = ops.pointwise(y1, w2, blk.conv_pw.out_channels, s2, b2, residual=x if blk.skip else None)
                    tape.append(("ds", blk, (tuple(x.shape), y1, s1, wdw, tk["pw"], relu_in)))
                elif blk.kind == "ir":
                    w1, s1, b1 = pk["pw"]
                    y1 = keep(ops.pointwise(x, w1, blk.conv_pw.out_channels, s1, b1, relu=True))
                    wdw, s2, b2 = pk["dw"]
                    y2 = keep(ops.depthwise(y1, wdw, blk.stride, s2, b2, relu=True))
                    w3, s3, b3 = pk["pwl"]
                    out = ops.pointwise(y2, w3, blk.conv_pwl.out_channels, s3, b3, residual=x if blk.skip else None)
                    tape.append(("ir", blk, (y1, s1, y2, s2, wdw, tk["pw"], tk["pwl"], relu_in)))
                else:
                    w1, s1, b1 = pk["pw"]
                    out = keep(ops.pointwise(x, w1, blk.conv.out_channels, s1, b1, relu=True))
                    tape.append(("cn", blk, (out, s1, tk["pw"], relu_in)))
                relu_in = None
                x = out
        out, hw_, _, raw, dims = head_forward(ops, x, head, clamp_n_exp, keep_pooled=False)      # the head is frozen: no pooled vectors kept
        ctx.tape = tape
        ctx.headrec = (hw_, raw, clamp_n_exp, dims)
        ctx.img_shape = (B, H, W)
        return out

    @staticmethod
    def backward(ctx, gout):
        if ctx.tape is None:
            raise L.second_backward("BackboneEvalGradFunction", "activations")
        tape = ctx.tape
        hw_, raw, n_exp, (B, hf, wf, Cf, N) = ctx.headrec
        ops = _EvalOps(raw.device, ctx.arith)
        lib, st = ops.lib, ops.st
        gout = clamp_grad(L.as_f32c(gout), raw, n_exp)
        g = torch.empty(B, hf, wf, Cf, device=raw.device)
        L.check(lib.smirk_gap_linear_backward_split16(L.ptr(gout), L.ptr(hw_), None, None, None, L.ptr(g), B, hf * wf, Cf, N, st))
        dimg = None
        for rec in reversed(tape):
            kind = rec[0]
            if kind == "cn":
                _, blk, (y, s1, wt, relu_in) = rec
                g = ops.pointwise(ops.relu_scale_backward(g, y, s1), wt, blk.conv.in_channels)
                if relu_in is not None:
                    g = ops.relu_scale_backward(g, *relu_in)
            elif kind == "ir":
                _, blk, (y1, s1, y2, s2, wdw, wt1, wt3, relu_in) = rec
                dy2 = ops.pointwise(g, wt3, blk.conv_pwl.in_channels)
                dz1 = ops.depthwise_backward(dy2, y2, s2, wdw, None, y1, s1, y1.shape, blk.stride)
                g = ops.pointwise(dz1, wt1, blk.conv_pw.in_channels, residual=g if blk.skip else None)
                if relu_in is not None:
                    g = ops.relu_scale_backward(g, *relu_in)
            elif kind == "ds":
                _, blk, (xshape, y1, s1, wdw, wt, relu_in) = rec
                dy1 = ops.pointwise(g, wt, blk.conv_pw.in_channels)
                y_in, s_in = relu_in if relu_in is not None else (None, None)
                g = ops.depthwise_backward(dy1, y1, s1, wdw, g if blk.skip else None, y_in, s_in, xshape, blk.stride)
            else:
                _, wst = rec
                Bi, H, W = ctx.img_shape
                dimg = torch.empty(Bi, 3, H, W, device=raw.device)
                L.check(lib.smirk_stem_conv_s2_dgrad_split16(L.ptr(g), L.ptr(wst), L.ptr(dimg), Bi, H, W, wst.shape[0], st))
        ctx.tape = ctx.headrec = None
        return None, None, None, dimg
