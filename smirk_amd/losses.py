"""The loss head of the reference trainer's first path (smirk_trainer.py:56-72, 97-101, 134-154) and the cycle loss (:304-313) on the MI355X.

    first = FirstPathLoss(config.train.loss_weights, optimize_shape, optimize_expression, enable_fuse_generator)
    loss, terms = first(encoder_output, flame_output['landmarks_fan'], flame_output['landmarks_mp'], batch, reconstructed_img=reconstructed_img,
                        extra={'perceptual_vgg_loss': vgg})             # two launches of libsmirk_hip.so (smirk_amd/csrc/losses.hip)
    loss.backward()                                                     # one launch
    losses = terms.as_dict()                                            # ONE device-to-host copy for all terms

The reference computes these terms in eager torch: a boolean-mask index (a `nonzero`, i.e. a host stall), `torch.sum(valid) == 0` (another), one `.item()` per
entry of `losses` (nine more) and about six passes over a [B, 3, 224, 224] tensor for the L1 term.  Here every term is a partial sum in float64 over chunks
whose layout depends on the shapes alone (no atomics: two calls return the same bits), the flags are read on the device, and nothing waits for the host.

`weighted_loss` is the general bridge (any mix of squared-error row terms and one-norm image terms); `cycle_loss` restates smirk_amd.cycle.cycle_loss over
it.  Networks that produce further terms — VGG, emotion, MICA — are not part of this package: their scalars enter `FirstPathLoss` through `extra`.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

CHUNK, MAX_TERMS = L.LOSS_CHUNK, L.LOSS_MAX_TERMS
WEIGHT_KEYS = ("landmark_loss", "perceptual_vgg_loss", "reconstruction_loss", "emotion_loss", "jaw_regularization", "expression_regularization",
               "shape_regularization", "cycle_loss", "mica_loss")                      # configs/config_train.yaml train.loss_weights
FUSED_TERMS = ("landmark_loss_fan", "landmark_loss_mp", "expression_regularization", "shape_regularization", "jaw_regularization", "reconstruction_loss")
EXTRA_TERMS = ("perceptual_vgg_loss", "emotion_loss", "mica_loss")
TERM_NAMES = FUSED_TERMS + EXTRA_TERMS                                                  # the keys of the trainer's `losses` dict, in its order


class Term:
    """One term of `weighted_loss`.  kind "mse": squared error over the first `cols` columns (default: all) of the rows of `pred` [rows, ...] (trailing
    dimensions flattened) whose entry in `flags` [rows] (bool or uint8; default: all) is set, against `target` (None = zeros); its value is F.mse_loss of that
    slice, 0 when the slice is empty.  kind "l1_image": F.l1_loss of `pred` [B, C, H, W] against `target`; with `loss_img` the call also returns the channel
    mean of |pred - target| [B, 1, H, W]."""

    def __init__(self, pred, target=None, flags=None, cols=None, weight=1.0, kind="mse", loss_img=False):
        self.pred, self.target, self.flags, self.cols, self.weight, self.kind, self.loss_img = pred, target, flags, cols, float(weight), kind, bool(loss_img)


def _prepare(terms):
    """Host-side validation and the fp32-contiguous, 16-byte aligned operands of every term.  Raises before anything touches the device."""
    terms = list(terms)
    if not 1 <= len(terms) <= MAX_TERMS:
        raise L.SmirkHipError(f"weighted_loss takes 1..{MAX_TERMS} terms, got {len(terms)}")
    for i, t in enumerate(terms):
        if t.kind not in ("mse", "l1_image"):
            raise L.SmirkHipError(f"term {i}: unknown kind {t.kind!r}")
        for name, x in (("pred", t.pred), ("target", t.target), ("flags", t.flags)):
            if x is None and name != "pred":
                continue
            if not torch.is_tensor(x):
                raise L.SmirkHipError(f"term {i}: {name} is not a tensor")
            if not x.is_cuda:
                raise L.SmirkHipError(f"smirk_amd runs on the MI355X HIP device only: term {i}: {name} is a CPU tensor (no CPU fallback exists)")
            if name != "pred" and x.requires_grad:
                raise L.SmirkHipError(f"term {i}: {name} requires grad; targets and flags are constants of the loss")
        if t.pred.dim() < 1 or t.pred.numel() == 0:
            raise L.SmirkHipError(f"term {i}: empty prediction")
        if t.target is not None and tuple(t.target.shape) != tuple(t.pred.shape):
            raise L.SmirkHipError(f"term {i}: target {tuple(t.target.shape)} does not match the prediction {tuple(t.pred.shape)}")
        rows = t.pred.shape[0]
        if t.kind == "l1_image":
            if t.pred.dim() != 4 or t.target is None or t.flags is not None or t.cols is not None:
                raise L.SmirkHipError(f"term {i}: an l1_image term takes a [B, C, H, W] prediction and a target, and neither flags nor cols")
        else:
            stride = t.pred.numel() // rows
            if t.cols is not None and not 1 <= int(t.cols) <= stride:
                raise L.SmirkHipError(f"term {i}: cols={t.cols} outside 1..{stride}")
            if t.loss_img:
                raise L.SmirkHipError(f"term {i}: loss_img belongs to l1_image terms")
            if t.flags is not None:
                if t.flags.dtype not in (torch.bool, torch.uint8):
                    raise L.SmirkHipError(f"term {i}: flags must be torch.bool or torch.uint8, got {t.flags.dtype}")
                if t.flags.numel() != rows:
                    raise L.SmirkHipError(f"term {i}: {t.flags.numel()} flags for {rows} rows")
    dev = terms[0].pred.device
    ops = []
    for i, t in enumerate(terms):
        if t.pred.device != dev or any(x is not None and x.device != dev for x in (t.target, t.flags)):
            raise L.SmirkHipError(f"term {i}: tensors on different devices")
        flags = None
        if t.flags is not None:
            flags = t.flags.reshape(-1).contiguous()
            flags = flags.view(torch.uint8) if flags.dtype == torch.bool else flags
        ops.append((L.aligned16(t.pred.detach()), None if t.target is None else L.aligned16(t.target), flags))
    return terms, ops


def _structs(terms, ops, loss_imgs, grads):
    arr = (L.SmirkLossTerm * len(terms))()
    for s, t, (pred, target, flags), img, grad in zip(arr, terms, ops, loss_imgs, grads):
        rows = pred.shape[0]
        stride = pred.numel() // rows
        s.pred, s.target = pred.data_ptr(), None if target is None else target.data_ptr()
        s.row_flags = None if flags is None else flags.data_ptr()
        s.rows, s.row_stride, s.cols = rows, stride, stride if t.cols is None else int(t.cols)
        s.kind = L.LOSS_ABS_IMAGE if t.kind == "l1_image" else L.LOSS_SQUARE
        s.C, s.HW = (pred.shape[1], pred.shape[2] * pred.shape[3]) if t.kind == "l1_image" else (0, 0)
        s.weight = t.weight
        s.loss_img = None if img is None else img.data_ptr()
        s.grad = None if grad is None else grad.data_ptr()
    return arr


_ws = L.Workspace()


class _WeightedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, terms, ops, *preds):
        lib, dev = L.lib(), ops[0][0].device
        n = len(terms)
        out_terms, total = torch.empty(n, device=dev), torch.empty((), device=dev)
        imgs = [torch.empty(p.shape[0], 1, p.shape[2], p.shape[3], device=dev) if t.loss_img else None for t, (p, _, _) in zip(terms, ops)]
        arr = _structs(terms, ops, imgs, [None] * n)
        ws = _ws.get(lib.smirk_loss_workspace_bytes(arr, n), dev)
        L.check(lib.smirk_loss_forward(arr, n, L.ptr(out_terms), L.ptr(total), C.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr()))
        # the operands go through save_for_backward: a detached view shares its version counter with the caller's tensor, so an in-place change of a
        # prediction between forward and backward raises torch's error instead of being used silently (copies made by _prepare hold the forward's values)
        ctx.save_for_backward(*[x for op in ops for x in op])
        ctx.terms, ctx.shapes = terms, [(p.shape, p.dtype) for p in preds]
        imgs = tuple(i for i in imgs if i is not None)
        ctx.mark_non_differentiable(out_terms, *imgs)
        return (total, out_terms) + imgs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, *_):
        lib, terms, saved = L.lib(), ctx.terms, ctx.saved_tensors
        ops = [tuple(saved[3 * i:3 * i + 3]) for i in range(len(terms))]
        n, dev = len(terms), ops[0][0].device
        need = ctx.needs_input_grad[2:]
        if not any(need):
            return (None,) * (2 + n)
        grads = [torch.empty_like(p) if w else None for (p, _, _), w in zip(ops, need)]
        arr = _structs(terms, ops, [None] * n, grads)
        ws = _ws.get(lib.smirk_loss_workspace_bytes(arr, n), dev)
        g = L.as_f32c(g_total)
        L.check(lib.smirk_loss_backward(arr, n, L.ptr(g), C.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr()))
        return (None, None) + tuple(None if x is None else x.view(s).to(d) for x, (s, d) in zip(grads, ctx.shapes))


def weighted_loss(terms, return_loss_img=False):
    """total = sum of weight * term over `terms` (a sequence of 1..MAX_TERMS `Term`s) in two launches, differentiable with respect to every prediction
    that requires grad (one launch, reading the upstream gradient on the device).  Returns (total, terms_tensor): a 0-dim fp32 tensor and the unweighted
    fp32 terms [len(terms)] as the trainer logs them (not differentiable); with `return_loss_img` a third entry, the list of the loss_img of each term
    (None where not asked for)."""
    terms, ops = _prepare(terms)
    out = _WeightedLoss.apply(terms, ops, *[t.pred for t in terms])
    if not return_loss_img:
        return out[0], out[1]
    imgs = iter(out[2:])
    return out[0], out[1], [next(imgs) if t.loss_img else None for t in terms]


class LossTerms:
    """The terms of one loss call: `names`, and `values`, the fp32 device tensor that holds them in that order.  `zeros` names the entries the trainer reports
    as the Python int 0 (terms that were switched off).  `as_dict()` makes ONE device-to-host copy for all of them, where the trainer calls `.item()` per entry
    (smirk_trainer.py:156-157).  `loss_img`: the [B, 1, H, W] channel mean of the L1 term when a reconstruction was given (smirk_trainer.py:100), else None."""

    def __init__(self, names, values, zeros=(), loss_img=None):
        self.names, self.values, self.zeros, self.loss_img = tuple(names), values, tuple(zeros), loss_img

    def as_dict(self):
        d = dict(zip(self.names, self.values.detach().tolist()))
        d.update({k: 0 for k in self.zeros})
        return {k: d[k] for k in [k for k in TERM_NAMES if k in d] + [k for k in d if k not in TERM_NAMES]}      # the trainer's keys in the trainer's order


def effective_weights(loss_weights, optimize_shape=True, optimize_expression=True, enable_fuse_generator=True):
    """The factor each entry of the trainer's `losses` has in loss_first_path (smirk_trainer.py:134-154): its configured weight, or 0 where its group is dropped."""
    unknown = set(loss_weights) - set(WEIGHT_KEYS)
    missing = set(WEIGHT_KEYS) - {"cycle_loss"} - set(loss_weights)
    if unknown or missing:
        raise L.SmirkHipError(f"loss_weights: unknown keys {sorted(unknown)}, missing keys {sorted(missing)} (expected those of configs/config_train.yaml)")
    w = {k: float(v) for k, v in loss_weights.items()}
    s, e, g = float(bool(optimize_shape)), float(bool(optimize_expression)), float(bool(enable_fuse_generator))
    return {"landmark_loss_fan": w["landmark_loss"], "landmark_loss_mp": w["landmark_loss"],
            "expression_regularization": e * w["expression_regularization"], "jaw_regularization": e * w["jaw_regularization"],
            "shape_regularization": s * w["shape_regularization"], "mica_loss": s * w["mica_loss"],
            "reconstruction_loss": g * w["reconstruction_loss"], "perceptual_vgg_loss": g * w["perceptual_vgg_loss"], "emotion_loss": g * w["emotion_loss"]}


class FirstPathLoss:
    """smirk_trainer.py:56-72, 97-101, 134-154.  `loss_weights`: a mapping with the keys of configs/config_train.yaml (train.loss_weights); the three switches
    are config.train.optimize_shape / optimize_expression and config.arch.enable_fuse_generator."""

    def __init__(self, loss_weights, optimize_shape=True, optimize_expression=True, enable_fuse_generator=True):
        self.enable_fuse_generator = bool(enable_fuse_generator)
        self.weights = effective_weights(loss_weights, optimize_shape, optimize_expression, enable_fuse_generator)

    def __call__(self, encoder_output, landmarks_fan, landmarks_mp, batch, reconstructed_img=None, base_output=None, extra=None):
        """encoder_output: the SmirkEncoder dict; landmarks_fan [B, 68, 2] / landmarks_mp [B, 105, 2]: the projected FLAME landmarks; batch: 'landmarks_fan',
        'flag_landmarks_fan' [B], 'landmarks_mp' and, with a reconstruction, 'img'; base_output: the base encoder's dict (use_base_model_for_regularization) or
        None for regularisation towards zero; extra: {name: scalar tensor} for perceptual_vgg_loss / emotion_loss / mica_loss computed elsewhere.
        Returns (loss_first_path, LossTerms)."""
        extra = dict(extra or {})
        if set(extra) - set(EXTRA_TERMS):
            raise L.SmirkHipError(f"extra: unknown terms {sorted(set(extra) - set(EXTRA_TERMS))} (expected a subset of {EXTRA_TERMS})")
        for k, v in extra.items():
            if not torch.is_tensor(v) or v.numel() != 1:
                raise L.SmirkHipError(f"extra[{k!r}] must be a scalar tensor")
            if not v.is_cuda:
                raise L.SmirkHipError(f"smirk_amd runs on the MI355X HIP device only: extra[{k!r}] is a CPU tensor (no CPU fallback exists)")
        if landmarks_fan.dim() != 3 or landmarks_fan.shape[1] < 17:
            raise L.SmirkHipError(f"landmarks_fan: expected [B, >= 17, 2], got {tuple(landmarks_fan.shape)}")
        w, base = self.weights, base_output or {}
        named = [("landmark_loss_fan", Term(landmarks_fan, batch["landmarks_fan"], flags=batch["flag_landmarks_fan"], cols=17 * landmarks_fan.shape[2],
                                            weight=w["landmark_loss_fan"])),                                                  # :57-58
                 ("landmark_loss_mp", Term(landmarks_mp, batch["landmarks_mp"], weight=w["landmark_loss_mp"]))]               # :60
        for name, key in (("expression_regularization", "expression_params"), ("shape_regularization", "shape_params"), ("jaw_regularization", "jaw_params")):
            named.append((name, Term(encoder_output[key], base.get(key), weight=w[name])))                                    # :64-72
        with_img = self.enable_fuse_generator and reconstructed_img is not None
        if with_img:
            named.append(("reconstruction_loss", Term(reconstructed_img, batch["img"], weight=w["reconstruction_loss"], kind="l1_image", loss_img=True)))   # :97-101
        total, values, imgs = weighted_loss([t for _, t in named], return_loss_img=True)
        names = [n for n, _ in named]
        if extra:                                                                      # terms computed elsewhere: added with their weights in eager torch
            xs = [extra[k].reshape(()).to(total.dtype) for k in EXTRA_TERMS if k in extra]
            for k, x in zip([k for k in EXTRA_TERMS if k in extra], xs):
                total = total + w[k] * x
            values = torch.cat([values, torch.stack(xs).detach()])
            names += [k for k in EXTRA_TERMS if k in extra]
        return total, LossTerms(names, values, zeros=[k for k in TERM_NAMES if k not in names], loss_img=imgs[-1] if with_img else None)


def cycle_loss(recon_feats, flame_feats, use_eyelids=True, generator_frozen=False):
    """smirk_trainer.py:304-313: the value of smirk_amd.cycle.cycle_loss, through `weighted_loss` (two launches instead of about a dozen)."""
    terms = [Term(recon_feats["expression_params"], flame_feats["expression_params"], weight=1.0),
             Term(recon_feats["jaw_params"], flame_feats["jaw_params"], weight=10.0)]
    if use_eyelids:
        terms.append(Term(recon_feats["eyelid_params"], flame_feats["eyelid_params"], weight=10.0))
    if not generator_frozen:
        terms.append(Term(recon_feats["shape_params"], flame_feats["shape_params"], weight=1.0))
    return weighted_loss(terms)[0]
