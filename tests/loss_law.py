"""The law smirk_amd.losses has to follow, in plain torch: the lines of smirk_trainer.py:56-72 (landmark and regularisation terms), :97-101 (L1 term and its
`loss_img`), :134-154 (grouping, switches, total) and :304-313 (cycle loss), written as the trainer writes them.  `head_dtype=torch.float64` evaluates the
loss head in float64 on whatever the inputs are (autograd hands the gradients back in the inputs' dtype): the arbiter of the GPU tests.  Seeded input makers
for both test files.  No test in here."""
import torch
import torch.nn.functional as F

WEIGHTS_TRAIN = dict(landmark_loss=100.0, perceptual_vgg_loss=10.0, reconstruction_loss=10.0, emotion_loss=0.0, jaw_regularization=1e-2,
                     expression_regularization=1e-3, shape_regularization=100, cycle_loss=1.0, mica_loss=0)           # configs/config_train.yaml
WEIGHTS_PRETRAIN = dict(WEIGHTS_TRAIN, perceptual_vgg_loss=0.0, reconstruction_loss=0.0, cycle_loss=0.0, mica_loss=10)  # configs/config_pretrain.yaml
LOSS_KEYS = ("landmark_loss_fan", "landmark_loss_mp", "expression_regularization", "shape_regularization", "jaw_regularization", "reconstruction_loss",
             "perceptual_vgg_loss", "emotion_loss", "mica_loss")                                                       # keys of the trainer's `losses`


def total_law(losses, w, optimize_shape, optimize_expression, enable_fuse_generator):
    """smirk_trainer.py:134-154 on a finished `losses` dict."""
    shape_losses = losses['shape_regularization'] * w['shape_regularization'] + losses['mica_loss'] * w['mica_loss']
    expression_losses = losses['expression_regularization'] * w['expression_regularization'] + losses['jaw_regularization'] * w['jaw_regularization']
    landmark_losses = losses['landmark_loss_fan'] * w['landmark_loss'] + losses['landmark_loss_mp'] * w['landmark_loss']
    fuse_generator_losses = losses['perceptual_vgg_loss'] * w['perceptual_vgg_loss'] + losses['reconstruction_loss'] * w['reconstruction_loss'] + \
        losses['emotion_loss'] * w['emotion_loss']
    return ((shape_losses if optimize_shape else 0) + (expression_losses if optimize_expression else 0) + (landmark_losses) +
            (fuse_generator_losses if enable_fuse_generator else 0))


def first_path_law(encoder_output, landmarks_fan, landmarks_mp, batch, w, reconstructed_img=None, base_output=None, extra=None, optimize_shape=True,
                   optimize_expression=True, enable_fuse_generator=True, head_dtype=None):
    """smirk_trainer.py:56-72, 97-101, 134-154.  Returns (loss_first_path, losses, loss_img); entries of `losses` are tensors, or the int 0 where the
    trainer has one."""
    c = (lambda t: t) if head_dtype is None else (lambda t: t.to(head_dtype))
    extra = extra or {}
    losses = {}
    valid_landmarks = batch['flag_landmarks_fan']
    losses['landmark_loss_fan'] = 0 if torch.sum(valid_landmarks) == 0 else F.mse_loss(c(landmarks_fan)[valid_landmarks, :17],
                                                                                         c(batch['landmarks_fan'])[valid_landmarks, :17])
    losses['landmark_loss_mp'] = F.mse_loss(c(landmarks_mp), c(batch['landmarks_mp']))
    for name, key in (('expression_regularization', 'expression_params'), ('shape_regularization', 'shape_params'), ('jaw_regularization', 'jaw_params')):
        base = torch.zeros_like(c(encoder_output[key])) if base_output is None else c(base_output[key])
        losses[name] = torch.mean((c(encoder_output[key]) - base) ** 2)
    loss_img = None
    if enable_fuse_generator and reconstructed_img is not None:
        reconstruction_loss = F.l1_loss(c(reconstructed_img), c(batch['img']), reduction='none')
        loss_img = reconstruction_loss.mean(dim=1, keepdim=True)
        losses['reconstruction_loss'] = reconstruction_loss.mean()
    else:
        losses['reconstruction_loss'] = 0
    for k in ('perceptual_vgg_loss', 'emotion_loss', 'mica_loss'):
        losses[k] = c(extra[k]) if k in extra else 0
    return total_law(losses, w, optimize_shape, optimize_expression, enable_fuse_generator), losses, loss_img


def cycle_law(recon_feats, flame_feats, use_eyelids=True, generator_frozen=False, head_dtype=None):
    """smirk_trainer.py:304-313"""
    c = (lambda t: t) if head_dtype is None else (lambda t: t.to(head_dtype))
    loss = 1.0 * F.mse_loss(c(recon_feats['expression_params']), c(flame_feats['expression_params'])) + \
        10.0 * F.mse_loss(c(recon_feats['jaw_params']), c(flame_feats['jaw_params']))
    if use_eyelids:
        loss = loss + 10.0 * F.mse_loss(c(recon_feats['eyelid_params']), c(flame_feats['eyelid_params']))
    if not generator_frozen:
        loss = loss + 1.0 * F.mse_loss(c(recon_feats['shape_params']), c(flame_feats['shape_params']))
    return loss


def term_law(kind, pred, target=None, flags=None, cols=None, head_dtype=torch.float64):
    """One general term of smirk_amd.losses.weighted_loss, written with the trainer's own expressions: the boolean-mask slice and F.mse_loss of :58 (the int 0
    when nothing takes part), F.l1_loss and its channel mean of :97-101.  Returns (value, loss_img or None)."""
    p = pred.to(head_dtype)
    t = torch.zeros_like(p) if target is None else target.to(head_dtype)
    if kind == "l1_image":
        e = F.l1_loss(p, t, reduction='none')
        return e.mean(), e.mean(dim=1, keepdim=True)
    p, t = p.reshape(p.shape[0], -1), t.reshape(t.shape[0], -1)
    cols = p.shape[1] if cols is None else cols
    valid = torch.ones(p.shape[0], dtype=torch.bool, device=p.device) if flags is None else flags.bool()
    if torch.sum(valid) == 0:
        return 0, None
    return F.mse_loss(p[valid, :cols], t[valid, :cols]), None


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------------------------------
def synth_first_path_inputs(B, seed=0, H=224, W=224, flags=None, with_base=False, device="cpu"):
    """Tensors with the shapes and ranges the first path's loss head sees at batch B: (encoder_output, landmarks_fan, landmarks_mp, batch, reconstructed_img,
    base_output).  flags: the [B] validity of the FAN landmarks (default: alternating, first one valid)."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.rand(*s, generator=g)
    n = lambda *s: torch.randn(*s, generator=g)
    enc = dict(expression_params=0.5 * n(B, 50), shape_params=0.5 * n(B, 300), jaw_params=0.1 * r(B, 3), eyelid_params=r(B, 2), pose_params=0.1 * n(B, 3),
               cam=torch.cat([5 + r(B, 1), 0.05 * n(B, 2)], 1))
    base = dict(expression_params=0.5 * n(B, 50), shape_params=0.5 * n(B, 300), jaw_params=0.1 * r(B, 3)) if with_base else None
    lf, lm = 2 * r(B, 68, 2) - 1, 2 * r(B, 105, 2) - 1
    flags = torch.tensor([i % 2 == 0 for i in range(B)]) if flags is None else torch.as_tensor(flags, dtype=torch.bool)
    batch = dict(img=r(B, 3, H, W), landmarks_fan=lf + 0.05 * n(B, 68, 2), landmarks_mp=lm + 0.05 * n(B, 105, 2), flag_landmarks_fan=flags)
    recon = (batch['img'] + 0.1 * n(B, 3, H, W)).clamp(0, 1)
    to = lambda d: None if d is None else {k: v.to(device) for k, v in d.items()}
    return to(enc), lf.to(device), lm.to(device), to(batch), recon.to(device), to(base)


def synth_cycle_feats(B, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(2000 + seed)
    mk = lambda: dict(expression_params=0.5 * torch.randn(B, 50, generator=g), jaw_params=0.1 * torch.rand(B, 3, generator=g),
                      eyelid_params=torch.rand(B, 2, generator=g), shape_params=0.5 * torch.randn(B, 300, generator=g))
    a, b = mk(), mk()
    return {k: v.to(device) for k, v in a.items()}, {k: v.to(device) for k, v in b.items()}
