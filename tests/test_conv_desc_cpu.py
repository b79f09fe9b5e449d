"""The glue every training schedule shares, without a GPU: _lib.conv_desc against the sixteen int32 fields of SmirkConvDesc written out by hand for each call
pattern of the schedules (generator_train, encoder_train / encoder_eval_grad, vgg_loss, mica), _lib.conv_launch's output shapes, _lib.version_key, and
encoder_train.clamp_grad against torch autograd through the reference's own clamp expression (smirk_encoder.py:105-108)."""
import struct

import pytest
import torch
import torch.nn.functional as F

from smirk_amd import _lib as L
from smirk_amd.encoder_train import clamp_grad

ZERO, REFLECT, NONE, RELU, NHWC, CONVT = 0, 1, 0, 1, 0, 1

# (conv_desc arguments) -> B, H, W, C0, C1, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, pad_mode, act, out_mode
CASES = {
    "generator 3x3 zero, two sources": (dict(B=2, H=32, W=48, c0=16, cout=32, k=3, c1=24), (2, 32, 48, 16, 24, 32, 3, 3, 1, 1, 1, 32, 48, ZERO, NONE, NHWC)),
    "generator 3x3 reflect": (dict(B=2, H=2, W=3, c0=512, cout=512, k=3, reflect=True), (2, 2, 3, 512, 0, 512, 3, 3, 1, 1, 1, 2, 3, REFLECT, NONE, NHWC)),
    "reflect layer's data gradient: pad 2, out_hw": (dict(B=2, H=2, W=3, c0=512, cout=512, k=3, pad=2, out_hw=(4, 5)),
                                                     (2, 2, 3, 512, 0, 512, 3, 3, 1, 2, 2, 4, 5, ZERO, NONE, NHWC)),
    "transposed 2x2 up-convolution": (dict(B=2, H=4, W=6, c0=256, cout=128, k=1, convt=True), (2, 4, 6, 256, 0, 128, 1, 1, 1, 0, 0, 4, 6, ZERO, NONE, CONVT)),
    "pointwise": (dict(B=3, H=7, W=5, c0=72, cout=24), (3, 7, 5, 72, 0, 24, 1, 1, 1, 0, 0, 7, 5, ZERO, NONE, NHWC)),
    "pointwise + ReLU": (dict(B=3, H=7, W=5, c0=24, cout=72, relu=True), (3, 7, 5, 24, 0, 72, 1, 1, 1, 0, 0, 7, 5, ZERO, RELU, NHWC)),
    "3x3 stride 2, not square": (dict(B=2, H=7, W=12, c0=8, cout=16, k=3, stride=2), (2, 7, 12, 8, 0, 16, 3, 3, 2, 1, 1, 4, 6, ZERO, NONE, NHWC)),
    "VGG 3x3 pad 1 + ReLU": (dict(B=2, H=16, W=24, c0=8, cout=64, k=3, relu=True), (2, 16, 24, 8, 0, 64, 3, 3, 1, 1, 1, 16, 24, ZERO, RELU, NHWC)),
}
for _h, _half in ((7, 4), (8, 4), (112, 56)):                         # MICA's (h - 1) // stride + 1 at stride 2
    CASES[f"MICA 3x3 stride 1 at {_h}"] = (dict(B=2, H=_h, W=_h, c0=64, cout=64, k=3, stride=1), (2, _h, _h, 64, 0, 64, 3, 3, 1, 1, 1, _h, _h, ZERO, NONE, NHWC))
    CASES[f"MICA 3x3 stride 2 at {_h}"] = (dict(B=2, H=_h, W=_h, c0=64, cout=128, k=3, stride=2),
                                           (2, _h, _h, 64, 0, 128, 3, 3, 2, 1, 1, _half, _half, ZERO, NONE, NHWC))
    CASES[f"MICA 1x1 stride 2 at {_h}"] = (dict(B=2, H=_h, W=_h, c0=64, cout=128, k=1, stride=2),
                                           (2, _h, _h, 64, 0, 128, 1, 1, 2, 0, 0, _half, _half, ZERO, NONE, NHWC))


@pytest.mark.parametrize("name", list(CASES))
def test_conv_desc_fields(name):
    kw, fields = CASES[name]
    kw = dict(kw)
    pos = [kw.pop(n) for n in ("B", "H", "W", "c0", "cout")]
    assert bytes(L.conv_desc(*pos, **kw)) == struct.pack("=16i", *fields)


@pytest.mark.parametrize("kw, shape", [(dict(B=2, H=4, W=6, c0=8, cout=16, k=1, convt=True), (2, 8, 12, 16)),
                                       (dict(B=2, H=7, W=9, c0=8, cout=16, k=3, stride=2), (2, 4, 5, 16)),
                                       (dict(B=1, H=2, W=3, c0=8, cout=8, k=3, pad=2, out_hw=(4, 5)), (1, 4, 5, 8))])
def test_conv_launch_output_shape(monkeypatch, kw, shape):
    """the launcher on CPU tensors: the pointer check is stubbed out and the entry records its arguments instead of launching"""
    monkeypatch.setattr(L, "ptr", lambda t, dtype=torch.float32, allow_none=False: None if t is None else t.data_ptr())
    seen = []
    entry = lambda *a: seen.append(a) or 0
    kw = dict(kw)
    d = L.conv_desc(*[kw.pop(n) for n in ("B", "H", "W", "c0", "cout")], **kw)
    x0, w, res = torch.zeros(1), torch.zeros(2), torch.zeros(3)
    out = L.conv_launch(entry, d, "stream", x0, w, residual=res)
    assert tuple(out.shape) == shape and out.dtype == torch.float32 and out.is_contiguous()
    assert seen == [(d, x0.data_ptr(), None, w.data_ptr(), None, None, res.data_ptr(), out.data_ptr(), "stream")]
    given = torch.empty(shape)
    assert L.conv_launch(entry, d, "stream", x0, w, out=given) is given and seen[-1][7] == given.data_ptr()
    monkeypatch.setattr(L, "lib", lambda: type("Lib", (), {"smirk_strerror": staticmethod(lambda c: b"refused")}))
    with pytest.raises(L.SmirkHipError, match="refused"):              # a refusal of the entry is raised, not returned
        L.conv_launch(lambda *a: L.SMIRK_ERR_BAD_ARG, d, "stream", x0, w)


def test_version_key_moves_with_storage_and_version():
    a, b = torch.zeros(3), torch.zeros(3)
    k0 = L.version_key((a, b))
    assert k0 == ((a.data_ptr(), a._version), (b.data_ptr(), b._version)) == L.version_key([a, b])
    b.add_(1)
    assert L.version_key((a, b)) != k0 and L.version_key((a,)) == k0[:1]


def _reference_clamps(p, n):
    """smirk_encoder.py:105-108 on the expression head's output"""
    return torch.cat([p[..., :n], torch.clamp(p[..., n:n + 2], 0, 1), F.relu(p[..., n + 2].unsqueeze(-1)), torch.clamp(p[..., n + 3:n + 5], -.2, .2)], -1)


@pytest.mark.parametrize("n_exp", [0, 50])
def test_clamp_grad_is_autograd_of_the_reference_clamps(n_exp):
    g = torch.Generator().manual_seed(n_exp)
    edge = torch.tensor([0.0, -0.0, 1.0, 0.2, -0.2, 0.5, -0.5, 1.5, 0.1, -0.1, 3e-8, -3e-8])
    B = 2 * edge.numel()
    raw = torch.randn(B, n_exp + 5, generator=g)
    for c in range(5):                                                  # every clamped column holds every edge value, each column in another order
        raw[:edge.numel(), n_exp + c] = edge.roll(c)
    gout = torch.randn(B, n_exp + 5, generator=g)
    p = raw.clone().requires_grad_(True)
    _reference_clamps(p, n_exp).backward(gout)
    got = clamp_grad(gout, raw, n_exp)
    assert got.is_contiguous() and torch.equal(got, p.grad)
    assert torch.equal(got[:, :n_exp], gout[:, :n_exp])                  # the expression block passes through untouched
    blocked = got[:, n_exp:] == 0
    assert blocked.any() and not blocked.all()                            # the edge values exercise both sides of every bound
    assert clamp_grad(gout, raw, -1) is gout                             # a head without clamps
