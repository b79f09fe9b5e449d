"""smirk_amd.vgg_loss without a GPU: every refusal of the new C entries (raw ctypes, dummy pointers: a refusal comes before anything touches the device), the
workspace query, the module's structure against the reference's state dict, the shim import, and the forced law of tests/vgg_law.py against the plain one."""
import ctypes as C
import importlib
import os
import re
import sys

import pytest
import torch

from vgg_law import CHANNELS, grad_of, state_dict_shapes, synth_images, synth_weights, vgg_forced_law, vgg_law

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, ODD = C.c_void_p(0x10000), C.c_void_p(0x10004)                    # never dereferenced; ODD is not 16-byte aligned
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def _half(*v):
    return (C.c_longlong * len(v))(*v)


def test_c_entries_refuse_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    # prepare and its backward
    prep = lambda x=P, y=P, mean=P, std=P, out=P, B=2, H=16, W=16: lib.smirk_vgg_prepare_split16(x, y, mean, std, out, B, H, W, None)
    pbwd = lambda d=P, std=P, dx=P, B=2, H=16, W=16, scale=1.0: lib.smirk_vgg_prepare_backward_split16(d, std, dx, B, H, W, scale, None)
    for name in ("x", "y", "out"):
        assert prep(**{name: None}) == BAD_ARG and prep(**{name: ODD}) == BAD_ARG, name
    assert prep(mean=None) == BAD_ARG and prep(std=None) == BAD_ARG
    for name in ("d", "dx"):
        assert pbwd(**{name: None}) == BAD_ARG and pbwd(**{name: ODD}) == BAD_ARG, name
    assert pbwd(std=None) == BAD_ARG
    for call in (prep, pbwd):
        for name in ("B", "H", "W"):
            assert call(**{name: 0}) == BAD_ARG and call(**{name: -4}) == BAD_ARG, name
    assert prep(B=1 << 10, H=1 << 10, W=1 << 10) == UNSUPPORTED and pbwd(B=1 << 11, H=1 << 10, W=1 << 10) == UNSUPPORTED      # 2 GiB and more
    # feature L1: partials, finalise, workspace
    good = _half(64 * 4096 * 8, 128 * 1024 * 8, 256 * 256 * 8, 512 * 64 * 8)
    need = lib.smirk_vgg_l1_workspace_bytes(good, 4)
    part = lambda f=P, Cc=64, tap=0, half=good, n=4, ws=P, nb=need: lib.smirk_vgg_l1_partials_split16(f, Cc, tap, half, n, ws, nb, None)
    fin = lambda half=good, n=4, ws=P, nb=need, terms=P, total=P: lib.smirk_vgg_l1_finalise(half, n, ws, nb, terms, total, None)
    assert part(f=None) == BAD_ARG and part(f=ODD) == BAD_ARG and part(ws=None) == BAD_ARG and part(ws=ODD) == BAD_ARG
    assert fin(ws=None) == BAD_ARG and fin(ws=ODD) == BAD_ARG and fin(terms=None) == BAD_ARG and fin(total=None) == BAD_ARG
    for call in (part, fin):
        assert call(half=None) == BAD_ARG and call(n=0) == BAD_ARG and call(n=-1) == BAD_ARG and call(n=5) == BAD_ARG
        assert call(half=_half(64, 0, 64, 64)) == BAD_ARG and call(half=_half(64, -64, 64, 64)) == BAD_ARG        # every tap is looked at
        assert call(half=_half(64, 68, 64, 64)) == BAD_ARG                                                         # not whole 8-channel groups
        assert call(half=_half(64, 64, 1 << 28, 64), nb=1 << 40) == UNSUPPORTED                                    # a [2, half] tensor of 2 GiB
        assert call(nb=need - 1) == WORKSPACE and call(nb=0) == WORKSPACE
    assert part(tap=-1) == BAD_ARG and part(tap=4) == BAD_ARG and part(tap=1, n=1) == BAD_ARG
    for c in (0, -8, 4, 12, 63):
        assert part(Cc=c) == BAD_ARG, c
    # ReLU / tap backward
    G = C.c_void_p(0x20000)
    relu = lambda fx=P, fy=P, d_in=P, g=G, dz=P, elems=4096, Cc=64, scale=1.0: lib.smirk_vgg_relu_tap_backward_split16(fx, fy, d_in, g, dz, elems, Cc, scale, None)
    assert relu(fx=None) == BAD_ARG and relu(dz=None) == BAD_ARG
    for name in ("fx", "fy", "d_in", "dz"):
        assert relu(**{name: ODD}) == BAD_ARG, name
    assert relu(fy=None, d_in=None) == BAD_ARG                                                                     # a layer that is not tapped needs its gradient
    assert relu(g=None) == BAD_ARG                                                                                 # a tapped layer reads the upstream gradient
    assert relu(elems=0) == BAD_ARG and relu(elems=-64) == BAD_ARG and relu(elems=4096 + 4) == BAD_ARG
    for c in (0, -8, 4, 12):
        assert relu(Cc=c) == BAD_ARG, c
    assert relu(elems=1 << 29) == UNSUPPORTED
    for bad in (0.0, -1.0, float("inf"), float("nan")):                                                           # the gradient scale: positive and finite
        assert relu(scale=bad) == BAD_ARG and pbwd(scale=bad) == BAD_ARG, bad


def test_workspace_query():
    from smirk_amd import _lib as L
    lib, chunk = L.lib(), 8 * L.VGG_L1_CHUNK
    one = lambda h: lib.smirk_vgg_l1_workspace_bytes(_half(h), 1)
    assert one(0) == 0 and one(-8) == 0 and one(12) == 0 and lib.smirk_vgg_l1_workspace_bytes(None, 1) == 0 and lib.smirk_vgg_l1_workspace_bytes(_half(8), 0) == 0
    assert lib.smirk_vgg_l1_workspace_bytes(_half(8, 8, 8, 8, 8), 5) == 0
    sizes = [one(h) for h in (8, chunk - 8, chunk, chunk + 8, 40 * chunk, 4000 * chunk)]
    assert sizes == sorted(sizes) and sizes[0] >= 8 and sizes[-1] >= 8 * 4000 and all(s % 256 == 0 for s in sizes)
    # the workload: B = 64 at 224 x 224, one partial per chunk of every tap
    taps = [64 * 224 * 224 * 64, 64 * 112 * 112 * 128, 64 * 56 * 56 * 256, 64 * 28 * 28 * 512]
    assert lib.smirk_vgg_l1_workspace_bytes(_half(*taps), 4) >= 8 * sum(-(-t // chunk) for t in taps)


def test_constants_and_abi_equal_the_header():
    from smirk_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "smirk_hip.h")).read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))
    assert (L.VGG_TAPS, L.VGG_L1_CHUNK) == (val("SMIRK_VGG_TAPS"), val("SMIRK_VGG_L1_CHUNK"))
    assert L.lib().smirk_abi_version() == L.ABI_VERSION >= 14
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"C ABI v{L.ABI_VERSION}" in readme and f"{len(L.EXPORTS)} entry points" in readme


def test_module_structure_loads_the_reference_state_dict():
    import smirk_amd
    from smirk_amd import VGGPerceptualLoss
    m = VGGPerceptualLoss(synth_weights(3))
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == state_dict_shapes()
    assert len(m.blocks) == 4 and all(isinstance(b, torch.nn.Sequential) for b in m.blocks)
    assert [k for b in m.blocks for k, _ in b.named_children()] == [str(i) for i in range(23)]
    assert all(not p.requires_grad for p in m.parameters()) and m.resize_to == (224, 224)
    # an nn.Sequential in torchvision's layout gives the same module, and a state dict saved from one loads into the other
    layers, cin = [], 3
    for k, c in enumerate(CHANNELS):
        if k in (2, 4, 7):
            layers.append(torch.nn.MaxPool2d(2, 2))
        layers += [torch.nn.Conv2d(cin, c, 3, padding=1), torch.nn.ReLU(inplace=True)]
        cin = c
    m2 = VGGPerceptualLoss(torch.nn.Sequential(*layers, torch.nn.MaxPool2d(2, 2)), resize_to=None)
    assert list(m2.state_dict()) == list(sd) and m2.resize_to is None
    m2.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), sd.values()))
    with pytest.raises(smirk_amd.SmirkHipError):
        VGGPerceptualLoss(synth_weights(3)[:9])
    with pytest.raises(smirk_amd.SmirkHipError):
        VGGPerceptualLoss(torch.nn.Sequential(*layers[:10]))
    with pytest.raises(smirk_amd.SmirkHipError, match="CPU"):
        m(*synth_images(1, 16, 16))                                                                                # CPU tensors: no fallback


def test_features_none_without_torchvision_is_an_import_error(monkeypatch):
    from smirk_amd import VGGPerceptualLoss
    monkeypatch.setitem(sys.modules, "torchvision", None)                                                          # `import torchvision` raises ImportError
    with pytest.raises(ImportError) as ei:
        VGGPerceptualLoss()
    assert type(ei.value) is ImportError


def test_shim_resolves_the_trainers_import(monkeypatch):
    """base_trainer.py:78 `from src.losses.VGGPerceptualLoss import VGGPerceptualLoss`"""
    import smirk_amd
    for name in [n for n in sys.modules if n == "src" or n.startswith("src.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(os.path.join(REPO, "integration", "shim"))
    m = importlib.import_module("src.losses.VGGPerceptualLoss")
    assert m.VGGPerceptualLoss is smirk_amd.VGGPerceptualLoss and m.__file__.startswith(os.path.join(REPO, "integration", "shim"))


@pytest.mark.parametrize("shape,resize_to", [((1, 16, 16), None), ((2, 24, 40), None), ((1, 16, 24), (32, 32))])
def test_forced_law_under_its_own_trace_is_the_law(shape, resize_to):
    """float64: forcing the decisions the law took itself changes neither its value nor its gradient (1e-12 of the value / of max|g|)"""
    B, H, W = shape
    w = synth_weights(1)
    x, y = (t.double() for t in synth_images(B, H, W, seed=2))
    tr = {}
    v, g = grad_of(lambda t: vgg_law(t, y, w, resize_to, tr)[0], x)
    vf, gf = grad_of(lambda t: vgg_forced_law(t, w, tr, resize_to), x)
    assert abs(float(v - vf)) <= 1e-12 * abs(float(v))
    assert float((g - gf).abs().max()) <= 1e-12 * float(g.abs().max())


def test_forced_law_under_an_fp32_trace_meets_the_fp32_gradient():
    """1 x 3 x 64 x 64: the float64 forced law under eager fp32's trace lies within 1e-6 of max|g| of eager fp32's own gradient (seen: 3.2e-7), where the
    plain float64 law may be further away by flipped decisions"""
    w = synth_weights(1)
    x, y = synth_images(1, 64, 64, seed=3)
    tr = {}
    _, g32 = grad_of(lambda t: vgg_law(t, y, w, None, tr)[0], x)
    _, gf = grad_of(lambda t: vgg_forced_law(t, w, tr), x.double())
    dist = float((g32.double() - gf).abs().max()) / float(gf.abs().max())
    print(f"eager fp32 against the forced float64 law under its trace: {dist:.2e} of max|g|")
    assert dist <= 1e-6
