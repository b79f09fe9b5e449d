"""smirk_amd.expression_loss without a GPU: the extension table of include/smirk_emotion.h, every refusal of its entries (raw ctypes, dummy pointers: a
refusal comes before anything touches the device), the module's structure against the reference's state dict keys, checkpoint loading, the shim import, the
conditions the GPU tests' inputs must meet, the law of tests/emotion_law.py against the reference's own ResNet (where the reference tree is present), the
module's host-side folding against the unfolded law, and the proof that the GPU bounds see four deliberate mistakes."""
import ctypes as C
import importlib
import os
import re
import sys

import pytest
import torch

import emotion_law as EL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, ODD = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x10004)       # never dereferenced; ODD is not 16-byte aligned
BAD_ARG, UNSUPPORTED = -1, -4
SMALL = (1, 1, 1, 1)


def test_extension_table_equals_the_header():
    from smirk_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "smirk_emotion.h")).read()
    declared = set(re.findall(r"\b(smirk_emotion_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.EMOTION_EXPORTS), declared ^ set(L.EMOTION_EXPORTS)
    assert L.EMOTION_EXPORTS == tuple(L.EMOTION_SIGS)
    assert not set(L.EMOTION_EXPORTS) & set(L.EXPORTS) and not set(L.EMOTION_EXPORTS) & set(L.MICA_EXPORTS)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))
    assert L.lib().smirk_emotion_abi_version() == L.EMOTION_ABI_VERSION == val("SMIRK_EMOTION_ABI_VERSION") == 1
    assert (L.EMOTION_STEM_COUT, L.EMOTION_STEM_K, L.EMOTION_STEM_KPAD) == (val("SMIRK_EMOTION_STEM_COUT"), val("SMIRK_EMOTION_STEM_K"), val("SMIRK_EMOTION_STEM_KPAD"))
    codes = dict(re.findall(r"SMIRK_EMOTION_(L2|L1|COS) = (\d)", hdr))
    assert {k.lower(): int(v) for k, v in codes.items()} == L.EMOTION_METRICS
    assert "smirk_emotion.h" in open(os.path.join(REPO, "README.md")).read()
    # the main table and the MICA table did not move
    assert L.lib().smirk_abi_version() == L.ABI_VERSION and L.lib().smirk_mica_abi_version() == L.MICA_ABI_VERSION


def test_stem_entries_refuse_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    stem = lambda gen=P, tar=Q, w=P, shift=Q, out=P, B=2, H=224, W=224: lib.smirk_emotion_stem_split16(gen, tar, w, shift, out, B, H, W, None)
    for name in ("gen", "tar", "w", "shift", "out"):
        assert stem(**{name: None}) == BAD_ARG and stem(**{name: ODD}) == BAD_ARG, name
    for name in ("B", "H", "W"):
        assert stem(**{name: 0}) == BAD_ARG and stem(**{name: -3}) == BAD_ARG, name
    assert stem(B=1 << 9, H=512, W=512) == UNSUPPORTED                                                 # the output [2B, 256, 256, 64] of 16 GiB
    assert stem(B=1, H=40000, W=8) == UNSUPPORTED and stem(B=1 << 30, H=1, W=1) == UNSUPPORTED
    dgrad = lambda dz=P, wd=Q, gup=P, inv=0.5, dimg=Q, B=2, H=224, W=224: lib.smirk_emotion_stem_dgrad_split16(dz, wd, gup, inv, dimg, B, H, W, None)
    for name in ("dz", "wd", "gup", "dimg"):
        assert dgrad(**{name: None}) == BAD_ARG and dgrad(**{name: ODD}) == BAD_ARG, name
    for name in ("B", "H", "W"):
        assert dgrad(**{name: 0}) == BAD_ARG and dgrad(**{name: -3}) == BAD_ARG, name
    for inv in (0.0, -1.0, float("inf"), float("nan")):
        assert dgrad(inv=inv) == BAD_ARG, inv
    assert dgrad(B=1 << 9, H=512, W=512) == UNSUPPORTED


def test_pool_and_helper_entries_refuse_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    pool = lambda x=P, y=Q, N=2, H=112, W=112, Cc=64: lib.smirk_emotion_maxpool_split16(x, y, N, H, W, Cc, None)
    back = lambda x=P, dy=Q, dx=P, N=2, H=112, W=112, Cc=64, relu=1: lib.smirk_emotion_maxpool_backward_split16(x, dy, dx, N, H, W, Cc, relu, None)
    for fn, names in ((pool, ("x", "y")), (back, ("x", "dy", "dx"))):
        for name in names:
            assert fn(**{name: None}) == BAD_ARG and fn(**{name: ODD}) == BAD_ARG, name
        for name in ("N", "H", "W"):
            assert fn(**{name: 0}) == BAD_ARG and fn(**{name: -1}) == BAD_ARG, name
        for c in (0, -8, 4, 12, 63):
            assert fn(Cc=c) == BAD_ARG, c
        assert fn(N=1 << 10, H=256, W=256, Cc=64) == UNSUPPORTED and fn(N=1, H=40000, W=2, Cc=8) == UNSUPPORTED          # 16 GiB; a side above 32767
    dil = lambda dz=P, y=Q, s=P, add=Q, out=P, N=2, Hl=7, Wl=4, H=13, W=8, Cc=64: lib.smirk_emotion_dilate2_split16(dz, y, s, add, out, N, Hl, Wl, H, W, Cc, None)
    assert dil(dz=None) == BAD_ARG and dil(out=None) == BAD_ARG
    for name in ("dz", "y", "s", "add", "out"):
        assert dil(**{name: ODD}) == BAD_ARG, name
    for name in ("N", "H", "W"):
        assert dil(**{name: 0}) == BAD_ARG and dil(**{name: -1}) == BAD_ARG, name
    for c in (0, -8, 4, 12, 63):
        assert dil(Cc=c) == BAD_ARG, c
    assert dil(Hl=6) == BAD_ARG and dil(Hl=8) == BAD_ARG and dil(Wl=3) == BAD_ARG and dil(Wl=5) == BAD_ARG and dil(H=15) == BAD_ARG      # Hl = ceil(H / 2), Wl alike
    assert dil(N=1 << 10, Hl=128, Wl=128, H=256, W=256) == UNSUPPORTED


def test_head_entries_refuse_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    fwd = lambda feat=P, pooled=Q, aux=P, loss=Q, mean=P, B=2, HW=49, Cc=2048, metric=0: lib.smirk_emotion_head_forward_split16(feat, pooled, aux, loss, mean, B, HW, Cc,
                                                                                                                                metric, None)
    bwd = lambda feat=P, pooled=Q, aux=P, g=Q, B=2, HW=49, Cc=2048, metric=0, lift=4.0: lib.smirk_emotion_head_backward_split16(feat, pooled, aux, g, B, HW, Cc, metric,
                                                                                                                                lift, None)
    for fn, names in ((fwd, ("feat", "pooled", "aux", "loss")), (bwd, ("feat", "pooled", "aux", "g"))):
        for name in names:
            assert fn(**{name: None}) == BAD_ARG and fn(**{name: ODD}) == BAD_ARG, name
        for name in ("B", "HW"):
            assert fn(**{name: 0}) == BAD_ARG and fn(**{name: -1}) == BAD_ARG, name
        for c in (0, -8, 4, 12, 2047):
            assert fn(Cc=c) == BAD_ARG, c
        for metric in (-1, 3, 7):
            assert fn(metric=metric) == BAD_ARG, metric
        assert fn(B=1 << 12, HW=49, Cc=2048) == UNSUPPORTED and fn(B=1, HW=40000, Cc=8) == UNSUPPORTED
    assert fwd(mean=ODD) == BAD_ARG                                                                    # nullable, but aligned when given
    for lift in (0.0, -2.0, float("inf"), float("nan")):
        assert bwd(lift=lift) == BAD_ARG, lift


def _fixture_shapes():
    out = {}
    for line in open(os.path.join(REPO, "tests", "golden", "emotion_state_keys.txt")):
        name, shape = line.split()
        out[name] = () if shape == "-" else tuple(int(s) for s in shape.split("x"))
    return out


def test_state_dict_keys_and_shapes_are_the_references():
    from smirk_amd import ExpressionLoss
    from smirk_amd.expression_loss import launches
    m = ExpressionLoss(EL.synth_checkpoint(EL.FULL, 2))
    want = _fixture_shapes()
    assert len(want) == 320
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert list(m.state_dict()) == list(want)                                                          # in the reference's order, too
    assert "backbone.fc.weight" in want                                                                # `fc` is present, as in the reference
    assert all(not p.requires_grad for p in m.parameters())
    m.train()
    assert not m.training and not any(mod.training for mod in m.modules())                             # running statistics whatever train() is called with
    assert launches(EL.FULL) == (56, 105) and launches(SMALL) == (20, 33)


def test_reference_format_checkpoint_loads():
    import smirk_amd
    from smirk_amd import ExpressionLoss
    ckpt = EL.synth_checkpoint(SMALL, 1)
    torch.manual_seed(0)
    m = ExpressionLoss(ckpt, layers=SMALL)
    sd = m.state_dict()
    for k, v in ckpt["state_dict"].items():
        if k.startswith("backbone.fc.") or k.startswith("linear."):
            continue
        assert torch.equal(sd[k], v), k
    assert not torch.equal(sd["backbone.fc.weight"], ckpt["state_dict"]["backbone.fc.weight"])          # `backbone.fc.*` is dropped: the module keeps its own
    assert not any(k.startswith("linear.") for k in sd) and len(sd) == len(ckpt["state_dict"]) - 2      # `linear.*` is dropped
    for key in ("backbone.fc.weight", "linear.bias"):                                                   # the reference deletes these keys: a file without them is not its format
        broken = {"state_dict": {k: v for k, v in ckpt["state_dict"].items() if k != key}}
        with pytest.raises(KeyError, match=key):
            ExpressionLoss(broken, layers=SMALL)
    with pytest.raises(smirk_amd.SmirkHipError, match="state_dict"):
        ExpressionLoss(ckpt["state_dict"], layers=SMALL)
    with pytest.raises(RuntimeError, match="size mismatch"):
        ExpressionLoss({"state_dict": {**ckpt["state_dict"], "backbone.conv1.weight": torch.zeros(64, 3, 3, 3)}}, layers=SMALL)
    img = EL.synth_images(1, 224, 224, 0)
    with pytest.raises(smirk_amd.SmirkHipError, match="CPU"):
        m(img, img)                                                                                     # CPU tensors: no fallback
    with pytest.raises(smirk_amd.SmirkHipError):
        m.backbone(img)                                                                                 # the layers are never called
    with pytest.raises(smirk_amd.SmirkHipError, match="four positive"):
        ExpressionLoss(ckpt, layers=(1, 1, 1))


def test_checkpoint_file_and_missing_file(tmp_path, monkeypatch):
    from smirk_amd import ExpressionLoss
    from smirk_amd.expression_loss import DEFAULT_CHECKPOINT
    ckpt = EL.synth_checkpoint(SMALL, 1)
    with pytest.raises(FileNotFoundError, match="checkpoint"):
        ExpressionLoss(str(tmp_path / "nothing.ckpt"), layers=SMALL)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="checkpoint"):                                          # None = the reference's path
        ExpressionLoss(layers=SMALL)
    assert DEFAULT_CHECKPOINT == "assets/ResNet50/checkpoints/deca-epoch=01-val_loss_total/dataloader_idx_0=1.27607644.ckpt"
    os.makedirs(os.path.dirname(tmp_path / DEFAULT_CHECKPOINT))
    torch.save(ckpt, tmp_path / DEFAULT_CHECKPOINT)
    m = ExpressionLoss(layers=SMALL)
    assert torch.equal(m.backbone.layer4[0].conv3.weight, ckpt["state_dict"]["backbone.layer4.0.conv3.weight"])


def test_shim_resolves_the_trainers_import(monkeypatch):
    """base_trainer.py `from src.losses.ExpressionLoss import ExpressionLoss`"""
    import smirk_amd
    for name in [n for n in sys.modules if n == "src" or n.startswith("src.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(os.path.join(REPO, "integration", "shim"))
    m = importlib.import_module("src.losses.ExpressionLoss")
    assert m.ExpressionLoss is smirk_amd.ExpressionLoss and m.__file__.startswith(os.path.join(REPO, "integration", "shim"))
    assert callable(smirk_amd.first_path.emotion_term)


@pytest.mark.parametrize("layers,seed,B,H,W", EL.NET_CASES, ids=[f"{sum(c[0])}blocks-{c[3]}x{c[4]}" for c in EL.NET_CASES])
def test_conditions_on_the_gpu_tests_inputs(layers, seed, B, H, W):
    ref = EL.case_reference(layers, seed, B, H, W)
    worst = max(ref["trace"], key=lambda nv: nv[1])
    f = ref["f64"]["features"]
    print(f"max |activation| {worst[1]:.1f} at {worst[0]}, max |feature| {float(f.abs().max()):.2f}, max |g - t| {float((f[:B] - f[B:]).abs().max()):.3f}, "
          f"loss {float(ref['f64']['loss']):.3g}, max |grad| {float(ref['f64']['grad'].abs().max()):.3g}")
    assert worst[1] < 100.0                                                                             # far inside the split16 range of 65504
    assert float((f[:B] - f[B:]).abs().max()) > 0.05 and float(ref["f64"]["grad"].abs().max()) > 0
    assert len(ref["trace"]) == 1 + sum(layers) and tuple(f.shape) == (2 * B, 2048)


@pytest.fixture()
def reference_resnet(monkeypatch):
    from oracle import sandbox as S
    if not S.available():
        pytest.skip("the reference tree is not present")
    for name in [n for n in sys.modules if n == "src" or n.startswith("src.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(S.REF_ROOT)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)                                              # the reference tree is read-only
    yield importlib.import_module("src.losses.resnet")                                                  # (ExpressionLoss.py itself imports torchvision)
    for name in [n for n in sys.modules if n == "src" or n.startswith("src.")]:
        sys.modules.pop(name, None)


@pytest.mark.parametrize("layers,seed", [(SMALL, 1), (EL.FULL, 2)], ids=["4blocks", "full"])
def test_law_is_the_references_arithmetic(reference_resnet, layers, seed):
    """the reference's own ResNet class and the three metrics of ExpressionLoss.py:53-65 in float64, values and the gradient; measured agreement 7e-16 relative
    on the features and 2e-14 on the gradient"""
    rn = reference_resnet
    ckpt, gen, tar = EL.synth_checkpoint(layers, seed), EL.synth_images(2, 224, 224, seed), EL.synth_images(2, 224, 224, seed + 100)
    net = rn.resnet50(num_classes=100, include_top=False, emoca_specific=True) if layers == EL.FULL else \
        rn.ResNet(rn.Bottleneck, list(layers), num_classes=100, include_top=False, emoca_specific=True)
    holder = torch.nn.Module()
    holder.backbone = net
    sd = {k: v for k, v in ckpt["state_dict"].items() if not k.startswith("backbone.fc.") and not k.startswith("linear.")}
    missing = holder.load_state_dict(sd, strict=False)                                                  # ExpressionLoss.py:34-43
    assert set(missing.missing_keys) == {"backbone.fc.weight", "backbone.fc.bias"} and not missing.unexpected_keys
    net = net.double().eval()
    for metric in EL.METRICS:
        x = gen.double().requires_grad_(True)
        gen_out, tar_out = net(x).view(2, -1), net(tar.double()).view(2, -1)
        if metric == "l2":
            loss = ((gen_out - tar_out) ** 2).mean(dim=1)
        elif metric == "l1":
            loss = torch.abs(gen_out - tar_out).mean(dim=1)
        else:
            loss = 1.0 - torch.nn.functional.cosine_similarity(gen_out, tar_out, dim=1)
        (grad,) = torch.autograd.grad(loss.mean(), x)
        law = EL.emotion_law(ckpt, gen, tar, layers, metric=metric)
        for name, got, want in (("features", law["features"], torch.cat([gen_out, tar_out]).detach()), ("loss", law["loss"], loss.mean().detach()), ("grad", law["grad"], grad)):
            rel = float((got - want).abs().max()) / float(want.abs().max())
            print(f"{sum(layers)} blocks, {metric}, {name}: law against the reference's classes {rel:.2e} relative")
            assert rel <= 1e-10, (metric, name)


def test_folding_reproduces_the_unfolded_law():
    """float64: the epilogue scales / shifts and the stem's three images of smirk_amd.expression_loss against the law's convolution and BatchNorm"""
    import torch.nn.functional as F
    from smirk_amd import ExpressionLoss
    from smirk_amd.expression_loss import bn_affine, fold_stem
    ckpt = EL.synth_checkpoint(SMALL, 1)
    m, sd = ExpressionLoss(ckpt, layers=SMALL), ckpt["state_dict"]
    g = torch.Generator().manual_seed(5)
    for name, bn in [(n, mod) for n, mod in m.backbone.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)]:
        x = torch.randn(2, bn.num_features, 3, 3, generator=g, dtype=torch.float64)
        s, t = bn_affine(bn)
        want = EL._norm(sd, name, x, torch.float64)
        assert s.dtype == torch.float64 and float((x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1) - want).abs().max()) <= 1e-10 * float(want.abs().max()), name
    fwd, shift, dgrad = fold_stem(m.backbone.conv1, m.backbone.bn1)
    assert tuple(fwd.shape) == (64, 160) and tuple(shift.shape) == (64,) and tuple(dgrad.shape) == (7, 7, 3, 64) and fwd.dtype == torch.float64
    assert torch.equal(fwd[:, 147:], torch.zeros(64, 13, dtype=torch.float64))
    img = torch.rand(1, 3, 9, 10, generator=g, dtype=torch.float64, requires_grad=True)
    want = EL._norm(sd, "bn1", F.conv2d(img, sd["backbone.conv1.weight"].double(), None, 2, 3), torch.float64)
    patches = F.unfold(img, 7, padding=3, stride=2).view(1, 3, 49, -1).permute(0, 3, 2, 1).reshape(1, -1, 147)      # [pixel][(ky * 7 + kx) * 3 + c]
    got = (patches @ fwd[:, :147].t() + shift).permute(0, 2, 1).reshape(want.shape)
    assert float((got - want).detach().abs().max()) <= 1e-10 * float(want.detach().abs().max())
    dz = torch.randn(want.shape, generator=g, dtype=torch.float64)
    (dimg,) = torch.autograd.grad(want, img, dz)
    via = F.conv_transpose2d(dz, dgrad.permute(3, 2, 0, 1), None, 2, 3, (0, 1))                        # wd[ky][kx][c][co] is the transposed convolution's weight
    assert float((via - dimg).abs().max()) <= 1e-10 * float(dimg.abs().max())


def test_gpu_bounds_see_four_mistakes():
    """Each of the three forward mistakes moves the law's features by more than 1000 times the bound tests/test_expression_loss_gpu.py holds them to (measured:
    3e4 - 4e5 times on the 4-block cases, 4e3 - 3e5 on the full network).  The dropped last ReLU mask leaves the forward unchanged and moves the image gradient by
    5 - 16 % of its norm: 9 - 20 times the Euclidean bound on the gradient, but only 0.8 - 2.5 times the maximum-norm bound, which eager fp32's own ReLU / max-pool
    switches make loose (emotion_law.bound_l2_of) - so the Euclidean bound is the one that must see it, and the head kernel's test checks the mask itself exactly."""
    for case in EL.NET_CASES[:2]:
        layers = case[0]
        ref = EL.case_reference(*case)
        for variant in ("stride_on_conv1", "pool_ceil", "drop_downsample_bn"):
            bound, _ = EL.bound_of(ref, "features")
            wrong = EL.emotion_law(ref["ckpt"], ref["gen"], ref["tar"], layers, variant=variant)
            moved = float((wrong["features"] - ref["f64"]["features"]).abs().max())
            print(f"{case[3]} x {case[4]}, {variant}: moves the features by {moved:.3g} = {moved / bound:.3g} x the bound {bound:.3g}")
            assert moved > 1000 * bound, variant
        wrong = EL.emotion_law(ref["ckpt"], ref["gen"], ref["tar"], layers, variant="no_last_relu_mask")
        assert torch.equal(wrong["features"], ref["f64"]["features"])
        (bound, _), (bound2, _) = EL.bound_of(ref, "grad"), EL.bound_l2_of(ref, "grad")
        moved, moved2 = float((wrong["grad"] - ref["f64"]["grad"]).abs().max()), float((wrong["grad"] - ref["f64"]["grad"]).norm())
        print(f"{case[3]} x {case[4]}, no_last_relu_mask: moves the gradient by {moved:.3g} = {moved / bound:.3g} x the maximum-norm bound and by {moved2:.3g} = "
              f"{moved2 / bound2:.3g} x the Euclidean bound {bound2:.3g}")
        assert moved2 > 5 * bound2
