"""smirk_amd.mica without a GPU: the extension table of include/smirk_mica.h, every refusal of its entries (raw ctypes, dummy pointers: a refusal comes before
anything touches the device), the module's structure against the reference's state dict keys, checkpoint loading, the shim import, the conditions the GPU
tests' inputs must meet, the law of tests/mica_law.py against the reference's own classes (where the reference tree is present), the module's host-side
folding against the unfolded law, and the proof that the GPU bounds see three deliberate mistakes."""
import ctypes as C
import importlib
import os
import re
import sys

import pytest
import torch

import mica_law as ML

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, ODD = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x10004)       # never dereferenced; ODD is not 16-byte aligned
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def test_extension_table_equals_the_header():
    from smirk_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "smirk_mica.h")).read()
    declared = set(re.findall(r"\b(smirk_mica_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.MICA_EXPORTS), declared ^ set(L.MICA_EXPORTS)
    assert L.MICA_EXPORTS == tuple(L.MICA_SIGS) and not set(L.MICA_EXPORTS) & set(L.EXPORTS)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))
    assert L.lib().smirk_mica_abi_version() == L.MICA_ABI_VERSION == val("SMIRK_MICA_ABI_VERSION") == 1
    assert (L.MICA_FC_MAX_B, L.MICA_HEAD_LAYERS, L.MICA_HEAD_MAX_DIM) == (val("SMIRK_MICA_FC_MAX_B"), val("SMIRK_MICA_HEAD_LAYERS"), val("SMIRK_MICA_HEAD_MAX_DIM"))
    assert "smirk_mica.h" in open(os.path.join(REPO, "README.md")).read()


def test_prepare_and_streaming_entries_refuse_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    prep = lambda img=P, out=Q, B=2, H=16, W=16: lib.smirk_mica_prepare_split16(img, out, B, H, W, None)
    for name in ("img", "out"):
        assert prep(**{name: None}) == BAD_ARG and prep(**{name: ODD}) == BAD_ARG, name
    for name in ("B", "H", "W"):
        assert prep(**{name: 0}) == BAD_ARG and prep(**{name: -4}) == BAD_ARG, name
    assert prep(B=1 << 10, H=1 << 8, W=1 << 8) == UNSUPPORTED                                          # [B, H, W, 8] of 2 GiB
    aff = lambda src=P, scale=Q, shift=Q, slope=Q, dst=P, M=49, Cc=64: lib.smirk_mica_affine_prelu_split16(src, scale, shift, slope, dst, M, Cc, None)
    assert aff(src=None) == BAD_ARG and aff(dst=None) == BAD_ARG
    for name in ("src", "scale", "shift", "slope", "dst"):
        assert aff(**{name: ODD}) == BAD_ARG, name
    for c in (0, -8, 4, 12, 63):
        assert aff(Cc=c) == BAD_ARG, c
    assert aff(M=0) == BAD_ARG and aff(M=-1) == BAD_ARG
    assert aff(M=1 << 23, Cc=64) == UNSUPPORTED and aff(M=1 << 40, Cc=8) == UNSUPPORTED                 # 2 GiB and more


def test_fc_entry_refuses_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    need = lib.smirk_mica_fc_workspace_bytes(3, 25088, 512)
    fc = lambda x=P, w=P, bias=P, out=Q, ws=Q, nb=need, B=3, K=25088, N=512: lib.smirk_mica_fc_split16(x, w, bias, out, ws, nb, B, K, N, None)
    for name in ("x", "w", "bias", "out", "ws"):
        assert fc(**{name: None}) == BAD_ARG and fc(**{name: ODD}) == BAD_ARG, name
    assert fc(B=0) == BAD_ARG and fc(B=-1) == BAD_ARG and fc(B=65, nb=1 << 40) == BAD_ARG
    assert fc(K=0) == BAD_ARG and fc(K=-8) == BAD_ARG and fc(K=25084) == BAD_ARG and fc(K=4) == BAD_ARG
    assert fc(N=0) == BAD_ARG and fc(N=-1) == BAD_ARG
    assert fc(K=1 << 20, N=1 << 10, nb=1 << 40) == UNSUPPORTED                                        # w of 4 GiB
    assert fc(nb=need - 1) == WORKSPACE and fc(nb=0) == WORKSPACE
    # the workspace query: 0 for what the entry refuses, enough for one fp32 partial per split, row and neuron otherwise
    q = lib.smirk_mica_fc_workspace_bytes
    assert q(0, 8, 1) == 0 and q(65, 8, 1) == 0 and q(1, 12, 1) == 0 and q(1, 8, 0) == 0 and q(1, 1 << 20, 1 << 10) == 0
    assert q(1, 8, 1) >= 4 and q(1, 8, 1) % 256 == 0
    assert need >= 4 * 3 * 512 and need % 256 == 0 and q(64, 25088, 512) >= 4 * 64 * 512 > q(3, 25088, 512) // 64


def test_head_entry_refuses_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()

    def head(dims=(512, 300, 300, 300, 300, 300), w=P, b=Q):
        h = L.SmirkMicaHead()
        for k in range(L.MICA_HEAD_LAYERS):
            h.layer[k].w, h.layer[k].b, h.layer[k].n_in, h.layer[k].n_out = w, b, dims[k], dims[k + 1]
        return h

    run = lambda feat=P, h=None, out=Q, B=2: lib.smirk_mica_head(feat, C.byref(h or head()), out, B, None)
    assert run(feat=None) == BAD_ARG and run(feat=ODD) == BAD_ARG and run(out=None) == BAD_ARG and run(out=ODD) == BAD_ARG
    assert lib.smirk_mica_head(P, None, Q, 2, None) == BAD_ARG
    assert run(B=0) == BAD_ARG and run(B=-3) == BAD_ARG
    assert run(h=head(w=None)) == BAD_ARG and run(h=head(b=None)) == BAD_ARG and run(h=head(w=ODD)) == BAD_ARG and run(h=head(b=ODD)) == BAD_ARG
    assert run(h=head(dims=(512, 0, 300, 300, 300, 300))) == BAD_ARG and run(h=head(dims=(512, 300, 300, 300, 300, -1))) == BAD_ARG
    broken = head()
    broken.layer[2].n_in = 299                                                                         # does not chain
    assert run(h=broken) == BAD_ARG
    assert run(h=head(dims=(L.MICA_HEAD_MAX_DIM + 1, 300, 300, 300, 300, 300))) == UNSUPPORTED
    assert run(h=head(dims=(512, 300, 300, 300, 300, L.MICA_HEAD_MAX_DIM + 1))) == UNSUPPORTED


def _fixture_shapes():
    out = {}
    for line in open(os.path.join(REPO, "tests", "golden", "mica_state_keys.txt")):
        name, shape = line.split()
        out[name] = () if shape == "-" else tuple(int(s) for s in shape.split("x"))
    return out


def test_state_dict_keys_and_shapes_are_the_references():
    from smirk_amd import MICA
    m = MICA(ML.synth_checkpoint(ML.FULL, 3))
    want = _fixture_shapes()
    assert len(want) == 935
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert list(m.state_dict()) == list(want)                                                          # in the reference's order, too
    assert all(not p.requires_grad for p in m.parameters())
    m.train()
    assert not m.training and not any(mod.training for mod in m.modules())                             # running statistics whatever train() is called with
    assert m.image_size == 112


def test_reference_format_checkpoint_loads():
    import smirk_amd
    from smirk_amd import MICA
    layers = (1, 1, 1, 1)
    ckpt = ML.synth_checkpoint(layers, 1)
    m = MICA(ckpt, layers=layers)
    sd = m.state_dict()
    for k, v in ckpt["arcface"].items():
        assert torch.equal(sd["arcface." + k], v), k
    for k, v in ckpt["flameModel"].items():
        if k.startswith("regressor."):                                                                 # the prefix is stripped, other flameModel keys are ignored
            assert torch.equal(sd[k], v), k
    assert len(sd) == len(ckpt["arcface"]) + len(ckpt["flameModel"]) - 1
    for part, key in (("arcface", "layer2.0.bn3.running_var"), ("flameModel", "regressor.network.2.bias")):      # a missing key raises
        broken = {p: dict(d) for p, d in ckpt.items()}
        del broken[part][key]
        with pytest.raises(RuntimeError, match=key.split(".")[-2]):
            MICA(broken, layers=layers)
    with pytest.raises(smirk_amd.SmirkHipError, match="arcface"):
        MICA({"flameModel": ckpt["flameModel"]}, layers=layers)
    with pytest.raises(RuntimeError):
        MICA(ckpt, layers=(1, 2, 1, 1))                                                                # the checkpoint is loaded strictly
    with pytest.raises(smirk_amd.SmirkHipError, match="CPU"):
        m(ML.synth_images(1, 0))                                                                       # CPU tensors: no fallback
    with pytest.raises(smirk_amd.SmirkHipError):
        m.regressor(torch.zeros(1, 512))                                                               # the layers are never called


def test_checkpoint_file_and_missing_file(tmp_path, monkeypatch):
    from smirk_amd import MICA
    layers = (1, 1, 1, 1)
    ckpt = ML.synth_checkpoint(layers, 1)
    with pytest.raises(FileNotFoundError, match="checkpoint"):
        MICA(str(tmp_path / "nothing.tar"), layers=layers)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="checkpoint"):                                          # None = assets/mica.tar, as in the reference
        MICA(layers=layers)
    os.makedirs(tmp_path / "assets")
    torch.save(ckpt, tmp_path / "assets" / "mica.tar")
    m = MICA(layers=layers)
    assert torch.equal(m.arcface.fc.weight, ckpt["arcface"]["fc.weight"])


def test_shim_resolves_the_trainers_import(monkeypatch):
    """base_trainer.py:94 `from src.models.MICA.mica import MICA`"""
    import smirk_amd
    for name in [n for n in sys.modules if n == "src" or n.startswith("src.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(os.path.join(REPO, "integration", "shim"))
    m = importlib.import_module("src.models.MICA.mica")
    assert m.MICA is smirk_amd.MICA and m.MappingNetwork is smirk_amd.MappingNetwork and m.__file__.startswith(os.path.join(REPO, "integration", "shim"))


@pytest.mark.parametrize("layers,seed,B", ML.NET_CASES, ids=[str(sum(c[0])) + "blocks" for c in ML.NET_CASES])
def test_conditions_on_the_gpu_tests_inputs(layers, seed, B):
    ref = ML.case_reference(layers, seed, B)
    worst = max(ref["trace"], key=lambda nv: nv[1])
    norms = ref["f64"]["features"].norm(dim=1)
    print(f"max |activation| {worst[1]:.1f} at {worst[0]}, feature norms {norms.tolist()}, max |shape| {float(ref['f64']['shape_params'].abs().max()):.3f}")
    assert worst[1] < 1e3
    assert float(norms.min()) > 1.0
    assert float(ref["f64"]["shape_params"].abs().max()) < 10.0
    assert len(ref["trace"]) == 1 + 2 * sum(layers) + 2


@pytest.fixture()
def reference_classes(monkeypatch):
    from oracle import sandbox as S
    if not S.available():
        pytest.skip("the reference tree is not present")
    for name in [n for n in sys.modules if n == "src" or n.startswith("src.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(S.REF_ROOT)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)                                              # the reference tree is read-only
    arc = importlib.import_module("src.models.MICA.arcface")
    mica = importlib.import_module("src.models.MICA.mica")
    yield arc, mica
    for name in [n for n in sys.modules if n == "src" or n.startswith("src.")]:
        sys.modules.pop(name, None)


@pytest.mark.parametrize("layers,seed", [((1, 1, 1, 1), 1), (ML.FULL, 3)], ids=["4blocks", "full"])
def test_law_is_the_references_arithmetic(reference_classes, layers, seed):
    arc, mica = reference_classes
    ckpt, img = ML.synth_checkpoint(layers, seed), ML.synth_images(2, seed)
    net = arc.IResNet(arc.IBasicBlock, list(layers))
    net.load_state_dict(ckpt["arcface"], strict=True)
    reg = mica.MappingNetwork(512, 300, 300, hidden=3)
    reg.load_state_dict({k.replace("regressor.", ""): v for k, v in ckpt["flameModel"].items() if "network" in k or "output" in k}, strict=True)
    net, reg = net.double().eval(), reg.double().eval()
    with torch.no_grad():
        feat = net(((img.double() - 0.5) / 0.5)[:, [2, 1, 0]])
        shape = reg(torch.nn.functional.normalize(feat))
    law = ML.mica_law(ckpt, img, layers)
    for name, got, want in (("features", law["features"], feat), ("shape_params", law["shape_params"], shape)):
        rel = float((got - want).abs().max()) / float(want.abs().max())
        print(f"{name}: law against the reference's classes {rel:.2e} relative")
        assert rel <= 1e-10, name


def test_folding_reproduces_the_unfolded_law():
    """float64: the epilogue scales / shifts and the permuted, folded FC matrix and bias of smirk_amd.mica against the law's BatchNorm / flatten / Linear"""
    from smirk_amd import MICA
    from smirk_amd.mica import bn_affine, fold_fc
    layers, seed = (1, 1, 1, 1), 1
    ckpt = ML.synth_checkpoint(layers, seed)
    m, sd = MICA(ckpt, layers=layers), ckpt["arcface"]
    g = torch.Generator().manual_seed(5)
    for name, bn in [(n, mod) for n, mod in m.arcface.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)]:
        x = torch.randn(2, bn.num_features, 3, 3, generator=g, dtype=torch.float64)
        s, t = bn_affine(bn)
        want = ML._norm(sd, name, x, torch.float64)
        assert s.dtype == torch.float64 and float((x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1) - want).abs().max()) <= 1e-10 * float(want.abs().max()), name
    x = torch.randn(2, 512, 7, 7, generator=g, dtype=torch.float64)                                    # the last block's output, NCHW
    w, b = fold_fc(m.arcface.fc, m.arcface.bn2, m.arcface.features, 49)
    flat = ML._norm(sd, "bn2", x, torch.float64).reshape(2, -1)
    want = ML._norm(sd, "features", torch.nn.functional.linear(flat, sd["fc.weight"].double(), sd["fc.bias"].double()), torch.float64)
    got = x.permute(0, 2, 3, 1).reshape(2, -1) @ w.t() + b                                             # what the FC kernel computes on the NHWC tensor
    assert w.dtype == torch.float64 and tuple(w.shape) == (512, 25088) and tuple(b.shape) == (512,)
    assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())


def test_gpu_feature_bound_sees_three_mistakes():
    """Each mistake moves the law's features by more than 100 times the bound tests/test_mica_gpu.py holds the features to."""
    layers, seed, B = ML.NET_CASES[0]
    ref = ML.case_reference(layers, seed, B)
    feat = ref["f64"]["features"]
    e32 = float((ref["f32"]["features"].double() - feat).abs().max())
    bound = max(4 * e32, 2e-6 * float(feat.abs().max()))
    for variant in ("nhwc_flatten", "no_reorder", ("drop_bn1", 0), ("drop_bn1", sum(layers) - 1)):
        moved = float((ML.mica_law(ref["ckpt"], ref["images"], layers, variant=variant)["features"] - feat).abs().max())
        print(f"{variant}: moves the features by {moved:.3g} = {moved / bound:.3g} x the bound {bound:.3g}")
        assert moved > 100 * bound, variant
