"""SmirkGenerator.precision = "f16x1" on the GPU: one fp16 MFMA per product block in every convolution of the levels smirk_generator_arith names, the launches
and the bits of "f16x3" everywhere else.

Accuracy is held to the law of tests/x1_law.py: err = max |y - y64| against the float64 oracle forward, and
    err_gpu <= 2 * err_emul + OUT_TOL
where err_emul is the law's own distance from float64 on the same input, computed here on the CPU.  The factor 2 is a margin, not a derivation: the emulation is one
sample of the rounding process the kernels are another sample of (the library rounds a composed decoder weight once where the law rounds twice; the two forms of the
law lie within 1.08 of each other on every shape below).  Measured err_gpu / err_emul: DESIGN.md 30."""
import re

import pytest
import torch

import generator_cases as GC
import x1_law as X
from oracle import assets as A
from oracle import generator_ref as G
from smirk_amd import _lib as L_

pytestmark = pytest.mark.gpu

OUT_TOL = 2e-5                                                        # tests/test_generator_gpu.py
RES = 5
# the smallest shapes that reach every family: (H = W, B, seed)
SHAPES = {
    "64x64-B16": (64, 16, 11),        # decoder level 3 composed, level 4 not
    "64x64-B67": (64, 67, 12),        # both deep levels composed, ragged last tile
    "32x32-B1": (32, 1, 13),          # nothing specialised
    "128x128-B2": (128, 2, 14),       # the smallest image whose 64 x 64 level reaches ring, pool-fused ring and upcat; enc1_fused and the fused tail
    "224x224-B2": (224, 2, 15),
}


def _input(S, B, seed):
    o = (224 - S) // 2
    return A.synth_generator_input(B, seed=seed)[:, :, o:o + S, o:o + S].contiguous()


@pytest.fixture(scope="module")
def sd():
    return G.synth_state_dict()


def _module(sd, precision):
    from smirk_amd import SmirkGenerator
    m = SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=RES)
    m.load_state_dict(sd, strict=True)
    m.precision = precision
    return m.cuda().eval()


@pytest.fixture(scope="module")
def x1(sd):
    return _module(sd, "f16x1")


@pytest.fixture(scope="module")
def x3(sd):
    return _module(sd, "f16x3")


@pytest.fixture(scope="module")
def arith(x1):
    a = X.arith(x1._weights())
    assert a["x1_from"] in (1, 2) and a["deep"] == "F16X1" and a["levels"] == ["F16X1" if l >= a["x1_from"] else "F16X3" for l in range(4)]
    return a


@pytest.fixture(scope="module")
def sd64(sd):
    return X.double_state_dict(sd)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_accuracy_against_the_law(x1, arith, sd64, shape):
    S, B, seed = SHAPES[shape]
    x = _input(S, B, seed)
    y64 = G.forward(sd64, x.double())
    err_emul = (X.forward(sd64, x.double(), RES, arith) - y64).abs().max().item()
    with torch.no_grad():
        y = x1(x.cuda())
    err_gpu = (y.cpu().double() - y64).abs().max().item()
    print("%s: err_gpu %.4e  err_emul %.4e  ratio %.3f" % (shape, err_gpu, err_emul, err_gpu / err_emul))
    assert torch.isfinite(y).all() and err_emul > 10 * OUT_TOL        # (the law is about a rounding that shows)
    assert err_gpu <= 2 * err_emul + OUT_TOL, (err_gpu, err_emul)


def _levels_of_launches(r):
    """the level of every launch of a single-chain forward that follows the plan report `r` (0..3, 4 = bottleneck + ResNet blocks), None for a launch that is no
    convolution of a level: input pack, weight composition, pooling, the final 1 x 1 + sigmoid"""
    enc = {"ENC1_FUSED": lambda l: [l], "CONV_POOLFUSED": lambda l: [l, l], "CONV_CONV_POOL": lambda l: [l, l, None]}
    dec = {"UPCAT": lambda l: [None, l], "UPDEEP": lambda l: [l, l], "PAIR": lambda l: [l, l]}
    out = [None] * len(GC.INPUT_LAUNCHES[L_.GEN_INPUTS[r.input]]) + [None] * bool(r.compose_mask)
    for l in range(4):
        out += enc[L_.GEN_ENCODER_FAMILIES[r.enc[l]]](l)
    out += [4] * (2 + 2 * RES)
    for l in (3, 2, 1, 0):
        out += dec[L_.GEN_DECODER_FAMILIES[r.dec[l][0]]](l) + [l]
    return out + [None] * (not r.fused_tail)



@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_launch_carries_the_arithmetic_of_its_level(x1, arith, shape):
    """between profile_start() and profile_stop(): the f16x1 tag on every convolution of a level the query calls F16X1, on no other launch"""
    S, B, _ = SHAPES[shape]
    r = L_.SmirkGeneratorPlanReport()
    assert L_.lib().smirk_generator_plan(x1._weights(), 6, 0, B, S, S, 0, r) == 0
    x = torch.zeros(B, 6, S, S, device="cuda")
    with torch.no_grad():
        L_.profile_start()
        try:
            x1(x)
            torch.cuda.synchronize()
        finally:
            names = [rec[0] for rec in L_.profile_stop()]
    levels = _levels_of_launches(r)
    assert len(names) == len(levels), (names, levels)
    want = {l: a == "F16X1" for l, a in enumerate(arith["levels"] + [arith["deep"]])}
    assert any(want.values()) and not all(want.values())
    for name, l in zip(names, levels):
        assert ("f16x1" in name) == (l is not None and want[l]), (name, l)
        if l is None:
            assert not re.match(GC.CONV + "|conv_halo_up", name), name        # the labelling above and the launch agree on what a convolution is


def test_the_levels_below_x1_from_keep_their_bits(x1, x3, arith):
    S, B, seed = SHAPES["128x128-B2"]
    x = _input(S, B, seed).cuda()
    t1, t3 = {}, {}
    with torch.no_grad():
        y1, y3 = x1(x, _taps=t1), x3(x, _taps=t3)
    torch.cuda.synchronize()
    for l in range(arith["x1_from"]):
        k = "enc%d" % (l + 1)
        assert torch.equal(t1[k].view(torch.int32), t3[k].view(torch.int32)), k
    assert not torch.equal(t1["enc4"].view(torch.int32), t3["enc4"].view(torch.int32)) and not torch.equal(y1, y3)       # ... and the arithmetic above them IS another


def test_pair_and_packed_entries_equal_forward(x1, sandbox):
    """forward_pair == forward(cat), and forward_packed after masking.demo_masked_image_packed == forward_pair after demo_masked_image under one PhiloxStream"""
    import os
    from oracle.flame_ref import FlameRef
    from smirk_amd import masking as M
    x = _input(64, 2, 21).cuda()
    with torch.no_grad():
        assert torch.equal(x1.forward_pair(x[:, :3].contiguous(), x[:, 3:].contiguous()), x1(x))
    cwd = os.getcwd(); os.chdir(sandbox)
    try:
        prob = M.load_probabilities_per_FLAME_triangle().cuda()
    finally:
        os.chdir(cwd)
    faces = torch.from_numpy(FlameRef(sandbox).faces).cuda()
    g = torch.Generator().manual_seed(61)
    img, rendered = torch.rand(2, 3, 64, 64, generator=g).cuda(), torch.rand(2, 3, 64, 64, generator=g)
    rendered[:, :, :32, :40] = 0.0                                       # background of the rendering
    rendered = rendered.cuda()
    hull = torch.ones(2, 1, 64, 64)
    hull[:, :, 16:48, 20:44] = 0
    hull = hull.cuda()
    tv = (torch.randn(2, 5023, 3, generator=g) * 0.9).cuda()
    with torch.no_grad():
        masked = M.demo_masked_image(img, hull, rendered, tv, faces, prob, mask_ratio=0.04, rng=M.PhiloxStream(5, 77))
        want = x1.forward_pair(rendered, masked)
        masked_p, packed = M.demo_masked_image_packed(img, hull, rendered, tv, faces, prob, mask_ratio=0.04, rng=M.PhiloxStream(5, 77))
        assert packed is not None and x1.accepts_packed()
        got = x1.forward_packed(packed)
    torch.cuda.synchronize()
    assert torch.equal(masked_p.view(torch.int32), masked.view(torch.int32)) and torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("chains", ["0", "2", "3"])
@pytest.mark.parametrize("B", [3, 20])
def test_sub_batch_chains_are_bitwise_the_single_chain(x1, chains, B, monkeypatch):
    x = _input(224, B, 31).cuda()
    monkeypatch.setenv("SMIRK_GEN_SPLIT_CHAINS", "0")
    with torch.no_grad():
        ref = x1(x).clone()
    monkeypatch.setenv("SMIRK_GEN_SPLIT_CHAINS", chains)
    with torch.no_grad():
        y = x1(x)
    torch.cuda.synchronize()
    assert torch.equal(y, ref)


def test_a_frame_does_not_depend_on_the_batch_it_travels_in(x1):
    x = _input(224, 20, 32).cuda()
    with torch.no_grad():
        y20 = x1(x).clone()
        y7 = x1(x[5:12].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y7, y20[5:12])


def test_overflow_raises_in_f16x1_too(sd):
    """the checkpoint of test_split_fp16_overflow_raises_instead_of_returning_nan_pixels: the epilogues of the one-MFMA kernels audit what they store"""
    import smirk_amd
    from smirk_amd import SmirkHipError, _lib as L
    bad = {k: (v * 1e4 if (k.endswith("conv1.weight") or k.endswith("conv2.weight")) else v) for k, v in sd.items()}
    m = _module(bad, "f16x1")
    x = _input(64, 2, 5).cuda()
    try:
        with torch.no_grad():
            m(x)
            with pytest.raises(SmirkHipError, match="split-fp16"):
                smirk_amd.check_numerics()
            m(x)
            torch.cuda.synchronize()
            with pytest.raises(SmirkHipError, match="split-fp16"):    # "raise on the next call"
                m(x)
    finally:
        torch.cuda.synchronize()
        L.lib().smirk_range_flag_clear()


def test_train_mode_ignores_the_inference_precision(sd):
    """.train() under precision "f16x1": `train_arith` alone decides the arithmetic — forward and every gradient bitwise those of precision "f16x3" """
    outs = []
    x = _input(64, 2, 51)
    w = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(52)).cuda()
    for precision in ("f16x3", "f16x1"):
        m = _module(sd, precision).train()
        m.train_arith = "f16x3"
        xg = x.cuda().requires_grad_(True)
        y = m(xg)
        (y * w).sum().backward()
        torch.cuda.synchronize()
        outs.append((y.detach(), xg.grad, {k: p.grad for k, p in m.named_parameters()}, dict(m.named_buffers())))
    (y3, g3, p3, b3), (y1, g1, p1, b1) = outs
    assert torch.equal(y1, y3) and torch.equal(g1, g3)
    assert set(p1) == set(p3) and all(p1[k] is not None and torch.equal(p1[k], p3[k]) for k in p3)
    assert all(torch.equal(b1[k], b3[k]) for k in b3)
