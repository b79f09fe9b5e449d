"""Decoder levels 3 / 4 of SmirkGenerator on the GPU with the ConvTranspose2d composed into the level's first convolution as two launches (conv_halo_up_kernel,
then the ordinary 3x3 convolution over the skip tensor with the first launch's output as its residual; conv_halo.hip), against a float64 run of the
oracle and against the two-launch levels ($SMIRK_IGEMM_HALO=0, set and unset around the one call).  The ConvTranspose biases are drawn N(0, 1): a wrong border
variant of the composed bias then shows far above the tolerances.  A level is composed when both of its launches have at least 1024 GEMM rows, so the shapes are
the smallest that reach each branch (level 4's coarse image is H/16 x W/16, level 3's H/8 x W/8; taps keep the whole batch in one chain).

The net is calibrated on WHOLE 224 x 224 frames, the batch oracle.generator_ref.synth_state_dict itself calibrates on and the one OUT_TOL was set with
(tests/test_generator_gpu.py): the cases here go up to whole frames, and every crop is a window of such a frame.  A first version copied
tests/test_upcat_gpu.py's calibration on one 64 x 64 window (its shapes are windows near that one); whole frames then drove dec1 to |x| ~ 70 instead of the
O(1) the calibration is for, and the error of BOTH paths sat at the bound (old pair 1.98e-05 .. 2.18e-05, composed pair 1.76e-05 .. 2.24e-05 over six input
seeds) — a property of the fixture, not of either path."""
import re

import pytest
import torch

from oracle import assets as A
from oracle import generator_ref as G

pytestmark = pytest.mark.gpu

OUT_TOL = 2e-5        # tests/test_generator_gpu.py: abs, on the sigmoid output
ACT_RTOL = 2e-4       # intermediate activations, relative to the tensor's max magnitude
CONVT = re.compile(r"conv_igemm_kernel<\d+,\d+,\d+,\d+,true,4>")
UP = "conv_halo_up_kernel"
# H, W, B, composed levels (level 4, level 3)
SHAPES = {
    "level3_only_64x64_B16": (64, 64, 16, (False, True)),          # level 3 coarse 8 x 8, M = 1024; level 4's 256 rows stay on the old path
    "ragged_64x64_B67": (64, 64, 67, (True, True)),                # level 4 coarse 4 x 4, M = 1072: ragged last tile
    "corners_32x32_B256": (32, 32, 256, (True, True)),             # level 4 coarse 2 x 2: every pixel a corner
    "nonsquare_64x96_B44": (64, 96, 44, (True, True)),             # width != height (level 4 coarse 4 x 6, M = 1056)
    "workload_224x224_B6": (224, 224, 6, (True, True)),            # coarse 14 and 28, tiles straddling images
}


@pytest.fixture(scope="module")
def net():
    from smirk_amd import SmirkGenerator
    sd = G.synth_state_dict(res_blocks=1, seed=4321, calibrate=False)
    g = torch.Generator().manual_seed(99)
    for lvl in (4, 3, 2, 1):
        sd[f"upconv{lvl}.bias"] = torch.randn(sd[f"upconv{lvl}.bias"].shape, generator=g)
    # BatchNorm statistics and the logit scale from one batch of whole frames (the oracle's own calibration batch), with those biases in place (activations O(1),
    # sigmoid not saturated)
    G.forward(sd, A.synth_generator_input(4, seed=777), 1, _calib=g)
    m = SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=1)
    m.load_state_dict(sd, strict=True)
    m.precision = "f16x3"
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return m.cuda().eval(), sd64


def _input(H, W, B, seed):
    """B crops of H x W from a few synthetic 224 x 224 frames (frame and crop offset both vary)"""
    nf = min(B, 8)
    base = A.synth_generator_input(nf, seed=seed)
    if H == 224 and W == 224:
        assert B <= nf
        return base[:B].contiguous()
    ys, xs = list(range(0, 224 - H + 1, 24)), list(range(0, 224 - W + 1, 24))
    crops = [base[i % nf, :, ys[(i // nf) % len(ys)]:, xs[(i // (nf * len(ys))) % len(xs)]:][:, :H, :W] for i in range(B)]
    return torch.stack(crops).contiguous()


@pytest.fixture(scope="module")
def cases(net):
    """per shape: the input and the float64 reference (output + taps), computed once"""
    _, sd64 = net
    out = {}
    for name, (H, W, B, _) in SHAPES.items():
        x = _input(H, W, B, seed=11 + H + W)
        taps = {}
        y = G.forward(sd64, x.double(), 1, taps=taps)
        out[name] = (x, y, {k: taps[k] for k in ("dec4", "dec3")})
    return out


def _run(m, x, taps=False):
    from smirk_amd.smirk_generator import split16_to_float
    with torch.no_grad():
        if not taps:
            return m(x.cuda()).cpu(), None
        t = {}
        y = m(x.cuda(), _taps=t)
        torch.cuda.synchronize()
        return y.cpu(), {k: split16_to_float(t[k]).permute(0, 3, 1, 2).cpu() for k in ("dec4", "dec3")}


def _names(m, x):
    from smirk_amd import _lib as L
    L.profile_start()
    try:
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()
    finally:
        recs = L.profile_stop()
    return [r[0] for r in recs]


@pytest.mark.parametrize("name", list(SHAPES))
def test_composed_levels_match_float64_and_the_two_launch_path(net, cases, name, monkeypatch):
    m, _ = net
    x, yr, tr = cases[name]
    y, t = _run(m, x, taps=True)                        # (taps: one chain over the whole batch, so a level's M is the table's)
    monkeypatch.setenv("SMIRK_IGEMM_HALO", "0")
    y0, t0 = _run(m, x, taps=True)
    monkeypatch.delenv("SMIRK_IGEMM_HALO")
    e_new, e_old = (y.double() - yr).abs().max().item(), (y0.double() - yr).abs().max().item()
    msg = f"{name}: max |out - float64| composed {e_new:.3g}, two-launch {e_old:.3g}"
    for k in ("dec4", "dec3"):
        mx = tr[k].abs().max().item()
        a_new, a_old = (t[k].double() - tr[k]).abs().max().item() / mx, (t0[k].double() - tr[k]).abs().max().item() / mx
        msg += f"; {k} rel composed {a_new:.3g}, two-launch {a_old:.3g}"
    print(msg)
    assert e_new < OUT_TOL, msg
    assert e_old < OUT_TOL, msg
    assert (y - y0).abs().max().item() < OUT_TOL, msg
    for k in ("dec4", "dec3"):
        mx = tr[k].abs().max().item()
        assert (t[k].double() - tr[k]).abs().max().item() / mx < ACT_RTOL, (k, msg)
        assert (t0[k].double() - tr[k]).abs().max().item() / mx < ACT_RTOL, (k, msg)


@pytest.mark.parametrize("name", list(SHAPES))
def test_profiler_names_the_new_launch_once_per_composed_level(net, cases, name, monkeypatch):
    m, _ = net
    x = cases[name][0].cuda()
    nlev = sum(SHAPES[name][3])
    on = _names(m, x)                                  # (the launch profiler keeps the whole batch in one chain)
    monkeypatch.setenv("SMIRK_IGEMM_HALO", "0")
    off = _names(m, x)
    monkeypatch.delenv("SMIRK_IGEMM_HALO")
    assert sum(n.startswith(UP) for n in on) == nlev, on
    assert sum(n.startswith("updeep_compose_kernel") for n in on) == 1, on
    assert not any(n.startswith((UP, "updeep_compose_kernel")) for n in off), off
    # four ConvTranspose levels in all; what levels 1 / 2 launch does not depend on this switch, the composed deep levels launch none
    assert sum(bool(CONVT.match(n)) for n in off) - sum(bool(CONVT.match(n)) for n in on) == nlev, (on, off)


def test_batch_invariant_and_repeatable(net, monkeypatch):
    """A single frame never has 1024 rows at these levels, so B against 2 B: 64 and 128 frames of 64 x 64 in ONE chain — level 4's M is 1024 / 2048, both composed."""
    m, _ = net
    x = _input(64, 64, 128, seed=31).cuda()
    monkeypatch.setenv("SMIRK_GEN_SPLIT_CHAINS", "0")
    names = _names(m, x[:64].contiguous())
    assert sum(n.startswith(UP) for n in names) == 2, names
    with torch.no_grad():
        y = m(x)
        assert torch.equal(y, m(x))
        assert torch.equal(y[:64], m(x[:64].contiguous()))
        assert torch.equal(y[64:], m(x[64:].contiguous()))


def test_chain_counts_bitwise_equal(net, monkeypatch):
    """1 / 2 / 3 sub-batch chains ($SMIRK_GEN_SPLIT_CHAINS = 0 / 2 / 3): 192 frames of 64 x 64 give every chain of level 4 at least 64 x 16 = 1024 rows, so each chain
    composes on its own side stream from the weights composed once ahead of the fork."""
    m, _ = net
    x = _input(64, 64, 192, seed=32).cuda()
    ys = {}
    with torch.no_grad():
        for chains in ("0", "2", "3"):
            monkeypatch.setenv("SMIRK_GEN_SPLIT_CHAINS", chains)
            ys[chains] = m(x)
        monkeypatch.setenv("SMIRK_IGEMM_HALO", "0")
        y_old = m(x)
    assert torch.equal(ys["0"], ys["2"])
    assert torch.equal(ys["0"], ys["3"])
    assert not torch.equal(ys["0"], y_old)              # the composed path ran (its rounding differs from the two-launch path's) ...
    assert (ys["0"] - y_old).abs().max().item() < OUT_TOL   # ... and agrees with it
