"""conv_upcat.hip on the GPU: decoder levels 1 / 2 of SmirkGenerator with the ConvTranspose2d composed into the convolution that reads it, against a float64
run of the oracle and against the two-launch path ($SMIRK_CONV_RING=0).  The ConvTranspose biases are drawn N(0, 1): a wrong border variant of the composed bias
then shows far above the tolerances.  Shapes: 64 x 64 and 64 x 96 take level 1 only (level 2's 32-pixel side is below the kernel's 64), 128 x 128 and 128 x 160
take both; 4 x 4 patches and more, so corner, edge and interior pixels of every class are present."""
import pytest
import torch

from oracle import assets as A
from oracle import generator_ref as G

pytestmark = pytest.mark.gpu

OUT_TOL = 2e-5        # tests/test_generator_gpu.py: abs, on the sigmoid output
ACT_RTOL = 2e-4       # intermediate activations, relative to the tensor's max magnitude
CONVT = "conv_igemm_kernel<128,128,2,2,true,4>"
SHAPES = {"64x64_B2": (64, 64, 2, 1), "64x96_B3": (64, 96, 3, 1), "128x128_B1": (128, 128, 1, 2), "128x160_B2": (128, 160, 2, 2)}   # H, W, B, composed levels


@pytest.fixture(scope="module")
def net():
    from smirk_amd import SmirkGenerator
    sd = G.synth_state_dict(res_blocks=1, seed=4321, calibrate=False)
    g = torch.Generator().manual_seed(99)
    for lvl in (4, 3, 2, 1):
        sd[f"upconv{lvl}.bias"] = torch.randn(sd[f"upconv{lvl}.bias"].shape, generator=g)
    # BatchNorm statistics and the logit scale from one small batch, with those biases in place (activations O(1), sigmoid not saturated)
    G.forward(sd, A.synth_generator_input(2, seed=777)[:, :, 64:128, 64:128].contiguous(), 1, _calib=g)
    m = SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=1)
    m.load_state_dict(sd, strict=True)
    m.precision = "f16x3"
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return m.cuda().eval(), sd64


@pytest.fixture(scope="module")
def cases(net):
    """per shape: the input and the float64 reference (output + taps), computed once"""
    _, sd64 = net
    out = {}
    for name, (H, W, B, _) in SHAPES.items():
        x = A.synth_generator_input(B, seed=11 + H + W)[:, :, 32:32 + H, 16:16 + W].contiguous()
        taps = {}
        y = G.forward(sd64, x.double(), 1, taps=taps)
        out[name] = (x, y, {k: taps[k] for k in ("dec2", "dec1")})
    return out


def _run(m, x, taps=False):
    from smirk_amd.smirk_generator import split16_to_float
    with torch.no_grad():
        if not taps:
            return m(x.cuda()).cpu(), None
        t = {}
        y = m(x.cuda(), _taps=t)
        torch.cuda.synchronize()
        return y.cpu(), {k: split16_to_float(t[k]).permute(0, 3, 1, 2).cpu() for k in ("dec2", "dec1")}


@pytest.mark.parametrize("name", list(SHAPES))
def test_composed_levels_match_float64_and_the_two_launch_path(net, cases, name, monkeypatch):
    m, _ = net
    x, yr, tr = cases[name]
    y, _ = _run(m, x)
    yt, t = _run(m, x, taps=True)
    monkeypatch.setenv("SMIRK_CONV_RING", "0")
    y0, _ = _run(m, x)
    monkeypatch.delenv("SMIRK_CONV_RING")
    e_new, e_old = (y.double() - yr).abs().max().item(), (y0.double() - yr).abs().max().item()
    msg = f"{name}: max |out - float64| composed {e_new:.3g}, two-launch {e_old:.3g}"
    assert e_new < OUT_TOL, msg
    assert (yt.double() - yr).abs().max().item() < OUT_TOL, msg
    assert (y - y0).abs().max().item() < OUT_TOL, msg
    for k in ("dec2", "dec1"):
        err = (t[k].double() - tr[k]).abs().max().item() / tr[k].abs().max().item()
        assert err < ACT_RTOL, (k, err, msg)


@pytest.mark.parametrize("name", list(SHAPES))
def test_profiler_names_the_composed_kernel_once_per_level(net, cases, name, monkeypatch):
    from smirk_amd import _lib as L
    m, _ = net
    x = cases[name][0].cuda()
    nlev = SHAPES[name][3]

    def names():
        L.profile_start()
        try:
            with torch.no_grad():
                m(x)
            torch.cuda.synchronize()
        finally:
            recs = L.profile_stop()
        return [r[0] for r in recs]

    on = names()
    monkeypatch.setenv("SMIRK_CONV_RING", "0")
    off = names()
    monkeypatch.delenv("SMIRK_CONV_RING")
    want = ["conv3x3_upcat_kernel<2>", "conv3x3_upcat_kernel<1>"][2 - nlev:]
    assert [n.split("[")[0] for n in on if n.startswith("conv3x3_upcat_kernel")] == want
    assert [n for n in on if n.startswith("upcat_compose_kernel")] == ["upcat_compose_kernel<2>", "upcat_compose_kernel<1>"][2 - nlev:]
    assert not any(n.startswith(("conv3x3_upcat_kernel", "upcat_compose_kernel")) for n in off)
    # four ConvTranspose levels in all: the composed ones launch none
    assert sum(n.startswith(CONVT) for n in off) - sum(n.startswith(CONVT) for n in on) == nlev, (on, off)


def test_batch_invariant_and_repeatable(net, cases):
    m, _ = net
    x = cases["128x160_B2"][0].cuda()
    with torch.no_grad():
        y = m(x)
        assert torch.equal(y, m(x))
        for i in range(x.shape[0]):
            assert torch.equal(y[i:i + 1], m(x[i:i + 1].contiguous())), i
    x = cases["64x96_B3"][0].cuda()
    with torch.no_grad():
        y = m(x)
        for i in range(x.shape[0]):
            assert torch.equal(y[i:i + 1], m(x[i:i + 1].contiguous())), i
