"""smirk_amd.augment on the MI355X: the two kernels against their host restatement (tests/augment_law.py: same Philox integers, float64), the seeding
contract shared with smirk_amd.masking, and cycle.second_path against its two halves."""
import os

import numpy as np
import pytest
import torch

from augment_law import n_counters, restate, synth_inputs, synth_templates

pytestmark = pytest.mark.gpu

# |kernel - restatement|: values stay below ~20; the fp32 Box-Muller (logf, sincospif, one sqrt) is within ~4e-7 relative of the float64 one at radius <= 5.8,
# times gains <= 3 and a few fp32 roundings of O(10) values (1e-6 each); a wiring error is >= 1e-2.
TOL = 2e-5
SEED, OFFSET = 0xC0FFEE1234567, (1 << 40) + 12345             # the offset crosses into the counter's high word


def _bank(width):
    from smirk_amd import TemplateBank
    return TemplateBank(synth_templates(width=width), num_expression=width).cuda()


@pytest.mark.parametrize("E,num_expression", [(50, 50), (50, 40), (100, 100), (100, 40)])
@pytest.mark.parametrize("B,Ke", [(1, 1), (3, 1), (5, 1), (2, 3), (64, 1), (257, 1), (1025, 4)])
def test_kernels_equal_the_restatement(B, Ke, E, num_expression):
    from smirk_amd import augment_flame_params
    from smirk_amd.masking import PhiloxStream
    enc = synth_inputs(B, E=E, S=300, seed=B + E)
    bank = _bank(num_expression)
    dev = {k: torch.from_numpy(v).cuda() for k, v in enc.items()}
    for use_eyelids in ((True, False) if (B, Ke) == (5, 1) else (True,)):
        stream = PhiloxStream(SEED, OFFSET)
        out, plan = augment_flame_params(dev, bank, Ke=Ke, num_expression=num_expression, use_eyelids=use_eyelids, _rng_stream=stream, _return_plan=True)
        assert stream.offset == OFFSET + n_counters(Ke * B, E)
        want, wplan = restate(enc, Ke, bank.table.cpu().numpy(), bank.offsets_host, num_expression, use_eyelids, SEED, OFFSET)
        assert np.array_equal(plan.cpu().numpy(), wplan)
        worst = 0.0
        for k in ("expression_params", "jaw_params", "eyelid_params"):
            assert tuple(out[k].shape) == want[k].shape and out[k].dtype == torch.float32 and not out[k].requires_grad
            worst = max(worst, float(np.abs(out[k].cpu().numpy().astype(np.float64) - want[k]).max()))
        print(f"B={B} Ke={Ke} E={E} ne={num_expression}: max |kernel - restatement| = {worst:.3e}")
        assert worst < TOL
        for k in ("shape_params", "pose_params", "cam"):
            assert torch.equal(out[k], torch.cat(Ke * [dev[k]]))


def test_seeding_contract():
    from smirk_amd import augment_flame_params
    from smirk_amd.masking import PhiloxStream
    bank = _bank(50)
    dev = {k: torch.from_numpy(v).cuda() for k, v in synth_inputs(32, seed=3).items()}
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)
    torch.manual_seed(123)
    a = augment_flame_params(dev, bank, Ke=2)
    b = augment_flame_params(dev, bank, Ke=2)
    torch.manual_seed(123)
    a2 = augment_flame_params(dev, bank, Ke=2)
    assert same(a, a2) and not same(a, b)                      # reproducible from torch's seed, successive calls differ
    assert set(a) == set(dev) and a["expression_params"].shape == (64, 50)
    # an explicit stream: reproducible, advances by the documented count, leaves torch's generators alone
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    s1, s2 = PhiloxStream(77, 1000), PhiloxStream(77, 1000)
    c, d = augment_flame_params(dev, bank, Ke=2, _rng_stream=s1), augment_flame_params(dev, bank, Ke=2, _rng_stream=s2)
    assert same(c, d) and s1.offset == s2.offset == 1000 + 64 * 50
    e = augment_flame_params(dev, bank, Ke=2, _rng_stream=s1)
    assert not same(c, e) and s1.offset == 1000 + 2 * 64 * 50
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), gpu_state)


def test_refusals_on_the_device():
    from smirk_amd import SmirkHipError, TemplateBank, augment_flame_params
    from smirk_amd.augment import MAX_ROWS
    dev = {k: torch.from_numpy(v).cuda() for k, v in synth_inputs(MAX_ROWS // 2 + 1, seed=1).items()}
    with pytest.raises(SmirkHipError):
        augment_flame_params(dev, _bank(50), Ke=2)             # Ke * B above the cap
    with pytest.raises(SmirkHipError):
        augment_flame_params(dev, TemplateBank(synth_templates()), Ke=1)       # bank left on the host
    with pytest.raises(SmirkHipError):
        augment_flame_params(dev, _bank(40), Ke=1)             # bank built for another num_expression


def test_second_path_is_augment_then_render(sandbox):
    """cycle.second_path == augment_flame_params followed by render_second_path, bit for bit, from the same generator state (B = 2, Ke = 2)."""
    from oracle import assets as A
    from smirk_amd import FLAME, Renderer, augment_flame_params, masking as MK
    from smirk_amd.cycle import render_second_path, second_path
    cwd = os.getcwd(); os.chdir(sandbox)
    try:
        flame, rend = FLAME().cuda(), Renderer().cuda()
        prob = MK.load_probabilities_per_FLAME_triangle().cuda()
    finally:
        os.chdir(cwd)
    B, Ke = 2, 2
    enc = {k: torch.from_numpy(v).cuda() for k, v in A.synth_flame_params(B, seed=21).items()}
    enc["cam"] = torch.from_numpy(A.synth_cam(B, seed=21)).cuda()
    img = A.synth_images(B, seed=21).cuda()
    masks = (A.synth_generator_input(B, seed=21)[:, 3:4] != 0).float().contiguous().cuda()
    bank = _bank(50)
    torch.manual_seed(99)
    feats, rendered, masked = second_path(flame, rend, enc, bank, img, masks, prob, MK, Ke=Ke)
    torch.manual_seed(99)
    feats2 = augment_flame_params(enc, bank, Ke=Ke)
    rendered2, masked2 = render_second_path(flame, rend, enc, feats2, img, masks, prob, MK, Ke=Ke)
    assert all(torch.equal(feats[k], feats2[k]) for k in feats2) and set(feats) == set(feats2)
    assert tuple(rendered.shape) == (Ke * B, 3, 224, 224) and torch.equal(rendered, rendered2) and torch.equal(masked, masked2)
    assert rendered.abs().sum() > 0 and torch.isfinite(masked).all()
