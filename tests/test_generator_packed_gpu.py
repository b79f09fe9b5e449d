"""SmirkGenerator.forward_packed (smirk_generator_forward_packed, include/smirk_handoff.h) against forward_pair, and the hull_mask= path of the pipelines with
the masking -> generator hand-off on and off ($SMIRK_DISABLE_MASKING_HANDOFF): the same bits, key for key."""
import os

import pytest
import torch

from oracle import assets as A
from oracle import generator_ref as G

pytestmark = pytest.mark.gpu

SWITCH = "SMIRK_DISABLE_MASKING_HANDOFF"


@pytest.fixture(scope="module")
def gen():
    from smirk_amd import SmirkGenerator
    m = SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=5)
    m.load_state_dict(G.synth_state_dict(), strict=True)
    return m.cuda().eval()


def _pack(rendered, masked):
    from smirk_amd import _lib as L
    B, _, H, W = rendered.shape
    out = torch.empty(B, H, W, 8, device=rendered.device)
    L.check(L.lib().smirk_pack_generator_input_split16(L.ptr(rendered), 3, L.ptr(masked), 3, L.ptr(out), B, H, W, L.stream_ptr()))
    return out


@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 32, 48)])
def test_forward_packed_equals_forward_pair(gen, B, H, W):
    x = A.synth_generator_input(B, seed=21)[:, :, 64:64 + H, 80:80 + W].contiguous().cuda()
    rendered, masked = x[:, :3].contiguous(), x[:, 3:].contiguous()
    with torch.no_grad():
        want = gen.forward_pair(rendered, masked)
        got = gen.forward_packed(_pack(rendered, masked))
    torch.cuda.synchronize()
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_forward_packed_refuses_what_it_does_not_serve(gen):
    from smirk_amd import SmirkHipError
    packed = torch.zeros(1, 32, 32, 8, device="cuda")
    with pytest.raises(SmirkHipError, match="packed"):
        gen.forward_packed(packed[..., :4])
    with pytest.raises(SmirkHipError, match="multiple of 16"):
        gen.forward_packed(torch.zeros(1, 40, 32, 8, device="cuda"))
    gen.precision = "f32"
    try:
        assert not gen.accepts_packed()
        with pytest.raises(SmirkHipError, match="f16x3"):
            gen.forward_packed(packed)
    finally:
        gen.precision = "f16x3"


def test_pipelines_with_the_hand_off_on_and_off(gen, sandbox, monkeypatch):
    from oracle import mobilenet_ref as MB
    from smirk_amd import FLAME, Renderer, SmirkEncoder
    from smirk_amd import masking as M
    from smirk_amd.pipeline import OverlappedPipeline, SmirkPipeline
    cwd = os.getcwd(); os.chdir(sandbox)
    try:
        fl, rn = FLAME().cuda(), Renderer().cuda()
        prob = M.load_probabilities_per_FLAME_triangle().cuda()
    finally:
        os.chdir(cwd)
    enc = SmirkEncoder(); enc.load_state_dict(MB.synth_encoder_state_dict()); enc = enc.cuda().eval()
    pipe = SmirkPipeline(enc, fl, rn, gen, face_probabilities=prob)
    img = A.synth_images(2, seed=9).cuda()
    hull = (A.synth_generator_input(2, seed=9)[:, 3:4] != 0).float().cuda()
    calls = []
    real = gen.forward_packed
    monkeypatch.setattr(gen, "forward_packed", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setenv(SWITCH, "1")
    off = pipe(img, hull_mask=hull, mask_rng=M.PhiloxStream(5, 77))
    assert not calls
    monkeypatch.delenv(SWITCH)
    on = pipe(img, hull_mask=hull, mask_rng=M.PhiloxStream(5, 77))
    assert len(calls) == 1                                                 # the packed entry really served the call
    run = OverlappedPipeline(pipe)
    assert run.submit(img, hull_mask=hull, mask_rng=M.PhiloxStream(5, 77)) is None
    over = run.flush()
    assert len(calls) == 2
    torch.cuda.synchronize()
    assert set(on) == set(off) == set(over) and "masked_img" in on and "reconstructed_img" in on
    for k, v in off.items():
        if torch.is_tensor(v):
            bits = torch.int32 if v.dtype == torch.float32 else v.dtype
            for other in (on, over):
                assert other[k].shape == v.shape and torch.equal(other[k].contiguous().view(bits), v.contiguous().view(bits)), k
        else:
            assert on[k] == v and over[k] == v, k
    assert bool((on["masked_img"] != img).any()) and torch.isfinite(on["reconstructed_img"]).all()
