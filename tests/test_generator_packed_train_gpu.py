"""SmirkGenerator.forward_pair_packed against forward_pair inside autograd: the same autograd function entered one step later (no torch.cat, no pack launch), so
the output, every parameter gradient, the gradient of `rendered` and the BatchNorm running statistics must be the same bits.  B * Ke = 4 frames of 32 x 32, the
smallest size the train-mode generator tests use."""
import pytest
import torch

from oracle import generator_ref as G

pytestmark = pytest.mark.gpu

B, HW = 4, 32


def _module(sd, arith):
    from smirk_amd import SmirkGenerator
    m = SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=5)
    m.load_state_dict(sd, strict=True)
    m.train_arith = arith
    return m.cuda().train()


def _inputs():
    from smirk_amd import _lib as L
    g = torch.Generator().manual_seed(4132)
    rendered = torch.rand(B, 3, HW, HW, generator=g)
    rendered[:, :, : HW // 2, : HW // 3] = 0.0                             # background of a rendering
    masked = torch.rand(B, 3, HW, HW, generator=g)
    wgt = torch.randn(B, 3, HW, HW, generator=g)
    rendered, masked, wgt = rendered.cuda(), masked.cuda(), wgt.cuda()
    packed = torch.empty(B, HW, HW, 8, device="cuda")
    L.check(L.lib().smirk_pack_generator_input_split16(L.ptr(rendered), 3, L.ptr(masked), 3, L.ptr(packed), B, HW, HW, L.stream_ptr()))
    return rendered, masked, packed, wgt


def _freeze_and_eval(m):
    """smirk_trainer.py:108-113"""
    for p in m.parameters():
        p.requires_grad_(False)
    m.eval()


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("arith", ["f16x3", "f16x1"])
def test_forward_pair_packed_is_forward_pair_bit_for_bit(arith, mode):
    sd = G.synth_state_dict()
    rendered, masked, packed, wgt = _inputs()
    ma, mb = _module(sd, arith), _module(sd, arith)
    if mode == "eval":
        _freeze_and_eval(ma); _freeze_and_eval(mb)
    ra, rb = rendered.clone().requires_grad_(True), rendered.clone().requires_grad_(True)
    pk = packed.clone().requires_grad_(True)
    ya = ma.forward_pair(ra, masked)
    yb = mb.forward_pair_packed(rb, pk)
    assert yb.requires_grad and torch.equal(ya, yb)
    (ya * wgt).sum().backward()
    (yb * wgt).sum().backward()
    torch.cuda.synchronize()
    assert ra.grad is not None and bool(ra.grad.any()) and torch.equal(ra.grad, rb.grad)
    assert pk.grad is None                                                 # nothing flows into the packed tensor
    seen = 0
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None), k
        if pa.grad is not None:
            assert torch.equal(pa.grad, pb.grad), k
            seen += 1
    assert seen == (len(list(ma.parameters())) if mode == "train" else 0)
    moved = 0
    for (k, ba), (_, bb) in zip(ma.named_buffers(), mb.named_buffers()):
        assert torch.equal(ba, bb), k
        moved += int(k.endswith("running_mean") and not torch.equal(ba.cpu(), sd[k]))
    assert (moved > 0) == (mode == "train")                                # batch statistics in train mode, the running ones in eval mode


def test_forward_pair_packed_refuses_what_it_does_not_serve():
    from smirk_amd import SmirkGenerator
    from smirk_amd._lib import SmirkHipError
    sd = G.synth_state_dict()
    rendered, masked, packed, _ = _inputs()
    m = _module(sd, "f16x3")
    m.precision = "f32"                                                    # today's train path refuses the exact-fp32 mode
    with pytest.raises(SmirkHipError, match="split-fp16"):
        m.forward_pair_packed(rendered, packed)
    m.precision = "f16x3"
    m.eval()                                                               # eval mode and nothing asks for a gradient: forward_packed's case
    with pytest.raises(SmirkHipError, match="forward_packed"):
        m.forward_pair_packed(rendered, packed)
    with torch.no_grad(), pytest.raises(SmirkHipError, match="forward_packed"):
        m.forward_pair_packed(rendered.clone().requires_grad_(True), packed)
    m.train()
    with pytest.raises(SmirkHipError, match="packed network input"):
        m.forward_pair_packed(rendered, packed[..., :6])
    with pytest.raises(SmirkHipError):
        m.forward_pair_packed(rendered[:, :, :16], packed)                 # `rendered` and `packed` of different frames
    m.train_arith = "bf16"
    with pytest.raises(SmirkHipError, match="train_arith"):
        m.forward_pair_packed(rendered, packed)
    three = SmirkGenerator(in_channels=3, out_channels=3, init_features=32, res_blocks=5).cuda().train()
    with pytest.raises(SmirkHipError, match="in_channels == 6"):
        three.forward_pair_packed(rendered, packed)
