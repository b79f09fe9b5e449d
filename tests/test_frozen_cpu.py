"""smirk_amd.frozen without a GPU: the frame that VGGPerceptualLoss, ExpressionLoss and MICA share.  The freeze and the pinned eval mode, the operand cache (what
it is keyed on, when it rebuilds, that a rebuild hands out a fresh object, that the device is part of the key), the float64 BatchNorm fold, the parameter
holder, checkpoint reading, the refusals of the input conditioning, and the single-use tape error.  Nothing here launches a kernel: every refusal comes first."""
import pytest
import torch
import torch.nn as nn


def _net(pin):
    from smirk_amd import frozen

    class Net(frozen.FrozenNetwork):
        pin_eval = pin

        def __init__(self):
            super().__init__()
            self.conv, self.bn, self.builds = nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), 0
            self.freeze()

        def _build_operands(self, dev):
            self.builds += 1
            return object()

    return Net()


CPU = torch.device("cpu")


def test_freeze_and_pinned_eval():
    for pin in (True, False):
        m = _net(pin)
        assert list(m.parameters()) and all(not p.requires_grad for p in m.parameters())
    m = _net(True)
    assert not m.training and not m.bn.training                                                          # freeze() of a pinned network leaves it in eval mode
    assert m.train(True) is m and not any(mod.training for mod in m.modules())
    assert m.train() is m and not any(mod.training for mod in m.modules())
    m = _net(False)
    assert m.training and m.train(False) is m and not any(mod.training for mod in m.modules())          # as nn.Module's
    assert m.train(True) is m and all(mod.training for mod in m.modules())


def test_operands_are_built_once_and_again_after_every_change():
    m = _net(True)
    ops = m._operands(CPU)
    assert m.builds == 1 and m._operands(CPU) is ops and m.builds == 1
    m.bn.num_batches_tracked += 1                                                                        # not read by the arithmetic
    assert m._operands(CPU) is ops and m.builds == 1
    changes = (lambda: m.conv.weight.mul_(2), lambda: m.bn.running_mean.add_(1), lambda: m.load_state_dict(m.state_dict()), lambda: m.to(torch.float32))
    for n, change in enumerate(changes):
        with torch.no_grad():
            change()
        new = m._operands(CPU)
        assert m.builds == 2 + n and new is not ops, n                                                   # a fresh object: the old one may sit on a tape
        assert m._operands(CPU) is new and m.builds == 2 + n
        ops = new


def test_device_and_dtype_are_checked_and_the_device_is_in_the_key():
    import smirk_amd
    other = torch.device("cuda", 0)                                                                      # only compared, never used: the check precedes any launch
    m = _net(False)
    with pytest.raises(smirk_amd.SmirkHipError, match="Net"):
        m._operands(other)
    ops = m._operands(CPU)
    with pytest.raises(smirk_amd.SmirkHipError, match="Net"):                                            # after a build for the parameters' device, too
        m._operands(other)
    assert m.builds == 1 and m._operands(CPU) is ops
    m.double()
    with pytest.raises(smirk_amd.SmirkHipError, match="fp32"):
        m._operands(CPU)
    assert m.builds == 1


def test_bn_affine_is_the_float64_fold_and_one_function():
    from smirk_amd import expression_loss, frozen, mica
    assert mica.bn_affine is expression_loss.bn_affine is frozen.bn_affine
    g = torch.Generator().manual_seed(0)
    bn = nn.BatchNorm2d(37, eps=1e-3)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(37, generator=g)); bn.bias.copy_(torch.randn(37, generator=g))
        bn.running_mean.copy_(torch.randn(37, generator=g)); bn.running_var.copy_(torch.rand(37, generator=g) + 0.1)
    s, t = frozen.bn_affine(bn)
    want_s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    want_t = bn.bias.detach().double() - bn.running_mean.double() * want_s
    assert s.dtype == t.dtype == torch.float64
    assert float(((s - want_s).abs() / want_s.abs()).max()) <= 1e-15 and float(((t - want_t).abs() / want_t.abs()).max()) <= 1e-15
    assert frozen.host64(bn.weight).dtype == torch.float64 and not frozen.host64(bn.weight).requires_grad


def test_holder_has_no_forward_and_names_its_owner():
    import smirk_amd
    from smirk_amd import frozen

    class Layer(frozen.Holder):
        owner = "Owner"

    with pytest.raises(smirk_amd.SmirkHipError, match=frozen.Holder.owner):
        frozen.Holder().forward()
    with pytest.raises(smirk_amd.SmirkHipError, match="Layer holds the parameters of smirk_amd.Owner .*call Owner"):
        Layer()(torch.zeros(1))


def test_read_checkpoint(tmp_path, monkeypatch):
    from smirk_amd import frozen
    ckpt = {"state_dict": {"w": torch.arange(3.0)}}
    assert frozen.read_checkpoint(ckpt, "assets/net.ckpt", "Net", "'state_dict'") is ckpt
    with pytest.raises(FileNotFoundError, match=r"Net: `checkpoint` = .*nothing.ckpt.*assets/net.ckpt.*'state_dict'"):
        frozen.read_checkpoint(tmp_path / "nothing.ckpt", "assets/net.ckpt", "Net", "'state_dict'")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="checkpoint"):                                           # None = the default path
        frozen.read_checkpoint(None, "assets/net.ckpt", "Net", "'state_dict'")
    torch.save(ckpt, tmp_path / "net.ckpt")
    for path in (tmp_path / "net.ckpt", str(tmp_path / "net.ckpt")):
        assert torch.equal(frozen.read_checkpoint(path, "assets/net.ckpt", "Net", "'state_dict'", weights_only=False)["state_dict"]["w"], ckpt["state_dict"]["w"])


class _OnDevice(torch.Tensor):
    """A host tensor that says it is on the device, to reach the refusals behind the CPU one; each of them raises before anything reads the data."""
    is_cuda = True


def test_image_refusals():
    import smirk_amd
    from smirk_amd import frozen
    img = torch.zeros(2, 3, 16, 16)
    dev = lambda *shape, **k: torch.zeros(*shape, **k).as_subclass(_OnDevice)
    with pytest.raises(smirk_amd.SmirkHipError, match="Net: a is a CPU tensor"):
        frozen.image_pair("Net", ("a", "b"), img, img)
    with pytest.raises(smirk_amd.SmirkHipError, match="Net: b is a CPU tensor"):
        frozen.image_pair("Net", ("a", "b"), dev(2, 3, 16, 16), img)
    with pytest.raises(smirk_amd.SmirkHipError, match="Net: images is a CPU tensor"):
        frozen.device_image("Net", "images", img)
    for bad in (None, [img], torch.zeros(3, 16, 16), torch.zeros(2, 4, 16, 16)):
        with pytest.raises(smirk_amd.SmirkHipError, match=r"Net: a must be a \[B, 3, H, W\] tensor"):
            frozen.image_pair("Net", ("a", "b"), bad, img)
        with pytest.raises(smirk_amd.SmirkHipError, match=r"Net: b must be a \[B, 3, H, W\] tensor"):
            frozen.image_pair("Net", ("a", "b"), dev(2, 3, 16, 16), bad)
        with pytest.raises(smirk_amd.SmirkHipError, match=r"Net: images must be a \[B, 3, H, W\] tensor"):
            frozen.device_image("Net", "images", bad)
    for shape in ((1, 3, 16, 16), (2, 3, 16, 24)):
        with pytest.raises(smirk_amd.SmirkHipError, match="one shape"):
            frozen.image_pair("Net", ("a", "b"), dev(2, 3, 16, 16), dev(*shape))
    with pytest.raises(smirk_amd.SmirkHipError, match="Net: b requires grad"):
        frozen.image_pair("Net", ("a", "b"), dev(2, 3, 16, 16, requires_grad=True), dev(2, 3, 16, 16, requires_grad=True))


def test_aligned16_and_second_backward():
    from smirk_amd import _lib as L
    t = torch.arange(40.0)
    assert L.aligned16(t) is t
    off = t[1:]
    assert off.data_ptr() & 15 == 4 and L.aligned16(off).data_ptr() & 15 == 0 and torch.equal(L.aligned16(off), off)
    assert L.aligned16(t.double()).dtype == torch.float32 and L.aligned16(t.view(4, 10).t()).is_contiguous()
    e = L.second_backward("F", "x")
    assert isinstance(e, RuntimeError) and str(e).startswith("F.backward") and "second time" in str(e) and "tape of x" in str(e)
    assert "retain_graph" in str(e) and "run the forward again" in str(e)
