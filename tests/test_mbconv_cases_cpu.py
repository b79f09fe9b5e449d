"""The MBConv block harness (tests/mbconv_cases.py) checked where no GPU is needed: its float64 reference against the oracle's own block modules, and its case
table against the kernel's template space and the backbones' block shapes (smirk_mbconv_supported is host code: the library loads without a device)."""
import pytest
import torch

import mbconv_cases as MC
from oracle import mobilenet_ref as M


def _oracle_block(block):
    """oracle.mobilenet_ref.IR / DS in float64 eval mode carrying the block's decoded weights; BatchNorm set so that its folded scale / shift are the case's
    (running_mean 0, running_var 1 - eps: the normalisation is the identity)"""
    c = block.case
    x64, we64, wp64 = MC.decoded(block)
    if c.kind == "ir":
        m = M.IR(c.cin, c.cout, c.stride, c.mid / c.cin)
        assert m.conv_pw.out_channels == c.mid
        convs = [(m.conv_pw, we64[:, :, None, None]), (m.conv_dw, block.wd.double()[:, None]), (m.conv_pwl, wp64[:, :, None, None])]
        bns = [m.bn1, m.bn2, m.bn3]
        aff = block.aff
    else:
        m = M.DS(c.cin, c.cout, c.stride)
        convs = [(m.conv_dw, block.wd.double()[:, None]), (m.conv_pw, wp64[:, :, None, None])]
        bns = [m.bn1, m.bn2]
        aff = block.aff[1:]
    m = m.double().eval()
    with torch.no_grad():
        for conv, w in convs:
            assert conv.weight.shape == w.shape
            conv.weight.copy_(w)
        for bn, (s, b) in zip(bns, aff):
            bn.weight.copy_(s.double()); bn.bias.copy_(b.double())
            bn.running_mean.zero_(); bn.running_var.fill_(1.0 - bn.eps)
    m.has_skip = c.residual          # the table also runs skip-capable shapes with the residual off
    return m, x64


@pytest.mark.parametrize("case", MC.CASES_FUSED + MC.UNSUPPORTED_PRODUCT_SHAPES, ids=MC.case_id)
def test_reference64_equals_the_oracle_block(case):
    """the harness's reference cannot share a padding (or wiring) mistake with the kernels: it equals the oracle's IR / DS module to 1e-12 relative"""
    block = MC.block_of(case)
    m, x64 = _oracle_block(block)
    with torch.no_grad():
        want = m(x64).permute(0, 2, 3, 1)
    got = MC.reference_of(case)
    Ho, Wo = (case.H + case.stride - 1) // case.stride, (case.W + case.stride - 1) // case.stride
    assert got.shape == want.shape == (case.B, Ho, Wo, case.cout)
    assert float(want.abs().max()) > 0.5                                      # not a degenerate all-zero block
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_reference_inputs_are_the_exact_split16_values():
    """the float64 reference reads what the kernels read: hi + lo / 2048 of the split16 encoding, within 2^-21 of the fp32 operand"""
    block = MC.block_of(MC.CASES_FUSED[0])
    x64, we64, wp64 = MC.decoded(block)
    for dec, src in ((x64.permute(0, 2, 3, 1), block.x), (we64, block.we), (wp64, block.wp)):
        err = (dec - src.double()).abs()
        assert float(err.max()) > 0.0 and bool((err <= 2.0 ** -21 * src.double().abs().clamp_min(2.0 ** -14)).all())


def test_table_reaches_every_instantiation_and_edge():
    """all 12 mbconv_fused_kernel<S, EXP, KS> instantiations, every geometry at both kinds, the ragged channel counts, residual on and off"""
    T = MC.CASES_FUSED
    assert {MC.kernel_variant(c) for c in T} == {(s, e, k) for s in (1, 2) for e in (True, False) for k in (1, 2, 3)}
    for kind in ("ir", "ds"):
        assert {(c.H, c.W) for c in T if c.stride == 1 and c.kind == kind} >= set(MC.GEOM_S1)
        assert {(c.H, c.W) for c in T if c.stride == 2 and c.kind == kind} >= set(MC.GEOM_S2)
    for s in (1, 2):
        ir = [c for c in T if c.kind == "ir" and c.stride == s]
        assert {c.cin for c in ir} >= {8, 16, 24, 40, 48}
        assert {c.cout for c in ir} >= {8, 24, 40, 72, 96}
        assert {c.cin for c in T if c.kind == "ds" and c.stride == s} >= {8, 16, 24, 40, 48}
    mids = {c.mid for c in T if c.kind == "ir"}
    assert mids >= {8, 72, 88, 104, 120} and max(mids) >= 192
    assert any(c.cout == 96 and c.stride == 1 for c in T)                      # 6 project tiles over 4 waves
    for kind in ("ir", "ds"):
        legal = [c for c in T if c.kind == kind and c.stride == 1 and c.cin == c.cout]
        assert any(c.residual for c in legal) and any(not c.residual for c in legal)
    assert {c.B for c in T} == {1, 2, 3}
    assert {c.stride for c in MC.BATCH_CASES} == {1, 2} and all(c in T and c.B == 3 for c in MC.BATCH_CASES)
    assert all(not c.residual or (c.stride == 1 and c.cin == c.cout) for c in T)


def test_table_holds_every_block_shape_the_kernel_accepts():
    """every DepthwiseSeparable / InvertedResidual block of both backbones that smirk_mbconv_supported accepts is in CASES_FUSED, every table case is accepted,
    and the one product shape the kernel refuses is the documented one"""
    from smirk_amd import _lib as L
    lib = L.lib()
    have = {(c.cin, c.mid, c.cout, c.stride, c.kind) for c in MC.CASES_FUSED}
    accepted = [s for s in MC.arch_block_shapes() if lib.smirk_mbconv_supported(s[0], s[1], s[2], s[3])]
    assert len(accepted) >= 10
    assert not [s for s in accepted if s not in have]
    assert all(lib.smirk_mbconv_supported(c.cin, c.mid, c.cout, c.stride) for c in MC.CASES_FUSED)
    for c in MC.UNSUPPORTED_PRODUCT_SHAPES:
        assert (c.cin, c.mid, c.cout, c.stride, c.kind) in MC.arch_block_shapes()
        assert not lib.smirk_mbconv_supported(c.cin, c.mid, c.cout, c.stride)
        assert lib.smirk_mbconv_lds_bytes(c.cin, c.mid, c.cout, c.stride) > 64 * 1024


def test_where_names_the_offending_indices():
    err = torch.zeros(2, 4, 5, 8, dtype=torch.float64)
    assert MC.where(err, 1e-6) == ""
    err[1, 3, :, 2] = 1.0
    err[0, 0, 4, 7] = float("nan")                                            # an element that was never written
    msg = MC.where(err, 1e-6)
    assert "6 of 320" in msg and "b=[0, 1]" in msg and "y=[0, 3]" in msg and "x=[0, 1, 2, 3, 4]" in msg and "c=[2, 7]" in msg
