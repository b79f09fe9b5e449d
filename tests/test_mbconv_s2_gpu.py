"""csrc/mbconv_s2.hip at the kernel level: smirk_mbconv_s2_split16 (one wave per 4 x 8 stride-2 output tile) must give the BITS of smirk_mbconv_fused_split16
(mbconv_fused_kernel<2, true, KS>, csrc/mbconv.hip) - the same operations in the same order - on every stride-2 InvertedResidual case of tests/mbconv_cases.py it
accepts and on two shapes that table does not reach, be batch invariant and deterministic, refuse what it does not serve without launching, and stay out of the
backbone under SMIRK_DISABLE_MBCONV_FUSED.  Outputs are written between guard bands into NaN pre-filled memory (mbconv_cases.Guarded)."""
import os

import pytest
import torch

import mbconv_cases as MC
from enc_tolerances import VS_FP64

pytestmark = pytest.mark.gpu

REL_TOL = 4e-6                 # tests/test_mbconv_block_gpu.py: max |out - float64| < REL_TOL * max(1, max |ref|)
PRODUCT_SHAPES = [(16, 64, 24), (16, 72, 24), (24, 72, 40), (24, 96, 40)]
GEOMETRIES = {(16, 16), (15, 17), (10, 13), (7, 9), (1, 1)}


def s2_supported(c):
    from smirk_amd import _lib as L
    return c.kind == "ir" and c.stride == 2 and not c.residual and bool(L.lib().smirk_mbconv_s2_supported(c.cin, c.mid, c.cout))


def call_s2(block, out, operands=None):
    """the raw return code of smirk_mbconv_s2_split16 writing to `out`"""
    from smirk_amd import _lib as L
    c = block.case
    t = MC._operands(block) if operands is None else operands
    code = L.lib().smirk_mbconv_s2_split16(*[L.ptr(v, allow_none=True) for v in t], L.ptr(out), c.B, c.H, c.W, c.cin, c.mid, c.cout, L.stream_ptr())
    torch.cuda.synchronize()
    return code


def run_s2(block):
    from smirk_amd import _lib as L
    c = block.case
    G = MC.Guarded(c.B, *MC._out_hw(c), c.cout)
    L.check(call_s2(block, G.out))
    return G.check("smirk_mbconv_s2_split16 " + MC.case_id(c))


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    g, w = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    assert not bool((g == MC.NAN_WORD).any()), f"{what}: output words still hold the NaN pre-fill"
    diff = (g != w)
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} of {diff.numel()} words differ from mbconv_fused_kernel; " + MC.where(diff.float().cpu(), 0.5)


def _accepted():
    return [c for c in MC.CASES_FUSED if c.kind == "ir" and c.stride == 2]


def test_the_accepted_cases_cover_the_product_shapes_and_every_geometry():
    acc = [c for c in _accepted() if s2_supported(c)]
    assert {(c.cin, c.mid, c.cout) for c in acc} >= set(PRODUCT_SHAPES)
    assert {(c.H, c.W) for c in acc} >= GEOMETRIES
    assert any(c.mid % 32 for c in acc)                # a ragged last chunk


@pytest.mark.parametrize("case", _accepted(), ids=MC.case_id)
def test_bitwise_against_the_workgroup_kernel(case):
    block = MC.block_of(case)
    if not s2_supported(case):                         # not one of the instantiated (KS, NT) pairs / mid over the LDS budget: refused, nothing launched
        from smirk_amd import _lib as L
        G = MC.Guarded(case.B, *MC._out_hw(case), case.cout)
        assert call_s2(block, G.out) == L.SMIRK_ERR_UNSUPPORTED
        assert MC.untouched(G.check("refused launch"))
        return
    _same_bits(run_s2(block), MC.run_fused(block), MC.case_id(case))


# 16-64-24 at 30 x 34, B = 3: 4 x 3 x 3 = 36 tiles = 9 workgroups, interior tiles whose halo is all real data; 24-96-40 at 10 x 13, B = 1: 2 tiles, so two waves of
# the only workgroup have no tile
EXTRA = [MC.Case(16, 64, 24, 2, "ir", 3, 30, 34, False), MC.Case(24, 96, 40, 2, "ir", 1, 10, 13, False)]


@pytest.mark.parametrize("case", EXTRA, ids=MC.case_id)
def test_shapes_beyond_the_table(case):
    assert s2_supported(case)
    block = MC.block_of(case)
    out = run_s2(block)
    _same_bits(out, MC.run_fused(block), MC.case_id(case))
    err, big = MC.errors(out, case)
    tol = REL_TOL * max(1.0, big)
    print(f"S2_VS_FP64 {MC.case_id(case):32s} max|err| {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e}  max|ref| {big:.3e}  bound {tol:.3e}")
    msg = MC.where(err, tol)
    assert not msg, f"{MC.case_id(case)}: {msg}"


@pytest.mark.parametrize("case", [MC.Case(24, 88, 40, 2, "ir", 3, 10, 13, False), MC.Case(16, 72, 24, 2, "ir", 3, 15, 17, False)], ids=MC.case_id)
def test_batch_invariance_and_determinism(case):
    """frame b alone is bit-identical to frame b inside a batch of 3; two runs of the batch are bit-identical"""
    block = MC.block_of(case)
    a = run_s2(block).clone()
    b = run_s2(block)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for f in range(case.B):
        one = block._replace(case=case._replace(B=1), x=block.x[f:f + 1], xs=block.xs[f:f + 1].contiguous())
        got = run_s2(one)
        assert torch.equal(got[0].view(torch.int32), a[f].view(torch.int32)), f"frame {f}"


def test_refusals_launch_nothing():
    from smirk_amd import _lib as L
    lib = L.lib()
    for cin, mid, cout in ((56, 96, 40), (24, 96, 104), (16, 64, 40), (24, 72, 24), (16, 104, 24), (16, 60, 24)):
        assert not lib.smirk_mbconv_s2_supported(cin, mid, cout), (cin, mid, cout)
    for case in (MC.Case(56, 96, 40, 2, "ir", 1, 10, 13, False), MC.Case(24, 96, 104, 2, "ir", 1, 10, 13, False)):
        G = MC.Guarded(case.B, *MC._out_hw(case), case.cout)
        assert call_s2(MC.block_of(case), G.out) == L.SMIRK_ERR_UNSUPPORTED, MC.case_id(case)
        assert MC.untouched(G.check("refused launch"))
    case = MC.Case(24, 96, 40, 2, "ir", 1, 10, 13, False)
    t = MC._operands(MC.block_of(case))
    t[1] = None                                         # wexp == NULL: this entry serves InvertedResidual blocks only
    G = MC.Guarded(case.B, *MC._out_hw(case), case.cout)
    assert call_s2(MC.block_of(case), G.out, operands=t) == L.SMIRK_ERR_BAD_ARG
    assert MC.untouched(G.check("refused launch"))


def test_the_switch_keeps_the_backbone_off_the_kernel():
    """SMIRK_DISABLE_MBCONV_FUSED: no mbconv_s2_wave_kernel launch (launch profiler), and the encoder's heads equal the default path's within the encoder tolerances"""
    from oracle import assets as A
    from oracle import mobilenet_ref as M
    from smirk_amd import SmirkEncoder
    from smirk_amd import _lib as L
    m = SmirkEncoder()
    m.load_state_dict(M.synth_encoder_state_dict(), strict=True)
    m = m.cuda().eval()
    img = A.synth_images(2, seed=23).cuda()

    def run():
        L.profile_start()
        with torch.no_grad():
            out = {k: v.cpu() for k, v in m(img).items()}
        torch.cuda.synchronize()
        return out, [r[0] for r in L.profile_stop()]
    got, names = run()
    assert sum(n.startswith("mbconv_s2_wave_kernel") for n in names) == 6, names      # two stride-2 blocks in each of the three backbones
    os.environ["SMIRK_DISABLE_MBCONV_FUSED"] = "1"
    try:
        ref, names_off = run()
    finally:
        del os.environ["SMIRK_DISABLE_MBCONV_FUSED"]
    assert not any(n.startswith("mbconv_s2_wave_kernel") or n.startswith("mbconv_fused_kernel") for n in names_off), names_off
    for k, tol in VS_FP64.items():
        assert (got[k] - ref[k]).abs().max().item() < tol, k
