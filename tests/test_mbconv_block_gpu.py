"""csrc/mbconv.hip at the kernel level: smirk_mbconv_fused_split16 (all 12 mbconv_fused_kernel<S, EXP, KS> instantiations), and next to it the image-resident
kernel and the unfused launch sequence it is compared with elsewhere, each against torch float64 on single small blocks (tests/mbconv_cases.py: shapes at
every tile edge, padding parity and channel raggedness; NaN pre-filled outputs between guard bands; failures name the offending b / y / x / c)."""
import pytest
import torch

import mbconv_cases as MC
from enc_tolerances import BLOCK_VS_FP64

pytestmark = pytest.mark.gpu

# max |out - float64| < REL_TOL * max(1, max |ref|): the bound test_mbconv_image_kernel_vs_float64 holds mbconv_image_kernel to - the same arithmetic class
# (f16x3 products, fp32 accumulation, D rounded to the 22-bit split16 format before the project GEMM)
REL_TOL = 4e-6

RUNNERS = dict(fused=MC.run_fused, image=MC.run_image, unfused=MC.run_unfused)


def _runs():
    out = []
    for c in MC.CASES_FUSED:
        out += [(c, "fused"), (c, "unfused")] + ([(c, "image")] if MC.image_supported(c) else [])
    return out


def _check(out, case, name):
    """finite everywhere (every element was written) and within the bound of the float64 reference; the figures are printed before they are asserted"""
    err, big = MC.errors(out, case)
    tol = BLOCK_VS_FP64.get((MC.case_id(case), name), REL_TOL) * max(1.0, big)
    finite = torch.isfinite(err)
    worst = float(err[finite].max()) if bool(finite.any()) else float("nan")
    print(f"BLOCK_VS_FP64 {name:8s} {MC.case_id(case):32s} max|err| {worst:.3e}  max|ref| {big:.3e}  rel {worst / max(1.0, big):.3e}  bound {tol:.3e}")
    assert bool(finite.all()), f"{name} {MC.case_id(case)}: output elements never written / not finite: " + MC.where(torch.where(finite, 0.0, float("nan")), 1.0)
    msg = MC.where(err, tol)
    assert not msg, f"{name} {MC.case_id(case)}: {msg}"


@pytest.mark.parametrize("case,name", _runs(), ids=lambda v: v if isinstance(v, str) else MC.case_id(v))
def test_block_kernel_vs_float64(case, name):
    _check(RUNNERS[name](MC.block_of(case)), case, name)


@pytest.mark.parametrize("case", MC.UNSUPPORTED_PRODUCT_SHAPES, ids=MC.case_id)
def test_product_shape_over_the_lds_budget_is_refused_and_served_by_the_other_paths(case):
    from smirk_amd import _lib as L
    block = MC.block_of(case)
    G = MC.Guarded(case.B, case.H, case.W, case.cout)
    assert MC.call_fused(block, G.out) == L.SMIRK_ERR_UNSUPPORTED
    assert MC.untouched(G.check("refused launch"))
    _check(MC.run_unfused(block), case, "unfused")
    assert MC.image_supported(case)
    _check(MC.run_image(block), case, "image")


@pytest.mark.parametrize("stride,cin", [(s, c) for s in (1, 2) for c in (16, 32, 48)])
def test_lds_limit(stride, cin):
    """the largest mid smirk_mbconv_supported accepts at Cout = 96 (asked of the library) runs and is right; mid + 8 is refused with nothing launched"""
    from smirk_amd import _lib as L
    lib = L.lib()
    mid = MC.lds_limit_mid(lib, stride, cin)
    assert lib.smirk_mbconv_lds_bytes(cin, mid, 96, stride) <= 64 * 1024 < lib.smirk_mbconv_lds_bytes(cin, mid + 32, 96, stride)
    hw = (9, 17) if stride == 1 else (15, 17)
    case = MC.Case(cin, mid, 96, stride, "ir", 2, *hw, False)
    print(f"LDS limit stride {stride} Cin {cin}: mid {mid}, {lib.smirk_mbconv_lds_bytes(cin, mid, 96, stride)} bytes")
    _check(MC.run_fused(MC.block_of(case)), case, "fused")
    over = case._replace(mid=mid + 8)
    assert not lib.smirk_mbconv_supported(cin, mid + 8, 96, stride)
    G = MC.Guarded(over.B, *MC._out_hw(over), over.cout)
    assert MC.call_fused(MC.block_of(over), G.out) == L.SMIRK_ERR_UNSUPPORTED
    assert MC.untouched(G.check("refused launch"))


@pytest.mark.parametrize("case", MC.BATCH_CASES, ids=MC.case_id)
def test_batch_invariance_and_determinism(case):
    """frame b alone is bit-identical to frame b inside a batch of 3; two runs of the batch are bit-identical"""
    block = MC.block_of(case)
    a = MC.run_fused(block).clone()
    b = MC.run_fused(block)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for f in range(case.B):
        one = block._replace(case=case._replace(B=1), x=block.x[f:f + 1], xs=block.xs[f:f + 1].contiguous())
        got = MC.run_fused(one)
        assert torch.equal(got[0].view(torch.int32), a[f].view(torch.int32)), f"frame {f}"


def test_argument_checks():
    """residual with stride 2 or Cin != Cout, and wexp == NULL with mid != Cin, are SMIRK_ERR_BAD_ARG; nothing is launched"""
    from smirk_amd import _lib as L

    def refused(case, residual, drop_wexp=False):
        block = MC.block_of(case)
        G = MC.Guarded(case.B, *MC._out_hw(case), case.cout)
        t = MC._operands(block)
        if drop_wexp:
            t[1] = t[2] = t[3] = None
        code = L.lib().smirk_mbconv_fused_split16(*[L.ptr(v, allow_none=True) for v in t], int(residual), L.ptr(G.out), case.B, case.H, case.W, case.cin,
                                                  case.mid, case.cout, case.stride, L.stream_ptr())
        assert MC.untouched(G.check("refused launch"))
        return code
    assert refused(MC.Case(24, 88, 24, 2, "ir", 1, 7, 9, False), residual=1) == L.SMIRK_ERR_BAD_ARG          # stride 2
    assert refused(MC.Case(24, 88, 40, 1, "ir", 1, 5, 3, False), residual=1) == L.SMIRK_ERR_BAD_ARG          # Cin != Cout
    assert refused(MC.Case(24, 24, 24, 2, "ds", 1, 7, 9, False), residual=1) == L.SMIRK_ERR_BAD_ARG
    assert refused(MC.Case(24, 88, 24, 1, "ir", 1, 5, 3, False), residual=0, drop_wexp=True) == L.SMIRK_ERR_BAD_ARG   # wexp == NULL with mid != Cin
