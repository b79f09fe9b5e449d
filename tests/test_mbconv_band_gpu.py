"""The halo-tile mode of csrc/mbconv_image.hip at the kernel level: smirk_mbconv_image_split16 on images larger than 224 pixels runs ONE WAVE per 2 x 14 output
band (mbi_band_body).  Every case is held to torch float64 on the exact split16 operand values at the bound of test_mbconv_image_kernel_vs_float64, must be batch
invariant and deterministic bit for bit, and must record the launch name the workgroup-per-tile body printed for the shape (tests/backbone_cases.py pins those
names for the backbones).  Outputs are written between guard bands into NaN pre-filled memory (mbconv_cases.Guarded)."""
import functools

import pytest
import torch

import mbconv_cases as MC

pytestmark = pytest.mark.gpu

REL_TOL = 4e-6                 # tests/test_encoder_gpu.py::test_mbconv_image_kernel_vs_float64: max |out - float64| < REL_TOL * max(1, max |ref|)

#            cin mid cout s  kind  B  H   W  residual
CASES = [MC.Case(40, 120, 40, 1, "ir", 3, 28, 28, True),      # 2 x 14 bands of 28 x 28: every band touches the image border; 126 bands, two waves of the last workgroup idle
         MC.Case(24, 72, 24, 1, "ir", 2, 56, 56, True),       # interior bands (the halo is all real data: no validity select), ragged last chunk (72 = 2 x 32 + 8)
         MC.Case(24, 88, 24, 1, "ir", 2, 28, 28, True),
         MC.Case(40, 120, 40, 1, "ir", 1, 28, 42, False),     # W = 3 x 14: a band column whose halo is interior in x
         MC.Case(40, 120, 48, 1, "ir", 1, 42, 28, False),     # H = 14 x 3; 42 bands do not fill whole workgroups
         MC.Case(48, 144, 48, 1, "ir", 5, 28, 28, True),      # Cin a multiple of 16: no k padding; 5 chunks
         # beyond the issue's list: mid over 34 chunks, so the depthwise / BN constants are restaged inside the chunk loop (two more workgroup barriers)
         MC.Case(24, 1096, 24, 1, "ir", 1, 28, 28, True)]


def _name(c):
    return f"mbconv_image_kernel<{(c.cin + 15) // 16},{(c.cout + 31) // 32},true,true>"


@functools.lru_cache(maxsize=None)
def _run(case):
    """(output of the whole batch, launch names recorded around the call); computed once per case, callers must not modify it"""
    from smirk_amd import _lib as L
    assert case.H * case.W > 224 and MC.image_supported(case)
    L.profile_start()
    try:
        out = MC.run_image(MC.block_of(case)).clone()
    finally:
        names = [r[0] for r in L.profile_stop()]
    return out, names


@pytest.mark.parametrize("case", CASES, ids=MC.case_id)
def test_against_float64(case):
    out, _ = _run(case)
    err, big = MC.errors(out, case)
    tol = REL_TOL * max(1.0, big)
    print(f"BAND_VS_FP64 {MC.case_id(case):34s} max|err| {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e}  max|ref| {big:.3e}  bound {tol:.3e}")
    msg = MC.where(err, tol)
    assert not msg, f"{MC.case_id(case)}: {msg}"


@pytest.mark.parametrize("case", CASES, ids=MC.case_id)
def test_batch_invariance_and_determinism(case):
    """two runs of the batch are bit-identical; frame b alone is bit-identical to frame b inside the batch"""
    a, _ = _run(case)
    block = MC.block_of(case)
    again = MC.run_image(block)
    assert torch.equal(a.view(torch.int32), again.view(torch.int32))
    for f in range(case.B):
        one = block._replace(case=case._replace(B=1), x=block.x[f:f + 1], xs=block.xs[f:f + 1].contiguous())
        got = MC.run_image(one)
        assert torch.equal(got[0].view(torch.int32), a[f].view(torch.int32)), f"frame {f}"


@pytest.mark.parametrize("case", CASES, ids=MC.case_id)
def test_the_launch_keeps_its_profiler_name(case):
    _, names = _run(case)
    assert names == [_name(case)], names
