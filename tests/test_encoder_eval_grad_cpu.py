"""smirk_amd.encoder_eval_grad without a GPU: every refusal of the two C entries (raw ctypes, dummy pointers: a refusal comes before anything touches the
device), ABI version and entry count, and the laws of tests/enc_eval_law.py against each other — the forced law under its own trace is the law, eager fp32
meets the forced law at rounding level, no ReLU unit's mask can go missing below the bound the GPU test holds the module to, and graph capture refuses the even step."""
import ctypes as C
import os
import re

import torch

import enc_eval_law as E
from oracle import mobilenet_ref as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, ODD = C.c_void_p(0x10000), C.c_void_p(0x10004)                    # never dereferenced; ODD is not 16-byte aligned
BAD_ARG, UNSUPPORTED = -1, -4


def test_c_entries_refuse_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    dw = lambda dy=P, y_out=P, s_out=P, w=P, add=P, y_in=P, s_in=P, dx=P, B=2, H=6, W=5, Cc=16, stride=1: \
        lib.smirk_dwconv3x3_eval_backward_split16(dy, y_out, s_out, w, add, y_in, s_in, dx, B, H, W, Cc, stride, None)
    for name in ("dy", "y_out", "s_out", "w", "dx"):
        assert dw(**{name: None}) == BAD_ARG, name
    for name in ("dy", "y_out", "add", "y_in", "dx"):
        assert dw(**{name: ODD}) == BAD_ARG, name
    assert dw(y_in=None) == BAD_ARG and dw(s_in=None) == BAD_ARG                  # the input unit's output and its factor come together
    for name in ("B", "H", "W", "Cc"):
        assert dw(**{name: 0}) == BAD_ARG and dw(**{name: -8}) == BAD_ARG, name
    for c in (4, 12, 63):
        assert dw(Cc=c) == BAD_ARG, c
    for s in (0, 3, -1, 4):
        assert dw(stride=s) == BAD_ARG, s
    assert dw(B=1 << 6, H=1 << 10, W=1 << 10, Cc=8) == UNSUPPORTED              # 2^29 elements = 2 GiB: 32-bit indexing
    assert dw(B=1 << 12, H=1 << 10, W=1 << 10, Cc=8) == UNSUPPORTED
    assert dw(B=1 << 9, H=1 << 10, W=1 << 10, Cc=8, stride=3) == BAD_ARG        # (a bad argument is reported first)
    relu = lambda dy=P, y=P, s=P, dz=P, Mm=24, Cc=16: lib.smirk_relu_scale_backward_split16(dy, y, s, dz, Mm, Cc, None)
    for name in ("dy", "y", "s", "dz"):
        assert relu(**{name: None}) == BAD_ARG, name
    for name in ("dy", "y", "dz"):
        assert relu(**{name: ODD}) == BAD_ARG, name
    for name in ("Mm", "Cc"):
        assert relu(**{name: 0}) == BAD_ARG and relu(**{name: -8}) == BAD_ARG, name
    for c in (4, 12, 63):
        assert relu(Cc=c) == BAD_ARG, c
    assert relu(Mm=1 << 26, Cc=8) == UNSUPPORTED and relu(Mm=1 << 40, Cc=8) == UNSUPPORTED and relu(Mm=(1 << 26) - 1, Cc=12) == BAD_ARG
    # the pooled head without a workspace is the one-launch form of N <= 64 only; the head's backward needs the pooled vectors for a weight gradient only
    for fn in (lib.smirk_gap_linear_split16, lib.smirk_gap_linear):
        assert fn(P, P, P, P, None, 2, 49, 960, 65, None) == BAD_ARG and fn(P, P, P, P, None, 2, 49, 960, 300, None) == BAD_ARG
        assert fn(None, P, P, P, None, 2, 49, 960, 55, None) == BAD_ARG and fn(P, P, P, P, None, 2, 0, 960, 55, None) == BAD_ARG
    assert lib.smirk_gap_linear_backward_split16(P, P, None, P, P, P, 2, 49, 960, 55, None) == BAD_ARG
    assert lib.smirk_gap_linear_backward_split16(P, P, None, None, P, P, 2, 49, 960, 55, None) == BAD_ARG


def test_abi_version_and_entry_count():
    from smirk_amd import _lib as L
    assert L.lib().smirk_abi_version() == L.ABI_VERSION == 17 and len(L.EXPORTS) == 116
    hdr = open(os.path.join(REPO, "include", "smirk_hip.h")).read()
    for name in ("smirk_dwconv3x3_eval_backward_split16", "smirk_relu_scale_backward_split16"):
        assert name in L.EXPORTS and re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "C ABI v17" in readme and "116 entry points" in readme


def test_forced_law_under_its_own_trace_is_the_law():
    """float64: forcing the decisions the law took itself changes neither its outputs nor its gradient (1e-12)"""
    ref = E.reference(M.synth_encoder_state_dict())
    for B, HW in ((3, 32), (2, 64)):
        img, tgt, tr = E.images(B, HW), E.targets(B), {}
        out, v, g = E.run(ref, img, tgt, record=tr)
        assert [len(tr[n]) for n in E.ENCODERS] == [23, 31, 31]
        outf, vf, gf = E.run(ref, img, tgt, trace=tr)
        assert abs(v - vf) <= 1e-12 * abs(v)
        assert all(float((out[k] - outf[k]).abs().max()) <= 1e-12 * max(1.0, float(out[k].abs().max())) for k in out)
        assert float((g - gf).abs().max()) <= 1e-12 * float(g.abs().max())


def test_fp32_meets_the_forced_law_and_no_mask_can_go_missing():
    """3 x 3 x 32 x 32.  Eager fp32 lies within 1e-4 of max|g| of the forced float64 law under fp32's own trace (seen: 1.3e-5).  Ignoring the mask of ANY ONE of
    the 85 ReLU units moves the float64 gradient by more than 1e-3 of max|g| (seen: 1.6e-1 for the least important unit), so the bound the GPU test holds the
    module to — max(4 x fp32's distance, 1e-6) of max|g| — cannot hide a missing mask."""
    esd = M.synth_encoder_state_dict()
    img, tgt = E.images(3, 32), E.targets(3)
    tr32 = {}
    _, _, g32 = E.run(E.reference(esd, torch.float32), img, tgt, record=tr32)
    ref = E.reference(esd)
    _, _, gf = E.run(ref, img, tgt, trace=tr32)
    dist = float((g32.double() - gf).abs().max()) / float(gf.abs().max())
    print(f"eager fp32 against the forced float64 law under its trace: {dist:.2e} of max|g|")
    assert dist <= 1e-4
    tr = {}
    _, _, g = E.run(ref, img, tgt, record=tr)
    gmax, moved = float(g.abs().max()), {}
    for n in E.ENCODERS:
        # the three backbones add up in the gradient: dropping a mask of one backbone moves only that backbone's term, so only its heads need to run
        heads = {"pose_encoder": ("pose_params", "cam"), "shape_encoder": ("shape_params",), "expression_encoder": ("expression_params", "jaw_params", "eyelid_params")}[n]
        w = {k: E.LOSS_W[k] for k in heads}
        _, _, base = E.run(ref, img, tgt, trace=tr, weights=w)
        for k in range(len(tr[n])):
            one = dict(tr)
            one[n] = list(tr[n])
            one[n][k] = torch.ones_like(tr[n][k])
            _, _, gk = E.run(ref, img, tgt, trace=one, weights=w)
            moved[(n, k)] = float((gk - base).abs().max()) / gmax
    least = min(moved, key=moved.get)
    print(f"{len(moved)} units; the least important mask {least} moves the gradient by {moved[least]:.2e} of max|g|")
    assert len(moved) == 85 and moved[least] > 1e-3


def test_graph_capture_keeps_refusing_anything_but_train_mode():
    """the even step is not captured: sub-encoders in .eval() under a train-mode container are refused before anything touches the device"""
    import pytest
    from smirk_amd import SmirkEncoder, SmirkGenerator
    from smirk_amd.cycle import graph_cycle_modules
    gen, enc = SmirkGenerator(6, 3, 32, 5).train(), SmirkEncoder().train()
    enc.pose_encoder.eval()
    assert enc.training
    with pytest.raises(ValueError, match="TRAIN-mode"):
        graph_cycle_modules(gen, enc, None, None)
