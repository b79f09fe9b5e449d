"""smirk_backbone_plan and smirk_backbone_workspace_bytes pinned, without a GPU (both read backbone_plan, a pure host function: csrc/network.hip).

The weights struct is built by hand from the architecture table; where backbone_args_ok wants pointers it gets dummy integers, and nothing dereferences them.  For the
36 cases of tests/backbone_cases.py the families the query reports must be the families that the launch groups of EXPECTED belong to (backbone_cases.FAMILY_LAUNCHES):
EXPECTED is what the parent commit launched on the GPU, so this holds the plan to the parent's choices on the build machine.  The workspace bytes at B = 1, 64 and
1024 were recorded on the parent commit as well."""
import ctypes as C
import os

import pytest

import backbone_cases as BC
from smirk_amd import _lib as L

DUMMY = 0x1000                                                       # "some device address": never dereferenced on the host


def weights(backbone, mutate=None):
    w = L.SmirkBackboneWeights()
    bl = [list(b) for b in BC.blocks(backbone)]
    if mutate:
        mutate(bl)
    w.n_blocks, w.precision, w.n_out, w.clamp_n_exp, w.stem_cout, w.feat_ch = len(bl), L.PRECISION_F16X3, 0, -1, BC.STEM_COUT, BC.blocks(backbone)[-1][4]
    w.stem.w = w.stem.scale = w.stem.shift = DUMMY
    for b, (kind, stride, cin, mid, cout, skip) in zip(w.blocks, bl):
        b.kind, b.stride, b.cin, b.mid, b.cout, b.skip = kind, stride, cin, mid, cout, skip
    return w


def plan(w, hw, switches=()):
    """family names smirk_backbone_plan reports with the switches set around the one call (or its error code)"""
    fam = (C.c_int * L.BACKBONE_MAX_BLOCKS)()
    env = BC.env_of(switches)
    os.environ.update(env)
    try:
        n = L.lib().smirk_backbone_plan(w, BC.B, hw[0], hw[1], fam, L.BACKBONE_MAX_BLOCKS)
    finally:
        for k in env:
            del os.environ[k]
    return n if n < 0 else [L.BACKBONE_FAMILIES[fam[i]] for i in range(n)]


@pytest.mark.parametrize("case", sorted(BC.CASES))
def test_query_reports_the_families_of_the_recorded_launches(case):
    backbone, hw, switches = BC.CASES[case]
    got = plan(weights(backbone), hw, switches)
    assert got == BC.families(BC.EXPECTED[case])
    assert len(got) == len(BC.blocks(backbone))
    assert (got[0] == "HEAD_FUSED") == (BC.EXPECTED[case][0] != BC.STEM_LAUNCH), "the head decision"


def test_family_names_follow_the_header_enum():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smirk_hip.h")).read()
    enum = re.findall(r"SMIRK_BACKBONE_([A-Z0-9_]+) = (\d+)", hdr)
    assert [name for name, _ in enum] == list(L.BACKBONE_FAMILIES) and [int(v) for _, v in enum] == list(range(len(enum)))
    assert set(BC.FAMILY_LAUNCHES) == set(L.BACKBONE_FAMILIES)


@pytest.mark.parametrize("backbone", sorted(BC.BACKBONES))
@pytest.mark.parametrize("hw", BC.SIZES, ids=lambda hw: "%dx%d" % hw)
def test_workspace_bytes_equal_the_recorded_ones(backbone, hw):
    w = weights(backbone)
    got = [L.lib().smirk_backbone_workspace_bytes(w, b, hw[0], hw[1]) for b in BC.WORKSPACE_B]
    assert got == BC.EXPECTED_WORKSPACE[backbone, hw]
    os.environ["SMIRK_DISABLE_MBCONV_FUSED"] = "1"                   # the layout holds the unfused temporaries whatever the switches say
    try:
        assert L.lib().smirk_backbone_workspace_bytes(w, BC.WORKSPACE_B[0], hw[0], hw[1]) == got[0]
    finally:
        del os.environ["SMIRK_DISABLE_MBCONV_FUSED"]


def test_broken_channel_chains_are_refused_by_every_entry_alike():
    """block.cin != the channels before it, and feat_ch != the last block's: SMIRK_ERR_BAD_ARG from the query and from the forward (before it touches the device),
    0 bytes from the workspace query"""
    lib = L.lib()
    P = C.c_void_p(DUMMY)

    def broken_block(bl):
        bl[3][2] += 8

    cases = [weights("small", broken_block), weights("small")]
    cases[1].feat_ch += 8
    for w in cases:
        assert plan(w, (224, 224)) == L.SMIRK_ERR_BAD_ARG
        assert lib.smirk_backbone_workspace_bytes(w, BC.B, 224, 224) == 0
        assert lib.smirk_backbone_forward(w, P, BC.B, 224, 224, None, P, P, 1 << 40, None) == L.SMIRK_ERR_BAD_ARG
    good = weights("small")
    assert plan(good, (31, 224)) == L.SMIRK_ERR_BAD_ARG and lib.smirk_backbone_plan(good, BC.B, 224, 224, None, 4) == L.SMIRK_ERR_BAD_ARG
    assert lib.smirk_backbone_plan(good, BC.B, 224, 224, None, 0) == len(BC.blocks("small")), "cap 0: the block count alone"
    need = lib.smirk_backbone_workspace_bytes(good, BC.B, 224, 224)
    assert lib.smirk_backbone_forward(good, P, BC.B, 224, 224, None, P, P, need - 1, None) == L.SMIRK_ERR_WORKSPACE
