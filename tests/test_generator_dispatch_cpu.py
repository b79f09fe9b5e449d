"""smirk_generator_plan and smirk_generator_workspace_bytes pinned, without a GPU (both read plan_generator, a pure host function: csrc/network.hip).

The weights struct is built by hand (generator_cases.weights); where an entry wants pointers it gets dummy integers, and nothing dereferences them.  For every case of
tests/generator_cases.py the launches that the query's report stands for (generator_cases.launches) must be the launches of EXPECTED: EXPECTED is what the parent commit
launched on the GPU, so this holds the plan to the parent's choices on the build machine.  The launch profiler keeps one chain, so for a case that forks, EXPECTED
pins everything outside the section, and each chain's section is pinned by the single-chain sibling case with that chain's frames."""
import ctypes as C
import os
import re

import pytest

import generator_cases as GC
from smirk_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(GC.DUMMY)


@pytest.fixture(scope="module")
def reports():
    return {case: GC.query(case) for case in GC.CASES}


@pytest.mark.parametrize("case", sorted(GC.CASES))
def test_query_reports_the_recorded_launches(reports, case):
    c, r = GC.CASES[case], reports[case]
    assert [nb for _, nb in r["chains"]] == list(c["chains"]) and [b0 for b0, _ in r["chains"]] == [sum(c["chains"][:k]) for k in range(len(c["chains"]))]
    assert r["section_from"] == 3
    for l in range(4):                                               # -1 exactly where a level is not split or the chain does not exist
        n = len(r["chains"]) if l >= r["section_from"] else 1
        assert [d is not None for d in r["dec"][l]] == [k < n for k in range(L.GEN_MAX_CHAINS)], (l, r["dec"][l])
    if c["cpu_only"]:
        return
    names = GC.EXPECTED[case]
    before, section, after = GC.launches(r)
    if c["refused"]:                                                 # the forward stops at the launch that refuses: a prefix of the plan
        assert GC.matches(names, (before + section + after)[:len(names)]), (names, r)
        return
    assert GC.matches(names[:len(before)], before), (names, r)
    assert GC.matches(names[len(names) - len(after):], after), (names, r)
    if len(r["chains"]) == 1:
        assert GC.matches(names[len(before):len(names) - len(after)], section), (names, r)
    for k, (_, nb) in enumerate(r["chains"]) if len(r["chains"]) > 1 else ():
        sib = GC.sibling(case, nb)
        sb, ss, sa = GC.launches(reports[sib])
        assert GC.matches(GC.EXPECTED[sib][len(sb):len(GC.EXPECTED[sib]) - len(sa)], GC.launches(r, k)[1]), (case, k, sib)


@pytest.mark.parametrize("case", sorted(c for c in GC.CASES if len(GC.CASES[c]["chains"]) > 1))
def test_a_chain_decides_like_a_batch_of_its_frames_where_the_weights_exist(reports, case):
    """dec[l][k] of a section level == dec[l][0] of the single-chain plan at B = the chain's frames whenever the whole batch composed the level's weights, PAIR
    otherwise — the 2 GiB case is the `otherwise`: 1350 frames alone compose level 3, 2700 frames build no weights for it"""
    r = reports[case]
    for l in range(r["section_from"], 4):
        for k, (_, nb) in enumerate(r["chains"]):
            alone = reports[GC.sibling(case, nb)]["dec"][l][0]
            assert r["dec"][l][k] == (alone if l in r["compose"] else "PAIR"), (l, k)
    if GC.CASES[case]["cpu_only"]:
        assert 3 not in r["compose"] and r["dec"][3][:2] == ["PAIR", "PAIR"] and r["dec"][2][0] == "PAIR"
        assert reports[GC.sibling(case, 1350)]["dec"][3][0] == "UPDEEP"


def test_the_cases_reach_every_family_and_input_step(reports):
    rs = [r for r in reports.values()]
    assert {r["input"] for r in rs} == set(L.GEN_INPUTS)
    assert {e for r in rs for e in r["enc"]} == set(L.GEN_ENCODER_FAMILIES)
    assert {d for r in rs for lv in r["dec"] for d in lv if d} == set(L.GEN_DECODER_FAMILIES)
    assert {len(r["compose"]) for r in rs} == {0, 1, 2} and {r["fused_tail"] for r in rs} == {False, True} and {len(r["chains"]) for r in rs} == {1, 2, 3}


def test_family_names_follow_the_header_enum():
    hdr = open(os.path.join(REPO, "include", "smirk_generator_plan.h")).read()
    for prefix, names in (("SMIRK_GEN_INPUT_", L.GEN_INPUTS), ("SMIRK_GEN_ENC_", L.GEN_ENCODER_FAMILIES), ("SMIRK_GEN_DEC_", L.GEN_DECODER_FAMILIES)):
        enum = re.findall(prefix + r"([A-Z0-9_]+) = (\d+)", hdr)
        assert [n for n, _ in enum] == list(names) and [int(v) for _, v in enum] == list(range(len(enum))), prefix
    assert int(re.search(r"#define\s+SMIRK_GEN_MAX_CHAINS\s+(\d+)", hdr).group(1)) == L.GEN_MAX_CHAINS
    assert set(GC.INPUT_LAUNCHES) == set(L.GEN_INPUTS) and set(GC.ENCODER_LAUNCHES) == set(L.GEN_ENCODER_FAMILIES)
    assert set(GC.DECODER_LAUNCHES) == set(L.GEN_DECODER_FAMILIES)


@pytest.mark.parametrize("key", sorted(GC.EXPECTED_WORKSPACE), ids=lambda k: "%s-%dx%d" % ((k[0],) + k[1]))
def test_workspace_bytes_equal_the_recorded_ones(key):
    name, (H, W) = key
    lib, w = L.lib(), GC.weights(*GC.WEIGHTS[name])
    got = [lib.smirk_generator_workspace_bytes(w, b, H, W) for b in GC.WORKSPACE_B]
    assert got == GC.EXPECTED_WORKSPACE[key]
    r = L.SmirkGeneratorPlanReport()
    for var, value in list(GC.KERNEL_SWITCHES.values()) + [("SMIRK_GEN_SPLIT_CHAINS", "3")]:       # the layout does not depend on the switches
        os.environ[var] = value
        try:
            assert lib.smirk_generator_workspace_bytes(w, GC.WORKSPACE_B[1], H, W) == got[1], var
            assert lib.smirk_generator_plan(w, w.in_channels, 0, GC.WORKSPACE_B[1], H, W, 0, r) == 0 and r.workspace_bytes == got[1], var
        finally:
            del os.environ[var]
    assert lib.smirk_generator_plan(w, w.in_channels, 0, GC.WORKSPACE_B[1], H, W, 1, r) == 0 and r.workspace_bytes == got[1], "taps"


def test_bad_arguments_are_refused_by_every_entry_alike():
    """SMIRK_ERR_BAD_ARG from the query, the forward and the packed forward (before anything touches the device), 0 bytes from the workspace query"""
    lib, r = L.lib(), L.SmirkGeneratorPlanReport()
    other_precision = GC.weights()
    other_precision.precision = 7
    bad = [(GC.weights(), dict(B=0)), (GC.weights(), dict(H=40)), (GC.weights(), dict(W=0)), (GC.weights(), dict(W=50)), (GC.weights(features=12), {}),
           (GC.weights(cin_pad=4), {}), (other_precision, {}), (GC.weights(out_channels=5), {}), (GC.weights(res_blocks=17), {}),
           (GC.weights("f32", cin_pad=6), {}), (GC.weights("f32", cin_pad=4), {})]
    for w, kw in bad:
        B, H, W = kw.get("B", 2), kw.get("H", 32), kw.get("W", 48)
        assert lib.smirk_generator_workspace_bytes(w, B, H, W) == 0, kw
        assert lib.smirk_generator_plan(w, w.in_channels, 0, B, H, W, 0, r) == L.SMIRK_ERR_BAD_ARG, kw
        assert lib.smirk_generator_forward(w, P, w.in_channels, None, 0, P, B, H, W, None, P, 1 << 40, None) == L.SMIRK_ERR_BAD_ARG, kw
        assert lib.smirk_generator_forward_packed(w, P, P, B, H, W, None, P, 1 << 40, None) == L.SMIRK_ERR_BAD_ARG, kw
    assert lib.smirk_generator_workspace_bytes(None, 2, 32, 48) == 0 and lib.smirk_generator_plan(None, 6, 0, 2, 32, 48, 0, r) == L.SMIRK_ERR_BAD_ARG
    good = GC.weights()
    assert lib.smirk_generator_plan(good, 6, 0, 2, 32, 48, 0, None) == L.SMIRK_ERR_BAD_ARG
    for ca, cb in ((5, 0), (3, 2), (0, 6), (7, -1)):                 # the sources do not add up to in_channels
        assert lib.smirk_generator_plan(good, ca, cb, 2, 32, 48, 0, r) == L.SMIRK_ERR_BAD_ARG, (ca, cb)
        assert lib.smirk_generator_forward(good, P, ca, P, cb, P, 2, 32, 48, None, P, 1 << 40, None) == L.SMIRK_ERR_BAD_ARG, (ca, cb)
    f32 = GC.weights("f32")
    assert lib.smirk_generator_plan(f32, 0, 0, 2, 32, 48, 0, r) == L.SMIRK_ERR_BAD_ARG, "the packed tensor is split-fp16"
    assert lib.smirk_generator_forward_packed(f32, P, P, 2, 32, 48, None, P, 1 << 40, None) == L.SMIRK_ERR_BAD_ARG
    # an fp32 pair that is not 3 + 3 on cin_pad 8: no pack kernel
    need = lib.smirk_generator_workspace_bytes(f32, 2, 32, 48)
    assert lib.smirk_generator_plan(f32, 4, 2, 2, 32, 48, 0, r) == L.SMIRK_ERR_UNSUPPORTED
    assert lib.smirk_generator_forward(f32, P, 4, P, 2, P, 2, 32, 48, None, P, need, None) == L.SMIRK_ERR_UNSUPPORTED
    # a workspace one byte short is refused before the device is touched, whatever the chain count
    for B in (2, 64):
        need = lib.smirk_generator_workspace_bytes(good, B, 32, 48)
        assert need > 0
        assert lib.smirk_generator_forward(good, P, 6, None, 0, P, B, 32, 48, None, P, need - 1, None) == L.SMIRK_ERR_WORKSPACE
        assert lib.smirk_generator_forward_packed(good, P, P, B, 32, 48, None, P, need - 1, None) == L.SMIRK_ERR_WORKSPACE
        assert lib.smirk_generator_forward(f32, P, 4, P, 2, P, B, 32, 48, None, P, 0, None) == L.SMIRK_ERR_WORKSPACE, "the workspace check comes first"


def test_extension_table_equals_the_header():
    hdr = open(os.path.join(REPO, "include", "smirk_generator_plan.h")).read()
    declared = set(re.findall(r"\b(smirk_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.GENPLAN_EXPORTS), declared ^ set(L.GENPLAN_EXPORTS)
    assert L.GENPLAN_EXPORTS == tuple(L.GENPLAN_SIGS) and len(L.GENPLAN_EXPORTS) == 2
    for other in (L.EXPORTS, L.MICA_EXPORTS, L.EMOTION_EXPORTS, L.OPTIM_EXPORTS, L.HANDOFF_EXPORTS):
        assert not set(L.GENPLAN_EXPORTS) & set(other)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    version = int(re.search(r"#define\s+SMIRK_GENPLAN_ABI_VERSION\s+(\d+)", hdr).group(1))
    lib = L.lib()
    assert lib.smirk_genplan_abi_version() == L.GENPLAN_ABI_VERSION == version == 1
    assert "smirk_generator_plan.h" in open(os.path.join(REPO, "README.md")).read()
    assert '"smirk_generator_plan.h"' in open(os.path.join(REPO, "smirk_amd", "build.py")).read()
    # the other tables and their versions did not move, and none of their headers declares the new entries
    assert lib.smirk_abi_version() == L.ABI_VERSION == 17 and len(L.EXPORTS) == 116
    assert lib.smirk_mica_abi_version() == L.MICA_ABI_VERSION and lib.smirk_emotion_abi_version() == L.EMOTION_ABI_VERSION
    assert lib.smirk_optim_abi_version() == L.OPTIM_ABI_VERSION and lib.smirk_handoff_abi_version() == L.HANDOFF_ABI_VERSION
    for name in ("smirk_hip.h", "smirk_mica.h", "smirk_emotion.h", "smirk_optim.h", "smirk_handoff.h"):
        text = open(os.path.join(REPO, "include", name)).read()
        assert not any(re.search(r"\b%s\b" % e, text) for e in L.GENPLAN_EXPORTS), name
    assert L.SMIRK_ERR_BAD_ARG == -1 and L.SMIRK_ERR_WORKSPACE == -2 and L.SMIRK_ERR_UNSUPPORTED == -4


def test_the_generator_half_decides_only_in_its_plan_functions():
    """in the generator half of network.hip, `*_eligible(`, `*_supported(` and `smirk_switch(` are called by plan_generator and gen_chain_wish alone"""
    src = open(os.path.join(REPO, "smirk_amd", "csrc", "network.hip")).read()
    half = src[src.index("struct Arena"):src.index("MobileNetV3-minimal backbone + pooled linear head")]
    code = "\n".join(line.split("//")[0] for line in half.splitlines())
    bodies = {m.group(1): m.end() for m in re.finditer(r"^(?:static |extern \"C\" )?[A-Za-z_][\w \*&:]*?\b(\w+)\([^;{}]*\) \{$", code, re.M)}
    starts = sorted(bodies.values())
    for m in re.finditer(r"\b\w+_(eligible|supported)\(|\bsmirk_switch\(", code):
        owner = [name for name, at in bodies.items() if at == max(s for s in starts if s <= m.start())][0]
        assert owner in ("plan_generator", "gen_chain_wish"), (owner, m.group(0))
