"""SmirkGenerator.precision = "f16x1" without a GPU: the extension table of include/smirk_generator_arith.h, what the plan and the workspace query say for the new
precision (both read plan_generator, a pure host function of csrc/network.hip), what the Python module accepts, and the emulation the GPU test is held to
(tests/x1_law.py)."""
import ctypes as C
import os
import re

import pytest
import torch

import generator_cases as GC
import x1_law as X
from smirk_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def x1_weights(features=32, in_channels=6, precision=L.PRECISION_F16X1, **kw):
    """the split-fp16 weights struct of generator_cases with another precision code"""
    w = GC.weights("f16x3", features, in_channels, **kw)
    w.precision = precision
    return w


def test_extension_table_equals_the_header():
    hdr = open(os.path.join(REPO, "include", "smirk_generator_arith.h")).read()
    declared = set(re.findall(r"\b(smirk_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.GENARITH_EXPORTS), declared ^ set(L.GENARITH_EXPORTS)
    assert L.GENARITH_EXPORTS == tuple(L.GENARITH_SIGS) and len(L.GENARITH_EXPORTS) == 2
    for other in (L.EXPORTS, L.MICA_EXPORTS, L.EMOTION_EXPORTS, L.OPTIM_EXPORTS, L.HANDOFF_EXPORTS, L.GENPLAN_EXPORTS):
        assert not set(L.GENARITH_EXPORTS) & set(other)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    version = int(re.search(r"#define\s+SMIRK_GENARITH_ABI_VERSION\s+(\d+)", hdr).group(1))
    lib = L.lib()
    assert lib.smirk_genarith_abi_version() == L.GENARITH_ABI_VERSION == version == 1
    assert "smirk_generator_arith.h" in open(os.path.join(REPO, "README.md")).read()
    assert '"smirk_generator_arith.h"' in open(os.path.join(REPO, "smirk_amd", "build.py")).read()
    # the other tables and their versions did not move, and none of their headers declares the new entries
    assert lib.smirk_abi_version() == L.ABI_VERSION == 17 and len(L.EXPORTS) == 116
    assert lib.smirk_genplan_abi_version() == L.GENPLAN_ABI_VERSION == 1 and len(L.GENPLAN_EXPORTS) == 2
    assert C.sizeof(L.SmirkGeneratorPlanReport) == 120                 # its report struct: 27 int32, padding, one uint64
    assert lib.smirk_mica_abi_version() == L.MICA_ABI_VERSION and lib.smirk_emotion_abi_version() == L.EMOTION_ABI_VERSION
    assert lib.smirk_optim_abi_version() == L.OPTIM_ABI_VERSION and lib.smirk_handoff_abi_version() == L.HANDOFF_ABI_VERSION
    for name in ("smirk_hip.h", "smirk_mica.h", "smirk_emotion.h", "smirk_optim.h", "smirk_handoff.h", "smirk_generator_plan.h"):
        text = open(os.path.join(REPO, "include", name)).read()
        assert not any(re.search(r"\b%s\s*\(" % e, text) for e in L.GENARITH_EXPORTS), name
    main = open(os.path.join(REPO, "include", "smirk_hip.h")).read()
    values = dict(re.findall(r"SMIRK_PRECISION_(\w+) = (\d+)", main))
    assert values == {"F32": "0", "F16X3": "1", "F16X1": "2"} and (L.PRECISION_F32, L.PRECISION_F16X3, L.PRECISION_F16X1) == (0, 1, 2)
    assert L.GEN_ARITH == X.ARITH == ("F32", "F16X3", "F16X1")


def test_arith_query():
    assert X.arith(GC.weights("f16x3")) == dict(x1_from=X.arith(x1_weights())["x1_from"], levels=["F16X3"] * 4, deep="F16X3")
    assert X.arith(GC.weights("f32"))["levels"] == ["F32"] * 4 and X.arith(GC.weights("f32"))["deep"] == "F32"
    for features in (32, 16):                                          # the arithmetic is the level's, whatever the width
        a = X.arith(x1_weights(features))
        assert a["x1_from"] in (1, 2)
        assert a["levels"] == ["F16X1" if l >= a["x1_from"] else "F16X3" for l in range(4)] and a["deep"] == "F16X1"
    lib, w = L.lib(), x1_weights()
    i, lv = C.c_int32(), (C.c_int32 * 4)()
    assert lib.smirk_generator_arith(None, C.byref(i), lv, C.byref(i)) == L.SMIRK_ERR_BAD_ARG
    assert lib.smirk_generator_arith(w, None, lv, C.byref(i)) == L.SMIRK_ERR_BAD_ARG
    assert lib.smirk_generator_arith(w, C.byref(i), None, C.byref(i)) == L.SMIRK_ERR_BAD_ARG
    assert lib.smirk_generator_arith(w, C.byref(i), lv, None) == L.SMIRK_ERR_BAD_ARG
    assert lib.smirk_generator_arith(x1_weights(precision=7), C.byref(i), lv, C.byref(i)) == L.SMIRK_ERR_BAD_ARG
    assert lib.smirk_generator_arith(w, C.byref(i), lv, C.byref(i)) == 0
    # no pointer is followed: the weights above hold none


def _query(case, precision):
    c = GC.CASES[case]
    ca, cb = {"forward": (c["in_channels"], 0), "pair": (3, 3), "packed": (0, 0)}[c["entry"]]
    r = L.SmirkGeneratorPlanReport()
    w = x1_weights(c["features"], c["in_channels"], precision)
    with GC.switches(case):
        assert L.lib().smirk_generator_plan(w, ca, cb, c["B"], c["H"], c["W"], int(c["taps"]), r) == 0
        nbytes = L.lib().smirk_generator_workspace_bytes(w, c["B"], c["H"], c["W"])
    assert nbytes == r.workspace_bytes
    return r


@pytest.mark.parametrize("case", sorted(c for c in GC.CASES if GC.CASES[c]["precision"] == "f16x3"))
def test_plan_and_workspace_equal_f16x3_up_to_the_families_without_a_one_mfma_form(case):
    """the same input step, chains, composed levels, tail and bytes; below x1_from the same families; from x1_from on, a family that exists in the three-MFMA form
    only (enc1_fused, conv_upcat at another width than 64 channels) becomes the plain one and every other family stays"""
    a, b = _query(case, L.PRECISION_F16X3), _query(case, L.PRECISION_F16X1)
    x1_from = X.arith(x1_weights())["x1_from"]
    for f in ("input", "nchain", "section_from", "compose_mask", "fused_tail", "workspace_bytes"):
        assert getattr(a, f) == getattr(b, f), f
    assert list(a.chain_b0) == list(b.chain_b0) and list(a.chain_nb) == list(b.chain_nb)
    enc, dec = L.GEN_ENCODER_FAMILIES, L.GEN_DECODER_FAMILIES
    for l in range(4):
        x1_level, c = l >= x1_from, GC.CASES[case]["features"] << l
        assert enc[b.enc[l]] == ("CONV_CONV_POOL" if x1_level and enc[a.enc[l]] == "ENC1_FUSED" else enc[a.enc[l]]), l
        for k in range(L.GEN_MAX_CHAINS):
            want = a.dec[l][k]
            if x1_level and want >= 0 and dec[want] == "UPCAT" and c != 64:
                want = dec.index("PAIR")
            assert b.dec[l][k] == want, (l, k)
    assert b.fused_tail == a.fused_tail and x1_from >= 1               # level 0 never changes: enc1_fused, the fused tail and the final 1 x 1 stay what they are


def test_the_packed_entry_and_the_refusals_know_the_precision():
    lib, r, P = L.lib(), L.SmirkGeneratorPlanReport(), C.c_void_p(GC.DUMMY)
    w = x1_weights()
    assert lib.smirk_generator_plan(w, 0, 0, 2, 32, 48, 0, r) == 0 and L.GEN_INPUTS[r.input] == "PACKED"
    need = lib.smirk_generator_workspace_bytes(w, 2, 32, 48)
    assert need == lib.smirk_generator_workspace_bytes(GC.weights(), 2, 32, 48) > 0
    assert lib.smirk_generator_forward(w, P, 6, None, 0, P, 2, 32, 48, None, P, need - 1, None) == L.SMIRK_ERR_WORKSPACE
    assert lib.smirk_generator_forward_packed(w, P, P, 2, 32, 48, None, P, need - 1, None) == L.SMIRK_ERR_WORKSPACE
    bad = x1_weights(cin_pad=4)                                        # split storage: the input is one 8-channel group
    assert lib.smirk_generator_workspace_bytes(bad, 2, 32, 48) == 0


def test_the_module_accepts_the_precision(monkeypatch):
    """fails on the parent commit: "f16x1" was an unknown precision there"""
    from smirk_amd import SmirkGenerator, SmirkHipError
    torch.manual_seed(3)
    m = SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=1).eval()
    assert m.precision == "f16x3"                                     # the default stays
    m.precision = "f16x1"
    w = m._weights()                                                  # the weight image is built on whatever device the parameters live on
    assert w.precision == L.PRECISION_F16X1 and w.cin_pad == 8 and m.accepts_packed()
    a = X.arith(w)
    assert a["deep"] == "F16X1" and a["levels"][3] == "F16X1" and a["levels"][0] == "F16X3"
    x3 = SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=1).eval()
    x3.load_state_dict(m.state_dict())
    P1, P3 = m._pack(), x3._pack()
    assert set(P1) == set(P3) and all(torch.equal(P1[k][0], P3[k][0]) for k in P1)      # the same weight images
    m.train()
    assert not m.accepts_packed()
    m.eval()
    m.precision = "f16x2"
    with pytest.raises(SmirkHipError, match="f16x2"):
        m._weights()
    monkeypatch.setenv("SMIRK_AMD_GENERATOR_PRECISION", "f16x1")
    assert SmirkGenerator(in_channels=6, out_channels=3, init_features=8, res_blocks=0).precision == "f16x1"
    wide = SmirkGenerator(in_channels=10, out_channels=3, init_features=8, res_blocks=0).eval()      # more than one input group: exact fp32, as under "f16x3"
    with pytest.warns(UserWarning, match="exact-fp32"):
        assert wide._weights().precision == L.PRECISION_F32 and not wide.accepts_packed()


def test_the_two_emulations_agree():
    """x1_law.forward against its composed form (the library rounds the composed decoder weights once, the law rounds twice): without rounding they are the same
    function up to the fp32 composition, and with it each stays within the margin the GPU test grants — factor 2 plus OUT_TOL — of the other's distance from float64"""
    from oracle import assets as A
    from oracle import generator_ref as G
    sd = X.double_state_dict(G.synth_state_dict(res_blocks=1))
    x = A.synth_generator_input(1, seed=41)[:, :, 80:144, 80:144].contiguous().double()
    d, skip = torch.randn(1, 256, 8, 8, dtype=torch.float64), torch.randn(1, 128, 16, 16, dtype=torch.float64)
    wup, bup, w3 = sd["upconv3.weight"], sd["upconv3.bias"], sd["decoder3.dec3conv1.weight"]
    plain = torch.nn.functional.conv2d(torch.cat((torch.nn.functional.conv_transpose2d(d, wup, bup, stride=2), skip), 1), w3, padding=1)
    assert (X._composed_first_conv(d, skip, wup, bup, w3, False) - plain).abs().max().item() < 1e-5 * plain.abs().max().item()
    ar = X.arith(x1_weights())
    y64 = G.forward(sd, x, res_blocks=1)
    none = dict(ar, levels=["F16X3"] * 4, deep="F16X3")
    assert torch.equal(X.forward(sd, x, 1, none), y64)                # nothing rounded: the oracle itself
    e1 = (X.forward(sd, x, 1, ar) - y64).abs().max().item()
    e2 = (X.forward(sd, x, 1, ar, compose=True) - y64).abs().max().item()
    print("err_emul %.3e  err_emul_composed %.3e" % (e1, e2))
    assert 1e-5 < e1 <= 2 * e2 + 2e-5 and e2 <= 2 * e1 + 2e-5
