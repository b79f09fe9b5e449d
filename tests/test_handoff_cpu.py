"""The extension table of include/smirk_handoff.h without a GPU: the table against its header, its version, and every refusal of its two launch entries
(raw ctypes, dummy pointers that are never dereferenced: a refusal comes before anything touches the device)."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, R, S, T, U = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000         # never dereferenced
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def test_extension_table_equals_the_header():
    from smirk_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "smirk_handoff.h")).read()
    declared = set(re.findall(r"\b(smirk_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.HANDOFF_EXPORTS), declared ^ set(L.HANDOFF_EXPORTS)
    assert L.HANDOFF_EXPORTS == tuple(L.HANDOFF_SIGS) and len(L.HANDOFF_EXPORTS) == 3
    for other in (L.EXPORTS, L.MICA_EXPORTS, L.EMOTION_EXPORTS, L.OPTIM_EXPORTS):
        assert not set(L.HANDOFF_EXPORTS) & set(other)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    version = int(re.search(r"#define\s+SMIRK_HANDOFF_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert L.lib().smirk_handoff_abi_version() == L.HANDOFF_ABI_VERSION == version == 1
    assert "smirk_handoff.h" in open(os.path.join(REPO, "README.md")).read()
    assert '"smirk_handoff.h"' in open(os.path.join(REPO, "smirk_amd", "build.py")).read()
    # the other tables and their versions did not move, and none of their headers declares the new entries
    lib = L.lib()
    assert lib.smirk_abi_version() == L.ABI_VERSION == 17 and len(L.EXPORTS) == 116
    assert lib.smirk_mica_abi_version() == L.MICA_ABI_VERSION and lib.smirk_emotion_abi_version() == L.EMOTION_ABI_VERSION
    assert lib.smirk_optim_abi_version() == L.OPTIM_ABI_VERSION
    for name in ("smirk_hip.h", "smirk_mica.h", "smirk_emotion.h", "smirk_optim.h"):
        text = open(os.path.join(REPO, "include", name)).read()
        assert not any(e in text for e in L.HANDOFF_EXPORTS), name


def test_the_switch_is_documented_where_the_switches_are():
    table = open(os.path.join(REPO, "smirk_amd", "csrc", "switches.h")).read().split("#pragma once")[0]
    assert re.search(r"^// SMIRK_DISABLE_MASKING_HANDOFF\s", table, re.M)
    assert "`SMIRK_DISABLE_MASKING_HANDOFF`" in open(os.path.join(REPO, "INTEGRATION.md")).read()


def _weights(precision=None, **kw):
    from smirk_amd import _lib as L
    w = L.SmirkGeneratorWeights()
    w.in_channels, w.out_channels, w.features, w.res_blocks, w.cin_pad = 6, 3, 32, 5, 8
    w.precision = L.PRECISION_F16X3 if precision is None else precision
    w.final_w, w.final_b = P, Q
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def test_generator_forward_packed_refuses_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    need = lib.smirk_generator_workspace_bytes(_weights(), 2, 32, 48)
    assert need > 0

    def call(w=None, packed=R, y=S, B=2, H=32, W=48, ws=T, ws_bytes=None):
        return lib.smirk_generator_forward_packed(_weights() if w is None else w, packed, y, B, H, W, None, ws, need if ws_bytes is None else ws_bytes, None)
    for name in ("packed", "y", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    assert lib.smirk_generator_forward_packed(None, R, S, 2, 32, 48, None, T, need, None) == BAD_ARG
    assert call(w=_weights(precision=L.PRECISION_F32)) == BAD_ARG                   # the packed tensor is the split-fp16 format: no other precision reads it
    assert call(w=_weights(precision=7)) == BAD_ARG
    assert call(w=_weights(final_w=None)) == BAD_ARG and call(w=_weights(final_b=None)) == BAD_ARG
    assert call(w=_weights(cin_pad=4)) == BAD_ARG and call(w=_weights(features=12)) == BAD_ARG
    for bad in (dict(B=0), dict(H=40), dict(W=0), dict(W=50)):
        assert call(**bad) == BAD_ARG, bad
    assert call(ws_bytes=0) == WORKSPACE and call(ws_bytes=need - 1) == WORKSPACE


def test_masking_handoff_refuses_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()

    def call(img=P, rendered=Q, hull=R, stride=32 * 48, pmask=S, B=2, H=32, W=48, p=0.05, masked=T, packed=U):
        return lib.smirk_masking_handoff(img, rendered, hull, stride, pmask, B, H, W, p, 1, 0, 0, masked, packed, None)
    for name in ("img", "rendered", "hull", "pmask", "masked", "packed"):
        assert call(**{name: None}) == BAD_ARG, name
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(stride=48), dict(stride=-1), dict(p=0.0), dict(p=-0.5), dict(p=float("nan"))):
        assert call(**bad) == BAD_ARG, bad
    # rows too wide for two workgroups per CU: the caller keeps the separate launches
    assert call(W=1024, stride=32 * 1024) == UNSUPPORTED and call(W=1024, stride=0) == UNSUPPORTED
