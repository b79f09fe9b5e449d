"""The extension table of include/smirk_train_handoff.h without a GPU: the table against its header, its version, the switch's documentation, and the decisions of
masking.train_masked_image_packed between the fused launches and the separate utilities (library and utilities stubbed: nothing touches a device)."""
import ctypes as C
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "SMIRK_DISABLE_TRAIN_HANDOFF"


def test_extension_table_equals_the_header():
    from smirk_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "smirk_train_handoff.h")).read()
    declared = set(re.findall(r"\b(smirk_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.TRAIN_HANDOFF_EXPORTS), declared ^ set(L.TRAIN_HANDOFF_EXPORTS)
    assert L.TRAIN_HANDOFF_EXPORTS == tuple(L.TRAIN_HANDOFF_SIGS) and len(L.TRAIN_HANDOFF_EXPORTS) == 3
    for other in (L.EXPORTS, L.MICA_EXPORTS, L.EMOTION_EXPORTS, L.OPTIM_EXPORTS, L.HANDOFF_EXPORTS, L.GENPLAN_EXPORTS, L.GENARITH_EXPORTS, L.DATA_EXPORTS,
                  L.VISUAL_EXPORTS):
        assert not set(L.TRAIN_HANDOFF_EXPORTS) & set(other)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    version = int(re.search(r"#define\s+SMIRK_TRAIN_HANDOFF_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert L.lib().smirk_train_handoff_abi_version() == L.TRAIN_HANDOFF_ABI_VERSION == version == 1
    rules = {n.lower(): int(v) for n, v in re.findall(r"#define\s+SMIRK_RENDERED_RULE_(\w+)\s+(\d+)", hdr)}
    assert rules == {n: i for i, n in enumerate(L.RENDERED_RULES)}
    assert "smirk_train_handoff.h" in open(os.path.join(REPO, "README.md")).read()
    assert '"smirk_train_handoff.h"' in open(os.path.join(REPO, "smirk_amd", "build.py")).read()
    # the other tables and their versions did not move, and none of their headers declares the new entries
    lib = L.lib()
    assert lib.smirk_abi_version() == L.ABI_VERSION == 17 and len(L.EXPORTS) == 116
    assert lib.smirk_handoff_abi_version() == L.HANDOFF_ABI_VERSION == 1 and len(L.HANDOFF_EXPORTS) == 3
    for name in os.listdir(os.path.join(REPO, "include")):
        if name != "smirk_train_handoff.h":
            text = open(os.path.join(REPO, "include", name)).read()
            assert not any(e in text for e in L.TRAIN_HANDOFF_EXPORTS), name


def test_the_switch_is_documented_where_the_switches_are():
    table = open(os.path.join(REPO, "smirk_amd", "csrc", "switches.h")).read().split("#pragma once")[0]
    assert re.search(r"^// " + SWITCH + r"\s", table, re.M)
    assert "`" + SWITCH + "`" in open(os.path.join(REPO, "INTEGRATION.md")).read()


class _Lib:
    """stands for libsmirk_hip.so: records the entries called, answers `handoff_code` from the hand-off launch"""

    def __init__(self, handoff_code=0):
        self.calls, self.handoff_code = [], handoff_code

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.handoff_code if name == "smirk_train_masking_handoff" else 0
        return entry


V, F = 11, 7


@pytest.fixture
def stubbed(monkeypatch):
    from smirk_amd import masking as M
    seen = {}

    def separate(img, hull_mask, rendered, tv_src, faces, prob, tv_dst, Ke, mask_ratio, radius, rule, random_mask, rng, S):
        seen["rng"], seen["S"] = rng, S
        offs = [rng(n)[1] for n in (1, 2, 3)] if isinstance(rng, M._Replay) else None     # the three offsets a replay hands out, in order
        seen["offsets"] = offs
        return "MASKED", {"points1": "P1"}
    monkeypatch.setattr(M, "_train_masked_separate", separate)
    monkeypatch.setattr(M, "_full_mesh", lambda faces: (None, {"faces": torch.zeros(F, 3, dtype=torch.int32)}, V, F))
    monkeypatch.setattr(M.L, "ptr", lambda t, dtype=torch.float32, allow_none=False: None)
    monkeypatch.setattr(M.L, "stream_ptr", lambda: None)
    monkeypatch.delenv(SWITCH, raising=False)

    def run(lib, B=2, Ke=1, C_=3, H=32, W=48, hull=None, second=False, rng=None, **kw):
        monkeypatch.setattr(M.L, "lib", lambda: lib)
        KB = Ke * B
        img, rendered = torch.zeros(B, C_, H, W), torch.zeros(KB, C_, H, W)
        hull = torch.ones(B, 1, H, W) if hull is None else hull
        tv_dst = torch.zeros(KB, V, 3) if second else None
        return M.train_masked_image_packed(img, hull, rendered, torch.zeros(B, V, 3), torch.zeros(F, 3), torch.ones(F), trans_verts_dst=tv_dst, Ke=Ke,
                                           mask_ratio=0.1, rng=rng, **kw)
    return M, seen, run


def test_the_fused_launches_serve_the_call_they_were_built_for(stubbed):
    M, seen, run = stubbed
    for second, Ke, hull in ((False, 1, None), (True, 2, None), (True, 3, torch.ones(1, 32, 48)), (True, 2, torch.ones(2, 32, 48))):
        lib, rng = _Lib(), M.PhiloxStream(5, 1000)
        masked, packed, coords = run(lib, Ke=Ke, second=second, hull=hull, rng=rng, want_coords=True,
                                     **(dict(rendered_rule="positive", random_mask=0.005) if second else {}))
        names = [n for n, _ in lib.calls]
        assert names == ["smirk_vertex_normals", "smirk_mask_face_weights", "smirk_sample_transfer_points", "smirk_train_masking_handoff"]   # four launches
        assert "rng" not in seen and packed.shape == (Ke * 2, 32, 48, 8) and masked.shape == (Ke * 2, 3, 32, 48)
        N, KB = int(0.1 * 32 * 32), Ke * 2
        assert rng.offset == 1000 + 2 * N + (KB * 32 * 48 + 3) // 4 + KB * 3 * 32 * 48                    # points, field, noise
        sample, handoff = lib.calls[2][1], lib.calls[3][1]
        assert sample[4:12] == (2, Ke, V, F, N, 32, 5, 1000)                                               # B, Ke, V, F, num, image_size = H, seed, offset
        assert handoff[3] == (0 if hull is not None and hull.shape[0] == 1 else 32 * 48)                   # ONE hull for every frame: batch stride 0
        assert handoff[6:12] == (2, Ke, N, 32, 48, int(second)) and handoff[13:16] == (5, 1000 + 2 * N, 1000 + 2 * N + (KB * 32 * 48 + 3) // 4)
        assert coords["points1"].shape == (2, N, 3) and coords["points2"].shape == (KB, N, 3) and coords["sampled_faces_indices"].dtype == torch.int64
        assert (coords["points2"] is coords["points1"]) == (not second)
    assert run(_Lib(), rng=M.PhiloxStream(5, 0))[2] is None                                                # coords only on request


@pytest.mark.parametrize("why,kw", [("radius", dict(mask_dilation_radius=15)), ("channels", dict(C_=1)), ("no field", dict(random_mask=0.0)),
                                    ("hull shape", dict(hull=torch.ones(2, 2, 32, 48))), ("quantised for a larger image", dict(image_size=224)),
                                    ("image narrower than high", dict(H=48, W=32)), ("switch", {})])
def test_packed_is_none_and_the_separate_utilities_draw_from_the_callers_stream(stubbed, monkeypatch, why, kw):
    M, seen, run = stubbed
    if why == "switch":
        monkeypatch.setenv(SWITCH, "1")
    lib, rng = _Lib(), M.PhiloxStream(5, 1000)
    masked, packed, coords = run(lib, rng=rng, want_coords=True, **kw)
    assert (masked, packed, coords) == ("MASKED", None, {"points1": "P1"}) and not lib.calls
    assert seen["rng"] is rng and seen["S"] == kw.get("image_size", kw.get("H", 32))
    assert run(lib, rng=rng, **kw) == ("MASKED", None, None)


def test_unsupported_replays_the_offsets_already_drawn(stubbed):
    M, seen, run = stubbed
    lib, rng = _Lib(handoff_code=M.L.SMIRK_ERR_UNSUPPORTED), M.PhiloxStream(5, 1000)
    masked, packed, coords = run(lib, Ke=2, second=True, rng=rng)
    N, KB = int(0.1 * 32 * 32), 4
    assert (masked, packed, coords) == ("MASKED", None, None) and lib.calls[-1][0] == "smirk_train_masking_handoff"
    assert seen["offsets"] == [1000, 1000 + 2 * N, 1000 + 2 * N + (KB * 32 * 48 + 3) // 4]
    assert rng.offset == 1000 + 2 * N + (KB * 32 * 48 + 3) // 4 + KB * 3 * 32 * 48                        # the stream ends where the fused call leaves it


def test_wrong_arguments_raise(stubbed):
    M, _, run = stubbed
    with pytest.raises(ValueError, match="rendered_rule"):
        run(_Lib(), rendered_rule="any")
    with pytest.raises(ValueError, match="trans_verts_dst"):
        run(_Lib(), Ke=2)
