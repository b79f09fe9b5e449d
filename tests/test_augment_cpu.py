"""smirk_amd.augment without a GPU: the law of the kernel's host restatement against the reference's law (tests/augment_law.py), the error paths of the C entry
(raw ctypes, nothing is launched) and the host side of the public API."""
import ctypes as C

import numpy as np
import pytest
import torch

from augment_law import ks_distance, reference_law, restate, synth_inputs, synth_templates

OK, BAD_ARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = C.c_void_p(0x1000)                                       # "some device address": never dereferenced on the host

B_LAW, KE_LAW, E_LAW = 16384, 4, 50
KS_CRIT = 1.95 * np.sqrt(2.0 / (B_LAW * KE_LAW // 4))        # alpha = 0.001, two samples of N/4 independent rows each: 0.0215


@pytest.fixture(scope="module")
def law():
    """both laws once, on the same inputs: (inputs, templates, bank arrays, restatement outputs, plan, reference outputs, reference group of every row)"""
    enc = synth_inputs(B_LAW, E=E_LAW, S=4, seed=11)
    templates = synth_templates()
    table = np.concatenate(list(templates.values()), 0)
    offsets = np.cumsum([0] + [len(t) for t in templates.values()])
    ours, plan = restate(enc, KE_LAW, table, offsets, E_LAW, True, seed=0x5EED5EED1234, offset=987654321)
    ref, gids = reference_law({k: torch.from_numpy(v) for k, v in enc.items()}, KE_LAW, templates, seed=2024, num_expression=E_LAW, _return_groups=True)
    ref = {k: v.numpy().astype(np.float64) for k, v in ref.items()}
    rgroup = np.empty(B_LAW * KE_LAW, dtype=np.int64)
    for g, ids in enumerate(gids):
        rgroup[ids.numpy()] = g
    return enc, templates, table, offsets, ours, plan, ref, rgroup


def _row_quantities(out, rows, group, e0):
    """per-row quantities of one law for the rows of one group: name -> sample"""
    ex = out["expression_params"][rows]
    q = {"expression std": (ex - e0[rows % len(e0)] if group == 0 else ex).std(axis=1), "expression max": np.abs(ex).max(axis=1)}
    for c in range(3):
        q[f"jaw[{c}]"] = out["jaw_params"][rows, c]
    for c in range(2):
        q[f"eyelid[{c}]"] = out["eyelid_params"][rows, c]
    return q


def test_restated_law_matches_reference_law(law):
    """Two-sample KS between the restatement and the reference's law, per group and per ROW quantity (the elements of a row share the scalars u, u': they are not
    pooled).  Measured on these inputs: the reference law against itself on two seeds gives D <= 0.014 for every quantity; a 5 % error in the noise scale
    (0.21 for 0.2) gives 0.039 and `1 + u` for `1 + 2u` gives 0.35, against the critical value 0.0215."""
    enc, _, _, _, ours, plan, ref, rgroup = law
    e0 = enc["expression_params"].astype(np.float64)
    worst = {}
    for g in range(4):
        a = _row_quantities(ours, np.nonzero(plan[:, 0] == g)[0], g, e0)
        b = _row_quantities(ref, np.nonzero(rgroup == g)[0], g, e0)
        for name in a:
            worst[(g, name)] = ks_distance(a[name], b[name])
    print({k: round(v, 4) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v > KS_CRIT}
    assert not bad, bad


def test_restated_law_exact_facts(law):
    enc, templates, table, offsets, ours, plan, ref, rgroup = law
    N = B_LAW * KE_LAW
    group, pos = plan[:, 0], plan[:, 1]
    sizes = [N // 4, 2 * N // 4 - N // 4, 3 * N // 4 - 2 * N // 4, N - 3 * N // 4]
    assert [int((group == g).sum()) for g in range(4)] == sizes == [int((rgroup == g).sum()) for g in range(4)]
    for g in range(4):
        assert np.array_equal(np.sort(pos[group == g]), np.arange(sizes[g]))
    m1 = np.nonzero(group == 1)[0]
    assert np.array_equal(np.sort(plan[m1, 2]), m1) and (plan[group != 1, 2] == -1).all()          # sources: a permutation of the group's own rows
    assert (plan[m1, 2] != m1).mean() > 0.99                                                       # ... and not the identity
    assert (ours["jaw_params"][group == 3] == 0).all()
    j0 = ours["jaw_params"][group != 3, 0]
    assert j0.min() >= 0 and j0.max() <= 0.5
    assert ours["eyelid_params"].min() >= 0 and ours["eyelid_params"].max() <= 1
    # template classes: uniform over CLASSES (two-level draw), rows uniform inside a class
    trow = plan[group == 2, 3].astype(np.int64)
    assert (plan[group != 2, 3] == -1).all() and trow.min() >= 0 and trow.max() < len(table)
    cls = np.searchsorted(offsets, trow, side="right") - 1
    n2, nc = len(trow), len(offsets) - 1
    cnt = np.bincount(cls, minlength=nc)
    assert np.abs(cnt - n2 / nc).max() < 6 * np.sqrt(n2 / nc * (1 - 1 / nc)), cnt
    for c in range(nc):
        k = offsets[c + 1] - offsets[c]
        inside = np.bincount(trow[cls == c] - offsets[c], minlength=k)
        assert inside.min() > 0 and np.abs(inside - cnt[c] / k).max() <= 6 * np.sqrt(cnt[c] / k), (c, inside)
    for k in ("shape_params", "pose_params", "cam"):
        assert np.array_equal(ours[k], np.concatenate(KE_LAW * [enc[k]]))


@pytest.mark.parametrize("N", [1, 2, 3, 5, 7])
def test_restated_groups_follow_the_reference_slices(N):
    enc = synth_inputs(N, seed=N)
    t = synth_templates()
    _, plan = restate(enc, 1, np.concatenate(list(t.values()), 0), np.cumsum([0] + [len(v) for v in t.values()]), 50, True, seed=5, offset=N)
    perm = np.arange(N)
    want = [len(s) for s in (perm[:N // 4], perm[N // 4:2 * N // 4], perm[2 * N // 4:3 * N // 4], perm[3 * N // 4:])]      # smirk_trainer.py:202
    assert [int((plan[:, 0] == g).sum()) for g in range(4)] == want


# ---- C entry: every refusal comes before anything touches the device ---------------------------------------------------------------------------------------
def _call(lib, **kw):
    off = kw.pop("offsets", (C.c_int32 * 4)(0, 1, 4, 9))
    a = dict(expression=P, jaw=P, eyelid=P, shape=P, pose=P, cam=P, B=4, E=50, S=300, Ke=2, num_expression=50, use_eyelids=1, templates=P, class_offsets=P,
             class_offsets_host=C.cast(off, C.c_void_p), n_classes=3, seed=1, offset=0, o_expression=P, o_jaw=P, o_eyelid=P, o_shape=P, o_pose=P, o_cam=P,
             plan=P, ws=P, ws_bytes=None, stream=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.smirk_cycle_augment_workspace_bytes(max(a["B"] * a["Ke"], 1))
    return lib.smirk_cycle_augment(*a.values())


def test_c_entry_error_paths():
    from smirk_amd import _lib as L
    from smirk_amd.augment import MAX_ROWS
    lib = L.lib()
    for name in ("expression", "jaw", "eyelid", "shape", "pose", "cam", "templates", "class_offsets", "class_offsets_host", "o_expression", "o_jaw", "o_eyelid",
                 "o_shape", "o_pose", "o_cam", "plan", "ws"):
        assert _call(lib, **{name: None}) == BAD_ARG, name
    assert _call(lib, B=0) == BAD_ARG and _call(lib, Ke=0) == BAD_ARG and _call(lib, E=0, num_expression=0) == BAD_ARG
    assert _call(lib, num_expression=51) == BAD_ARG                                               # more template columns than the expression has
    assert _call(lib, n_classes=0) == BAD_ARG                                                     # empty bank
    assert _call(lib, offsets=(C.c_int32 * 4)(0, 1, 1, 9)) == BAD_ARG                             # an empty class
    assert _call(lib, offsets=(C.c_int32 * 4)(1, 2, 4, 9)) == BAD_ARG                             # offsets do not start at 0
    need = lib.smirk_cycle_augment_workspace_bytes(8)
    assert need >= 8 * 8 and lib.smirk_cycle_augment_workspace_bytes(MAX_ROWS) >= need
    assert _call(lib, ws_bytes=need - 1) == WORKSPACE
    assert _call(lib, B=MAX_ROWS // 2 + 1, ws_bytes=1 << 30) == UNSUPPORTED                        # Ke * B one pair of rows above the cap
    assert _call(lib, B=1 << 30, Ke=4, ws_bytes=1 << 30) == UNSUPPORTED                            # ... and a product that does not fit an int
    assert MAX_ROWS >= 8192


# ---- public API, host side -----------------------------------------------------------------------------------------------------------------------------------
def test_public_api_on_the_host(tmp_path):
    import smirk_amd
    from smirk_amd import SmirkHipError, TemplateBank, augment_flame_params, load_templates
    from smirk_amd.augment import TEMPLATE_CLASSES, n_counters
    templates = synth_templates()
    bank = TemplateBank(templates, num_expression=40)
    assert bank.offsets.tolist() == [0, 1, 4, 11, 23, 28] and bank.offsets.dtype == torch.int32 and bank.n_classes == 5
    assert tuple(bank.table.shape) == (28, 40) and bank.table.dtype == torch.float32
    assert np.array_equal(bank.table[4:11].numpy(), list(templates.values())[2][:, :40])
    with pytest.raises(ValueError):
        TemplateBank({"a": np.zeros((2, 30), np.float32)}, num_expression=50)
    with pytest.raises(ValueError):
        TemplateBank({"a": np.zeros((0, 50), np.float32)})
    enc = {k: torch.from_numpy(v) for k, v in synth_inputs(4).items()}
    with pytest.raises(SmirkHipError):
        augment_flame_params(enc, TemplateBank(templates))                                         # CPU tensors: no fallback
    assert n_counters(8, 50) == 400 and n_counters(8, 2) == 32
    assert smirk_amd.augment_flame_params is augment_flame_params
    # load_templates: the reference's directory layout and class filter (utils.py:5-25)
    root = tmp_path / "expression_templates_famos"
    for subject, cls, n in (("subj1_", TEMPLATE_CLASSES[0], 3), ("subj1_", "not_a_class", 2), ("subj2_", TEMPLATE_CLASSES[-1], 1)):
        d = root / subject / cls
        d.mkdir(parents=True)
        for i in range(n):
            np.save(d / f"{i}.npy", {"expression": np.full((1, 100), float(i), np.float32)}, allow_pickle=True)
    (root / "subj1_" / "clip.mp4").write_bytes(b"")
    (root / "readme.txt").write_text("x")
    got = load_templates(str(root))
    assert set(got) == {"subj1_" + TEMPLATE_CLASSES[0], "subj2_" + TEMPLATE_CLASSES[-1]}
    assert got["subj1_" + TEMPLATE_CLASSES[0]].shape == (3, 100) and got["subj2_" + TEMPLATE_CLASSES[-1]].shape == (1, 100)
    assert tuple(TemplateBank(got).table.shape) == (4, 50)
