"""smirk_amd.optim without a GPU: the extension table of include/smirk_optim.h, every refusal of its entries (raw ctypes, dummy pointers: a refusal comes
before anything touches the device), the chunk layout of tests/optim_law.py's tensors computed independently, the law against torch.optim.Adam and
torch.nn.utils.clip_grad_norm_ in float64, the constructor's refusals, the state dict against torch.optim.Adam's, and the proof that the GPU bounds see five
deliberate mistakes."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import optim_law as OL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, R, S, ODD2 = 0x10000, 0x20000, 0x30000, 0x40000, 0x10002                   # never dereferenced; ODD2 is not 4-byte aligned
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def test_extension_table_equals_the_header():
    from smirk_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "smirk_optim.h")).read()
    declared = set(re.findall(r"\b(smirk_optim_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.OPTIM_EXPORTS), declared ^ set(L.OPTIM_EXPORTS)
    assert L.OPTIM_EXPORTS == tuple(L.OPTIM_SIGS)
    for other in (L.EXPORTS, L.MICA_EXPORTS, L.EMOTION_EXPORTS):
        assert not set(L.OPTIM_EXPORTS) & set(other)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))
    assert L.lib().smirk_optim_abi_version() == L.OPTIM_ABI_VERSION == val("SMIRK_OPTIM_ABI_VERSION") == 1
    assert L.OPTIM_CHUNK == val("SMIRK_OPTIM_CHUNK") and L.OPTIM_CHUNK % 4 == 0
    kinds = dict(re.findall(r"SMIRK_OPTIM_KIND_(NORM|SCALE|ADAM) = (\d)", hdr))
    assert (L.OPTIM_KIND_NORM, L.OPTIM_KIND_SCALE, L.OPTIM_KIND_ADAM) == (int(kinds["NORM"]), int(kinds["SCALE"]), int(kinds["ADAM"]))
    assert C.sizeof(L.SmirkOptimTensor) == 40 and C.sizeof(L.SmirkOptimStep) == 16
    assert "smirk_optim.h" in open(os.path.join(REPO, "README.md")).read()
    # the other tables and their versions did not move
    assert L.lib().smirk_abi_version() == L.ABI_VERSION and L.lib().smirk_mica_abi_version() == L.MICA_ABI_VERSION
    assert L.lib().smirk_emotion_abi_version() == L.EMOTION_ABI_VERSION
    for name in ("smirk_hip.h", "smirk_mica.h", "smirk_emotion.h"):
        assert "smirk_optim" not in open(os.path.join(REPO, "include", name)).read().lower(), name
    assert '"smirk_optim.h"' in open(os.path.join(REPO, "smirk_amd", "build.py")).read()


def _rows(numels, param=P, exp_avg=Q, exp_avg_sq=R, grad=S, step_size=1e-3, bc=0.5):
    from smirk_amd import _lib as L
    n = len(numels)
    t, s = (L.SmirkOptimTensor * n)(), (L.SmirkOptimStep * n)()
    for k, numel in enumerate(numels):
        t[k].param, t[k].exp_avg, t[k].exp_avg_sq, t[k].numel, t[k].first_chunk = param, exp_avg, exp_avg_sq, numel, -7
        s[k].grad, s[k].step_size, s[k].bias_correction2_sqrt = grad, step_size, bc
    return t, s


def _plan(numels, kinds=7, with_steps=True, n=None, **kw):
    from smirk_amd import _lib as L
    t, s = _rows(numels, **kw)
    total = C.c_longlong(-1)
    code = L.lib().smirk_optim_plan(t, s if with_steps else None, len(numels) if n is None else n, kinds, C.byref(total))
    return code, total.value, [r.first_chunk for r in t]


def test_plan_refusals_and_layout():
    from smirk_amd import _lib as L
    lib = L.lib()
    assert _plan([5, 0, 4097]) == (0, 3, [0, 1, 1])                                 # numel 0 is legal and owns no chunk
    assert _plan([5], with_steps=False) == (0, 1, [0])
    for n in (0, -1):
        assert _plan([5], n=n)[0] == BAD_ARG
    for kinds in (0, 8, -1):
        assert _plan([5], kinds=kinds)[0] == BAD_ARG
    assert _plan([5, -1])[0] == BAD_ARG
    for name in ("param", "exp_avg", "exp_avg_sq"):
        for bad in (None, ODD2):
            assert _plan([5], **{name: bad})[0] == BAD_ARG, (name, bad)
            assert _plan([5], kinds=3, **{name: bad})[0] == 0, (name, bad)         # the clip does not need them
            assert _plan([0], **{name: None})[0] == 0                               # nor does a tensor without elements
    for bad in (None, ODD2):
        for kinds in (1, 2, 4):
            assert _plan([5], kinds=kinds, grad=bad)[0] == BAD_ARG
    for ss in (-1.0, float("inf"), float("nan")):
        assert _plan([5], step_size=ss)[0] == BAD_ARG and _plan([5], kinds=3, step_size=ss)[0] == 0
    for bc in (0.0, -0.5, float("inf"), float("nan")):
        assert _plan([5], bc=bc)[0] == BAD_ARG
    assert _plan([1 << 31])[0] == UNSUPPORTED and _plan([(1 << 31) - 1])[0] == 0
    many = [(1 << 31) - 1] * 4097                                                   # 4097 x 2^19 chunks > 2^31 - 1
    assert _plan(many)[0] == UNSUPPORTED and _plan(many[:4095])[0] == 0
    code, total, first = _plan([5, 1 << 31])
    assert code == UNSUPPORTED and first == [-7, -7] and total == -1               # nothing is written on a refusal
    t, _ = _rows([5])
    assert lib.smirk_optim_plan(None, None, 1, 7, C.byref(C.c_longlong())) == BAD_ARG and lib.smirk_optim_plan(t, None, 1, 7, None) == BAD_ARG


def test_chunk_layout_of_the_cases_matches_an_independent_count():
    from smirk_amd import _lib as L
    numels = [math.prod(s) for _, s in OL.CASES]
    code, total, first = _plan(numels)
    want_first, want_total = OL.expected_chunks()
    assert code == 0 and first == want_first and total == want_total
    t, _ = _rows(numels)
    tot = C.c_longlong()
    assert L.lib().smirk_optim_plan(t, None, len(numels), 7, C.byref(tot)) == 0
    cmap = (C.c_int * total)()
    assert L.lib().smirk_optim_chunk_map(t, len(numels), cmap, total) == 0
    want = [i for i, k in enumerate(numels) for _ in range(-(-k // OL.C))]
    assert list(cmap) == want
    for bad_total in (total - 1, total + 1, -1):
        assert L.lib().smirk_optim_chunk_map(t, len(numels), cmap, bad_total) == BAD_ARG
    assert L.lib().smirk_optim_chunk_map(t, len(numels), None, total) == BAD_ARG and L.lib().smirk_optim_chunk_map(None, 1, cmap, 1) == BAD_ARG
    t[3].first_chunk += 1
    assert L.lib().smirk_optim_chunk_map(t, len(numels), cmap, total) == BAD_ARG


def test_launch_entries_refuse_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    assert lib.smirk_optim_grad_norm_workspace_bytes(0) == 256 and lib.smirk_optim_grad_norm_workspace_bytes(33) == 512
    assert lib.smirk_optim_grad_norm_workspace_bytes(-1) == 0 and lib.smirk_optim_grad_norm_workspace_bytes(1 << 31) == 0
    norm = lambda t=P, s=Q, m=R, n=3, total=9, max_norm=0.1, ws=S, ws_bytes=256, out=P: lib.smirk_optim_grad_norm(t, s, m, n, total, max_norm, ws, ws_bytes, out, None)
    scale = lambda t=P, s=Q, m=R, n=3, total=9, coef=S: lib.smirk_optim_scale_grads(t, s, m, n, total, coef, None)
    adam = lambda t=P, s=Q, m=R, n=3, total=9, b1=0.9, b2=0.999, eps=1e-8, gs=None: lib.smirk_optim_adam_step(t, s, m, n, total, b1, b2, eps, gs, None)
    for fn in (norm, scale, adam):
        for name in ("t", "s", "m"):
            assert fn(**{name: None}) == BAD_ARG and fn(**{name: ODD2}) == BAD_ARG, name
        for n in (0, -2):
            assert fn(n=n) == BAD_ARG
        assert fn(total=-1) == BAD_ARG and fn(total=1 << 31) == UNSUPPORTED
    for name in ("ws", "out"):
        assert norm(**{name: None}) == BAD_ARG and norm(**{name: ODD2}) == BAD_ARG, name
    for mx in (-0.1, float("inf"), float("nan")):
        assert norm(max_norm=mx) == BAD_ARG
    assert norm(ws_bytes=0) == WORKSPACE and norm(total=33, ws_bytes=256) == WORKSPACE
    assert scale(coef=None) == BAD_ARG and scale(coef=ODD2) == BAD_ARG and adam(gs=ODD2) == BAD_ARG
    for name in ("b1", "b2"):
        for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
            assert adam(**{name: bad}) == BAD_ARG, (name, bad)
    for bad in (-1e-8, float("nan"), float("inf")):
        assert adam(eps=bad) == BAD_ARG
    assert scale(total=0, m=None) == 0 and adam(total=0, m=None) == 0              # nothing to do is not an error, and launches nothing


@pytest.mark.parametrize("hyper", range(len(OL.HYPERS)))
def test_law_equals_torch_in_float64(hyper):
    lw, rf = OL.law(hyper), OL.ref(hyper, OL.MAX_NORM, torch.float64)
    worst = 0.0
    for k, (l, r) in enumerate(zip(lw, rf)):
        assert l["t"] == r["t"]
        assert abs(l["norm"] - r["norm"]) <= 1e-12 * l["norm"]
        for q in ("p", "m", "v", "clipped"):
            for i, name in enumerate(OL.NAMES):
                if l[q][i] is None:
                    assert r[q][i] is None, (q, name, k)
                    continue
                scale = float(l[q][i].abs().max()) if l[q][i].numel() else 0.0
                err = OL.distance(r[q][i], l[q][i])
                worst = max(worst, err / scale if scale else err)
                assert err <= 1e-12 * scale, (q, name, k, err, scale)
    print(f"law against torch.optim.Adam + clip_grad_norm_ in float64, hyper {hyper}: largest relative distance {worst:.2e}")
    assert lw[0]["coef"] < 0.05                                                     # the clip is active on these inputs
    # what the input set promises
    params, grads = OL.inputs()
    assert all(float(params[OL.NAMES.index(n)].abs().max()) == 0.0 for n in OL.ZERO_START)
    name, step, count = OL.ZEROS_IN_GRAD
    assert int((grads[step - 1][OL.NAMES.index(name)] == 0).sum()) >= count
    assert lw[-1]["t"][OL.NAMES.index("never")] == 0 and lw[-1]["t"][OL.NAMES.index("skip3")] == OL.STEPS - 1 and lw[-1]["m"][OL.NAMES.index("never")] is None


@pytest.mark.parametrize("variant", ["no_bias_correction1", "no_bias_correction2", "eps_inside_sqrt", "step_off_by_one", "clip_not_clamped"])
def test_the_bounds_see_a_deliberate_mistake(variant):
    """each wrong law must sit more than 100 x the bound away from the right one in some tensor"""
    for hyper in range(len(OL.HYPERS)):
        max_norm = 1e3 if variant == "clip_not_clamped" else OL.MAX_NORM             # the clamp matters only where no clipping is needed
        lw, rf, wrong = OL.law(hyper, max_norm), OL.ref32(hyper, max_norm), OL.law(hyper, max_norm, variant)
        best = 0.0
        for l, r, w in zip(lw, rf, wrong):
            for i in range(len(OL.NAMES)):
                if l["p"][i] is not None and l["p"][i].numel():
                    best = max(best, OL.distance(w["p"][i], l["p"][i]) / OL.state_bound(r["p"][i], l["p"][i]))
        print(f"{variant}, hyper {hyper}: moves a parameter tensor by {best:.3g} x its bound")
        assert best > 100.0, (variant, hyper, best)


def test_constructor_refusals_name_the_option():
    from smirk_amd import Adam
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(weight_decay=1e-4), dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(fused=True),
               dict(decoupled_weight_decay=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            Adam(p, **kw)
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            Adam(p, **kw)
    opt = Adam(p)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(2))], amsgrad=True))


def test_state_dict_structure_equals_torch_and_cpu_steps_raise():
    from smirk_amd import Adam, SmirkHipError, clip_grad_norm_
    ps = [torch.nn.Parameter(torch.randn(s)) for s in ((5,), (2, 3))]
    ours, theirs = Adam(ps, lr=2e-3, betas=(0.5, 0.999)), torch.optim.Adam(ps, lr=2e-3, betas=(0.5, 0.999))
    assert isinstance(ours, torch.optim.Optimizer)
    assert ours.state_dict() == theirs.state_dict() and list(ours.param_groups[0]) == list(theirs.param_groups[0]) and ours.defaults == theirs.defaults
    for p in ps:
        p.grad = torch.ones_like(p)
    theirs.step()
    ours.load_state_dict(theirs.state_dict())                                      # torch's state loads here ...
    sd = ours.state_dict()
    assert list(sd["state"][0]) == ["step", "exp_avg", "exp_avg_sq"] and sd["state"][0]["step"].device.type == "cpu" and sd["state"][0]["step"].dtype == torch.float32
    torch.optim.Adam(ps).load_state_dict(sd)                                       # ... and goes back
    with pytest.raises(SmirkHipError, match="CPU"):
        ours.step()
    with pytest.raises(SmirkHipError, match="CPU"):
        clip_grad_norm_(ps, 0.1)
    with pytest.raises(SmirkHipError, match="norm_type"):
        clip_grad_norm_(ps, 0.1, norm_type=1.0)
    zero = clip_grad_norm_([torch.nn.Parameter(torch.zeros(2))], 0.1)              # no gradients: a zero tensor, like torch
    assert float(zero) == 0.0 and float(torch.nn.utils.clip_grad_norm_([torch.nn.Parameter(torch.zeros(2))], 0.1)) == 0.0
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(ours, T_max=5, eta_min=1e-5)          # schedulers take it as any torch optimiser
    ours.param_groups[0]["lr"] = 1e-4
    ours.zero_grad()
    assert all(p.grad is None for p in ps) and sched.get_last_lr()
