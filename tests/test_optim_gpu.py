"""smirk_amd.optim on the MI355X against the float64 law of tests/optim_law.py (bounds and their reasons are stated there): the clip, the Adam steps under
both of the reference's hyper-parameter sets with its scheduler, bitwise properties, skipped gradients, state interchange with torch.optim.Adam, the absence
of host synchronisation, launch counts and one whole chain through generator and frozen encoder."""
import copy

import pytest
import torch

import optim_law as OL

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device_params():
    """the cases on the device; "view" is a leaf whose storage starts 4 bytes into an allocation"""
    params, _ = OL.inputs()
    out = []
    for (name, _), p in zip(OL.CASES, params):
        if name == "view":
            base = torch.zeros(p.numel() + 4, device=DEV)
            q = base[1:1 + p.numel()]
            q.copy_(p)
            q = q.detach().requires_grad_()
            assert q.data_ptr() % 16 == 4 and q.is_contiguous()
        else:
            q = p.to(DEV).requires_grad_()
        out.append(q)
    return out


def _set_grads(ps, k):
    """the gradients of step k + 1 as fresh device tensors (as after zero_grad()); the "view" case gets a 4-byte-aligned gradient on odd steps"""
    _, grads = OL.inputs()
    for (name, _), p, g in zip(OL.CASES, ps, grads[k]):
        if g is None:
            p.grad = None
        elif name == "view" and k % 2 == 1:
            base = torch.zeros(g.numel() + 4, device=DEV)
            base[1:1 + g.numel()].copy_(g)
            p.grad = base[1:1 + g.numel()]
            assert p.grad.data_ptr() % 16 == 4
        else:
            p.grad = g.to(DEV)


def _snapshot(ps, opts):
    state = {}
    for o in opts:
        state.update(o.state)
    st = [state.get(p, {}) for p in ps]
    return dict(p=[p.detach().cpu().clone() for p in ps], m=[s["exp_avg"].cpu().clone() if s else None for s in st],
                v=[s["exp_avg_sq"].cpu().clone() if s else None for s in st], t=[int(s["step"]) if s else 0 for s in st])


def _run(hyper, mode="inplace", per_tensor=False, steps=OL.STEPS, max_norm=OL.MAX_NORM):
    """the five steps with the scheduler.  mode: "inplace" (clip, then step), "deferred" (clip(defer=True), step(grad_scale=coef)) or None (no clip)"""
    from smirk_amd import Adam, clip_grad_norm_
    h = OL.HYPERS[hyper]
    ps = _device_params()
    groups = [[p] for p in ps] if per_tensor else [ps]
    opts = [Adam(g, lr=h["lr"], betas=h["betas"], eps=h["eps"]) for g in groups]
    scheds = [OL._schedule(o, h["lr"]) for o in opts]
    out = []
    for k in range(steps):
        _set_grads(ps, k)
        coef = norm = None
        if mode == "inplace":
            norm = clip_grad_norm_(ps, max_norm)
        elif mode == "deferred":
            norm, coef = clip_grad_norm_(ps, max_norm, defer=True)
        clipped = [None if p.grad is None else p.grad.cpu().clone() for p in ps]
        for o, s in zip(opts, scheds):
            o.step(grad_scale=coef)
            s.step()
        rec = _snapshot(ps, opts)
        rec.update(norm=None if norm is None else norm.cpu(), clipped=clipped)
        out.append(rec)
    return out


@pytest.fixture(scope="module")
def runs():
    """computed once and shared, left unchanged: the in-place run of each hyper-parameter set"""
    return {h: _run(h) for h in range(len(OL.HYPERS))}


def _same_bits(a, b):
    for ra, rb in zip(a, b):
        assert ra["t"] == rb["t"]
        for q in ("p", "m", "v"):
            for x, y in zip(ra[q], rb[q]):
                assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), q


def test_clip_norm_coef_and_scaled_gradients_follow_the_law():
    from smirk_amd import clip_grad_norm_
    ps = _device_params()
    _set_grads(ps, 1)                                                              # step 2: the 4-byte-aligned gradient view and the exact zeros
    before = [None if p.grad is None else p.grad.clone() for p in ps]
    norm64, coef64 = OL.clip_law([g.cpu() for g in before if g is not None], OL.MAX_NORM)
    norm, coef = clip_grad_norm_(ps, OL.MAX_NORM, defer=True)
    assert norm.dim() == 0 and norm.dtype == torch.float32 and norm.is_cuda and coef.shape == (1,) and coef.dtype == torch.float32
    assert all(g is None or torch.equal(p.grad, g) for p, g in zip(ps, before))    # deferred: the gradients in memory are not rewritten
    en, ec = abs(float(norm) - norm64) / norm64, abs(float(coef) - coef64) / coef64
    print(f"norm {float(norm):.9g} (float64 {norm64:.12g}): relative error {en:.2e}, {en / OL.NORM_REL:.3f} of the bound; coef {float(coef):.9g}: {ec:.2e}, "
          f"{ec / OL.COEF_REL:.3f} of the bound")
    assert en <= OL.NORM_REL and ec <= OL.COEF_REL
    norm2 = clip_grad_norm_(ps, OL.MAX_NORM)
    assert torch.equal(norm2, norm)
    worst = 0.0
    for p, g in zip(ps, before):
        if g is None or g.numel() == 0:
            continue
        want = g.cpu().double() * coef64
        ratio = float(((p.grad.cpu().double() - want).abs() / OL.ulp32(want)).max())
        worst = max(worst, ratio)
    print(f"clipped gradients: largest distance to g * coef64 {worst:.3f} ulp (bound {OL.CLIP_ULPS})")
    assert worst <= OL.CLIP_ULPS
    name, _, count = OL.ZEROS_IN_GRAD
    assert int((ps[OL.NAMES.index(name)].grad == 0).sum()) >= count


def test_gradients_that_need_no_clipping_stay_bit_identical():
    from smirk_amd import clip_grad_norm_
    ps = _device_params()
    _set_grads(ps, 0)
    before = [None if p.grad is None else p.grad.clone() for p in ps]
    norm, coef = clip_grad_norm_(ps, 1e3, defer=True)
    assert float(coef) == 1.0
    norm2 = clip_grad_norm_(ps, 1e3)
    assert torch.equal(norm, norm2) and all(g is None or torch.equal(p.grad, g) for p, g in zip(ps, before))
    single = torch.nn.Parameter(torch.zeros(3, device=DEV))
    single.grad = torch.tensor([3.0, 0.0, 4.0], device=DEV)
    assert float(clip_grad_norm_(single, 10.0)) == 5.0                             # a lone tensor, as torch accepts it
    single.grad = torch.tensor([float("nan"), 0.0, 4.0], device=DEV)
    n, c = clip_grad_norm_([single], 10.0, defer=True)
    assert torch.isnan(n) and torch.isnan(c)                                       # as torch.clamp: a NaN norm gives a NaN coefficient
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_([single], 10.0, error_if_nonfinite=True)


@pytest.mark.parametrize("hyper", range(len(OL.HYPERS)))
def test_adam_with_clip_and_scheduler_follows_the_law(runs, hyper):
    got, lw = runs[hyper], OL.law(hyper)
    OL.check_states(got, hyper, what="clip + Adam")
    for k, (g, l) in enumerate(zip(got, lw)):
        assert abs(float(g["norm"]) - l["norm"]) <= OL.NORM_REL * l["norm"], k
        for i, want in enumerate(l["clipped"]):
            if want is not None and want.numel():
                assert float(((g["clipped"][i].double() - want).abs() / OL.ulp32(want)).max()) <= OL.CLIP_ULPS, (k, OL.NAMES[i])


@pytest.mark.parametrize("hyper", range(len(OL.HYPERS)))
def test_adam_without_clip_follows_the_law(hyper):
    got = _run(hyper, mode=None)
    OL.check_states(got, hyper, max_norm=None, what="Adam")


def test_bitwise_two_runs_deferred_clip_and_one_call_per_tensor(runs):
    _same_bits(_run(0), runs[0])                                                   # two runs are identical
    _same_bits(_run(0, mode="deferred"), runs[0])                                  # the clip in registers = the clip in memory
    _same_bits(_run(1, mode="deferred", per_tensor=True), runs[1])                 # one launch per tensor = one multi-tensor launch


def test_skipped_gradient_semantics_equal_torch(runs):
    params, _ = OL.inputs()
    rf = OL.ref32(0)
    for g, r in zip(runs[0], rf):
        assert g["t"] == r["t"]
    never, skip3 = OL.NAMES.index("never"), OL.NAMES.index("skip3")
    last = runs[0][-1]
    assert last["t"][never] == 0 and last["m"][never] is None and last["v"][never] is None and rf[-1]["m"][never] is None
    assert torch.equal(last["p"][never], params[never])                            # never updated
    assert last["t"][skip3] == OL.STEPS - 1
    for q in ("p", "m", "v"):
        assert torch.equal(runs[0][2][q][skip3], runs[0][1][q][skip3])             # untouched by step 3


def _manual_steps(opt, ps, lrs, first, last):
    for k in range(first, last):
        _set_grads(ps, k)
        for group in opt.param_groups:
            group["lr"] = lrs[k]                                                   # base_trainer.py:39-66 sets it the same way
        opt.step()


@pytest.mark.parametrize("direction", ["ours_to_torch", "torch_to_ours"])
def test_state_interchange_with_torch_adam(direction):
    from smirk_amd import Adam
    h, lrs = OL.HYPERS[0], OL.learning_rates(OL.HYPERS[0]["lr"])
    kw = dict(lr=h["lr"], betas=h["betas"], eps=h["eps"])
    pa = _device_params()
    first = (Adam if direction == "ours_to_torch" else torch.optim.Adam)(pa, **kw)
    _manual_steps(first, pa, lrs, 0, 2)
    pb = [p.detach().clone().requires_grad_() for p in pa]                         # clones: the view case becomes 16-byte aligned, its restored state too
    second = (torch.optim.Adam if direction == "ours_to_torch" else Adam)(pb, **kw)
    second.load_state_dict(copy.deepcopy(first.state_dict()))                      # as after a save / load: torch hands the `step` tensors over by reference
    assert all(torch.equal(second.state[b]["exp_avg"], first.state[a]["exp_avg"]) for a, b in zip(pa, pb) if first.state.get(a))
    _manual_steps(first, pa, lrs, 2, 3)
    _manual_steps(second, pb, lrs, 2, 3)
    lw, rf = OL.law(0, None)[2:3], OL.ref32(0, None)[2:3]
    for what, ps, opt in (("first", pa, first), ("second", pb, second)):
        OL.check_states([_snapshot(ps, [opt])], 0, None, what=f"{direction} {what}", ref_record=rf, law_record=lw)


def test_no_host_synchronisation():
    """clip + both forms of the step under torch's sync debug mode, after one warm-up step (library load, plans, the pinned pool)"""
    from smirk_amd import Adam, clip_grad_norm_
    ps = _device_params()
    opt = Adam(ps, **OL.HYPERS[0])
    _set_grads(ps, 0)
    clip_grad_norm_(ps, OL.MAX_NORM); opt.step()
    grads = [[None if g is None else g.to(DEV) for g in row] for row in OL.inputs()[1][1:3]]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            for p, g in zip(ps, grads[0]):
                p.grad = g
            clip_grad_norm_(ps, OL.MAX_NORM); opt.step()
            for p, g in zip(ps, grads[1]):                                         # the set of tensors with a gradient changes: a re-plan
                p.grad = g
            _, coef = clip_grad_norm_(ps, OL.MAX_NORM, defer=True); opt.step(grad_scale=coef)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("this torch build does not honour torch.cuda.set_sync_debug_mode('error'): a probe .item() under it did not raise")
    assert opt.state[ps[0]]["step"] == 3


def test_launch_counts():
    from smirk_amd import Adam, _lib as L, clip_grad_norm_
    ps = _device_params()
    opt = Adam([dict(params=ps[:5]), dict(params=ps[5:], lr=1e-4)], **OL.HYPERS[0])
    _set_grads(ps, 0)
    clip_grad_norm_(ps, OL.MAX_NORM); opt.step()                                   # warm-up
    torch.cuda.synchronize()

    def launches(fn):
        L.profile_start()
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in L.profile_stop()]
    assert launches(lambda: clip_grad_norm_(ps, OL.MAX_NORM)) == ["optim_sumsq_partials", "optim_norm_finalise", "optim_scale"]
    assert launches(opt.step) == ["optim_adam"] * 2                                # one per group
    coef = []
    assert launches(lambda: coef.append(clip_grad_norm_(ps, OL.MAX_NORM, defer=True)[1])) == ["optim_sumsq_partials", "optim_norm_finalise"]
    assert launches(lambda: opt.step(grad_scale=coef[0])) == ["optim_adam"] * 2


def test_refusals_on_the_device():
    from smirk_amd import Adam, SmirkHipError, clip_grad_norm_
    def one(t, g):
        p = torch.nn.Parameter(t)
        p.grad = g
        return [p]
    with pytest.raises(SmirkHipError, match="fp32"):
        Adam(one(torch.zeros(4, device=DEV, dtype=torch.float64), torch.zeros(4, device=DEV, dtype=torch.float64))).step()
    with pytest.raises(SmirkHipError, match="contiguous"):
        Adam(one(torch.zeros(4, 4, device=DEV), torch.zeros(4, 4, device=DEV).t())).step()
    with pytest.raises(SmirkHipError, match="contiguous"):
        Adam(one(torch.zeros(4, 4, device=DEV).t(), torch.zeros(4, 4, device=DEV))).step()
    with pytest.raises(SmirkHipError, match="contiguous"):
        clip_grad_norm_(one(torch.zeros(4, 4, device=DEV), torch.zeros(4, 4, device=DEV).t()), 0.1)
    with pytest.raises(SmirkHipError, match="sparse"):
        Adam(one(torch.zeros(4, 4, device=DEV), torch.zeros(4, 4, device=DEV).to_sparse())).step()
    with pytest.raises(SmirkHipError, match="one-element"):
        Adam(one(torch.zeros(4, device=DEV), torch.zeros(4, device=DEV))).step(grad_scale=torch.ones(2, device=DEV))
    with pytest.raises(SmirkHipError, match="CPU"):
        Adam(one(torch.zeros(4, device=DEV), torch.zeros(4, device=DEV))).step(grad_scale=torch.ones(1))


def test_whole_chain_generator_through_frozen_encoder():
    """B = 2 at 64 x 64: generator in .train(), encoder frozen + .eval(); cycle_forward -> backward -> optimiser_stage (deferred clip + Adam) against the float64
    law on the same gradients, with torch.optim.Adam + torch.nn.utils.clip_grad_norm_ on cloned parameters (CPU, fp32) as the reference of the bound."""
    from oracle import generator_ref as G, make_cycle_golden as MC, mobilenet_ref as M
    from smirk_amd import Adam, SmirkEncoder, SmirkGenerator
    from smirk_amd.cycle import cycle_forward, optimiser_stage
    rendered, masked, feats = MC.inputs(2, 64)
    gen = SmirkGenerator(in_channels=6, out_channels=3, init_features=8, res_blocks=1)
    gen.load_state_dict(G.synth_state_dict(features=8, res_blocks=1)); gen = gen.cuda().train()
    enc = SmirkEncoder(); enc.load_state_dict(M.synth_encoder_state_dict(), strict=True); enc = enc.cuda().train()
    for n in ("pose_encoder", "shape_encoder", "expression_encoder"):
        m = getattr(enc, n)
        for p in m.parameters():
            p.requires_grad_(False)
        m.eval()
    h = OL.HYPERS[0]
    gen_opt = Adam(gen.parameters(), **h)
    enc_opt = Adam(enc.expression_encoder.parameters(), lr=0.25e-3)
    loss, _, _ = cycle_forward(gen, enc, rendered.cuda(), masked.cuda(), {k: v.cuda() for k, v in feats.items()}, freeze_generator=False)
    loss.backward()
    names, ps = zip(*gen.named_parameters())
    assert all(p.grad is not None for p in ps) and all(p.grad is None for p in enc.parameters())
    p0, g0 = [p.detach().cpu().clone() for p in ps], [p.grad.cpu().clone() for p in ps]
    norm = optimiser_stage(ps, enc_opt, gen_opt, max_norm=OL.MAX_NORM)               # the encoder's step: no gradient anywhere, nothing launched
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(ps, g0))               # deferred: gradients stay unscaled
    assert len(enc_opt.state) == 0
    # the reference on clones
    qs = [torch.nn.Parameter(p.clone()) for p in p0]
    for q, g in zip(qs, g0):
        q.grad = g.clone()
    ref_opt = torch.optim.Adam(qs, foreach=False, **h)
    ref_norm = torch.nn.utils.clip_grad_norm_(qs, OL.MAX_NORM, foreach=False)
    ref_opt.step()
    # the law
    norm64, coef64 = OL.clip_law(g0, OL.MAX_NORM)
    assert abs(float(norm) - norm64) <= OL.NORM_REL * norm64 and abs(float(ref_norm) - norm64) <= 1e-5 * norm64
    worst = (0.0, "")
    for name, p, q, pp, g in zip(names, ps, qs, p0, g0):
        z = torch.zeros_like(pp, dtype=torch.float64)
        lp, lm, lv = OL.adam_law(pp.double(), z, z, g.double() * coef64, 1, h["lr"], *h["betas"], h["eps"])
        for what, got, ref, law in (("p", p.detach(), q.detach(), lp), ("m", gen_opt.state[p]["exp_avg"], ref_opt.state[q]["exp_avg"], lm),
                                    ("v", gen_opt.state[p]["exp_avg_sq"], ref_opt.state[q]["exp_avg_sq"], lv)):
            err, bound = OL.distance(got, law), OL.state_bound(ref, law)
            worst = max(worst, (err / bound, f"{what}[{name}]"))
            assert err <= bound, f"{what}[{name}]: |HIP - law| {err:.3e} > bound {bound:.3e}"
        assert int(gen_opt.state[p]["step"]) == 1
    print(f"whole chain: norm {float(norm):.6g}, coef {coef64:.4g}; largest error / bound {worst[0]:.3f} at {worst[1]}")
