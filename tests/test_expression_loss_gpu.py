"""smirk_amd.expression_loss on the MI355X against float64 (tests/emotion_law.py for the module; the kernels' own formulas for the entries of
include/smirk_emotion.h).

Bounds.  A split16 value carries 22 significant bits and every fp32 operation rounds once, so the derived bounds have the project's form 2^-20 * sum |terms|,
plus n 2^-24 sum |terms| where one fp32 accumulator adds n terms (the form of the fully connected layer's bound in tests/test_mica_gpu.py):
  stem forward     (2^-20 + 160 * 2^-24) (sum |img w| + |shift|): both operands split (2 * 2^-22), the dropped lo x lo product (2^-22), the stored result
                   (2^-22), 160 accumulations
  stem gradient    (1024 + 4) 2^-24 sum |dz w| |gup inv_lift|: at most 16 taps x 64 channels in one fp32 FMA chain, the decoded inputs exact, three products
  average pool     (HW + 1) 2^-24 mean |v|
  max-pool, its backward and the adjoint helper are exact: copies, sums of at most four values chosen so that they are exact, one product and one sum rounded
  as fp32 torch rounds them
Where no bound can be derived (the loss of the head and its gradient; the whole module) the convention of tests/enc_tolerances.py holds: the distance to
float64 may be 4 times that of eager fp32 torch evaluating the same law on the same inputs, with a floor of 2^-20 max |ref| (emotion_law.bound_of); the
image gradient is held to the same in the Euclidean norm too (emotion_law.bound_l2_of says why).  Every
test prints its largest error / bound ratio before it asserts."""
import pytest
import torch
import torch.nn.functional as F

import emotion_law as EL

pytestmark = pytest.mark.gpu
E20, E24 = 2.0 ** -20, 2.0 ** -24
STEM_SHAPES = [(1, 7, 7), (2, 13, 18), (1, 224, 224)]


def _dev():
    return torch.device("cuda")


def to_split16(x):
    """fp32 [..., C] -> (split16 storage as a float32-typed tensor of the same shape, the float64 values it carries)"""
    hi = x.half()
    lo = ((x - hi.float()) * 2048.0).half()
    pair = torch.stack([hi.reshape(*x.shape[:-1], -1, 8), lo.reshape(*x.shape[:-1], -1, 8)], dim=-2).contiguous()
    return pair.view(torch.float32).reshape(x.shape), hi.double() + lo.double() / 2048.0


def from_split16(t):
    h = t.contiguous().view(torch.float16).reshape(*t.shape[:-1], -1, 2, 8).double()
    return (h[..., 0, :] + h[..., 1, :] / 2048.0).reshape(t.shape)


def _ratio(what, err, bound):
    ok = bound > 0
    r = float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0
    print(f"{what}: largest error / bound = {r:.3f}")
    assert bool((err[~ok] == 0).all()), what                                                             # where the bound is 0 the result is exact
    return r


def _peek_and_clear():
    from smirk_amd import _lib as L
    torch.cuda.synchronize()
    tripped = L.lib().smirk_range_flag_peek()
    L.lib().smirk_range_flag_clear()
    return bool(tripped)


def _stem_operands():
    """the stem of synth_checkpoint((1, 1, 1, 1), 1), folded here in float64 and rounded to fp32: (w' [64, 3, 7, 7], shift [64]) and the two images the entries read"""
    sd = EL.synth_checkpoint((1, 1, 1, 1), 1)["state_dict"]
    s = sd["backbone.bn1.weight"].double() / torch.sqrt(sd["backbone.bn1.running_var"].double() + 1e-5)
    shift = (sd["backbone.bn1.bias"].double() - sd["backbone.bn1.running_mean"].double() * s).float()
    w = (sd["backbone.conv1.weight"].double() * s.view(-1, 1, 1, 1)).float()
    fwd = torch.zeros(64, 160)
    fwd[:, :147] = w.permute(0, 2, 3, 1).reshape(64, 147)
    return w, shift, fwd, w.permute(2, 3, 1, 0).contiguous()


# ---- the entries -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", STEM_SHAPES)
def test_stem_forward(B, H, W):
    from smirk_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    w, shift, fwd, _ = _stem_operands()
    g = torch.Generator().manual_seed(H * W)
    gen, tar = (torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255.0 for _ in range(2))
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    out = torch.full((2 * B, Ho, Wo, 64), float("nan"), device=_dev())
    wd, sd, gd, td = fwd.to(_dev()), shift.to(_dev()), gen.to(_dev()), tar.to(_dev())
    L.check(lib.smirk_emotion_stem_split16(L.ptr(gd), L.ptr(td), L.ptr(wd), L.ptr(sd), L.ptr(out), B, H, W, st))
    img = torch.cat([gen, tar]).double()
    want = torch.relu(F.conv2d(img, w.double(), shift.double(), 2, 3)).permute(0, 2, 3, 1)
    terms = (F.conv2d(img.abs(), w.double().abs(), shift.double().abs(), 2, 3)).permute(0, 2, 3, 1)
    got = from_split16(out).cpu()
    assert tuple(want.shape) == (2 * B, Ho, Wo, 64) and torch.isfinite(got).all()
    assert _ratio(f"stem forward {B, H, W}", (got - want).abs(), (E20 + 160 * E24) * terms) <= 1.0
    assert not _peek_and_clear()
    bad = tar.clone()
    bad[B - 1, 2, H - 1, W // 2] = float("nan")                                                          # a NaN pixel from outside trips the flag
    bd = bad.to(_dev())
    L.check(lib.smirk_emotion_stem_split16(L.ptr(gd), L.ptr(bd), L.ptr(wd), L.ptr(sd), L.ptr(out), B, H, W, st))
    assert _peek_and_clear()


@pytest.mark.parametrize("B,H,W", STEM_SHAPES)
def test_stem_data_gradient(B, H, W):
    from smirk_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    w, _, _, wdg = _stem_operands()
    g = torch.Generator().manual_seed(H + W)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    dzs, dz64 = to_split16(torch.randn(B, Ho, Wo, 64, generator=g))
    gup, inv_lift = torch.randn(B, generator=g), 2.0 ** -10
    dzd, wd, gd = dzs.to(_dev()), wdg.to(_dev()), gup.to(_dev())
    runs = []
    for _ in range(2):
        dimg = torch.full((B, 3, H, W), float("nan"), device=_dev())
        L.check(lib.smirk_emotion_stem_dgrad_split16(L.ptr(dzd), L.ptr(wd), L.ptr(gd), inv_lift, L.ptr(dimg), B, H, W, st))
        runs.append(dimg)
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))                             # two runs agree bit for bit
    pad = ((H + 1) % 2, (W + 1) % 2)
    f = (gup.double() * inv_lift).view(B, 1, 1, 1)
    want = F.conv_transpose2d(dz64.permute(0, 3, 1, 2), w.double(), None, 2, 3, pad) * f
    terms = F.conv_transpose2d(dz64.permute(0, 3, 1, 2).abs(), w.double().abs(), None, 2, 3, pad) * f.abs()
    got = runs[0].double().cpu()
    assert tuple(want.shape) == (B, 3, H, W) and torch.isfinite(got).all()
    assert _ratio(f"stem data gradient {B, H, W}", (got - want).abs(), (1024 + 4) * E24 * terms) <= 1.0


@pytest.mark.parametrize("N,H,W,Cc", [(1, 3, 3, 8), (2, 14, 9, 64), (1, 112, 112, 64)])
def test_maxpool_forward_and_backward(N, H, W, Cc):
    """Values on a grid of 1/4 in [-1, 2]: every window has ties, most of them positive, so the first-maximum rule decides where the gradient goes; gradients on a
    grid of 1/64, so that the sums of up to four of them are exact.  The reference is ATen's CPU max_pool2d in float64 and autograd through it."""
    from smirk_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    g = torch.Generator().manual_seed(N + H)
    x = torch.randint(-4, 9, (N, H, W, Cc), generator=g).float() / 4.0
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    dy = torch.randint(-64, 65, (N, Ho, Wo, Cc), generator=g).float() / 64.0
    xs, x64 = to_split16(x)
    dys, dy64 = to_split16(dy)
    xd, dyd = xs.to(_dev()), dys.to(_dev())
    y = torch.full((N, Ho, Wo, Cc), float("nan"), device=_dev())
    L.check(lib.smirk_emotion_maxpool_split16(L.ptr(xd), L.ptr(y), N, H, W, Cc, st))
    xr = x64.permute(0, 3, 1, 2).clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    assert tuple(yr.shape) == (N, Cc, Ho, Wo)
    assert torch.equal(from_split16(y).cpu(), yr.detach().permute(0, 2, 3, 1))
    (dxr,) = torch.autograd.grad(yr, xr, dy64.permute(0, 3, 1, 2))
    dxr = dxr.permute(0, 2, 3, 1)
    windows = F.unfold(F.pad(x64.permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(N, Cc, 9, Ho * Wo)
    top = windows.max(dim=2, keepdim=True).values
    ties = int((((windows == top).sum(dim=2) > 1) & (top[:, :, 0] > 0)).sum())                           # windows whose positive maximum occurs more than once
    assert ties > 0
    for relu_mask in (0, 1):
        dx = torch.full((N, H, W, Cc), float("nan"), device=_dev())
        L.check(lib.smirk_emotion_maxpool_backward_split16(L.ptr(xd), L.ptr(dyd), L.ptr(dx), N, H, W, Cc, relu_mask, st))
        want = dxr * (x64 > 0) if relu_mask else dxr
        assert torch.equal(from_split16(dx).cpu(), want), relu_mask
    print(f"max-pool {N, H, W, Cc}: exact, forward and backward ({ties} windows with a tied positive maximum)")
    assert not _peek_and_clear()


@pytest.mark.parametrize("N,Hl,Wl,Cc,H,W", [(1, 1, 1, 8, 1, 1), (1, 1, 1, 8, 2, 2), (2, 7, 4, 64, 13, 8), (2, 7, 4, 64, 14, 7)])
def test_adjoint_helper(N, Hl, Wl, Cc, H, W):
    """all eight null combinations of s, y and add, compared exactly with the formula evaluated by fp32 torch and stored as split16"""
    from smirk_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    g = torch.Generator().manual_seed(H * 7 + W)
    dzs, dz64 = to_split16(torch.randn(N, Hl, Wl, Cc, generator=g))
    ys, y64 = to_split16(torch.relu(torch.randn(N, Hl, Wl, Cc, generator=g)))
    adds, add64 = to_split16(torch.randn(N, H, W, Cc, generator=g))
    s = torch.rand(Cc, generator=g) + 0.5
    s[Cc // 2] = -1.5
    dzd, yd, addd, sd = dzs.to(_dev()), ys.to(_dev()), adds.to(_dev()), s.to(_dev())
    for combo in range(8):
        use_s, use_y, use_add = combo & 1, combo & 2, combo & 4
        out = torch.full((N, H, W, Cc), float("nan"), device=_dev())
        L.check(lib.smirk_emotion_dilate2_split16(L.ptr(dzd), L.ptr(yd) if use_y else None, L.ptr(sd) if use_s else None, L.ptr(addd) if use_add else None,
                                                  L.ptr(out), N, Hl, Wl, H, W, Cc, st))
        v = dz64.float()                                                                               # the decoded values are fp32 numbers
        if use_s:
            v = v * s
        if use_y:
            v = torch.where(y64 > 0, v, torch.zeros_like(v))
        want = torch.zeros(N, H, W, Cc)
        want[:, ::2, ::2] = v
        if use_add:
            want = want + add64.float()
        assert torch.equal(from_split16(out).cpu(), to_split16(want)[1]), combo
    assert not _peek_and_clear()
    assert lib.smirk_emotion_dilate2_split16(L.ptr(dzd), None, None, None, L.ptr(out), N, Hl, Wl, H + 2, W, Cc, st) == L.SMIRK_ERR_BAD_ARG


@pytest.mark.parametrize("B,Cc", [(1, 16), (3, 16), (1, 2048), (3, 2048)])
@pytest.mark.parametrize("metric", EL.METRICS)
def test_head_forward_and_backward(B, Cc, metric):
    from smirk_amd import _lib as L
    from smirk_amd.expression_loss import lift_of
    lib, st = L.lib(), L.stream_ptr()
    HW = 49
    g = torch.Generator().manual_seed(B + Cc)
    pre = torch.randn(2 * B, HW, Cc, generator=g) + 0.25
    zero_row = metric == "cos" and B > 1                                                               # (with one sample the whole gradient would be zero)
    if zero_row:
        pre[2 * B - 1] = -1.0                                                                          # a zero feature row (the last sample's target) after the ReLU
    fs, f64 = to_split16(torch.relu(pre))
    fd = fs.to(_dev())
    code, lift = L.EMOTION_METRICS[metric], lift_of(metric, Cc, HW)

    def law(dtype):
        x = f64[:B].to(dtype).clone().requires_grad_(True)
        pooled = torch.cat([x, f64[B:].to(dtype)]).mean(dim=1)
        loss = EL.loss_law(pooled[:B], pooled[B:], metric, False)
        (grad,) = torch.autograd.grad(loss.sum(), x)
        return pooled.detach(), loss.detach(), grad * (f64[:B] > 0)

    p64, l64, g64 = law(torch.float64)
    p32, l32, g32 = law(torch.float32)
    for use_mean in (False, True):
        pooled, aux, loss = (torch.full(s, float("nan"), device=_dev()) for s in ((2 * B, Cc), (B, 4), (B,)))
        mean = torch.full((), float("nan"), device=_dev()) if use_mean else None
        L.check(lib.smirk_emotion_head_forward_split16(L.ptr(fd), L.ptr(pooled), L.ptr(aux), L.ptr(loss), L.ptr(mean, allow_none=True), B, HW, Cc, code, st))
        assert _ratio(f"pooled {B, Cc}", (pooled.double().cpu() - p64).abs(), (HW + 1) * E24 * f64.abs().mean(dim=1)) <= 1.0
        lb = max(4 * float((l32.double() - l64).abs().max()), E20 * float(l64.abs().max()))
        le = float((loss.double().cpu() - l64).abs().max())
        print(f"head {metric} B = {B}, C = {Cc}: loss error {le:.3g}, bound {lb:.3g}, error / bound = {le / lb:.3f}")
        assert torch.isfinite(loss).all() and le <= lb
        if use_mean:
            assert abs(float(mean) - float(l64.mean())) <= lb
    out = torch.full((B, HW, Cc), float("nan"), device=_dev())
    L.check(lib.smirk_emotion_head_backward_split16(L.ptr(fd[:B]), L.ptr(pooled), L.ptr(aux), L.ptr(out), B, HW, Cc, code, lift, st))
    got = from_split16(out).cpu() / lift
    gb = max(4 * float((g32.double() - g64).abs().max()), E20 * float(g64.abs().max()))
    ge = float((got - g64).abs().max())
    print(f"head {metric} B = {B}, C = {Cc}: seed error {ge:.3g}, bound {gb:.3g}, error / bound = {ge / gb:.3f}, max |seed| lifted {float(from_split16(out).abs().max()):.3g}")
    assert torch.isfinite(got).all() and ge <= gb
    assert torch.equal(got[f64[:B] == 0], torch.zeros_like(got[f64[:B] == 0]))                           # the last ReLU's mask
    if zero_row:
        assert torch.equal(got[B - 1], torch.zeros_like(got[B - 1])) and abs(float(loss[B - 1]) - 1.0) <= lb       # the zero target row: loss 1, no gradient
    if metric == "cos":
        zero_gen = fs.clone()
        zero_gen[0] = 0.0                                                                              # a zero gen row: the eps clamp, a finite loss of 1
        zd = zero_gen.to(_dev())
        L.check(lib.smirk_emotion_head_forward_split16(L.ptr(zd), L.ptr(pooled), L.ptr(aux), L.ptr(loss), None, B, HW, Cc, code, st))
        assert torch.isfinite(loss).all() and float(loss[0]) == 1.0
    assert not _peek_and_clear()


# ---- the whole module --------------------------------------------------------------------------------------------------------------------------------------
_modules = {}
IDS = [f"{sum(c[0])}blocks-{c[3]}x{c[4]}" for c in EL.NET_CASES]


def _module(layers, seed):
    from smirk_amd import ExpressionLoss
    if (layers, seed) not in _modules:
        _modules[(layers, seed)] = ExpressionLoss(EL.synth_checkpoint(layers, seed), layers=layers).to(_dev())
    return _modules[(layers, seed)]


@pytest.mark.parametrize("layers,seed,B,H,W", EL.NET_CASES, ids=IDS)
def test_whole_module(layers, seed, B, H, W):
    ref = EL.case_reference(layers, seed, B, H, W)
    m = _module(layers, seed)
    gen, tar = ref["gen"].to(_dev()).requires_grad_(True), ref["tar"].to(_dev())
    trace = {}
    loss = m(gen, tar, _trace=trace)
    loss.backward()
    got = {"features": trace["features"], "loss": loss.detach(), "grad": gen.grad}
    assert loss.shape == () and loss.dtype == torch.float32 and tuple(gen.grad.shape) == (B, 3, H, W)
    results = {}
    for name in ("features", "loss", "grad"):
        bound, e32 = EL.bound_of(ref, name)
        want = ref["f64"][name]
        err = float((got[name].double().cpu() - want).abs().max())
        results[name] = (err, bound)
        print(f"{sum(layers)} blocks {H} x {W}, {name}: error {err:.3g}, eager fp32 {e32:.3g}, max |ref| {float(want.abs().max()):.3g}, error / bound = {err / bound:.3f}")
    bound2, e32 = EL.bound_l2_of(ref, "grad")
    err2 = float((gen.grad.double().cpu() - ref["f64"]["grad"]).norm())
    results["grad, Euclidean"] = (err2, bound2)
    print(f"{sum(layers)} blocks {H} x {W}, grad in the Euclidean norm: error {err2:.3g}, eager fp32 {e32:.3g}, |ref| {float(ref['f64']['grad'].norm()):.3g}, error / bound = {err2 / bound2:.3f}")
    assert not _peek_and_clear()                                                                       # the range flag is clear after the run
    assert all(p.grad is None for p in m.parameters())
    for name, (err, bound) in results.items():
        assert err <= bound, name


SMALL = EL.NET_CASES[1]


def _small():
    layers, seed, B, H, W = SMALL
    ref = EL.case_reference(*SMALL)
    return _module(layers, seed), ref, ref["gen"].to(_dev()), ref["tar"].to(_dev())


def test_gradient_is_linear_in_the_upstream_gradient():
    """2^-12 times the loss: the same relative error as the unscaled gradient's bound; a per-sample upstream vector on use_mean=False, for 'l2' and 'cos'"""
    layers, seed, B, H, W = SMALL
    m, ref, gen, tar = _small()
    bound, _ = EL.bound_of(ref, "grad")
    x = gen.clone().requires_grad_(True)
    (m(x, tar) * 2.0 ** -12).backward()
    err = float((x.grad.double().cpu() * 2.0 ** 12 - ref["f64"]["grad"]).abs().max())
    print(f"upstream 2^-12: error / bound = {err / bound:.3f}")
    assert err <= bound
    up = torch.tensor([0.75, -2.5])[:B]
    for metric in ("l2", "cos"):
        f64 = EL.emotion_law(ref["ckpt"], ref["gen"], ref["tar"], layers, torch.float64, metric, False, up)
        f32 = EL.emotion_law(ref["ckpt"], ref["gen"], ref["tar"], layers, torch.float32, metric, False, up)
        x = gen.clone().requires_grad_(True)
        loss = m(x, tar, use_mean=False, metric=metric)
        (loss * up.to(_dev())).sum().backward()
        for name, got in (("loss", loss.detach()), ("grad", x.grad)):
            b = max(4 * float((f32[name].double() - f64[name]).abs().max()), E20 * float(f64[name].abs().max()))
            e = float((got.double().cpu() - f64[name]).abs().max())
            print(f"per-sample upstream, {metric}, {name}: error {e:.3g}, bound {b:.3g}, error / bound = {e / b:.3f}")
            assert tuple(got.shape) == tuple(f64[name].shape) and e <= b, (metric, name)
    assert not _peek_and_clear()


def test_second_backward_raises_and_no_grad_keeps_nothing():
    import smirk_amd
    m, ref, gen, tar = _small()
    x = gen.clone().requires_grad_(True)
    loss = m(x, tar)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    for requires in (False, True):                                                                     # under no_grad, or without a gradient to compute, nothing is kept
        x = gen.clone().requires_grad_(requires)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        if requires:
            with torch.no_grad():
                out = m(x, tar)
        else:
            out = m(x, tar)
        torch.cuda.synchronize()
        kept = torch.cuda.memory_allocated() - before                                                  # with the result alive: a tape would be tens of MB
        assert not out.requires_grad and out.grad_fn is None and kept <= 4096, kept
        del out
    with pytest.raises(smirk_amd.SmirkHipError, match="requires grad"):
        m(gen, tar.clone().requires_grad_(True))
    with pytest.raises(smirk_amd.SmirkHipError, match="193"):
        m(gen[:, :, :192], tar[:, :, :192])
    with pytest.raises(ValueError, match="Unknown metric"):
        m(gen, tar, metric="l3")


def test_second_call_does_not_wait_for_the_host():
    m, ref, gen, tar = _small()
    x = gen.clone().requires_grad_(True)
    first = m(x, tar)
    first.backward()
    g1 = x.grad.clone()
    x.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = m(x, tar)
        second.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first.detach().view(torch.int32), second.detach().view(torch.int32)) and torch.equal(g1.view(torch.int32), x.grad.view(torch.int32))


def test_weight_cache_follows_an_in_place_change():
    from smirk_amd import ExpressionLoss
    layers, seed, B, H, W = SMALL
    ckpt = EL.synth_checkpoint(layers, seed)
    _, ref, gen, tar = _small()
    m = ExpressionLoss(ckpt, layers=layers).to(_dev())

    def run(mod):
        x = gen.clone().requires_grad_(True)
        loss = mod(x, tar)
        loss.backward()
        return loss.detach().clone(), x.grad

    before = run(m)
    m.backbone.layer2[0].bn2.running_var.add_(0.5)
    after = run(m)
    changed = {"state_dict": dict(ckpt["state_dict"])}
    changed["state_dict"]["backbone.layer2.0.bn2.running_var"] = ckpt["state_dict"]["backbone.layer2.0.bn2.running_var"] + 0.5
    fresh = run(ExpressionLoss(changed, layers=layers).to(_dev()))
    assert not torch.equal(before[0], after[0])
    assert torch.equal(after[0].view(torch.int32), fresh[0].view(torch.int32)) and torch.equal(after[1].view(torch.int32), fresh[1].view(torch.int32))


@pytest.mark.parametrize("layers,seed", [((1, 1, 1, 1), 1), (EL.FULL, 2)], ids=["4blocks", "16blocks"])
def test_launch_count(layers, seed):
    from smirk_amd import _lib as L
    from smirk_amd.expression_loss import launches
    m = _module(layers, seed)
    gen, tar = EL.synth_images(1, 193, 224, 9).to(_dev()), EL.synth_images(1, 193, 224, 10).to(_dev())
    x = gen.clone().requires_grad_(True)
    m(x, tar).backward()                                                                                # packs the weights
    L.profile_start()
    loss = m(x, tar)
    forward = len(L.profile_stop())
    L.profile_start()
    loss.backward()
    recs = L.profile_stop()
    print(sorted({r[0] for r in recs}))
    assert (forward, len(recs)) == launches(layers)
    assert launches(EL.FULL) == (56, 105)


def test_emotion_term_of_the_first_path():
    """smirk_trainer.py:108-119 over the real small generator: the gradient reaches rendered_img, the generator's parameters get none and are trainable again
    afterwards, its mode is restored, and the value is the module's own on the eval-mode reconstruction"""
    from oracle import generator_ref as G
    from smirk_amd import SmirkGenerator, first_path
    m = _module((1, 1, 1, 1), 1)
    gen = SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=5)
    gen.load_state_dict(G.synth_state_dict(), strict=True)
    gen = gen.cuda().train()
    g = torch.Generator().manual_seed(11)
    rendered = torch.rand(2, 3, 224, 224, generator=g).to(_dev()).requires_grad_(True)
    masked, img = torch.rand(2, 3, 224, 224, generator=g).to(_dev()), EL.synth_images(2, 224, 224, 12).to(_dev())
    for mode in (True, False):
        gen.train(mode)
        rendered.grad = None
        value = first_path.emotion_term(gen, m, rendered, masked, img)
        assert gen.training == mode and all(p.requires_grad for p in gen.parameters())
        value.backward()
        assert value.shape == () and rendered.grad is not None and torch.isfinite(rendered.grad).all() and float(rendered.grad.abs().max()) > 0
        assert all(p.grad is None for p in gen.parameters()) and all(p.grad is None for p in m.parameters())
    for p in gen.parameters():                                                                         # the same steps by hand, then the module itself
        p.requires_grad_(False)
    gen.eval()
    reconstructed = gen(torch.cat([rendered, masked], dim=1))
    for p in gen.parameters():
        p.requires_grad_(True)
    direct = m(reconstructed, img, metric="l2", use_mean=False).mean().detach()
    assert torch.equal(direct.view(torch.int32), value.detach().view(torch.int32))
    assert not _peek_and_clear()
