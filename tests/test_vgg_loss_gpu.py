"""smirk_amd.VGGPerceptualLoss on the MI355X against the float64 law of tests/vgg_law.py evaluated on the device.

The kernels around the convolutions (csrc/vgg_loss.hip) are tested on crafted operands whose decisions are exact by construction.  The whole module is tested
with its decisions FORCED: a plain float64 gradient differs from any fp32-class evaluation by flipped ReLU / sign decisions (6-9e-4 in relative L2 at 224 x 224
for eager fp32 itself), so the gradient is compared with the float64 law evaluated under the module's own trace, and the yardstick is what eager fp32 achieves
under ITS own trace.  Bounds: 4 x eager fp32's distance (f16x3 dot products have fp32-GEMM error; the 4 covers the accumulation order) with the
project's floor of 1e-6; 2^-21 for an fp32 value stored as a split16 pair (22 significand bits, one more rounding upstream).
Largest ratios to the bounds seen on one MI355X: DESIGN §16."""
import ctypes as C
import os

import pytest
import torch

from loss_law import WEIGHTS_TRAIN, synth_first_path_inputs
from vgg_law import STD, MEAN, grad_of, synth_images, synth_weights, vgg_forced_law, vgg_law

pytestmark = pytest.mark.gpu
REL_SPLIT = 2.0 ** -21
FLOOR = 1e-6


def _lib():
    from smirk_amd import _lib as L
    return L, L.lib(), L.stream_ptr()


def _to_split16(v):
    """fp32 [..., C] (C % 8 == 0) -> a split16 tensor of the same shape (float32-typed storage); host-side restatement of the format"""
    g = v.reshape(-1, 8)
    hi = g.half()
    lo = ((g - hi.float()) * 2048.0).half()
    return torch.stack([hi, lo], 1).contiguous().view(torch.float32).reshape(v.shape)


def _from_split16(t):
    h = t.contiguous().view(torch.float16).reshape(-1, 2, 8).float()
    return (h[:, 0] + h[:, 1] / 2048.0).reshape(t.shape)


def _representable(v):
    """rounds fp32 values to ones the split16 format carries exactly"""
    return _from_split16(_to_split16(v))


# ---- the kernels on crafted operands ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,prefill", [((1, 16, 16), False), ((2, 24, 40), False), ((3, 16, 8), True)])
def test_prepare_and_its_backward(shape, prefill):
    L, lib, st = _lib()
    B, H, W = shape
    x, y = synth_images(B, H, W, seed=5, device="cuda")
    mean, std = torch.tensor(MEAN, device="cuda"), torch.tensor(STD, device="cuda")
    out = torch.full((2 * B, H, W, 8), float("nan") if prefill else 0.0, device="cuda")
    L.check(lib.smirk_vgg_prepare_split16(L.ptr(x), L.ptr(y), L.ptr(mean), L.ptr(std), L.ptr(out), B, H, W, st))
    got = _from_split16(out).double()
    ref = (torch.cat([x, y]).double() * 0.5 + 0.5 - mean.double().view(1, 3, 1, 1)) / std.double().view(1, 3, 1, 1)
    assert torch.equal(got[..., 3:], torch.zeros_like(got[..., 3:]))                                      # the padded channels, exactly
    assert float((got[..., :3] - ref.permute(0, 2, 3, 1)).abs().max()) <= REL_SPLIT * float(ref.abs().max())
    d = _representable(torch.randn(B, H, W, 8, device="cuda"))
    dx = torch.full((B, 3, H, W), float("nan") if prefill else 0.0, device="cuda")
    sd = _to_split16(d)
    L.check(lib.smirk_vgg_prepare_backward_split16(L.ptr(sd), L.ptr(std), L.ptr(dx), B, H, W, 0.25, st))
    ref = d[..., :3].double().permute(0, 3, 1, 2) * 0.5 * 0.25 / std.double().view(1, 3, 1, 1)
    assert float((dx.double() - ref).abs().max()) <= REL_SPLIT * float(ref.abs().max())


def test_prepare_trips_the_range_flag():
    import smirk_amd
    L, lib, st = _lib()
    x, y = synth_images(1, 16, 16, seed=6, device="cuda")
    x[0, 1, 3, 5] = 1e6
    mean, std = torch.tensor(MEAN, device="cuda"), torch.tensor(STD, device="cuda")
    out = torch.empty(2, 16, 16, 8, device="cuda")
    L.check(lib.smirk_vgg_prepare_split16(L.ptr(x), L.ptr(y), L.ptr(mean), L.ptr(std), L.ptr(out), 1, 16, 16, st))
    with pytest.raises(smirk_amd.SmirkHipError, match="range"):
        smirk_amd.check_numerics()
    torch.cuda.synchronize()
    lib.smirk_range_flag_clear()
    assert lib.smirk_range_flag_peek() == 0


@pytest.mark.parametrize("C_", [64, 512])
@pytest.mark.parametrize("groups", [4095, 4096, 4097])
def test_feature_l1(C_, groups):
    """halves of `groups` 8-channel groups around the chunk edge; value within 5e-7 relative of the float64 sum of the decoded operands (one rounding of the fp32
    term, 6e-8, on a float64 accumulation: the bound DESIGN §14 derives); two calls return the same bits"""
    L, lib, st = _lib()
    half_groups, n = groups, groups * 8
    f = _to_split16(torch.randn(2, n, device="cuda") * 3)
    half = (C.c_longlong * 1)(n)
    ws = torch.empty(lib.smirk_vgg_l1_workspace_bytes(half, 1), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= 8 * -(-half_groups // L.VGG_L1_CHUNK)
    res = []
    for _ in range(2):
        ws.fill_(0xFF)
        terms, total = torch.empty(1, device="cuda"), torch.empty((), device="cuda")
        L.check(lib.smirk_vgg_l1_partials_split16(L.ptr(f), C_, 0, half, 1, C.c_void_p(ws.data_ptr()), ws.numel(), st))
        L.check(lib.smirk_vgg_l1_finalise(half, 1, C.c_void_p(ws.data_ptr()), ws.numel(), L.ptr(terms), L.ptr(total), st))
        res.append((terms.clone(), total.clone()))
    v = _from_split16(f).double()
    ref = float((v[0] - v[1]).abs().sum()) / n
    assert abs(float(res[0][0][0]) - ref) <= 5e-7 * ref and abs(float(res[0][1]) - ref) <= 5e-7 * ref
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_feature_l1_four_taps_and_their_total():
    L, lib, st = _lib()
    shapes = [(2, 70, 64), (2, 33, 128), (2, 4096 * 8 // 256 + 1, 256), (2, 5, 512)]
    fs = [_to_split16(torch.randn(2 * b, m, c, device="cuda")) for b, m, c in shapes]
    half = (C.c_longlong * 4)(*[f.numel() // 2 for f in fs])
    ws = torch.empty(lib.smirk_vgg_l1_workspace_bytes(half, 4), dtype=torch.uint8, device="cuda")
    terms, total = torch.empty(4, device="cuda"), torch.empty((), device="cuda")
    for k in (2, 0, 3, 1):                                                                                # the layout depends on the shapes, not on the call order
        L.check(lib.smirk_vgg_l1_partials_split16(L.ptr(fs[k]), shapes[k][2], k, half, 4, C.c_void_p(ws.data_ptr()), ws.numel(), st))
    L.check(lib.smirk_vgg_l1_finalise(half, 4, C.c_void_p(ws.data_ptr()), ws.numel(), L.ptr(terms), L.ptr(total), st))
    ref = []
    for f, (b, _, _) in zip(fs, shapes):
        v = _from_split16(f).double()
        ref.append(float((v[:b] - v[b:]).abs().mean()))
    for k in range(4):
        assert abs(float(terms[k]) - ref[k]) <= 5e-7 * ref[k], k
    assert abs(float(total) - sum(ref)) <= 5e-7 * sum(ref)


@pytest.mark.parametrize("mode,scale", [("tap", 1.0), ("tap", 65536.0), ("tap_deepest", 1.0), ("plain", 1.0)])
def test_relu_tap_backward(mode, scale):
    """fx is 0 or >= 1e-3 and fx - fy is 0 or >= 1e-3 in magnitude, so the mask and the sign are the same in any arithmetic; 33 x 35 pixels x 64 channels are
    several workgroups and not a whole number of them"""
    L, lib, st = _lib()
    g_ = torch.Generator().manual_seed(9)
    shape = (1, 33, 35, 64)
    r = lambda: torch.rand(shape, generator=g_).cuda()
    fx = _representable(torch.where(r() < 0.4, torch.zeros(shape, device="cuda"), 1e-3 + 3 * r()))
    delta = torch.where(r() < 0.5, 1e-3 + r(), -(1e-3 + r()))
    tie = r() < 0.1                                                                                        # planted ties: fy = fx exactly
    fy = torch.where(tie, fx, _representable((fx + delta).clamp_min(0)))
    ok = ((fx - fy).abs() >= 1e-3 - 1e-6) | (fx == fy)
    fy = torch.where(ok, fy, fx)                                                                           # (clamping at 0 may have produced a small difference)
    tie = fx == fy
    d_in = _representable(torch.randn(shape, generator=g_).cuda())
    g = torch.tensor(1.7, device="cuda")
    dz = torch.full(shape, float("nan"), device="cuda")
    n = fx.numel()
    P = L.ptr
    sx, sy, sd = _to_split16(fx), _to_split16(fy), _to_split16(d_in)                                      # (kept alive: the entry takes raw pointers)
    L.check(lib.smirk_vgg_relu_tap_backward_split16(P(sx), P(sy) if mode != "plain" else None, P(sd) if mode != "tap_deepest" else None, P(g), P(dz), n, 64, scale, st))
    got = _from_split16(dz)
    mask = (fx > 0).float()
    din = d_in if mode != "tap_deepest" else torch.zeros_like(d_in)
    gc = g * torch.tensor(scale / n, dtype=torch.float64).float().cuda()                                  # fp32: g * fl(scale / numel)
    ref = (din + (gc * torch.sign(fx - fy) if mode != "plain" else 0.0)) * mask
    assert float((got - ref).abs().max()) <= REL_SPLIT * float(ref.abs().max())
    assert torch.equal(got[fx == 0], torch.zeros_like(got[fx == 0])) and bool((fx == 0).any())
    if mode == "tap":
        assert bool(tie.any()) and torch.equal(got[tie], (d_in * mask)[tie])                              # sign(0) = 0: exactly d_in * mask


# ---- the whole module -------------------------------------------------------------------------------------------------------------------------------------------
CASES = {"1x16x16": ((1, 16, 16), None), "2x24x40": ((2, 24, 40), None), "3x16x32": ((3, 16, 32), None), "1x64x64": ((1, 64, 64), None),
         "1x224x224": ((1, 224, 224), (224, 224)), "resize 2x112x96": ((2, 112, 96), (224, 224))}
_cache = {}


def _module(resize_to, seed=1):
    from smirk_amd import VGGPerceptualLoss
    key = ("module", resize_to, seed)
    if key not in _cache:
        _cache[key] = VGGPerceptualLoss(synth_weights(seed), resize_to=resize_to).cuda()
    return _cache[key]


def _case(name):
    """one evaluation of everything a case's checks need: the module (value, terms, gradient, trace), the float64 law, eager fp32, and the float64 forced law
    under the module's and under eager fp32's trace; computed once and left unchanged"""
    if name in _cache:
        return _cache[name]
    (B, H, W), resize_to = CASES[name]
    w = synth_weights(1, device="cuda")
    x, y = synth_images(B, H, W, seed=B * 1000 + H, device="cuda")
    mod = _module(resize_to)
    c = dict(x=x, y=y, w=w, resize_to=resize_to, mod=mod)
    xm = x.clone().requires_grad_(True)
    c["trace"] = {}
    loss = mod(xm, y, _trace=c["trace"])
    loss.backward()
    c["loss"], c["dx"], c["terms"] = loss.detach(), xm.grad, c["trace"]["terms"]
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        tr, terms = {}, []

        def law(t):
            total, ts = vgg_law(t, y, w, resize_to, tr)
            terms[:] = [v.detach() for v in ts]
            return total
        c["v" + tag], c["g" + tag] = grad_of(law, x.to(dt))
        c["t" + tag], c["tr" + tag] = list(terms), tr
    dbl = lambda tr: {k: [t.double() for t in v] for k, v in tr.items() if k in ("relu_x", "tap_y")}
    c["forced_mod"] = grad_of(lambda t: vgg_forced_law(t, w, dbl(c["trace"]), resize_to), x.double())[1]
    c["forced_32"] = grad_of(lambda t: vgg_forced_law(t, w, dbl(c["tr32"]), resize_to), x.double())[1]
    torch.cuda.synchronize()
    _cache[name] = c
    return c


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / float(b.double().abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_trace_follows_the_float64_law(name):
    """(1) every ReLU output of the x rows and every tap feature of the y rows"""
    c = _case(name)
    worst = 0.0
    for key in ("relu_x", "tap_y"):
        assert len(c["trace"][key]) == len(c["tr64"][key]) == (10 if key == "relu_x" else 4)
        for k, (mine, a64, a32) in enumerate(zip(c["trace"][key], c["tr64"][key], c["tr32"][key])):
            assert mine.dtype == torch.float32 and tuple(mine.shape) == tuple(a64.shape)
            bound = max(4 * _rel(a32, a64), FLOOR)
            worst = max(worst, _rel(mine, a64) / bound)
            assert _rel(mine, a64) <= bound, (key, k, _rel(mine, a64), bound)
    print(f"[vgg ratio] trace {name}: {worst:.3f}")


@pytest.mark.parametrize("name", list(CASES))
def test_value_follows_the_float64_law(name):
    """(2) the four terms and the total; continuous in the decisions"""
    c = _case(name)
    worst = 0.0
    for mine, v64, v32 in zip(list(c["terms"]) + [c["loss"]], c["t64"] + [c["v64"]], c["t32"] + [c["v32"]]):
        bound = max(4 * abs(float(v32) - float(v64)), FLOOR * abs(float(v64)))
        worst = max(worst, abs(float(mine) - float(v64)) / bound)
        assert abs(float(mine) - float(v64)) <= bound, (float(mine), float(v64), bound)
    print(f"[vgg ratio] value {name}: {worst:.3f}")


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_is_the_adjoint_of_the_modules_own_decisions(name):
    """(3) against the float64 forced law under the module's trace; the yardstick is eager fp32 against the forced law under eager fp32's trace.
    (4) the unforced cap: relative L2 distance from the plain float64 gradient at most 0.05 (eager fp32: 3e-7 .. 9e-4; a dropped tap: 0.18 .. 0.54)"""
    c = _case(name)
    g32 = _rel(c["g32"], c["forced_32"])
    bound = max(4 * g32, FLOOR)
    mine = _rel(c["dx"], c["forced_mod"])
    l2 = float((c["dx"].double() - c["g64"]).norm() / c["g64"].norm())
    print(f"[vgg ratio] gradient {name}: {mine / bound:.3f} (module {mine:.2e}, eager fp32 {g32:.2e}); unforced relative L2 {l2:.2e}")
    assert c["dx"].dtype == torch.float32 and tuple(c["dx"].shape) == tuple(c["x"].shape)
    assert mine <= bound, (mine, bound)
    assert l2 <= 0.05, l2


@pytest.mark.parametrize("name", ["2x24x40", "1x224x224"])
def test_upstream_gradient_scales_the_result(name):
    """(5) every backward kernel is linear in the upstream gradient g; the fp32 roundings of g * coef and of each split16 store (2^-22 relative) move the
    result by less than 1e-6 of max|g|"""
    c = _case(name)
    x = c["x"].clone().requires_grad_(True)
    (3 * c["mod"](x, c["y"])).backward()
    assert _rel(x.grad, 3 * c["dx"]) <= FLOOR


def test_no_grad_keeps_no_tape():
    """(6)"""
    c = _case("1x64x64")
    with torch.no_grad():
        c["mod"](c["x"], c["y"])                                                                          # (the workspace and the packed weights exist now)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        loss = c["mod"](c["x"].clone().requires_grad_(True), c["y"])
    assert not loss.requires_grad and loss.grad_fn is None
    loss2 = c["mod"](c["x"], c["y"])                                                                      # grad mode on, nothing requires grad
    assert not loss2.requires_grad and loss2.grad_fn is None
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - before <= 4096                                                 # two scalars (and their terms), no activations
    assert torch.equal(loss, c["loss"]) and torch.equal(loss2, c["loss"])


def test_refusals():
    """(7) and the shapes the network cannot take"""
    import smirk_amd
    c = _case("1x16x16")
    mod, x, y = c["mod"], c["x"], c["y"]
    with pytest.raises(smirk_amd.SmirkHipError, match="requires grad"):
        mod(x, y.clone().requires_grad_(True))
    xg = x.clone().requires_grad_(True)
    loss = mod(xg, y)
    loss.backward()
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    with pytest.raises(smirk_amd.SmirkHipError, match="CPU"):
        mod(x.cpu(), y)
    for h, w in ((20, 16), (16, 12), (8, 16)):
        with pytest.raises(smirk_amd.SmirkHipError, match="multiples of 8"):
            mod(torch.zeros(1, 3, h, w, device="cuda"), torch.zeros(1, 3, h, w, device="cuda"))
    with pytest.raises(smirk_amd.SmirkHipError, match="2 GiB"):                                           # refused on the host: nothing of that size is allocated
        mod(torch.zeros(1, 3, 1, 1, device="cuda").expand(86, 3, 224, 224), torch.zeros(1, 3, 1, 1, device="cuda").expand(86, 3, 224, 224))


@pytest.mark.parametrize("name", ["3x16x32", "1x224x224"])
def test_two_runs_are_bitwise_equal(name):
    """(8)"""
    c = _case(name)
    x = c["x"].clone().requires_grad_(True)
    loss = c["mod"](x, c["y"])
    loss.backward()
    assert torch.equal(loss.detach(), c["loss"]) and torch.equal(x.grad, c["dx"])


def test_batch_64_at_224():
    """The workload's size (the largest activation is 1.53 GiB, group indices pass 2^24): 32 copies of the two images of the 224 x 224 case.  Every term is the
    mean over identical copies, and every image's gradient is that of the small case divided by 32 (a power of two: only the kernels' choice of tile and
    accumulation order for the larger batch can move it), both within the project's floor."""
    c = _case("1x224x224")
    x = c["x"].repeat(64, 1, 1, 1).requires_grad_(True)
    loss = c["mod"](x, c["y"].repeat(64, 1, 1, 1))
    loss.backward()
    assert abs(float(loss.detach()) - float(c["loss"])) <= FLOOR * float(c["loss"])
    g = x.grad * 64
    assert all(_rel(g[i:i + 1], c["dx"]) <= FLOOR for i in (0, 31, 63))
    assert torch.equal(g[0], g[63]) or _rel(g[0:1], g[63:64]) <= FLOOR


def test_no_host_synchronisation():
    """(9) forward and backward under torch's synchronisation debug mode"""
    c = _case("2x24x40")
    x = c["x"].clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = c["mod"](x, c["y"])
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(x.grad, c["dx"])


def test_a_weight_changed_in_place_is_packed_again():
    """(10) the operand images follow the weights' version counters"""
    from smirk_amd import VGGPerceptualLoss
    c = _case("1x16x16")
    mod = VGGPerceptualLoss(synth_weights(1), resize_to=None).cuda()
    a = mod(c["x"], c["y"])
    assert torch.equal(a, c["loss"])
    packed = [f.data_ptr() for f in mod._packed[1][0]]                                                    # the ten forward images of the frame's (key, (wf, wd, bias))
    assert torch.equal(mod(c["x"], c["y"]), a) and packed == [f.data_ptr() for f in mod._packed[1][0]]      # unchanged weights: packed once
    with torch.no_grad():
        mod.convs()[9].weight.mul_(2.0)
    b = mod(c["x"], c["y"])
    w = [(wt * (2.0 if k == 9 else 1.0), bs) for k, (wt, bs) in enumerate(c["w"])]
    ref = vgg_law(c["x"].double(), c["y"], w)[0]
    assert not torch.equal(a, b) and abs(float(b) - float(ref)) <= 1e-5 * float(ref)


# ---- inside the first path ---------------------------------------------------------------------------------------------------------------------------------------
def test_first_path_takes_the_module_as_its_perceptual_term(sandbox):
    """B = 2, 224 x 224, synthetic weights, the weights of configs/config_train.yaml: the logged term is the module's value, and its weight moves the
    generator's gradient"""
    from oracle import assets as A
    from oracle import generator_ref as G
    from oracle import mobilenet_ref as M
    from smirk_amd import FLAME, FirstPathLoss, Renderer, SmirkEncoder, SmirkGenerator, masking
    from smirk_amd.first_path import first_path
    cwd = os.getcwd(); os.chdir(sandbox)
    try:
        fl, rn = FLAME().cuda(), Renderer().cuda()
        prob = masking.load_probabilities_per_FLAME_triangle()
    finally:
        os.chdir(cwd)
    enc = SmirkEncoder(); enc.load_state_dict(M.synth_encoder_state_dict()); enc = enc.cuda().train()
    gen = SmirkGenerator(6, 3, 32, 5); gen.load_state_dict(G.synth_state_dict()); gen = gen.cuda().train()
    B = 2
    batch = synth_first_path_inputs(B, seed=31, device="cuda")[3]
    batch["img"] = A.synth_images(B, seed=81).cuda()
    yy, xx = torch.meshgrid(torch.arange(224.0), torch.arange(224.0), indexing="ij")
    batch["mask"] = (((yy - 112) ** 2 + (xx - 112) ** 2) > 80 ** 2).float()[None, None].repeat(B, 1, 1, 1).cuda()
    vgg = _module((224, 224))
    seen = {}

    def extra(out):
        seen["value"] = vgg(out["reconstructed_img"], batch["img"])
        return {"perceptual_vgg_loss": seen["value"]}

    grads = {}
    for tag, weights in (("on", WEIGHTS_TRAIN), ("off", dict(WEIGHTS_TRAIN, perceptual_vgg_loss=0))):
        loss, terms, out = first_path(enc, fl, rn, gen, FirstPathLoss(weights), batch, prob, extra=extra, _rng_stream=masking.PhiloxStream(7))
        loss.backward()
        assert terms.as_dict()["perceptual_vgg_loss"] == float(seen["value"]) > 0
        grads[tag] = [p.grad.clone() for p in gen.parameters()]
        for p in list(gen.parameters()) + list(enc.parameters()):
            p.grad = None
    assert all(torch.isfinite(g).all() for g in grads["on"])
    moved = [float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) for a, b in zip(grads["on"], grads["off"])]
    assert max(moved) > 1e-2, max(moved)
