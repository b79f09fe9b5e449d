"""smirk_amd.mica on the MI355X against float64 (tests/mica_law.py for the network; the kernels' own formulas for the entries of include/smirk_mica.h).

Bounds.  A split16 value carries 22 significant bits and every fp32 operation rounds once, so the derived bounds have the form 2^-20 * sum |terms| (the style of
tests/enc_eval_law.py):
  prepare        2^-20 |v|, the pad channels exactly 0
  affine/PReLU   2^-20 (|x s| + |t|) max(1, |a|)
  fc             (K 2^-24 + 2^-20) sum_k |x w| + 2^-24 |bias| per element: K fp32 additions in any order, the decoded inputs exact
Where no bound can be derived (the head's normalisation and five layers; the whole network) the convention of tests/enc_tolerances.py holds: the distance to
float64 may be 4 times that of eager fp32 torch evaluating the same law on the same inputs (4, not 2: one box's sample maximum made the suite flaky at 2), with
a floor of 1e-6 max |ref| for the head and 2e-6 max |ref| for the network.  Every test prints its largest error / bound ratio before it asserts."""
import ctypes as C

import pytest
import torch

import mica_law as ML

pytestmark = pytest.mark.gpu
E20, E24 = 2.0 ** -20, 2.0 ** -24


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
    r = float((err / bound).max())
    print(f"{what}: largest error / bound = {r:.3f}")
    return r


def _peek_and_clear():
    from smirk_amd import _lib as L
    torch.cuda.synchronize()
    tripped = L.lib().smirk_range_flag_peek()
    L.lib().smirk_range_flag_clear()
    return bool(tripped)


# ---- the entries -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 3, 5), (1, 112, 112)])
def test_prepare(B, H, W):
    from smirk_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    # 8-bit pixels, as the data loader delivers them: |v| = |2 k / 255 - 1| >= 1 / 255, inside the range where the format keeps its 22 bits
    img = torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(H)).float() / 255.0
    out = torch.full((B, H, W, 8), float("nan"), device=_dev())
    L.check(lib.smirk_mica_prepare_split16(L.ptr(img.to(_dev())), L.ptr(out), B, H, W, st))
    got = from_split16(out).cpu()
    want = ((img.double() - 0.5) / 0.5)[:, [2, 1, 0]].permute(0, 2, 3, 1)
    assert torch.equal(got[..., 3:], torch.zeros_like(got[..., 3:]))
    assert _ratio("prepare", (got[..., :3] - want).abs(), E20 * want.abs()) <= 1.0
    assert not _peek_and_clear()
    bad = img.clone()
    bad[B - 1, 1, H - 1, W // 2] = float("nan")                                                         # a NaN from outside trips the flag
    L.check(lib.smirk_mica_prepare_split16(L.ptr(bad.to(_dev())), L.ptr(out), B, H, W, st))
    assert _peek_and_clear()


@pytest.mark.parametrize("M,Cc", [(1, 8), (255, 8), (257, 72), (49, 512)])
def test_affine_prelu(M, Cc):
    from smirk_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    g = torch.Generator().manual_seed(M + Cc)
    x = torch.randn(M, Cc, generator=g) * 3
    x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.05), x)                                        # nothing in fp16's subnormal range except the planted zeros
    x[0, 0], x[M // 2, Cc // 2], x[M - 1, Cc - 1] = 0.0, 0.0, -2.5                                       # planted exact zeros and a negative
    xs, x64 = to_split16(x)
    scale, shift = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    scale[Cc // 3] = -1.25
    slope = torch.rand(Cc, generator=g) * 0.75 - 0.25
    slope[0], slope[1], slope[Cc - 1] = 0.0, 1.0, -0.5                                                   # slopes 0, 1 and negative
    xs_d = xs.to(_dev())
    worst = 0.0
    for mask in range(8):
        s, t, a = (v if mask >> k & 1 else None for k, v in enumerate((scale, shift, slope)))
        sd, td, ad = (None if v is None else v.to(_dev()) for v in (s, t, a))
        out = torch.full((M, Cc), float("nan"), device=_dev())
        L.check(lib.smirk_mica_affine_prelu_split16(L.ptr(xs_d), L.ptr(sd, allow_none=True), L.ptr(td, allow_none=True), L.ptr(ad, allow_none=True), L.ptr(out), M, Cc, st))
        s64 = torch.ones(Cc, dtype=torch.float64) if s is None else s.double()
        t64 = torch.zeros(Cc, dtype=torch.float64) if t is None else t.double()
        a64 = torch.ones(Cc, dtype=torch.float64) if a is None else a.double()
        z = x64 * s64 + t64
        want = torch.where(z > 0, z, a64 * z)
        bound = E20 * ((x64 * s64).abs() + t64.abs()) * a64.abs().clamp_min(1.0)
        err = (from_split16(out).cpu() - want).abs()
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0)
        assert bool((err <= bound).all()), mask                                                        # where the bound is 0 (a planted zero) the result is exact
        if s is None and t is None:
            assert torch.equal(from_split16(out).cpu()[x64 == 0], torch.zeros_like(x64[x64 == 0])), mask          # exact zeros stay exact zeros
        inplace = xs_d.clone()
        L.check(lib.smirk_mica_affine_prelu_split16(L.ptr(inplace), L.ptr(sd, allow_none=True), L.ptr(td, allow_none=True), L.ptr(ad, allow_none=True), L.ptr(inplace), M, Cc,
                                                    st))
        assert torch.equal(inplace.view(torch.int32), out.view(torch.int32)), mask                     # in place = out of place, bit for bit
    print(f"affine / PReLU [{M}, {Cc}]: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("B,K,N", [(1, 8, 1), (2, 392, 5), (3, 25088, 512), (64, 25088, 16)])
def test_fc(B, K, N):
    from smirk_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    g = torch.Generator().manual_seed(B + N)
    xs, x64 = to_split16(torch.randn(B, K, generator=g) * 2)
    w, bias = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    xd, wd, bd = xs.to(_dev()), w.to(_dev()), bias.to(_dev())
    need = lib.smirk_mica_fc_workspace_bytes(B, K, N)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())
    runs = []
    for _ in range(2):
        out = torch.full((B, N), float("nan"), device=_dev())
        ws.fill_(0xFF)
        L.check(lib.smirk_mica_fc_split16(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(out), C.c_void_p(ws.data_ptr()), need, B, K, N, st))
        runs.append(out)
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))                           # two runs agree bit for bit
    want = x64 @ w.double().t() + bias.double()
    bound = (K * E24 + E20) * (x64.abs() @ w.double().abs().t()) + E24 * bias.double().abs()
    assert _ratio(f"fc [{B}, {K}, {N}]", (runs[0].double().cpu() - want).abs(), bound) <= 1.0
    assert lib.smirk_mica_fc_split16(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(out), C.c_void_p(ws.data_ptr()), 1 << 40, 65, K, N, st) == L.SMIRK_ERR_BAD_ARG


def _head_struct(linears):
    """five (weight, bias) CPU pairs -> (SmirkMicaHead, the device tensors it points to)"""
    from smirk_amd import _lib as L
    head, keep = L.SmirkMicaHead(), []
    for k, (w, b) in enumerate(linears):
        wd, bd = w.contiguous().to(_dev()), b.contiguous().to(_dev())
        keep += [wd, bd]
        head.layer[k].w, head.layer[k].b, head.layer[k].n_in, head.layer[k].n_out = wd.data_ptr(), bd.data_ptr(), w.shape[1], w.shape[0]
    return head, keep


@pytest.mark.parametrize("B,dims", [(1, (512, 300, 300)), (3, (512, 300, 300)), (64, (512, 300, 300)), (1, (16, 8, 8))])
def test_head(B, dims):
    from smirk_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    z, hid, n_out = dims
    g = torch.Generator().manual_seed(B + z)
    if dims == (512, 300, 300):
        linears = None
        ckpt = ML.synth_checkpoint((1, 1, 1, 1), 1)
        fm = ckpt["flameModel"]
        pairs = [(fm[f"regressor.network.{j}.weight"], fm[f"regressor.network.{j}.bias"]) for j in range(4)] + [(fm["regressor.output.weight"], fm["regressor.output.bias"])]
    else:
        ckpt = None
        sizes = [(z, hid), (hid, hid), (hid, hid), (hid, hid), (hid, n_out)]
        pairs = linears = [(torch.randn(fo, fi, generator=g) / fi ** 0.5, torch.randn(fo, generator=g) * 0.1) for fi, fo in sizes]
    feat = torch.randn(B, z, generator=g) * 10
    feat[B // 2] = 0.0                                                                                  # a zero feature row: the eps clamp, a finite result
    head, keep = _head_struct(pairs)
    out = torch.full((B, n_out), float("nan"), device=_dev())
    L.check(lib.smirk_mica_head(L.ptr(feat.to(_dev())), C.byref(head), L.ptr(out), B, st))
    want = ML.head_law(ckpt, feat, torch.float64, linears)
    e32 = float((ML.head_law(ckpt, feat, torch.float32, linears).double() - want).abs().max())
    bound = max(4 * e32, 1e-6 * float(want.abs().max()))
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    print(f"head B = {B} {dims}: error {err:.3g}, eager fp32 {e32:.3g}, error / bound = {err / bound:.3f}")
    assert err <= bound
    del keep


# ---- the whole network -------------------------------------------------------------------------------------------------------------------------------------
_modules = {}


def _module(layers, seed):
    from smirk_amd import MICA
    if (layers, seed) not in _modules:
        _modules[(layers, seed)] = MICA(ML.synth_checkpoint(layers, seed), layers=layers).to(_dev())
    return _modules[(layers, seed)]


@pytest.mark.parametrize("layers,seed,B", ML.NET_CASES, ids=[str(sum(c[0])) + "blocks" for c in ML.NET_CASES])
def test_whole_network(layers, seed, B):
    ref = ML.case_reference(layers, seed, B)
    m, img = _module(layers, seed), ref["images"].to(_dev())
    got = {"features": m.arcface_features(img), "shape_params": m(img)["shape_params"]}
    assert tuple(got["shape_params"].shape) == (B, 300) and got["shape_params"].dtype == torch.float32
    results = {}
    for name in ("features", "shape_params"):
        want = ref["f64"][name]
        e32 = float((ref["f32"][name].double() - want).abs().max())
        bound = max(4 * e32, 2e-6 * float(want.abs().max()))
        err = float((got[name].double().cpu() - want).abs().max())
        results[name] = (err, bound)
        print(f"{sum(layers)} blocks, B = {B}, {name}: error {err:.3g}, eager fp32 {e32:.3g}, max |ref| {float(want.abs().max()):.3g}, error / bound = {err / bound:.3f}")
    for name, (err, bound) in results.items():
        assert err <= bound, name


@pytest.mark.parametrize("D", [300, 100])
def test_loss_and_gradient(D):
    layers, seed, B = ML.NET_CASES[0]
    ref = ML.case_reference(layers, seed, B)
    m = _module(layers, seed)
    s = torch.randn(B, D, generator=torch.Generator().manual_seed(D))
    sd = s.to(_dev()).requires_grad_(True)
    loss = m.calculate_mica_shape_loss(sd, ref["images"].reshape(B, 3 * 112 * 112).to(_dev()))          # img given flat
    loss.backward()
    target = ref["f64"]["shape_params"][:, :D]
    want = float(((s.double() - target) ** 2).mean())
    rel = abs(float(loss.detach()) - want) / want
    g64 = 2 * (s.double() - target) / (B * D)
    grel = float((sd.grad.double().cpu() - g64).abs().max()) / float(g64.abs().max())
    print(f"D = {D}: loss relative error {rel:.3g} (bound 1e-5), gradient {grel:.3g} of max |g| (bound 1e-6)")
    assert loss.shape == () and rel <= 1e-5
    assert sd.grad.shape == sd.shape and torch.isfinite(sd.grad).all() and grel <= 1e-6                 # GRAD_REL of tests/test_losses_gpu.py
    assert torch.equal(sd.grad[g64.to(_dev()) == 0], torch.zeros_like(sd.grad[g64.to(_dev()) == 0]))
    assert all(p.grad is None for p in m.parameters())


def test_refusals_on_the_device():
    import smirk_amd
    m = _module(*ML.NET_CASES[0][:2])
    with pytest.raises(smirk_amd.SmirkHipError, match="112"):
        m(torch.zeros(1, 3, 96, 96, device=_dev()))
    with pytest.raises(smirk_amd.SmirkHipError, match="requires grad"):
        m(torch.zeros(1, 3, 112, 112, device=_dev(), requires_grad=True))
    with pytest.raises(smirk_amd.SmirkHipError):
        m(torch.zeros(1, 4, 112, 112, device=_dev()))


def test_chunks_of_64_equal_separate_calls():
    layers, seed, _ = ML.NET_CASES[0]
    m, img = _module(layers, seed), ML.synth_images(65, 7).to(_dev())
    whole = m(img)["shape_params"]
    head, tail = m(img[:64])["shape_params"], m(img[64:])["shape_params"]
    assert tuple(whole.shape) == (65, 300)
    assert torch.equal(whole[:64].view(torch.int32), head.view(torch.int32)) and torch.equal(whole[64:].view(torch.int32), tail.view(torch.int32))


def test_second_call_does_not_wait_for_the_host():
    layers, seed, B = ML.NET_CASES[0]
    m, img = _module(layers, seed), ML.case_reference(layers, seed, B)["images"].to(_dev())
    s = torch.zeros(B, 300, device=_dev(), requires_grad=True)
    first = m(img)["shape_params"]
    m.calculate_mica_shape_loss(s, img)
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = m(img)["shape_params"]
        m.calculate_mica_shape_loss(s, img).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))


def test_weight_cache_follows_an_in_place_change():
    from smirk_amd import MICA
    layers, seed, B = ML.NET_CASES[0]
    ckpt = ML.synth_checkpoint(layers, seed)
    m, img = MICA(ckpt, layers=layers).to(_dev()), ML.case_reference(layers, seed, B)["images"].to(_dev())
    before = m(img)["shape_params"].clone()
    m.arcface.layer2[0].bn1.running_mean.add_(0.5)
    after = m(img)["shape_params"]
    changed = {p: dict(d) for p, d in ckpt.items()}
    changed["arcface"]["layer2.0.bn1.running_mean"] = ckpt["arcface"]["layer2.0.bn1.running_mean"] + 0.5
    fresh = MICA(changed, layers=layers).to(_dev())(img)["shape_params"]
    assert not torch.equal(before, after)
    assert torch.equal(after.view(torch.int32), fresh.view(torch.int32))


def test_range_flag_reports_an_overflow_on_the_next_forward():
    import smirk_amd
    from smirk_amd import MICA
    layers, seed, B = ML.NET_CASES[0]
    m, img = MICA(ML.synth_checkpoint(layers, seed), layers=layers).to(_dev()), ML.case_reference(layers, seed, B)["images"].to(_dev())
    for mod in m.arcface.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.weight.mul_(1e3)
    m(img)
    torch.cuda.synchronize()
    with pytest.raises(smirk_amd.SmirkHipError, match="MICA"):
        m(img)
    assert not _peek_and_clear()                                                                       # the raise cleared the flag and launched nothing


@pytest.mark.parametrize("layers,seed,B", ML.NET_CASES[:2], ids=["4blocks", "5blocks"])
def test_launch_count(layers, seed, B):
    from smirk_amd import _lib as L
    m, img = _module(layers, seed), ML.case_reference(layers, seed, B)["images"].to(_dev())
    m(img)                                                                                              # packs the weights
    L.profile_start()
    m(img)
    recs = L.profile_stop()
    n_blocks, n_fc = sum(layers), 2
    print(sorted({r[0] for r in recs}))
    assert len(recs) == 1 + 2 + 4 * n_blocks + 4 + n_fc + 1
