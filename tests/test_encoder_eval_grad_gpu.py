"""GPU parity of the even training step's encoder pass (smirk_amd/encoder_eval_grad.py): SmirkEncoder frozen and in .eval() as `utils.freeze_module` leaves it,
inside an autograd graph whose backward yields the image gradient (base_trainer.py:258-268; smirk_trainer.py:367-368, :300, :375).

The two new kernels are held to float64 on crafted operands with per-element bounds.  The whole encoder is held (a) to float64 head by head, (b) to the FORCED
float64 law of tests/enc_eval_law.py under the module's own ReLU decisions — an affine map of the image, so the gradient is checked at rounding level, with the
distance of eager fp32 from the same law under ITS decisions as the yardstick (factor 4: the margin for one box and one BLAS build, tests/enc_tolerances.py) —
and (c) to the unforced float64 gradient with caps on the share of flipped decisions and on the relative L2 distance."""
import functools

import pytest
import torch

import enc_eval_law as E
from enc_tolerances import VS_FP64
from oracle import generator_ref as G
from oracle import mobilenet_ref as M

pytestmark = pytest.mark.gpu


# ---- the kernels on crafted operands ------------------------------------------------------------------------------------------------------------------------
def _to_split16(x):
    """fp32 [..., C] -> (split16 storage on the GPU, the float64 values it carries)"""
    from smirk_amd.smirk_generator import _split16, split16_to_float
    C = x.shape[-1]
    s = _split16(x.reshape(-1, C).contiguous()).reshape(x.shape).contiguous().cuda()
    v = split16_to_float(s.reshape(1, 1, -1, C)).reshape(x.shape)
    return s, v.double().cpu()


def _pad_lead(n, s):
    return 1 if s == 1 else max((-(-n // s) - 1) * s + 3 - n, 0) // 2


def _crafted(g, shape, zeros):
    """values in +-[0.25, 2] with exact zeros planted in `zeros` of the places (and a few negative ones, which a stored ReLU output never has: masked too)"""
    x = (torch.rand(shape, generator=g) * 1.75 + 0.25) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    if zeros:
        x = torch.where(torch.rand(shape, generator=g) < zeros, torch.zeros(()), x)
    return x


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (1, 2, 2, 8), (3, 5, 7, 72), (2, 8, 6, 16)])
def test_fused_depthwise_backward_kernel_vs_float64(B, H, W, C, stride):
    from smirk_amd import _lib as L
    from smirk_amd.smirk_generator import split16_to_float
    lib, P = L.lib(), L.ptr
    Ho, Wo = -(-H // stride), -(-W // stride)
    pt, pl = _pad_lead(H, stride), _pad_lead(W, stride)
    g = torch.Generator().manual_seed(1000 * B + 100 * H + 10 * W + stride)
    dy_s, dy = _to_split16(_crafted(g, (B, Ho, Wo, C), 0))
    yo_s, yo = _to_split16(_crafted(g, (B, Ho, Wo, C), 0.3))
    yi_s, yi = _to_split16(_crafted(g, (B, H, W, C), 0.3))
    add_s, add = _to_split16(_crafted(g, (B, H, W, C), 0))
    s_out, s_in, w = _crafted(g, (C,), 0), _crafted(g, (C,), 0), _crafted(g, (9, C), 0)
    s_out_d, s_in_d, w_d = s_out.cuda(), s_in.cuda(), w.cuda()
    # float64, as a scatter from the outputs (the kernel gathers)
    t = dy * s_out.double() * (yo > 0)
    conv, mag = torch.zeros(B, H, W, C, dtype=torch.float64), torch.zeros(B, H, W, C, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            oy = [o for o in range(Ho) if 0 <= o * stride - pt + ky < H]
            ox = [o for o in range(Wo) if 0 <= o * stride - pl + kx < W]
            if not oy or not ox:
                continue
            iy, ix = torch.tensor([o * stride - pt + ky for o in oy])[:, None], torch.tensor([o * stride - pl + kx for o in ox])[None, :]
            term = t[:, torch.tensor(oy)[:, None], torch.tensor(ox)[None, :]] * w[ky * 3 + kx].double()
            conv[:, iy, ix] += term
            mag[:, iy, ix] += (dy * s_out.double())[:, torch.tensor(oy)[:, None], torch.tensor(ox)[None, :]].abs() * w[ky * 3 + kx].double().abs()
    assert float(yo.eq(0).sum()) > 0 or yo.numel() <= 8
    for with_add in (False, True):
        for with_in in (False, True):
            ref = conv + (add if with_add else 0.0)
            bound = 2.0 ** -20 * mag * (s_in.double().abs() if with_in else 1.0) + (2.0 ** -20 * add.abs() if with_add else 0.0)
            if with_in:
                ref = ref * s_in.double() * (yi > 0)
            dx = torch.full((B, H, W, C), float("nan"), device="cuda")
            L.check(lib.smirk_dwconv3x3_eval_backward_split16(P(dy_s), P(yo_s), P(s_out_d), P(w_d), P(add_s if with_add else None, allow_none=True),
                                                              P(yi_s if with_in else None, allow_none=True), P(s_in_d if with_in else None, allow_none=True),
                                                              P(dx), B, H, W, C, stride, L.stream_ptr()))
            got = split16_to_float(dx).double().cpu()
            assert torch.isfinite(got).all()
            if with_in:
                assert bool((got[yi <= 0] == 0).all())
            err = (got - ref).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max()) if float(bound.max()) > 0 else 0.0
            print(f"B{B} {H}x{W} C{C} s{stride} add={with_add} y_in={with_in}: max error / bound = {ratio:.3f}")
            assert bool((err <= bound).all()), (with_add, with_in, ratio)


@pytest.mark.parametrize("Mrows,C", [(1, 8), (85, 24), (256, 8), (257, 8)])          # M * C / 8 = 1, 255, 256, 257 groups
def test_relu_scale_backward_kernel_vs_float64(Mrows, C):
    from smirk_amd import _lib as L
    from smirk_amd.smirk_generator import split16_to_float
    g = torch.Generator().manual_seed(Mrows)
    dy_s, dy = _to_split16(_crafted(g, (1, 1, Mrows, C), 0))
    y_s, y = _to_split16(_crafted(g, (1, 1, Mrows, C), 0.3))
    s = _crafted(g, (C,), 0)
    s_d = s.cuda()
    dz = torch.full((1, 1, Mrows, C), float("nan"), device="cuda")
    L.check(L.lib().smirk_relu_scale_backward_split16(L.ptr(dy_s), L.ptr(y_s), L.ptr(s_d), L.ptr(dz), Mrows, C, L.stream_ptr()))
    got = split16_to_float(dz).double().cpu()
    ref = dy * s.double() * (y > 0)
    assert bool((got[y <= 0] == 0).all()) and torch.isfinite(got).all()
    err, bound = (got - ref).abs(), 2.0 ** -21 * (dy * s.double()).abs()
    print(f"M{Mrows} C{C}: max error / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ---- the whole encoder ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _esd():
    return M.synth_encoder_state_dict()


@functools.lru_cache(maxsize=None)
def _laws(B, HW):
    """computed once per shape and shared: float64 (outputs, gradient, trace), eager fp32 (outputs, gradient) and fp32's distance from the forced law under its trace"""
    img, tgt = E.images(B, HW), E.targets(B)
    ref64 = E.reference(_esd())
    tr64, tr32 = {}, {}
    o64, _, g64 = E.run(ref64, img, tgt, record=tr64)
    o32, _, g32 = E.run(E.reference(_esd(), torch.float32), img, tgt, record=tr32)
    _, _, gf32 = E.run(ref64, img, tgt, trace=tr32)
    d32 = float((g32.double() - gf32).abs().max()) / float(gf32.abs().max())
    return dict(img=img, tgt=tgt, ref64=ref64, o64=o64, g64=g64, tr64=tr64, o32=o32, g32=g32, d32=d32)


def _frozen_encoder(sd=None, trace=False):
    """SmirkEncoder as utils.freeze_module leaves its three sub-encoders: requires_grad False + .eval(), the container itself in train mode"""
    from smirk_amd import SmirkEncoder
    enc = SmirkEncoder(); enc.load_state_dict(_esd() if sd is None else sd, strict=True); enc = enc.cuda().train()
    for n in E.ENCODERS:
        m = getattr(enc, n)
        for p in m.parameters():
            p.requires_grad_(False)
        m.eval()
        if trace:
            m.encoder._trace = []
    return enc


def _step(enc, img, tgt, scale=1.0):
    x = img.detach().cuda().requires_grad_(True)
    out = enc(x)
    (scale * E.loss_of(out, {k: v.cuda() for k, v in tgt.items()})).backward()
    return {k: v.detach() for k, v in out.items()}, x.grad


def _grad_bound(law):
    return max(4 * law["d32"], 1e-6)


def _head_bounds(law):
    return {k: max(VS_FP64[k], 4 * float((law["o32"][k].double() - law["o64"][k]).abs().max())) for k in law["o64"]}


@pytest.mark.parametrize("B,HW", E.SHAPES)
def test_frozen_eval_encoder_image_gradient_vs_float64(B, HW):
    law = _laws(B, HW)
    enc = _frozen_encoder(trace=True)
    buffers = {k: b.clone() for k, b in enc.named_buffers()}
    out, dimg = _step(enc, law["img"], law["tgt"])                            # 1. backward succeeds (NotImplementedError without the feature)
    assert dimg is not None and torch.isfinite(dimg).all()
    tr = E.module_trace(enc)
    for n in E.ENCODERS:
        getattr(enc, n).encoder._trace = None
    assert all(torch.equal(b, buffers[k]) for k, b in enc.named_buffers())    # running statistics and num_batches_tracked: bit-identical
    assert all(p.grad is None for p in enc.parameters())
    with torch.no_grad():
        plain = enc(law["img"].cuda())
    hb = _head_bounds(law)
    for k in law["o64"]:                                                       # 2. every head, autograd path and no_grad path of the same module
        e, ep = float((out[k].double().cpu() - law["o64"][k]).abs().max()), float((plain[k].double().cpu() - law["o64"][k]).abs().max())
        print(f"{k}: |out - float64| {e:.2e} (no_grad forward {ep:.2e}), bound {hb[k]:.2e}")
        assert e <= hb[k] and ep <= hb[k], k
    share = E.trace_differences(tr, law["tr64"]) / E.trace_size(tr)            # 3. decisions that differ from float64's
    _, _, gf = E.run(law["ref64"], law["img"], law["tgt"], trace=tr)           # 4. the forced law under the module's own decisions
    gmax = float(gf.abs().max())
    dist = float((dimg.double().cpu() - gf).abs().max()) / gmax
    l2 = float((dimg.double().cpu() - law["g64"]).norm() / law["g64"].norm())  # 5. unforced
    print(f"B{B} {HW}x{HW}: decisions differing from float64's {share:.2e} of {E.trace_size(tr)}; against the forced law {dist:.2e} of max|g| "
          f"(eager fp32: {law['d32']:.2e}; ratio to the bound {dist / _grad_bound(law):.3f}); unforced relative L2 {l2:.2e}")
    assert share <= 1e-5
    assert dist <= _grad_bound(law)
    assert l2 <= 0.05


def test_scaled_loss_determinism_and_streams(monkeypatch):
    law = _laws(3, 32)
    enc = _frozen_encoder(trace=True)
    _, g3 = _step(enc, law["img"], law["tgt"], scale=3.0)
    _, _, gf = E.run(law["ref64"], law["img"], law["tgt"], trace=E.module_trace(enc))
    assert float((g3.double().cpu() - 3 * gf).abs().max()) <= _grad_bound(law) * float((3 * gf).abs().max())
    for n in E.ENCODERS:
        getattr(enc, n).encoder._trace = None
    o1, g1 = _step(enc, law["img"], law["tgt"])
    o2, g2 = _step(enc, law["img"], law["tgt"])
    assert torch.equal(g1, g2) and all(torch.equal(o1[k], o2[k]) for k in o1)
    monkeypatch.setenv("SMIRK_ENCODER_TRAIN_SERIAL", "1")                       # the container is in train mode: the one-stream order applies to this path too
    o3, g3s = _step(enc, law["img"], law["tgt"])
    monkeypatch.delenv("SMIRK_ENCODER_TRAIN_SERIAL")
    enc._train_serial = True
    o4, g4 = _step(enc, law["img"], law["tgt"])
    assert torch.equal(g1, g3s) and torch.equal(g1, g4) and all(torch.equal(o1[k], o3[k]) and torch.equal(o1[k], o4[k]) for k in o1)


def test_no_host_synchronisation_from_the_second_call_on():
    law = _laws(3, 32)
    enc = _frozen_encoder()
    tgt = {k: v.cuda() for k, v in law["tgt"].items()}
    x = law["img"].cuda()
    enc(x.clone().requires_grad_(True))["cam"].sum().backward()                # first call: packs and caches the weights
    torch.cuda.synchronize()
    xi = x.clone().requires_grad_(True)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                                      # the guard is armed: a probe .item() raises under it
            torch.ones(1, device="cuda").item()
        E.loss_of(enc(xi), tgt).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert float(xi.grad.abs().max()) > 0


def test_second_backward_raises_and_no_grad_keeps_nothing():
    law = _laws(3, 32)
    enc = _frozen_encoder()
    x = law["img"].cuda().requires_grad_(True)
    loss = E.loss_of(enc(x), {k: v.cuda() for k, v in law["tgt"].items()})
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    del loss
    x = x.detach()

    def allocated():
        torch.cuda.synchronize()
        torch.empty(1, device="cuda")                                          # an allocation lets the allocator return blocks whose side-stream use has ended
        return torch.cuda.memory_allocated()

    with torch.no_grad():
        enc(x)                                                                 # warm: workspaces and caches exist
    level = allocated()
    with torch.no_grad():
        out = enc(x)
    assert not any(v.requires_grad for v in out.values())
    del out
    assert allocated() == level


def test_a_trainable_head_keeps_the_loud_cut():
    law = _laws(3, 32)
    enc = _frozen_encoder()
    for p in enc.expression_encoder.expression_layers.parameters():
        p.requires_grad_(True)
    out = enc(law["img"].cuda().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        out["expression_params"].sum().backward()


def test_running_statistics_changed_in_place_are_followed_after_train_eval():
    law = _laws(3, 32)
    enc = _frozen_encoder()
    _step(enc, law["img"], law["tgt"])                                         # fills the caches
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.mul_(1.5)
    for n in E.ENCODERS:
        getattr(enc, n).train(); getattr(enc, n).eval()
    out, dimg = _step(enc, law["img"], law["tgt"])
    sd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    o64, _, g64 = E.run(E.reference(sd), law["img"], law["tgt"])
    o32, _, _ = E.run(E.reference(sd, torch.float32), law["img"], law["tgt"])
    hb = _head_bounds(dict(o64=o64, o32=o32))
    for k in o64:
        assert float((o64[k] - law["o64"][k]).abs().max()) > 10 * hb[k], k                             # the new statistics matter
        assert float((out[k].double().cpu() - o64[k]).abs().max()) <= hb[k], k
    assert float((dimg.double().cpu() - g64).norm() / g64.norm()) <= 0.05


def test_range_flag_trips_on_a_huge_upstream_gradient():
    import smirk_amd
    from smirk_amd import _lib as L
    law = _laws(3, 32)
    enc = _frozen_encoder()
    x = law["img"].cuda().requires_grad_(True)
    out = enc(x)
    out["shape_params"].backward(torch.full_like(out["shape_params"], 1e30))
    with pytest.raises(smirk_amd.SmirkHipError, match="split-fp16"):
        smirk_amd.check_numerics()
    assert L.lib().smirk_range_flag_peek() == 0
    smirk_amd.check_numerics()


def test_train_arith_f16x1_is_honoured():
    """the 16-bit class on the pointwise convolutions, forward and data gradient: differs from f16x3, and is no further from the float64 gradient than 4 x the
    distance the TRAIN-mode path in f16x1 shows from ITS float64 oracle on the same inputs.
    Both distances are relative L2, so a common factor on the loss cancels; the loss is scaled by 2^-12 here because at 3 x 3 x 32 x 32 the TRAIN-mode gradient
    itself leaves the split-fp16 range (|x| < 65520) at scale 1: batch statistics over three 1 x 1 feature maps give invstd up to 1 / sqrt(eps) layer after
    layer.  Float64 autograd through the oracle shows activation gradients up to 1.5e5; measured on the MI355X, the train-mode path raises its range flag and
    returns NaN at scale 1 in both arithmetics and at 2^-4 in f16x1, and is finite at 2^-12 (max |dimg| 21 in f16x3, 349 in f16x1)."""
    from smirk_amd import SmirkEncoder
    from smirk_amd.cycle import set_train_arith
    law = _laws(3, 32)
    scale = 2.0 ** -12
    enc = _frozen_encoder()
    _, g3 = _step(enc, law["img"], law["tgt"], scale=scale)
    set_train_arith(None, enc, "f16x1")
    _, g1 = _step(enc, law["img"], law["tgt"], scale=scale)
    assert not torch.equal(g1, g3)
    d_eval = float((g1.double().cpu() - scale * law["g64"]).norm() / (scale * law["g64"]).norm())
    # TRAIN mode (batch statistics), every parameter frozen, f16x1, against float64 autograd through the oracle in .train()
    ref = M.SmirkEncoderRef(); ref.load_state_dict(_esd()); ref = ref.double().train()
    for p in ref.parameters():
        p.requires_grad_(False)
    x64 = law["img"].double().requires_grad_(True)
    (scale * E.loss_of(ref(x64), law["tgt"])).backward()
    tr = SmirkEncoder(); tr.load_state_dict(_esd()); tr = tr.cuda().train()
    for p in tr.parameters():
        p.requires_grad_(False)
    set_train_arith(None, tr, "f16x1")
    _, gt = _step(tr, law["img"], law["tgt"], scale=scale)
    d_train = float((gt.double().cpu() - x64.grad).norm() / x64.grad.norm())
    print(f"f16x1 relative L2 from float64: eval-mode path {d_eval:.2e}, train-mode path {d_train:.2e}")
    assert torch.isfinite(gt).all() and d_eval <= 4 * d_train


def _launch_counts():
    from smirk_amd import _lib as L
    law = _laws(3, 32)
    enc = _frozen_encoder().expression_encoder
    kinds = [blk.kind for st in enc.encoder.blocks for blk in st]
    x = law["img"].cuda().requires_grad_(True)
    enc(x)["expression_params"].sum().backward()                               # caches
    torch.cuda.synchronize()
    x.grad = None
    L.profile_start()
    out = enc(x)
    torch.cuda.synchronize()
    fwd = [r[0] for r in L.profile_stop()]
    L.profile_start()
    (out["expression_params"].sum() + out["jaw_params"].sum() + out["eyelid_params"].sum()).backward()
    torch.cuda.synchronize()
    bwd = [r[0] for r in L.profile_stop()]
    return kinds, fwd, bwd


def test_launch_count_of_one_expression_backbone_backward():
    """library launches of the backward: head, then cn 2 / ir 3 / ds 2 per block, then the stem"""
    kinds, _, bwd = _launch_counts()
    bound = 1 + sum({"cn": 2, "ir": 3, "ds": 2}[k] for k in kinds) + 1
    print(f"library launches: backward {len(bwd)} (<= {bound})")
    assert 0 < len(bwd) <= bound
    assert sum("dw_eval_bwd_kernel" in k for k in bwd) == sum(k in ("ir", "ds") for k in kinds) and sum("relu_scale_bwd_kernel" in k for k in bwd) == kinds.count("cn")


def test_launch_count_of_one_expression_backbone_forward():
    """library launches of the forward: at most 1 (stem) + ds 2 / ir 3 / cn 1 per block + 2 (head: pooled Linear in one launch, the clamps)"""
    kinds, fwd, _ = _launch_counts()
    bound = 1 + sum({"ds": 2, "ir": 3, "cn": 1}[k] for k in kinds) + 2
    print(f"library launches: forward {len(fwd)} (<= {bound})")
    assert 0 < len(fwd) <= bound
    assert fwd[-2:] == ["gap_pool_linear_kernel", "expression_clamps_kernel"]


@pytest.mark.parametrize("HW,C,N", [(1, 576, 6), (49, 960, 55), (12, 72, 64), (7, 8, 1)])
def test_one_launch_head_equals_the_two_launch_head_bit_for_bit(HW, C, N):
    """smirk_gap_linear_split16 / smirk_gap_linear without a workspace (N <= 64): one launch, the outputs of the two-launch form bit for bit"""
    from smirk_amd import _lib as L
    g = torch.Generator().manual_seed(HW * 1000 + N)
    B = 3
    feat_s, _ = _to_split16(torch.randn(B, 1, HW, C, generator=g))
    feat32 = torch.randn(B, HW, C, generator=g).cuda()
    w, bias = torch.randn(N, C, generator=g).cuda(), torch.randn(N, generator=g).cuda()
    for fn, feat in ((L.lib().smirk_gap_linear_split16, feat_s), (L.lib().smirk_gap_linear, feat32)):
        two, one, ws = torch.full((B, N), float("nan"), device="cuda"), torch.full((B, N), float("nan"), device="cuda"), torch.empty(B, C, device="cuda")
        L.check(fn(L.ptr(feat), L.ptr(w), L.ptr(bias), L.ptr(two), L.ptr(ws), B, HW, C, N, L.stream_ptr()))
        L.profile_start()
        L.check(fn(L.ptr(feat), L.ptr(w), L.ptr(bias), L.ptr(one), None, B, HW, C, N, L.stream_ptr()))
        torch.cuda.synchronize()
        assert [r[0] for r in L.profile_stop()] == ["gap_pool_linear_kernel"]
        assert torch.isfinite(two).all() and torch.equal(one, two)


# ---- the even step -------------------------------------------------------------------------------------------------------------------------------------------
def test_even_step_generator_learns_through_the_frozen_encoder():
    """B = 2 at 64 x 64: generator in .train(), encoder frozen + .eval(); cycle_forward -> backward -> clip_grad_norm_(generator, 0.1) against the float64 chain
    oracle.generator_ref.train_forward -> SmirkEncoderRef.eval() -> cycle_loss, with the fp32 chain's spread as the yardstick (tests/test_cycle_gpu.py's rule)"""
    from oracle import make_cycle_golden as MC
    from smirk_amd import SmirkGenerator
    from smirk_amd.cycle import cycle_forward, cycle_loss
    rendered, masked, feats = MC.inputs(2, 64)
    gsd = G.synth_state_dict()

    def chain(dtype):
        params, buffers = G.split_state_dict(gsd, dtype)
        recon = G.train_forward(params, buffers, torch.cat([rendered, masked], 1).to(dtype))
        out = E.reference(_esd(), dtype)(recon)
        loss = cycle_loss(out, {k: v.to(dtype) for k, v in feats.items()})
        loss.backward()
        return float(loss.detach()), float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values())))

    l64, n64 = chain(torch.float64)
    _, n32 = chain(torch.float32)
    gen = SmirkGenerator(6, 3, 32, 5); gen.load_state_dict(gsd); gen = gen.cuda().train()
    enc = _frozen_encoder()
    buffers = {k: b.clone() for k, b in enc.named_buffers()}
    loss, _, _ = cycle_forward(gen, enc, rendered.cuda(), masked.cuda(), {k: v.cuda() for k, v in feats.items()}, freeze_generator=False)
    loss.backward()
    gnorm = float(torch.nn.utils.clip_grad_norm_(gen.parameters(), 0.1))
    spread = abs(n32 - n64) / n64
    print(f"even step: loss {loss.item():.6f} (float64 {l64:.6f}); generator gradient norm {gnorm:.4f} (float64 {n64:.4f}, fp32 chain spread {spread:.2e})")
    assert abs(loss.item() - l64) <= 1e-3 * abs(l64)
    assert abs(gnorm - n64) / n64 <= max(5e-3, 3 * spread)
    for k, p in gen.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    assert all(p.grad is None for p in enc.parameters())
    assert all(torch.equal(b, buffers[k]) for k, b in enc.named_buffers())
