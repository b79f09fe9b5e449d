"""The encoder's unfused primitives, each against torch float64 at the kernel level (csrc/encoder_ops.hip, the 1 x 1 implicit GEMMs of csrc/conv.hip), and the
exact-fp32 encoder mode end to end.  The fused block kernels are compared with these kernels elsewhere; here the comparator itself is pinned.  Outputs are written
between guard bands into NaN pre-filled regions (tests/mbconv_cases.py)."""
import pytest
import torch
import torch.nn.functional as F

import mbconv_cases as MC
from enc_tolerances import VS_FP64
from oracle import assets as A
from oracle import mobilenet_ref as M
from test_conv_gpu import TOL as CONV_TOL

pytestmark = pytest.mark.gpu

STENCIL_TOL = 3e-6      # * max(1, max |ref|): the bound of test_encoder_head_fused_kernel_vs_float64 - the same fp32 stencil followed by a split
GEOMS = [(1, 1), (2, 3), (9, 7), (14, 14), (57, 33)]


def _dev(t):
    return t.float().contiguous().cuda()


def _split_nhwc(x):
    from smirk_amd.smirk_generator import _split16
    return _split16(x.reshape(-1, x.shape[-1])).reshape(x.shape)


def _decode(t):
    from smirk_amd.smirk_generator import split16_to_float
    return split16_to_float(t).cpu().double()


def _guarded(shape, split):
    return MC.Guarded(*shape, nan_word=MC.NAN_WORD if split else MC.NAN_WORD_F32)


def _assert_close(got, ref, tol, what):
    err = (got - ref).abs()
    big = float(ref.abs().max())
    finite = torch.isfinite(err)
    worst = float(err[finite].max()) if bool(finite.any()) else float("nan")
    print(f"OPS_VS_FP64 {what}: max|err| {worst:.3e}  max|ref| {big:.3e}  bound {tol:.3e}")
    assert bool(finite.all()), f"{what}: elements never written / not finite: " + MC.where(torch.where(finite, 0.0, float("nan")).double(), 1.0)
    msg = MC.where(err, tol)
    assert not msg, f"{what}: {msg}"


# ---- depthwise 3 x 3 ---------------------------------------------------------------------------------------------------------------------------------------------
def _dw_ref64(x64_nhwc, wd, sc, sh, stride, relu):
    C = wd.shape[0]
    conv = M.Conv2dSame(C, C, 3, stride, 0, groups=C, bias=False).double()
    with torch.no_grad():
        conv.weight.copy_(wd.double()[:, None])
        y = conv(x64_nhwc.permute(0, 3, 1, 2)) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1).contiguous()


def _dw_case(B, H, W, C, split, seed):
    """the depthwise entry on one input at both strides, with and without ReLU, against float64 on the values it reads"""
    from smirk_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g)
    wd = torch.randn(C, 3, 3, generator=g) * 0.4
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    xd = _dev(_split_nhwc(x)) if split else _dev(x)
    x64 = _decode(xd) if split else x.double()
    w9, scd, shd = _dev(wd.reshape(C, 9).t()), _dev(sc), _dev(sh)
    fn = L.lib().smirk_dwconv3x3_split16 if split else L.lib().smirk_dwconv3x3
    P = L.ptr
    for stride in (1, 2):
        for relu in (0, 1):
            Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
            G = _guarded((B, Ho, Wo, C), split)
            L.check(fn(P(xd), P(w9), P(scd), P(shd), P(G.out), B, H, W, C, stride, relu, L.stream_ptr()))
            what = f"{'smirk_dwconv3x3_split16' if split else 'smirk_dwconv3x3'} B{B} {H}x{W} C{C} stride {stride} relu {relu}"
            out = G.check(what)
            ref = _dw_ref64(x64, wd, sc, sh, stride, relu)
            _assert_close(_decode(out) if split else out.cpu().double(), ref, STENCIL_TOL * max(1.0, float(ref.abs().max())), what)


@pytest.mark.parametrize("C", [8, 24, 200, 960])
@pytest.mark.parametrize("hw", GEOMS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_dwconv3x3_split16_vs_float64(hw, C):
    """as inference uses it: folded BN scale / shift, ReLU on and off, both strides (TF-SAME padding on both parities)"""
    _dw_case(1 if hw == (57, 33) else 3, *hw, C, True, seed=hw[0] * 1000 + C)


def test_dwconv3x3_split16_row_loop_wraps():
    """B * Ho = 16800 > the 16384-workgroup grid: the kernel's row loop takes a second pass"""
    _dw_case(140, 240, 2, 8, True, seed=5)


@pytest.mark.parametrize("C", [4, 12, 72])
@pytest.mark.parametrize("hw", GEOMS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_dwconv3x3_fp32_vs_float64(hw, C):
    """the exact-fp32 mode's depthwise kernel"""
    _dw_case(1 if hw == (57, 33) else 3, *hw, C, False, seed=hw[0] * 1000 + C + 1)


# ---- stem --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout", [16, 64])
@pytest.mark.parametrize("hw", [(32, 32), (45, 37), (33, 64)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_stem_conv_s2_vs_float64(hw, cout):
    """3 x 3 stride-2 TF-SAME conv 3 -> Cout on the NCHW image + BN + ReLU -> NHWC, split16 and fp32 outputs"""
    from smirk_amd import _lib as L
    H, W = hw
    B = 2
    g = torch.Generator().manual_seed(H * 100 + cout)
    img = torch.rand(B, 3, H, W, generator=g)
    ws = torch.randn(cout, 3, 3, 3, generator=g) * 0.4
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    conv = M.Conv2dSame(3, cout, 3, 2, 0, bias=False).double()
    with torch.no_grad():
        conv.weight.copy_(ws.double())
        ref = F.relu(conv(img.double()) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert ref.shape == (B, Ho, Wo, cout)
    t = [_dev(img), _dev(ws.permute(0, 2, 3, 1).reshape(cout, 27)), _dev(sc), _dev(sh)]
    P = L.ptr
    for split in (True, False):
        fn = L.lib().smirk_stem_conv_s2_split16 if split else L.lib().smirk_stem_conv_s2
        G = _guarded((B, Ho, Wo, cout), split)
        L.check(fn(*[P(v) for v in t], P(G.out), B, H, W, cout, L.stream_ptr()))
        what = f"{'smirk_stem_conv_s2_split16' if split else 'smirk_stem_conv_s2'} {H}x{W} Cout {cout}"
        out = G.check(what)
        _assert_close(_decode(out) if split else out.cpu().double(), ref, STENCIL_TOL * max(1.0, float(ref.abs().max())), what)


# ---- pointwise implicit GEMM -------------------------------------------------------------------------------------------------------------------------------------
def _pointwise_layers():
    """every distinct (Cin, Cout, relu, residual) 1 x 1 convolution of the two backbones, from smirk_amd.smirk_encoder's architecture table"""
    from smirk_amd.smirk_encoder import _ARCH, MobileNetV3Features
    out = set()
    for name in _ARCH:
        for stage in MobileNetV3Features(name).blocks:
            for blk in stage:
                if blk.kind == "ds":
                    out.add((blk.conv_pw.in_channels, blk.conv_pw.out_channels, False, bool(blk.skip)))
                elif blk.kind == "ir":
                    out.add((blk.conv_pw.in_channels, blk.conv_pw.out_channels, True, False))
                    out.add((blk.conv_pwl.in_channels, blk.conv_pwl.out_channels, False, bool(blk.skip)))
                else:
                    out.add((blk.conv.in_channels, blk.conv.out_channels, True, False))
    return sorted(out)


@pytest.mark.parametrize("bhw", [(3, 7, 7), (2, 9, 11)], ids=lambda v: "%dx%dx%d" % v)
@pytest.mark.parametrize("layer", _pointwise_layers(), ids=lambda v: f"{v[0]}-{v[1]}{'_relu' if v[2] else ''}{'_res' if v[3] else ''}")
def test_pointwise_igemm_vs_float64(layer, bhw):
    """smirk_conv_igemm_f16x3 and smirk_conv_igemm_f32 as 1 x 1 convolutions at every width the backbones use, M = B * H * W ragged (147 / 198 rows)"""
    from smirk_amd import _lib as L
    from smirk_amd.smirk_generator import _split16, split16_to_float
    cin, cout, relu, residual = layer
    B, H, W = bhw
    g = torch.Generator().manual_seed(cin * 1000 + cout + H)
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) * (1.5 / cin ** 0.5)
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    res = torch.randn(B, H, W, cout, generator=g) if residual else None

    def ref64(x64, w64, r64):
        y = torch.einsum("bhwk,nk->bhwn", x64, w64) * sc.double() + sh.double()
        if r64 is not None:
            y = y + r64
        return F.relu(y) if relu else y
    d = L.SmirkConvDesc()
    d.B, d.H, d.W, d.C0, d.C1, d.Cout = B, H, W, cin, 0, cout
    d.KH = d.KW = d.stride = 1
    d.pad_t = d.pad_l = 0
    d.Ho, d.Wo, d.pad_mode = H, W, L.PAD_ZERO
    d.act, d.out_mode = (L.ACT_RELU if relu else L.ACT_NONE), L.OUT_NHWC
    P, N = L.ptr, (lambda t: L.ptr(t, allow_none=True))
    scd, shd = _dev(sc), _dev(sh)
    # exact fp32
    xd, wd, rd = _dev(x), _dev(w), (_dev(res) if residual else None)
    G = _guarded((B, H, W, cout), False)
    L.check(L.lib().smirk_conv_igemm_f32(d, P(xd), None, P(wd), P(scd), P(shd), N(rd), P(G.out), L.stream_ptr()))
    what = f"smirk_conv_igemm_f32 1x1 {cin}->{cout} M {B * H * W}"
    _assert_close(G.check(what).cpu().double(), ref64(x.double(), w.double(), res.double() if residual else None), CONV_TOL, what)
    # split-fp16 x3, reference on the decoded operands
    xs, wsp, rs = _dev(_split_nhwc(x)), _dev(_split16(w.contiguous())), (_dev(_split_nhwc(res)) if residual else None)
    w64 = split16_to_float(wsp.reshape(1, 1, cout, cin)).reshape(cout, cin).cpu().double()
    G = _guarded((B, H, W, cout), True)
    L.check(L.lib().smirk_conv_igemm_f16x3(d, P(xs), None, P(wsp), P(scd), P(shd), N(rs), P(G.out), L.stream_ptr()))
    what = f"smirk_conv_igemm_f16x3 1x1 {cin}->{cout} M {B * H * W}"
    _assert_close(_decode(G.check(what)), ref64(_decode(xs), w64, _decode(rs) if residual else None), CONV_TOL, what)


# ---- pooled linear head ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6, 55, 300])
@pytest.mark.parametrize("C", [8, 576, 960])
@pytest.mark.parametrize("HW", [1, 49, 50])
def test_gap_linear_vs_float64(HW, C, N):
    """global average pool + Linear, fp32 and split16 features: against float64 mean + Linear on the values read, bound 4 x the error of the same computation in
    torch-CPU fp32 + 1e-6 (the rule of test_encoder_error_budget_against_float64)"""
    from smirk_amd import _lib as L
    B = 3
    g = torch.Generator().manual_seed(HW * 10000 + C * 10 + N)
    feat = torch.randn(B, HW, C, generator=g).abs() * 3.0
    w = torch.randn(N, C, generator=g) / C ** 0.5
    bias = torch.randn(N, generator=g) * 0.1
    wd, bd = _dev(w), _dev(bias)
    P = L.ptr
    for split in (False, True):
        fd = _dev(_split_nhwc(feat)) if split else _dev(feat)
        f32 = _decode(fd.reshape(B, HW, 1, C)).float().reshape(B, HW, C) if split else feat
        ref = F.linear(f32.double().mean(1), w.double(), bias.double())
        e_cpu = float((F.linear(f32.mean(1), w, bias).double() - ref).abs().max())
        ws = torch.empty(B * C, device="cuda")
        G = _guarded((B, 1, 1, N), False)
        fn = L.lib().smirk_gap_linear_split16 if split else L.lib().smirk_gap_linear
        L.check(fn(P(fd), P(wd), P(bd), P(G.out), P(ws), B, HW, C, N, L.stream_ptr()))
        what = f"{'smirk_gap_linear_split16' if split else 'smirk_gap_linear'} HW {HW} C {C} N {N} (torch-CPU fp32 error {e_cpu:.3e})"
        _assert_close(G.check(what).cpu().double().reshape(B, 1, 1, N), ref.reshape(B, 1, 1, N), 4.0 * e_cpu + 1e-6, what)


# ---- ExpressionEncoder clamps ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 257])
def test_expression_clamps_bit_equal_to_torch(B):
    """eyelids clamp(0, 1), jaw[0] relu, jaw[1:] clamp(-0.2, 0.2), everything else untouched: bit-equal to the torch ops of the reference's ExpressionEncoder.forward
    run on the same device, with values exactly at 0, 1, +-0.2 and negative zero in every clamped column"""
    from smirk_amd import _lib as L
    n = 50
    g = torch.Generator().manual_seed(B)
    p = torch.randn(B, n + 5, generator=g)
    special = torch.tensor([0.0, 1.0, -0.0, -0.2, 0.2, 1.0 + 2.0 ** -23, -(2.0 ** -149), 0.2 + 2.0 ** -26, -0.2 - 2.0 ** -26, 2.0 ** -149, -1.0, 3.0])
    if B == 1:
        p[0, n:] = special[:5]
    else:
        for col in range(5):
            for k in range(len(special)):
                p[7 + col + 5 * k, n + col] = special[k]
    G = MC.Guarded(B, 1, 1, n + 5, nan_word=MC.NAN_WORD_F32)
    G.out.copy_(p.reshape(B, 1, 1, n + 5))
    src = G.out.clone().reshape(B, n + 5)
    want = src.clone()
    want[:, n:n + 2] = torch.clamp(src[..., n:n + 2], 0, 1)
    want[:, n + 2:] = torch.cat([F.relu(src[..., n + 2].unsqueeze(-1)), torch.clamp(src[..., n + 3:n + 5], -.2, .2)], dim=-1)
    L.check(L.lib().smirk_expression_clamps(L.ptr(G.out), B, n, L.stream_ptr()))
    got = G.check("smirk_expression_clamps").reshape(B, n + 5)
    diff = (got.view(torch.int32) != want.view(torch.int32)).nonzero().tolist()
    assert not diff, [(i, j, float(src[i, j]), float(got[i, j]), float(want[i, j])) for i, j in diff[:20]]
    assert torch.equal(got[:, :n].view(torch.int32), src[:, :n].view(torch.int32))


# ---- exact-fp32 encoder mode -------------------------------------------------------------------------------------------------------------------------------------
def test_exact_fp32_encoder_mode_against_float64(monkeypatch):
    """SMIRK_AMD_ENCODER_PRECISION=f32 (smirk_stem_conv_s2, smirk_dwconv3x3, smirk_conv_igemm_f32, smirk_gap_linear): the whole encoder under the error-budget
    rule of test_encoder_error_budget_against_float64"""
    import smirk_amd.smirk_encoder as SE
    monkeypatch.setattr(SE, "PRECISION", "f32")          # read per call, part of the pack key
    sd = M.synth_encoder_state_dict()
    m = SE.SmirkEncoder()
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    img = A.synth_images(2, seed=91)
    ref32 = M.SmirkEncoderRef(); ref32.load_state_dict(sd); ref32.eval()
    ref64 = M.SmirkEncoderRef(); ref64.load_state_dict(sd); ref64 = ref64.double().eval()
    with torch.no_grad():
        r64, r32, hip = ref64(img.double()), ref32(img), m(img.cuda())
    torch.cuda.synchronize()
    for enc in (m.pose_encoder, m.shape_encoder, m.expression_encoder):
        assert enc.encoder._split is False and enc.encoder._packed_key[0] == "f32"
    for k in VS_FP64:
        e_cpu = (r32[k].double() - r64[k]).abs().max().item()
        e_hip = (hip[k].cpu().double() - r64[k]).abs().max().item()
        print(f"OPS_VS_FP64 exact-fp32 encoder {k}: HIP {e_hip:.3e}  torch-CPU fp32 {e_cpu:.3e}  bound {min(4.0 * e_cpu + 2e-6, VS_FP64[k]):.3e}")
        assert e_hip <= 4.0 * e_cpu + 2e-6, (k, e_hip, e_cpu)
        assert e_hip < VS_FP64[k], (k, e_hip)
