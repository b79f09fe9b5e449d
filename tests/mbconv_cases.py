"""Per-block harness for the encoder's MBConv kernels (a plain module shared by tests/test_mbconv_block_gpu.py and tests/test_mbconv_cases_cpu.py).

One timm "minimal" block, seeded, small, with a torch float64 reference on the operands' exact split16 values and three ways of running it on the device:

    run_fused    smirk_mbconv_fused_split16            csrc/mbconv.hip        8x8 (stride 1) / 4x8 (stride 2) output tiles
    run_image    smirk_mbconv_image_split16            csrc/mbconv_image.hip  where smirk_mbconv_image_supported
    run_unfused  1x1 igemm -> depthwise -> 1x1 igemm   the launch sequence of smirk_backbone_forward for a block no fused kernel serves

Every runner writes into the middle of a larger device buffer: the output region is pre-filled with fp16 NaNs (an element the kernel never stores decodes to
NaN) and is fenced by guard bands of a fixed bit pattern that must come back bitwise untouched (a stray store inside memory the test owns is reported).
Everything above the runners is CPU-only and holds no device code: the case table can be inspected without a GPU."""
import collections
import functools
import zlib

import torch

Case = collections.namedtuple("Case", "cin mid cout stride kind B H W residual")
Block = collections.namedtuple("Block", "case x xs we wes wd wp wps aff")

GUARD_WORD = 0x5A5AA5A5          # guard bands (int32 words)
NAN_WORD = 0x7E007E00            # two fp16 quiet NaNs: every half of the pre-filled output region is a NaN, whichever of hi / lo it becomes
NAN_WORD_F32 = 0x7FC00000        # the same for a plain fp32 output


def case_id(c):
    return f"{c.kind}{c.cin}-{c.mid}-{c.cout}_s{c.stride}_{c.B}x{c.H}x{c.W}{'_res' if c.residual else ''}"


def case_seed(c):
    return zlib.crc32(case_id(c).encode())


def kernel_variant(c):
    """(S, EXP, KS) of the mbconv_fused_kernel instantiation that serves the case: KS = 16-wide k-steps of the expand GEMM = ceil(Cin / 16)"""
    return (c.stride, c.kind == "ir", (c.cin + 15) // 16)


def make_block(cin, mid, cout, stride, kind, B, H, W, seed, residual=False):
    """Seeded operands of one block, scaled as in test_mbconv_image_kernel_vs_float64 (activations stay O(1 - 10)): kind "ir" = InvertedResidual (expand,
    depthwise, project), kind "ds" = DepthwiseSeparable (mid == cin, no expand).  CPU tensors; `xs`, `wes`, `wps` are the split16 encodings the kernels read."""
    from smirk_amd.smirk_generator import _split16
    assert kind in ("ir", "ds") and (kind == "ir" or mid == cin)
    assert not residual or (stride == 1 and cin == cout)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g)
    we = torch.randn(mid, cin, generator=g) * (1.5 / cin ** 0.5) if kind == "ir" else None
    wd = torch.randn(mid, 3, 3, generator=g) * 0.4
    wp = torch.randn(cout, mid, generator=g) * (1.5 / mid ** 0.5)
    aff = [(torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.2) for n in (mid, mid, cout)]
    if kind == "ds":
        aff[0] = None
    xs = _split16(x.reshape(-1, cin)).reshape(B, H, W, cin)
    wes = _split16(we.contiguous()) if kind == "ir" else None
    wps = _split16(wp.contiguous())
    return Block(Case(cin, mid, cout, stride, kind, B, H, W, bool(residual)), x, xs, we, wes, wd, wp, wps, aff)


@functools.lru_cache(maxsize=None)
def block_of(case):
    return make_block(*case[:8], seed=case_seed(case), residual=case.residual)


def decoded(block):
    """float64 values the kernels actually see: x NCHW, wexp [mid][cin] (None for "ds"), wproj [cout][mid], decoded from the split16 encodings"""
    from smirk_amd.smirk_generator import split16_to_float
    c = block.case
    x64 = split16_to_float(block.xs).double().permute(0, 3, 1, 2)
    we64 = split16_to_float(block.wes.reshape(1, 1, c.mid, c.cin)).reshape(c.mid, c.cin).double() if c.kind == "ir" else None
    wp64 = split16_to_float(block.wps.reshape(1, 1, c.cout, c.mid)).reshape(c.cout, c.mid).double()
    return x64, we64, wp64


def reference64(block):
    """torch float64 evaluation of the block on the exact split16 values of x, wexp and wproj -> NHWC [B][Ho][Wo][cout].  Plain F.conv2d; the depthwise
    convolution's TF-SAME padding is oracle.mobilenet_ref.Conv2dSame's (at stride 1 it pads 1 / 1, at stride 2 by the parity of the input size)."""
    import torch.nn.functional as F
    from oracle.mobilenet_ref import Conv2dSame
    c = block.case
    x64, we64, wp64 = decoded(block)
    bc = lambda t: t.double()[None, :, None, None]
    with torch.no_grad():
        e = x64
        if c.kind == "ir":
            e = F.relu(F.conv2d(x64, we64[:, :, None, None]) * bc(block.aff[0][0]) + bc(block.aff[0][1]))
        dw = Conv2dSame(c.mid, c.mid, 3, c.stride, 0, groups=c.mid, bias=False).double()
        dw.weight.copy_(block.wd.double()[:, None])
        d = F.relu(dw(e) * bc(block.aff[1][0]) + bc(block.aff[1][1]))
        ref = F.conv2d(d, wp64[:, :, None, None]) * bc(block.aff[2][0]) + bc(block.aff[2][1])
        if c.residual:
            ref = ref + x64
    return ref.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def reference_of(case):
    """computed once per case and shared (callers must not modify it)"""
    return reference64(block_of(case))


def where(err, tol):
    """'' when err (NHWC, non-negative; NaN counts as over) is below tol everywhere, otherwise the distinct b / y / x / c indices over it (40 each at most)"""
    bad = ~(err < tol)
    if not bool(bad.any()):
        return ""
    idx = bad.nonzero()
    parts = [f"{int(bad.sum())} of {bad.numel()} elements over {tol:.3e} (max {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e})"]
    for k, name in enumerate("byxc"):
        u = torch.unique(idx[:, k]).tolist()
        parts.append(f"{name}={u[:40]}{' ...' if len(u) > 40 else ''}")
    return "  ".join(parts)


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------------------
# A tile is 8 x 8 outputs at stride 1 and 4 rows x 8 columns at stride 2 (9 x 17 input halo): the geometries are the smallest that reach each edge.
GEOM_S1 = [(8, 8),       # one tile, every halo pixel outside the image
           (9, 17),      # one-pixel remainder on both axes
           (5, 3),       # smaller than a tile
           (16, 24)]     # interior tiles whose halo is real data
GEOM_S2 = [(16, 16),     # even: leading pad 0
           (15, 17),     # odd: leading pad 1
           (10, 13),     # mixed parity
           (7, 9),
           (1, 1)]


def _table():
    T = []
    add = lambda *a, res=False: T.append(Case(*a, bool(res)))
    # geometry x one block of each kind (mid 88: not a multiple of the 32-channel chunk), B = 1 .. 3
    for i, (h, w) in enumerate(GEOM_S1):
        add(24, 88, 24, 1, "ir", 1 + i % 3, h, w, res=True)
        add(24, 24, 24, 1, "ds", 1 + (i + 1) % 3, h, w, res=True)
    for i, (h, w) in enumerate(GEOM_S2):
        add(24, 88, 40, 2, "ir", 1 + i % 3, h, w)
        add(24, 24, 40, 2, "ds", 1 + (i + 1) % 3, h, w)
    # channels, stride 1 (9 x 17: ragged tiles on both axes; 16 x 24: interior tiles).  Cin 8 (half of the first 16-wide k-step is padding) .. 48 = KS 1 .. 3,
    # mid below one chunk / ragged / several chunks, Cout 8 .. 96 (96: 6 project tiles over 4 waves), residual on and off
    add(8, 8, 8, 1, "ir", 2, 9, 17, res=True)
    add(8, 8, 8, 1, "ir", 1, 9, 17)
    add(8, 72, 40, 1, "ir", 3, 9, 17)
    add(16, 64, 16, 1, "ir", 2, 9, 17, res=True)
    add(16, 120, 8, 1, "ir", 1, 16, 24)
    add(16, 104, 96, 1, "ir", 3, 9, 17)
    add(24, 104, 72, 1, "ir", 2, 9, 17)
    add(24, 192, 96, 1, "ir", 1, 16, 24)
    add(40, 8, 40, 1, "ir", 3, 9, 17, res=True)
    add(40, 88, 72, 1, "ir", 2, 16, 24)
    add(48, 72, 48, 1, "ir", 1, 9, 17)
    add(48, 96, 96, 1, "ir", 2, 9, 17)
    # channels, stride 2 (15 x 17 / 10 x 13); Cin 40 - 48 fits the LDS budget up to mid 96 only
    add(8, 8, 8, 2, "ir", 2, 15, 17)
    add(8, 104, 24, 2, "ir", 1, 10, 13)
    add(16, 120, 96, 2, "ir", 3, 15, 17)
    add(24, 72, 8, 2, "ir", 2, 10, 13)
    add(24, 256, 72, 2, "ir", 1, 15, 17)
    add(40, 88, 72, 2, "ir", 3, 10, 13)
    add(40, 8, 24, 2, "ir", 1, 15, 17)
    add(48, 72, 96, 2, "ir", 2, 15, 17)
    add(48, 96, 40, 2, "ir", 3, 10, 13)
    # the block shapes the product runs on this kernel: large backbone 16-64-24 s2, 24-72-40 s2; small backbone 16-72-24 s2, 24-96-40 s2
    add(16, 64, 24, 2, "ir", 2, 15, 17)
    add(24, 72, 40, 2, "ir", 3, 16, 16)
    add(16, 72, 24, 2, "ir", 2, 10, 13)
    add(24, 96, 40, 2, "ir", 1, 15, 17)
    # the stride-1 shapes it takes over from the halo-tiled kernel under SMIRK_DISABLE_MBCONV_TILE (40-240-40: see UNSUPPORTED_PRODUCT_SHAPES)
    add(24, 72, 24, 1, "ir", 2, 16, 24, res=True)
    add(24, 88, 24, 1, "ir", 3, 9, 17)
    add(40, 120, 40, 1, "ir", 2, 9, 17, res=True)
    add(40, 120, 48, 1, "ir", 1, 16, 24)
    add(48, 144, 48, 1, "ir", 3, 9, 17, res=True)
    # wexp == NULL (DepthwiseSeparable, the EXP = false instantiations): Cin = mid 8 .. 48, both strides, residual where legal; incl. the backbones' first blocks
    for i, cm in enumerate((8, 16, 24, 40, 48)):
        add(cm, cm, cm, 1, "ds", 1 + (i + 2) % 3, 9, 17, res=True)
        add(cm, cm, (24, 96, 8, 72, 40)[i], 1, "ds", 1 + (i + 1) % 3, 16, 24)
        add(cm, cm, (16, 40, 72, 8, 96)[i], 2, "ds", 1 + i % 3, (15, 10)[i % 2], (17, 13)[i % 2])
    add(16, 16, 16, 2, "ds", 2, 16, 16)
    add(40, 40, 40, 1, "ds", 2, 8, 8)               # Cin == Cout at stride 1 with the residual off
    assert len(set(T)) == len(T)
    return T


CASES_FUSED = _table()
# batch invariance / determinism: one stride-1 (residual, KS = 3) and one stride-2 case of the table with B = 3, ragged tiles on both axes
BATCH_CASES = [Case(48, 144, 48, 1, "ir", 3, 9, 17, True), Case(40, 88, 72, 2, "ir", 3, 10, 13, False)]

# 40 -> 240 -> 40 stride 1 (both 28 x 28 blocks of the small backbone) is listed among the shapes that run on this kernel under SMIRK_DISABLE_MBCONV_TILE, but
# smirk_mbconv_supported refuses it: 65664 bytes of LDS against the 65536 budget (midp = 256 -> 13 312 bytes of depthwise / BN constants).  With the switch set the
# backbone runs these two blocks unfused.  The GPU test asserts the refusal and holds the other two runners to float64 on this shape.
UNSUPPORTED_PRODUCT_SHAPES = [Case(40, 240, 40, 1, "ir", 2, 9, 17, True)]


def arch_block_shapes():
    """every (cin, mid, cout, stride, kind) DepthwiseSeparable / InvertedResidual block of the two backbones, from smirk_amd.smirk_encoder's architecture table"""
    from smirk_amd.smirk_encoder import _ARCH, MobileNetV3Features
    out = []
    for name in _ARCH:
        for stage in MobileNetV3Features(name).blocks:
            for blk in stage:
                if blk.kind == "ds":
                    out.append((blk.conv_dw.in_channels, blk.conv_dw.in_channels, blk.conv_pw.out_channels, blk.stride, "ds"))
                elif blk.kind == "ir":
                    out.append((blk.conv_pw.in_channels, blk.conv_pw.out_channels, blk.conv_pwl.out_channels, blk.stride, "ir"))
    return sorted(set(out))


def lds_limit_mid(lib, stride, cin, cout=96):
    """the largest mid (a multiple of 8) smirk_mbconv_supported accepts for this (stride, Cin, Cout): asked of the library, not written down"""
    ok = [m for m in range(8, 4096, 8) if lib.smirk_mbconv_supported(cin, m, cout, stride)]
    assert ok, (stride, cin, cout)
    return max(ok)


# ---- device side ---------------------------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """[guard | output region | guard] in one device allocation: `out` is the float32-typed [B][Ho][Wo][cout] view the kernel writes"""

    def __init__(self, B, Ho, Wo, cout, nan_word=NAN_WORD):
        n = B * Ho * Wo * cout
        self.g = g = (max(Wo * cout, 1) + 63) // 64 * 64           # >= one output row, keeps the region 256-byte aligned
        self.buf = torch.full((g + n + g,), GUARD_WORD, dtype=torch.int32, device="cuda")
        self.buf[g:g + n] = nan_word
        self.out = self.buf[g:g + n].view(torch.float32).view(B, Ho, Wo, cout)

    def check(self, what):
        torch.cuda.synchronize()
        g = self.g
        for name, band in (("before", self.buf[:g]), ("after", self.buf[-g:])):
            bad = (band != GUARD_WORD).nonzero().flatten()
            assert bad.numel() == 0, f"{what}: {bad.numel()} guard words {name} the output were overwritten, first at word {int(bad[0])} of {g}"
        return self.out


def untouched(out):
    """True when the region still holds its NaN pre-fill bit for bit (nothing was launched)"""
    return bool((out.contiguous().view(torch.int32) == NAN_WORD).all())


def _dev(t):
    return None if t is None else t.float().contiguous().cuda()


def _operands(block):
    """device operands in the order of the smirk_mbconv_*_split16 argument lists: x, wexp, s1, b1, wdw [9][mid], s2, b2, wproj, s3, b3"""
    a = block.aff
    c = block.case
    return [_dev(block.xs), _dev(block.wes), _dev(a[0][0]) if a[0] else None, _dev(a[0][1]) if a[0] else None, _dev(block.wd.reshape(c.mid, 9).t()),
            _dev(a[1][0]), _dev(a[1][1]), _dev(block.wps), _dev(a[2][0]), _dev(a[2][1])]


def _out_hw(c):
    return (c.H + c.stride - 1) // c.stride, (c.W + c.stride - 1) // c.stride


def call_fused(block, out, residual=None):
    """the raw return code of smirk_mbconv_fused_split16 writing to `out`"""
    from smirk_amd import _lib as L
    c = block.case
    N = lambda t: L.ptr(t, allow_none=True)
    t = _operands(block)
    res = c.residual if residual is None else residual
    code = L.lib().smirk_mbconv_fused_split16(*[N(v) for v in t], int(res), L.ptr(out), c.B, c.H, c.W, c.cin, c.mid, c.cout, c.stride, L.stream_ptr())
    torch.cuda.synchronize()
    return code


def run_fused(block):
    from smirk_amd import _lib as L
    c = block.case
    G = Guarded(c.B, *_out_hw(c), c.cout)
    L.check(call_fused(block, G.out))
    return G.check("smirk_mbconv_fused_split16 " + case_id(c))


def image_supported(c):
    from smirk_amd import _lib as L
    return c.kind == "ir" and c.stride == 1 and bool(L.lib().smirk_mbconv_image_supported(c.H, c.W, c.cin, c.mid, c.cout, 1))


def run_image(block):
    from smirk_amd import _lib as L
    c = block.case
    assert image_supported(c)
    G = Guarded(c.B, c.H, c.W, c.cout)
    t = _operands(block)
    L.check(L.lib().smirk_mbconv_image_split16(*[L.ptr(v) for v in t], int(c.residual), L.ptr(G.out), c.B, c.H, c.W, c.cin, c.mid, c.cout, L.stream_ptr()))
    return G.check("smirk_mbconv_image_split16 " + case_id(c))


def pointwise_f16x3(x, w, scale, shift, relu, residual, out):
    """1 x 1 smirk_conv_igemm_f16x3 on split16 NHWC `x` -> `out`"""
    from smirk_amd import _lib as L
    B, H, W, C = x.shape
    d = L.SmirkConvDesc()
    d.B, d.H, d.W, d.C0, d.C1, d.Cout = B, H, W, C, 0, w.shape[0]
    d.KH = d.KW = d.stride = 1
    d.pad_t = d.pad_l = 0
    d.Ho, d.Wo, d.pad_mode = H, W, L.PAD_ZERO
    d.act, d.out_mode = (L.ACT_RELU if relu else L.ACT_NONE), L.OUT_NHWC
    P = L.ptr
    L.check(L.lib().smirk_conv_igemm_f16x3(d, P(x), None, P(w), P(scale), P(shift), P(residual, allow_none=True), P(out), L.stream_ptr()))


def run_unfused(block):
    """pointwise + BN + ReLU -> depthwise + BN + ReLU -> pointwise + BN (+ x): what smirk_backbone_forward issues for a block no fused kernel serves"""
    from smirk_amd import _lib as L
    c = block.case
    Ho, Wo = _out_hw(c)
    x, we, s1, b1, wd, s2, b2, wp, s3, b3 = _operands(block)
    G = Guarded(c.B, Ho, Wo, c.cout)
    e = x
    if c.kind == "ir":
        e = torch.empty(c.B, c.H, c.W, c.mid, device="cuda")
        pointwise_f16x3(x, we, s1, b1, True, None, e)
    d = torch.empty(c.B, Ho, Wo, c.mid, device="cuda")
    P = L.ptr
    L.check(L.lib().smirk_dwconv3x3_split16(P(e), P(wd), P(s2), P(b2), P(d), c.B, c.H, c.W, c.mid, c.stride, 1, L.stream_ptr()))
    pointwise_f16x3(d, wp, s3, b3, False, x if c.residual else None, G.out)
    return G.check("unfused launch sequence " + case_id(c))


def errors(out, case):
    """|decoded split16 output - float64 reference| (NHWC, float64; NaN where an element was never written) and the reference's max |value|"""
    from smirk_amd.smirk_generator import split16_to_float
    ref = reference_of(case)
    got = split16_to_float(out).cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs(), float(ref.abs().max())
