"""Case table and float64 reference of the convolution dispatch (a plain module shared by tests/test_conv_cases_cpu.py and tests/test_conv_branches_gpu.py).

Every case is the smallest layer that reaches one branch of conv_dispatch_one / igemm_plan (csrc/conv.hip) at a geometry where that branch's index map can go wrong:
non-square images in both orientations for the specialised families (ring, patch, halo, ping-pong), ragged last tiles in M and N for the implicit GEMM, the descriptor
fields no caller uses (stride 2, pads other than (k - 1) / 2, scale without shift, residual with ReLU) and the ConvTranspose 2 x 2 scatter.  A case names the kernel
the f16x3 entry must launch for it (`prefix`, as the launch profiler records it), so a dispatch change cannot move a case off its branch unnoticed.

conv_ref64 is include/smirk_hip.h's paragraph on SmirkConvDesc written out with index arithmetic: it shares no code with torch.nn.functional, against which
tests/test_conv_cases_cpu.py proves it before it judges a kernel.  Nothing here touches a device."""
import collections
import functools
import zlib

import torch

Case = collections.namedtuple("Case", "id family B H W C0 C1 Cout k stride pad_t pad_l Ho Wo reflect convt epi env prefix f32_prefix")

# epilogue -> (scale, shift, residual, ReLU): out = act(conv * scale + shift + residual)
EPILOGUES = {
    "raw": (0, 0, 0, 0),
    "bn_relu": (1, 1, 0, 1),
    "shift": (0, 1, 0, 0),
    "scale": (1, 0, 0, 0),
    "shift_relu": (0, 1, 0, 1),
    "bn_res": (1, 1, 1, 0),            # the generator's residual blocks: conv + BatchNorm + skip, no activation
    "bn_res_relu": (1, 1, 1, 1),
    "res_relu": (0, 0, 1, 1),
}
NO_RESIDUAL = ("raw", "bn_relu", "shift", "scale", "shift_relu")
FAMILIES = ("ring", "patch_resident", "patch_streamed", "halo", "pingpong", "pingpong_forced", "igemm", "convt")
SPECIALISED = ("ring", "patch_resident", "patch_streamed", "halo", "pingpong")

CASES = []


def _add(family, geom, ch, prefix, k=3, epi="raw", reflect=False, stride=1, pad=None, out=None, env=(), convt=False, f32_prefix=None, tag=""):
    B, H, W = geom
    C0, C1, Cout = ch
    pt, pl = ((k - 1) // 2,) * 2 if pad is None else pad
    Ho, Wo = ((H + 2 * pt - k) // stride + 1, (W + 2 * pl - k) // stride + 1) if out is None else out
    cid = (f"{family}-{B}x{H}x{W}-{C0}+{C1}-{Cout}-k{k}" + (f"s{stride}" if stride != 1 else "") + (f"p{pt}{pl}" if pad is not None else "") +
           (f"o{Ho}x{Wo}" if out is not None else "") + ("-reflect" if reflect else "") + f"-{epi}" + (f"-{tag}" if tag else ""))
    assert all(c.id != cid for c in CASES), cid
    CASES.append(Case(cid, family, B, H, W, C0, C1, Cout, k, stride, pt, pl, Ho, Wo, bool(reflect), bool(convt), epi, tuple(env), prefix, f32_prefix))


# ---- ring (conv_ring.hip): Cout 64, or Cout 32 with >= 64 input channels; H, W multiples of 16, H >= 64 (W is not bounded below: one patch per row at W = 16) ----
RING_GEOMS = [(1, 64, 16), (2, 80, 48), (1, 64, 112)]
_ring_ch = [(32, 0, 64), (64, 64, 64), (32, 32, 32), (64, 0, 32)]
_ring_epi = ["raw", "bn_relu", "shift"]
for gi, geom in enumerate(RING_GEOMS):
    for ci, ch in enumerate(_ring_ch):
        _add("ring", geom, ch, f"conv3x3_ring_kernel<{ch[2] // 32}>", epi=_ring_epi[(gi + ci) % 3])

# ---- patch, weights resident in LDS (conv_patch.hip).  Cout 32 with one chunk: two single-stage workgroups per CU <1,1,16,1>; Cout 32 with two chunks: <1,2,16,1>;
#      Cout 64: <2,2,16,1>.  8, 16, 32: buffer-addressed halo DMA; 24, 40: pointer-addressed (use_buf = 0); (32, 8) and 40: a partial last chunk ----------------------
_patch_ch = [((8, 0, 32), "<1,1,16,1>"), ((16, 0, 64), "<2,2,16,1>"), ((24, 0, 32), "<1,1,16,1>"), ((40, 0, 32), "<1,2,16,1>"), ((32, 0, 32), "<1,1,16,1>"),
             ((32, 8, 32), "<1,2,16,1>"), ((24, 0, 64), "<2,2,16,1>")]
for gi, geom in enumerate(RING_GEOMS):
    for ci, (ch, inst) in enumerate(_patch_ch):
        _add("patch_resident", geom, ch, "conv3x3_patch_kernel" + inst, epi=_ring_epi[(gi + ci) % 3])
# (40 -> 64 does not fit LDS resident and is no whole number of chunks for the streamed kernel: the generic walk of the 128 x 64 tile on a large image)
_add("igemm", (1, 64, 16), (40, 0, 64), "conv_igemm_kernel<128,64,2,2,true,0>", epi="bn_relu", tag="patch_refuses")

# ---- patch, weights streamed (Cout 64, >= 128 input channels in whole chunks; 96 and 160: pointer-addressed) ----------------------------------------------------
for gi, geom in enumerate([(1, 64, 16), (2, 80, 48), (1, 64, 112)]):
    _add("patch_streamed", geom, (96, 32, 64), "conv3x3_patch_stream_kernel", epi=_ring_epi[gi % 3])
    _add("patch_streamed", geom, (160, 0, 64), "conv3x3_patch_stream_kernel", epi=_ring_epi[(gi + 1) % 3])
    _add("patch_streamed", geom, (128, 0, 64), "conv3x3_patch_stream_kernel", epi=_ring_epi[(gi + 2) % 3], env=(("SMIRK_CONV_RING", "0"),))

# ---- halo (conv_halo.hip): W <= 63, M >= 1024, N % 128 == 0.  NPA = ceil((256 + 2 (W + 1)) / 64): 5 up to W = 31, 6 above.  Every M below leaves a ragged
#      last 256-row tile; tiles straddle images; W = 2 and H = 2 make every pixel a border pixel --------------------------------------------------------------------
HALO_GEOMS = [(6, 14, 14), (3, 31, 12), (13, 40, 2), (19, 2, 31), (2, 17, 31), (2, 17, 32), (2, 9, 63)]
_halo_ch = [(32, 0, 128), (64, 32, 128), (32, 0, 256)]
_halo_epi = ["raw", "bn_relu", "bn_res", "bn_res_relu"]
for gi, geom in enumerate(HALO_GEOMS):
    for ri, reflect in enumerate((False, True)):
        n = 2 * gi + ri
        _add("halo", geom, _halo_ch[n % 3], f"conv_halo_kernel<{5 if geom[2] <= 31 else 6},0>", epi=_halo_epi[n % 4], reflect=reflect)
_add("halo", (3, 31, 12), (32, 0, 128), "conv_halo_kernel<5,0>", epi="raw", reflect=True)        # (a raw reflect case: the statistics epilogue under reflect)
_add("halo", (2, 17, 32), (64, 32, 128), "conv_halo_kernel<6,0>", epi="res_relu")

# ---- ping-pong as the dispatcher reaches it by default: too wide for the halo kernel (W >= 64), at most 256 pixels per image, M >= 1024 ------------------------------
_PP = "conv_pp_kernel<3>"
_add("pingpong", (8, 2, 64), (32, 0, 128), _PP, epi="raw")
_add("pingpong", (8, 2, 64), (64, 64, 128), _PP, epi="bn_res", reflect=True)
_add("pingpong", (4, 4, 64), (64, 64, 128), _PP, epi="bn_relu")
_add("pingpong", (4, 4, 64), (32, 0, 128), _PP, epi="bn_res_relu", reflect=True)
_add("pingpong", (4, 2, 128), (32, 0, 128), _PP, epi="bn_res")
_add("pingpong", (4, 2, 128), (64, 64, 128), _PP, epi="raw", reflect=True)
_add("pingpong", (5, 1, 256), (64, 64, 128), _PP, epi="bn_res_relu")
_add("pingpong", (5, 1, 256), (32, 0, 128), _PP, epi="raw")
_add("pingpong", (9, 2, 64), (32, 0, 256), _PP, epi="bn_relu", reflect=True)                     # ragged last tile (M = 1152), two N tiles
# ... and forced onto shapes the halo kernel takes by default (the only way to an H > W image on this kernel)
_PP_ENV = (("SMIRK_IGEMM_HALO", "0"), ("SMIRK_IGEMM_PP", "all"))
_add("pingpong_forced", (3, 31, 12), (64, 32, 128), _PP, epi="bn_res", reflect=True, env=_PP_ENV)
_add("pingpong_forced", (3, 31, 12), (32, 0, 128), _PP, epi="raw", env=_PP_ENV)
# two images that each fill the halo / ping-pong kernels' minimum of 1024 rows on their own: the batch-invariance cases of these two families
_add("halo", (2, 40, 31), (64, 32, 128), "conv_halo_kernel<5,0>", epi="bn_res", reflect=True)
_add("pingpong_forced", (2, 40, 31), (64, 32, 128), _PP, epi="bn_relu", env=_PP_ENV)

# ---- implicit GEMM: every (tile, K walk) tests/test_conv_dispatch_gpu.py records, at three tiny geometries (several images per tile, one pixel per image) ----
_G = "conv_igemm_kernel"
IGEMM_WALKS = [
    # (C0, C1, Cout), k, f16x3 instantiation, fp32 instantiation
    ((64, 0, 128), 3, "<128,128,2,2,true,5>", "<128,128,2,2,false,1>"),
    ((32, 32, 128), 3, "<128,128,2,2,true,5>", "<128,128,2,2,false,1>"),
    ((32, 0, 128), 3, "<128,128,2,2,true,4>", "<128,128,2,2,false,1>"),
    ((96, 0, 128), 3, "<128,128,2,2,true,4>", "<128,128,2,2,false,1>"),
    ((64, 0, 64), 3, "<128,64,2,2,true,4>", "<128,64,2,2,false,1>"),
    ((32, 0, 32), 3, "<256,32,4,1,true,4>", "<256,32,4,1,false,1>"),
    ((64, 0, 64), 1, "<128,64,2,2,true,4>", "<128,64,2,2,false,1>"),
    ((72, 0, 24), 1, "<256,32,4,1,true,2>", "<256,32,4,1,false,2>"),
    ((40, 0, 120), 1, "<128,128,2,2,true,2>", "<128,128,2,2,false,2>"),
    ((8, 0, 32), 3, "<256,32,4,1,true,0>", "<256,32,4,1,false,0>"),
    ((16, 0, 64), 3, "<128,64,2,2,true,0>", "<128,64,2,2,false,0>"),
]
IGEMM_GEOMS = [(1, 5, 7), (2, 9, 11), (3, 1, 1)]
_ig_epi = ["raw", "bn_relu", "scale", "bn_res_relu", "shift", "bn_res", "res_relu", "shift_relu"]
_n = 0
for ch, k, inst, inst32 in IGEMM_WALKS:
    for geom in IGEMM_GEOMS:
        _add("igemm", geom, ch, _G + inst, k=k, epi="raw" if geom == (2, 9, 11) else _ig_epi[_n % 8], f32_prefix=_G + inst32)
        _n += 1
        if k == 3 and geom[1] >= 2:
            _add("igemm", geom, ch, _G + inst, k=k, epi=_ig_epi[_n % 8], reflect=True, f32_prefix=_G + inst32)
            _n += 1
# ragged N: the last N tile of each tile shape is partly outside the weight tensor and the output
RAGGED_N = {72: "<128,128,2,2,true,4>", 136: "<128,128,2,2,true,4>", 40: "<128,64,2,2,true,4>", 8: "<256,32,4,1,true,4>", 24: "<256,32,4,1,true,4>"}
for _i, (cout, inst) in enumerate(RAGGED_N.items()):
    _add("igemm", (2, 9, 11), (32, 0, cout), _G + inst, epi=("raw", "bn_res_relu", "bn_relu", "scale", "raw")[_i], tag="raggedN")
_add("igemm", (2, 9, 11), (72, 0, 40), _G + "<128,64,2,2,true,2>", k=1, epi="bn_relu", tag="raggedN")
# two sources of different widths: an odd chunk count (buffer-addressed tap-major walk) and a second source that is no whole chunk (generic walk)
_add("igemm", (2, 9, 11), (64, 32, 128), _G + "<128,128,2,2,true,4>", epi="raw", tag="two_widths")
_add("igemm", (2, 9, 11), (64, 32, 128), _G + "<128,128,2,2,true,4>", epi="bn_res", reflect=True, tag="two_widths")
_add("igemm", (2, 9, 11), (32, 8, 32), _G + "<256,32,4,1,true,0>", epi="bn_relu", tag="two_widths")
_add("igemm", (2, 9, 11), (32, 8, 64), _G + "<128,64,2,2,true,0>", epi="raw", reflect=True, tag="two_widths")
# stride 2, 3 x 3, pad 1: (9, 7) -> (5, 4); the last tap ends exactly one pixel past the bottom / right edge, so reflect is legal.  One case per K walk
STRIDE2_3X3 = [((64, 0, 128), "<128,128,2,2,true,5>"), ((32, 0, 128), "<128,128,2,2,true,4>"), ((8, 0, 32), "<256,32,4,1,true,0>"), ((32, 0, 32), "<256,32,4,1,true,4>")]
for _i, (ch, inst) in enumerate(STRIDE2_3X3):
    _add("igemm", (2, 9, 7), ch, _G + inst, stride=2, epi=("raw", "bn_relu", "bn_res", "raw")[_i])
    _add("igemm", (2, 9, 7), ch, _G + inst, stride=2, epi=("bn_res_relu", "raw", "scale", "shift")[_i], reflect=True)
# stride 2, 1 x 1, pad 0 on the same input
_add("igemm", (2, 9, 7), (64, 0, 64), _G + "<128,64,2,2,true,4>", k=1, stride=2, epi="raw")
_add("igemm", (2, 9, 7), (40, 0, 120), _G + "<128,128,2,2,true,2>", k=1, stride=2, epi="bn_res_relu")
# stride 2 with no leading pad and a trailing pad implied by Ho, Wo (TensorFlow "same": (8, 6) -> (4, 3), the last tap one pixel past the edge)
_add("igemm", (2, 8, 6), (32, 0, 128), _G + "<128,128,2,2,true,4>", stride=2, pad=(0, 0), out=(4, 3), epi="raw")
_add("igemm", (2, 8, 6), (8, 0, 32), _G + "<256,32,4,1,true,0>", stride=2, pad=(0, 0), out=(4, 3), epi="bn_relu")
# 3 x 3 without padding (Ho = H - 2), and padding on one axis only
_add("igemm", (2, 9, 11), (64, 0, 128), _G + "<128,128,2,2,true,5>", pad=(0, 0), epi="raw")
_add("igemm", (2, 9, 11), (32, 0, 32), _G + "<256,32,4,1,true,4>", pad=(0, 0), epi="bn_res_relu")
_add("igemm", (2, 9, 11), (32, 0, 128), _G + "<128,128,2,2,true,4>", pad=(0, 1), epi="raw")
_add("igemm", (2, 9, 11), (8, 0, 32), _G + "<256,32,4,1,true,0>", pad=(1, 0), epi="shift_relu", reflect=True)

# ---- ConvTranspose2d(k = 2, s = 2) as a 1 x 1 GEMM with N = 4 Cout ordered (dy, dx, co) and a 2 x 2 pixel scatter; scale / shift are indexed by co ------------------
for geom in [(1, 3, 5), (2, 8, 8), (3, 7, 7)]:                      # M = 15 (one ragged tile), 128 (one whole tile), 147 (a whole and a ragged tile)
    for epi in ("raw", "shift_relu"):
        _add("convt", geom, (64, 0, 32), _G + "<128,128,2,2,true,4>", k=1, epi=epi, convt=True, f32_prefix=_G + "<128,128,2,2,false,1>")
_add("convt", (2, 5, 3), (32, 0, 40), _G + "<128,128,2,2,true,4>", k=1, epi="bn_relu", convt=True, tag="raggedN")      # N = 160: the second N tile is ragged

BY_ID = {c.id: c for c in CASES}


def igemm_name(c, split, x1=False):
    """the conv_igemm_kernel instantiation igemm_plan (csrc/conv.hip) chooses for the case's channels when no specialised family takes it, operands below 2 GiB:
    the N ladder of the tile, then the K walk.  tests/test_conv_cases_cpu.py holds this against every name tests/test_conv_dispatch_gpu.py recorded"""
    n = c.Cout * (4 if c.convt else 1)
    tile = "128,128,2,2" if n > 64 else "128,64,2,2" if n > 32 else "256,32,4,1"
    c32 = c.C0 % 32 == 0 and c.C1 % 32 == 0
    if split and c32:
        pow2 = c.C0 & (c.C0 - 1) == 0 and c.C1 & (c.C1 - 1) == 0
        walk = 5 if (n > 64 and c.k == 3 and pow2 and ((c.C0 + c.C1) // 32) % 2 == 0) else 4
    else:
        walk = 1 if c32 else 2 if c.k == 1 else 0
    return f"conv_igemm_kernel<{tile},{'true' if split else 'false'},{walk}>" + ("[f16x1]" if x1 else "")


def x1_prefix(c):
    """what the f16x1 entry launches: the halo family has a one-MFMA kernel of its own, every other specialised family leaves the case to the implicit GEMM"""
    if c.family == "halo":
        return c.prefix.replace("conv_halo_kernel<", "conv_halo_x1_kernel<").replace(",0>", ">")
    return igemm_name(c, True, True)

# ---- fused entries -------------------------------------------------------------------------------------------------------------------------------------------------
# smirk_conv3x3_pool_f16x3: (B, H, W, C0, C1), Cout = 64, BatchNorm + ReLU epilogue as the generator's encoder blocks
POOL_CASES = [(1, 64, 16, 32, 0), (2, 80, 48, 64, 64), (1, 64, 112, 32, 0), (2, 80, 48, 32, 0)]
# smirk_conv3x3_tail_f16x3: (B, H, W, C0, C1, fcout), Cout = 32
TAIL_CASES = [(B, H, W, C0, C1, f) for (B, H, W) in ((1, 64, 16), (2, 80, 48)) for (C0, C1) in ((32, 0), (32, 32)) for f in (1, 3, 4)]
# one case per specialised family on a non-square geometry with B > 1 whose image b must equal the same image run alone, bit for bit; the image alone stays on the
# case's kernel (tests/test_conv_cases_cpu.py checks the list against the table)
BATCH_INVARIANT = [next(c.id for c in CASES if c.family == f and c.B == 2 and (c.H, c.W) == hw and (c.C0, c.C1) == ch)
                   for f, hw, ch in (("ring", (80, 48), (64, 64)), ("patch_resident", (80, 48), (32, 8)), ("patch_streamed", (80, 48), (96, 32)),
                                     ("halo", (40, 31), (64, 32)), ("pingpong_forced", (40, 31), (64, 32)))]


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------------------------
def case_seed(c):
    return zlib.crc32(c.id.encode())


def split16_act(t):
    """fp32 NHWC -> split16 NHWC (float32-typed storage), on the CPU"""
    from smirk_amd.smirk_generator import _split16
    return _split16(t.reshape(-1, t.shape[-1]).contiguous()).reshape(t.shape)


def decode(s):
    """split16 [..., C] -> the values it carries (hi + lo / 2048), float32 (exact: the kernels' own join)"""
    h = s.contiguous().view(torch.float16).reshape(*s.shape[:-1], s.shape[-1] // 8, 2, 8).float()
    return (h[..., 0, :] + h[..., 1, :] / 2048.0).reshape(s.shape)


def decode_hi(s):
    """split16 [..., C] -> its hi halves alone (what the f16x1 product multiplies), float32"""
    h = s.contiguous().view(torch.float16).reshape(*s.shape[:-1], s.shape[-1] // 8, 2, 8).float()
    return h[..., 0, :].reshape(s.shape)


Operands = collections.namedtuple("Operands", "x0 x1 w scale shift res")      # split16 x0, x1, w, res (CPU); fp32 scale, shift


def make_operands(c, seed=None):
    """seeded normals: weights x 0.05, scale in [0.5, 1.5]; converted to split16 ONCE, here"""
    from smirk_amd.smirk_generator import _split16
    g = torch.Generator().manual_seed(case_seed(c) if seed is None else seed)
    sc, sh, rs, _ = EPILOGUES[c.epi]
    n = c.Cout * (4 if c.convt else 1)
    x0 = split16_act(torch.randn(c.B, c.H, c.W, c.C0, generator=g))
    x1 = split16_act(torch.randn(c.B, c.H, c.W, c.C1, generator=g)) if c.C1 else None
    w = _split16(torch.randn(n, c.k * c.k * (c.C0 + c.C1), generator=g) * 0.05)
    scale = (torch.rand(c.Cout, generator=g) + 0.5) if sc else None
    shift = torch.randn(c.Cout, generator=g) if sh else None
    res = split16_act(torch.randn(*out_shape(c), generator=g)) if rs else None
    return Operands(x0, x1, w, scale, shift, res)


@functools.lru_cache(maxsize=None)
def operands_of(cid):
    return make_operands(BY_ID[cid])


def out_shape(c):
    return (c.B, 2 * c.Ho, 2 * c.Wo, c.Cout) if c.convt else (c.B, c.Ho, c.Wo, c.Cout)


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------------------------------------
def _taps(n_out, stride, pad, k, n_in, reflect):
    """for tap t: (clamped input index of every output index, validity mask).  index = o * stride - pad + t; reflect folds ONE pixel at either end"""
    o = torch.arange(n_out)
    res = []
    for t in range(k):
        i = o * stride - pad + t
        if reflect:
            assert int(i.min()) >= -1 and int(i.max()) <= n_in and n_in >= 2, "reflect padding reaches one pixel"
            i = torch.where(i < 0, -i, i)
            i = torch.where(i >= n_in, 2 * n_in - 2 - i, i)
            ok = torch.ones(n_out, dtype=torch.bool)
        else:
            ok = (i >= 0) & (i < n_in)
        res.append((i.clamp(0, n_in - 1), ok))
    return res


def conv_ref64(x, w, k, stride, pad_t, pad_l, Ho, Wo, reflect, convt=False, scale=None, shift=None, res=None, relu=False):
    """x [B][H][W][Cin] (the channel concat of the sources), w [N][k * k * Cin] ordered (ky, kx, c) -> float64 NHWC output.
    convt: k = 1, N = 4 Cout ordered (dy, dx, co), out[b][2 y + dy][2 x + dx][co]"""
    x, w = x.double(), w.double()
    B, H, W, Cin = x.shape
    N = w.shape[0]
    assert w.shape[1] == k * k * Cin
    wt = w.reshape(N, k, k, Cin)
    rows, cols = _taps(Ho, stride, pad_t, k, H, reflect), _taps(Wo, stride, pad_l, k, W, reflect)
    out = torch.zeros(B, Ho, Wo, N, dtype=torch.float64)
    for ky, (iy, oky) in enumerate(rows):
        for kx, (ix, okx) in enumerate(cols):
            patch = x[:, iy][:, :, ix] * (oky[:, None] & okx[None, :])[None, :, :, None]
            out += patch @ wt[:, ky, kx, :].T
    if convt:
        assert k == 1 and N % 4 == 0
        co = N // 4
        out = out.reshape(B, Ho, Wo, 2, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ho, 2 * Wo, co)
    if scale is not None:
        out = out * scale.double()
    if shift is not None:
        out = out + shift.double()
    if res is not None:
        out = out + res.double()
    return out.clamp_min(0.0) if relu else out


def reference(c, ops, hi_only=False):
    """float64 result of case c on the exactly representable values of its converted operands (hi_only: the f16x1 product, which multiplies the hi halves of the
    activations and weights; the residual enters the epilogue whole in either mode)"""
    dec = decode_hi if hi_only else decode
    x = dec(ops.x0) if ops.x1 is None else torch.cat([dec(ops.x0), dec(ops.x1)], -1)
    relu = bool(EPILOGUES[c.epi][3])
    return conv_ref64(x, dec(ops.w), c.k, c.stride, c.pad_t, c.pad_l, c.Ho, c.Wo, c.reflect, c.convt, ops.scale, ops.shift,
                      None if ops.res is None else decode(ops.res), relu)


@functools.lru_cache(maxsize=None)
def reference_of(cid, hi_only=False):
    return reference(BY_ID[cid], operands_of(cid), hi_only)


def tail_ref64(y, fw, fb):
    """the generator's tail on the float64 NHWC activation y: 1 x 1 conv fw [fcout][C] + fb, sigmoid -> NCHW"""
    z = y @ fw.double().T + fb.double()
    return torch.sigmoid(z).permute(0, 3, 1, 2).contiguous()


def maxpool_ref64(y):
    """2 x 2 / 2 max-pool of a float64 NHWC tensor with even H, W"""
    B, H, W, C = y.shape
    return y.reshape(B, H // 2, 2, W // 2, 2, C).amax(dim=(2, 4))
