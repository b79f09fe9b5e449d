"""The convolution branch table (tests/conv_cases.py) checked where no GPU is needed: that it covers every kernel family, orientation, epilogue, stride form and ragged
tile the dispatcher can be wrong at (so a later edit cannot thin it silently), and that its float64 reference equals torch.nn.functional composed independently."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC

CASES = CC.CASES


def _of(family):
    fams = (family,) if isinstance(family, str) else family
    return [c for c in CASES if c.family in fams]


# ---- (a) coverage --------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_family_is_in_the_table_and_ids_are_unique():
    assert {c.family for c in CASES} == set(CC.FAMILIES)
    assert len({c.id for c in CASES}) == len(CASES)
    for c in CASES:
        assert c.epi in CC.EPILOGUES and c.prefix
        assert c.C0 % 8 == 0 and c.C1 % 8 == 0 and c.Cout % 8 == 0 and c.C0 > 0
        assert not c.reflect or (c.H >= 2 and c.W >= 2 and c.pad_t <= 1 and c.pad_l <= 1)
        # a case stays small: the float64 reference of the largest one is ~1.5 GFLOP on the host
        assert 2 * c.B * c.Ho * c.Wo * c.Cout * (4 if c.convt else 1) * c.k * c.k * (c.C0 + c.C1) < 2e9, c.id


@pytest.mark.parametrize("family", ["ring", "patch_resident", "patch_streamed", "halo", ("pingpong", "pingpong_forced")])
def test_every_specialised_family_runs_wide_and_tall_images(family):
    cs = _of(family)
    assert any(c.H < c.W for c in cs) and any(c.H > c.W for c in cs), family
    assert any(c.B > 1 for c in cs)


def test_the_seeded_branches_of_each_family_are_present():
    def has(family, geom, ch, **kw):
        return any((c.B, c.H, c.W) == geom and (c.C0, c.C1, c.Cout) == ch and all(getattr(c, k) == v for k, v in kw.items()) for c in _of(family))
    for geom in [(1, 64, 16), (2, 80, 48), (1, 64, 112)]:
        for ch in [(32, 0, 64), (64, 64, 64), (32, 32, 32), (64, 0, 32)]:
            assert has("ring", geom, ch, prefix=f"conv3x3_ring_kernel<{ch[2] // 32}>")
        for ch in [(8, 0, 32), (16, 0, 64), (24, 0, 32), (32, 0, 32), (32, 8, 32)]:
            assert has("patch_resident", geom, ch)
    for geom in [(1, 64, 16), (2, 80, 48)]:
        assert has("patch_streamed", geom, (96, 32, 64)) and has("patch_streamed", geom, (160, 0, 64))
        assert has("patch_streamed", geom, (128, 0, 64), env=(("SMIRK_CONV_RING", "0"),))
    assert {c.prefix for c in _of("patch_resident")} >= {"conv3x3_patch_kernel<1,1,16,1>", "conv3x3_patch_kernel<2,2,16,1>"}
    assert {c.epi for c in _of("ring")} >= {"raw", "bn_relu", "shift"}
    # pointer-addressed patch kernels: a channel count that is no power of two, resident and streamed
    assert any(c.C0 & (c.C0 - 1) for c in _of("patch_resident")) and any(c.C0 & (c.C0 - 1) for c in _of("patch_streamed"))
    # halo: every geometry under both paddings; both NPA instantiations; a ragged last 256-row tile in at least half of the cases; M >= 1024
    halo = _of("halo")
    for geom in CC.HALO_GEOMS:
        assert {c.reflect for c in halo if (c.B, c.H, c.W) == geom} == {False, True}, geom
    assert CC.HALO_GEOMS == [(6, 14, 14), (3, 31, 12), (13, 40, 2), (19, 2, 31), (2, 17, 31), (2, 17, 32), (2, 9, 63)]
    assert {c.prefix for c in halo} == {"conv_halo_kernel<5,0>", "conv_halo_kernel<6,0>"}
    assert {(c.C0, c.C1, c.Cout) for c in halo} == {(32, 0, 128), (64, 32, 128), (32, 0, 256)}
    assert {c.epi for c in halo} >= {"raw", "bn_relu", "bn_res", "bn_res_relu"}
    assert all(c.B * c.H * c.W >= 1024 and c.W <= 63 for c in halo)
    assert 2 * sum((c.B * c.H * c.W) % 256 != 0 for c in halo) >= len(halo)
    for c in halo:
        assert c.prefix == f"conv_halo_kernel<{(256 + 2 * (c.W + 1) + 63) // 64},0>"
    # ping-pong by default: W >= 64 and at most 256 pixels per image, so H is 1 to 4
    pp = _of("pingpong")
    for geom in [(8, 2, 64), (4, 4, 64), (4, 2, 128), (5, 1, 256)]:
        assert any((c.B, c.H, c.W) == geom for c in pp)
    assert all(c.W >= 64 and c.H * c.W <= 256 and c.B * c.H * c.W >= 1024 and not c.env for c in pp)
    assert all(not c.reflect for c in pp if c.H == 1) and any(c.reflect and c.H == 2 for c in pp)
    assert {(c.C0, c.C1, c.Cout) for c in pp} >= {(32, 0, 128), (64, 64, 128)}
    assert any((c.B, c.H, c.W) == (3, 31, 12) and dict(c.env) == {"SMIRK_IGEMM_HALO": "0", "SMIRK_IGEMM_PP": "all"} for c in _of("pingpong_forced"))
    # implicit GEMM: every recorded (tile, walk) at the three tiny geometries, reflect where it is legal
    ig = _of("igemm")
    for ch, k, inst, inst32 in CC.IGEMM_WALKS:
        for geom in CC.IGEMM_GEOMS:
            mine = [c for c in ig if (c.B, c.H, c.W) == geom and (c.C0, c.C1, c.Cout, c.k) == ch + (k,) and c.stride == 1 and c.pad_t == c.pad_l == (k - 1) // 2]
            assert {c.reflect for c in mine} == ({False, True} if k == 3 and geom[1] >= 2 else {False}), (ch, geom)
            assert all(c.prefix == "conv_igemm_kernel" + inst and c.f32_prefix == "conv_igemm_kernel" + inst32 for c in mine)
    assert {c.prefix[len("conv_igemm_kernel"):] for c in ig} >= {"<128,128,2,2,true,5>", "<128,128,2,2,true,4>", "<128,128,2,2,true,2>", "<128,64,2,2,true,4>",
                                                                "<128,64,2,2,true,0>", "<256,32,4,1,true,4>", "<256,32,4,1,true,2>", "<256,32,4,1,true,0>"}
    assert {c.f32_prefix[len("conv_igemm_kernel"):] for c in ig if c.f32_prefix} >= {"<128,128,2,2,false,1>", "<128,128,2,2,false,2>", "<256,32,4,1,false,0>"}
    assert any(c.C1 and c.C0 != c.C1 for c in ig)
    # ConvTranspose scatter
    ct = _of("convt")
    for geom in [(1, 3, 5), (2, 8, 8)]:
        assert {c.epi for c in ct if (c.B, c.H, c.W, c.C0, c.Cout) == geom + (64, 32)} == {"raw", "shift_relu"}
    assert all(c.convt and c.k == 1 and c.stride == 1 and c.C1 == 0 and (c.Ho, c.Wo) == (c.H, c.W) for c in ct)
    assert any((c.B * c.H * c.W) % 128 for c in ct)
    # fused entries
    assert {(B, H, W) for B, H, W, _, _ in CC.POOL_CASES} == set(CC.RING_GEOMS)
    assert set(CC.TAIL_CASES) == {(B, H, W, C0, C1, f) for (B, H, W) in ((1, 64, 16), (2, 80, 48)) for (C0, C1) in ((32, 0), (32, 32)) for f in (1, 3, 4)}


def test_every_epilogue_combination_is_in_the_table():
    assert {c.epi for c in CASES} == set(CC.EPILOGUES)
    flags = {CC.EPILOGUES[c.epi] for c in CASES}
    assert (1, 0, 0, 0) in flags and (0, 1, 0, 0) in flags                          # scale without shift, shift without scale
    assert any(f[2] and f[3] for f in flags) and any(f[2] and not f[3] for f in flags)      # residual with and without ReLU
    assert all(c.epi in CC.NO_RESIDUAL for c in _of(("ring", "patch_resident", "patch_streamed", "convt")))     # (these branches take no residual)
    for fam in ("halo", ("pingpong", "pingpong_forced"), "igemm"):
        assert any(CC.EPILOGUES[c.epi] == (1, 1, 1, 1) for c in _of(fam)) and any(CC.EPILOGUES[c.epi] == (1, 1, 1, 0) for c in _of(fam)), fam
    # raw cases also run the statistics entry: every family has one
    assert all(any(c.epi == "raw" for c in _of(f)) for f in CC.FAMILIES)


def test_both_stride_2_forms_and_the_unusual_pads_are_in_the_table():
    s2 = [c for c in CASES if c.stride == 2]
    assert any(c.k == 3 and (c.pad_t, c.pad_l) == (1, 1) and (c.H, c.W, c.Ho, c.Wo) == (9, 7, 5, 4) for c in s2)
    assert any(c.k == 1 and (c.pad_t, c.pad_l) == (0, 0) and (c.H, c.W, c.Ho, c.Wo) == (9, 7, 5, 4) for c in s2)
    assert {c.prefix for c in s2 if c.k == 3} >= {"conv_igemm_kernel" + i for _, i in CC.STRIDE2_3X3}      # every K walk derives its own rows from the stride
    assert any(c.reflect for c in s2)
    assert any(c.k == 3 and c.pad_t == 0 and (c.Ho - 1) * c.stride + c.k > c.H for c in s2)                 # trailing pad implied by Ho alone
    assert any(c.k == 3 and (c.pad_t, c.pad_l) == (0, 0) and (c.Ho, c.Wo) == (c.H - 2, c.W - 2) for c in CASES)
    assert any(c.k == 3 and c.pad_t != c.pad_l for c in CASES)


def test_every_tile_shape_has_a_ragged_last_n_tile():
    ragged = {c.Cout: c.prefix for c in _of("igemm") if c.id.endswith("raggedN") and c.k == 3}
    assert {n: p[len("conv_igemm_kernel"):] for n, p in ragged.items()} == CC.RAGGED_N
    assert set(CC.RAGGED_N) == {72, 136, 40, 8, 24}
    for n, inst in CC.RAGGED_N.items():
        bn = int(inst.split(",")[1])
        assert {n > 64: 128, 32 < n <= 64: 64, n <= 32: 32}[True] == bn and n % bn != 0
    assert any(c.convt and (4 * c.Cout) % 128 for c in CASES)


def test_expected_kernel_names_are_the_ones_the_dispatch_test_recorded():
    """conv_cases.igemm_name / x1_prefix (what the branch test expects of the f16x1, fp32 and igemm-family f16x3 launches) reproduce every name recorded in
    tests/test_conv_dispatch_gpu.py, and every igemm / convt case of the table carries the prefix igemm_name gives it"""
    import test_conv_dispatch_gpu as D

    def as_case(shape, convt, family="igemm", prefix=""):
        B, H, W, C0, C1, Cout, k = shape
        return CC.Case("recorded", family, B, H, W, C0, C1, Cout, k, 1, (k - 1) // 2, (k - 1) // 2, H, W, False, convt, "raw", (), prefix, None)
    for name, (shape, env, convt) in D.SPLIT_CASES.items():
        x3, x1 = D.EXPECTED_SPLIT[name][0][0], D.EXPECTED_SPLIT[name][1][0]
        if x3.startswith("conv_igemm_kernel"):
            assert x3 == CC.igemm_name(as_case(shape, convt), True), name
        family = "halo" if x3.startswith("conv_halo_kernel") else "igemm"
        assert x1.startswith(CC.x1_prefix(as_case(shape, convt, family, x3.split("[")[0]))), name
    for name, shape in D.F32_CASES.items():
        assert D.EXPECTED_F32[name] == [CC.igemm_name(as_case(shape, False), False)], name
    for c in CASES:
        if c.family in ("igemm", "convt"):
            assert c.prefix == CC.igemm_name(c, True), c.id
        assert c.f32_prefix is None or c.f32_prefix == CC.igemm_name(c, False), c.id


def test_batch_invariance_cases_stay_on_their_kernel_when_an_image_runs_alone():
    cs = [CC.BY_ID[i] for i in CC.BATCH_INVARIANT]
    assert {c.family for c in cs} == {"ring", "patch_resident", "patch_streamed", "halo", "pingpong_forced"}
    for c in cs:
        assert c.B > 1 and c.H != c.W
        if c.family in ("halo", "pingpong_forced"):
            assert c.H * c.W >= 1024                                                 # one image alone still has the four 256-row tiles these kernels ask for


# ---- (b) the reference against torch.nn.functional -------------------------------------------------------------------------------------------------------------------
def _functional(c, x, w, scale, shift, res):
    """the same layer composed from F.pad / F.conv2d / F.conv_transpose2d on NCHW float64 tensors"""
    relu = bool(CC.EPILOGUES[c.epi][3])
    xn = x.permute(0, 3, 1, 2)
    cin = x.shape[-1]
    if c.convt:
        wt = w.reshape(2, 2, c.Cout, cin).permute(3, 2, 0, 1)                         # [(dy, dx, co)][c] -> ConvTranspose2d's [c][co][dy][dx]
        y = F.conv_transpose2d(xn, wt, stride=2)
    else:
        pb = max(0, (c.Ho - 1) * c.stride - c.pad_t + c.k - c.H)
        pr = max(0, (c.Wo - 1) * c.stride - c.pad_l + c.k - c.W)
        xp = F.pad(xn, (c.pad_l, pr, c.pad_t, pb), mode="reflect" if c.reflect else "constant")
        y = F.conv2d(xp, w.reshape(-1, c.k, c.k, cin).permute(0, 3, 1, 2), stride=c.stride)[:, :, :c.Ho, :c.Wo]
    if scale is not None:
        y = y * scale.double()[None, :, None, None]
    if shift is not None:
        y = y + shift.double()[None, :, None, None]
    if res is not None:
        y = y + res.permute(0, 3, 1, 2)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1)


def _smallest(family):
    return min(_of(family), key=lambda c: c.B * c.H * c.W * (c.C0 + c.C1) * c.Cout)


SELF_CHECK = [c for c in CASES if c.family in ("igemm", "convt") and c.H <= 16] + [_smallest(f) for f in CC.SPECIALISED + ("pingpong_forced",)]


@pytest.mark.parametrize("case", SELF_CHECK, ids=lambda c: c.id)
def test_reference64_equals_torch_functional(case):
    """two sources as a channel concat, stride 2 with the trailing pad Ho / Wo imply, pad 0, one-axis pads, reflect, the (dy, dx, co) order of the ConvTranspose form:
    conv_ref64's index arithmetic and F's padded convolution agree to float64 round-off on float64 operands of the case's shapes"""
    c = case
    g = torch.Generator().manual_seed(CC.case_seed(c))
    sc, sh, rs, _ = CC.EPILOGUES[c.epi]
    x0 = torch.randn(c.B, c.H, c.W, c.C0, generator=g, dtype=torch.float64)
    x1 = torch.randn(c.B, c.H, c.W, c.C1, generator=g, dtype=torch.float64) if c.C1 else None
    w = torch.randn(c.Cout * (4 if c.convt else 1), c.k * c.k * (c.C0 + c.C1), generator=g, dtype=torch.float64) * 0.05
    scale = torch.rand(c.Cout, generator=g, dtype=torch.float64) + 0.5 if sc else None
    shift = torch.randn(c.Cout, generator=g, dtype=torch.float64) if sh else None
    res = torch.randn(*CC.out_shape(c), generator=g, dtype=torch.float64) if rs else None
    x = x0 if x1 is None else torch.cat([x0, x1], -1)
    mine = CC.conv_ref64(x, w, c.k, c.stride, c.pad_t, c.pad_l, c.Ho, c.Wo, c.reflect, c.convt, scale, shift, res, bool(CC.EPILOGUES[c.epi][3]))
    ref = _functional(c, x, w, scale, shift, res)
    assert mine.shape == ref.shape == CC.out_shape(c)
    assert (mine - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_reference64_refuses_a_reflect_reach_of_two_pixels():
    x, w = torch.randn(1, 5, 5, 8, dtype=torch.float64), torch.randn(8, 72, dtype=torch.float64)
    CC.conv_ref64(x, w, 3, 1, 1, 1, 5, 5, True)
    with pytest.raises(AssertionError):
        CC.conv_ref64(x, w, 3, 1, 1, 1, 6, 5, True)                                   # a sixth output row: the last tap would read row H + 1
    with pytest.raises(AssertionError):
        CC.conv_ref64(x, w, 3, 1, 2, 1, 5, 5, True)


def test_tail_and_pool_references_equal_torch_functional():
    g = torch.Generator().manual_seed(5)
    y = torch.randn(2, 6, 10, 32, generator=g, dtype=torch.float64)
    fw, fb = torch.randn(3, 32, generator=g, dtype=torch.float64), torch.randn(3, generator=g, dtype=torch.float64)
    ref = torch.sigmoid(F.conv2d(y.permute(0, 3, 1, 2), fw[:, :, None, None], fb))
    assert (CC.tail_ref64(y, fw, fb) - ref).abs().max().item() < 1e-14
    assert torch.equal(CC.maxpool_ref64(y), F.max_pool2d(y.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))


def test_operands_decode_to_what_the_split_format_carries():
    """decode / decode_hi of a converted tensor: within the format's 2^-21 of the fp32 value, and exactly its fp16 rounding; a case's operands are seeded"""
    c = CC.BY_ID[CC.BATCH_INVARIANT[0]]
    x = torch.randn(2, 3, 5, 16, generator=torch.Generator().manual_seed(1))
    s = CC.split16_act(x)
    assert s.shape == x.shape and s.dtype == torch.float32
    assert ((CC.decode(s) - x).abs() / x.abs().clamp_min(2.0 ** -10)).max().item() < 2.0 ** -21
    assert torch.equal(CC.decode_hi(s), x.half().float())
    a, b = CC.make_operands(c), CC.make_operands(c)
    assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))
    assert a.x1 is not None and a.scale is None and a.shift is not None and a.res is None
