"""Which kernel the convolution dispatcher launches for a layer, and how many BatchNorm partial-sum rows it reports (conv.hip conv_dispatch_one / igemm_plan).

Every case is the smallest layer that reaches one branch of the dispatch: kernel family (ring, patch, halo, ping-pong, implicit GEMM), tile shape, K walk.  The public
entries run between profile_start() and profile_stop(); the recorded launch names, their number and the statistics entry's `rows` must equal EXPECTED.  EXPECTED was
recorded by running this same table on the commit BEFORE the dispatch was rewritten around IgemmPlan: the rewrite must choose what that commit chose.  The instantiation
name is conv_igemm_kernel<BM,BN,WGM,WGN,SPLIT,KWALK> with KWALK 0 generic, 1 fast, 2 1x1 partial chunk, 3 channel-major, 4 buffer-addressed ("lean"), 5 lean channel-major.
The >= 2 GiB fallbacks (pointer-based walks in split mode, batch chunks) cannot be reached with tiny layers; tests/test_scale_gpu.py runs the chunked path."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# id: (B, H, W, C0, C1, Cout, k), environment switches set around every single call, ConvTranspose scatter
SPLIT_CASES = {
    "lean_cm_128x128": ((1, 8, 8, 64, 0, 128, 3), {}, False),
    "lean_cm_two_sources": ((1, 8, 8, 32, 32, 128, 3), {}, False),
    "lean_odd_chunk_count": ((1, 8, 8, 32, 0, 128, 3), {}, False),
    "lean_non_pow2_channels": ((1, 8, 8, 96, 0, 128, 3), {}, False),
    "tile_128x64": ((1, 8, 8, 64, 0, 64, 3), {}, False),
    "tile_256x32": ((1, 8, 8, 32, 0, 32, 3), {}, False),
    "1x1_whole_chunks": ((2, 14, 14, 64, 0, 64, 1), {}, False),
    "1x1_partial_chunk_72": ((2, 7, 7, 72, 0, 24, 1), {}, False),
    "1x1_partial_chunk_40": ((1, 14, 14, 40, 0, 120, 1), {}, False),
    "generic_walk": ((1, 16, 16, 8, 0, 32, 3), {}, False),
    "convt_scatter": ((1, 8, 8, 64, 0, 32, 1), {}, True),
    "halo_npa5": ((6, 14, 14, 32, 0, 128, 3), {}, False),
    "halo_npa6": ((1, 63, 63, 32, 0, 128, 3), {}, False),
    "pingpong_default": ((8, 2, 64, 32, 0, 128, 3), {}, False),
    "pingpong_halo_off": ((6, 14, 14, 32, 0, 128, 3), {"SMIRK_IGEMM_HALO": "0"}, False),
    "ring_cout64": ((1, 64, 64, 32, 0, 64, 3), {}, False),
    "ring_cout32_two_sources": ((1, 64, 64, 32, 32, 32, 3), {}, False),
    "patch_resident_c8": ((1, 64, 64, 8, 0, 32, 3), {}, False),
    "patch_resident_c32": ((1, 64, 64, 32, 0, 32, 3), {}, False),
    "patch_resident_cout64": ((1, 64, 64, 16, 0, 64, 3), {}, False),
    "patch_streamed_two_sources": ((1, 64, 64, 96, 32, 64, 3), {}, False),
    "patch_streamed_ring_off": ((1, 64, 64, 128, 0, 64, 3), {"SMIRK_CONV_RING": "0"}, False),
    "patch_and_ring_disabled": ((1, 64, 64, 32, 0, 64, 3), {"SMIRK_DISABLE_PATCH_KERNEL": "1"}, False),
}
F32_CASES = {
    "f32_3x3_whole_chunks": (1, 8, 8, 64, 0, 128, 3),
    "f32_3x3_c8": (1, 16, 16, 8, 0, 32, 3),
    "f32_1x1_c40": (1, 14, 14, 40, 0, 120, 1),
}

# Recorded on the parent commit (see the module docstring).  Split cases: launches of smirk_conv_igemm_f16x3, of smirk_conv_igemm_f16x1, of
# smirk_conv_igemm_stats_split16 with x1 = 0 and its rows, the same with x1 = 1.
EXPECTED_SPLIT = {
    "1x1_partial_chunk_40": [["conv_igemm_kernel<128,128,2,2,true,2>"], ["conv_igemm_kernel<128,128,2,2,true,2>[f16x1]"], ["conv_igemm_kernel<128,128,2,2,true,2>"], 4, ["conv_igemm_kernel<128,128,2,2,true,2>[f16x1]"], 4],
    "1x1_partial_chunk_72": [["conv_igemm_kernel<256,32,4,1,true,2>"], ["conv_igemm_kernel<256,32,4,1,true,2>[f16x1]"], ["conv_igemm_kernel<256,32,4,1,true,2>"], 4, ["conv_igemm_kernel<256,32,4,1,true,2>[f16x1]"], 4],
    "1x1_whole_chunks": [["conv_igemm_kernel<128,64,2,2,true,4>"], ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], ["conv_igemm_kernel<128,64,2,2,true,4>"], 8, ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], 8],
    "convt_scatter": [["conv_igemm_kernel<128,128,2,2,true,4>"], ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], ["conv_igemm_kernel<128,128,2,2,true,4>"], 0, ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], 0],
    "generic_walk": [["conv_igemm_kernel<256,32,4,1,true,0>"], ["conv_igemm_kernel<256,32,4,1,true,0>[f16x1]"], ["conv_igemm_kernel<256,32,4,1,true,0>"], 0, ["conv_igemm_kernel<256,32,4,1,true,0>[f16x1]"], 0],
    "halo_npa5": [["conv_halo_kernel<5,0>[256x128,8w,halo]"], ["conv_halo_x1_kernel<5>[256x128,8w,halo,f16x1]"], ["conv_halo_kernel<5,0>[256x128,8w,halo]"], 20, ["conv_halo_x1_kernel<5>[256x128,8w,halo,f16x1]"], 20],
    "halo_npa6": [["conv_halo_kernel<6,0>[256x128,8w,halo]"], ["conv_halo_x1_kernel<6>[256x128,8w,halo,f16x1]"], ["conv_halo_kernel<6,0>[256x128,8w,halo]"], 64, ["conv_halo_x1_kernel<6>[256x128,8w,halo,f16x1]"], 64],
    "lean_cm_128x128": [["conv_igemm_kernel<128,128,2,2,true,5>"], ["conv_igemm_kernel<128,128,2,2,true,5>[f16x1]"], ["conv_igemm_kernel<128,128,2,2,true,5>"], 2, ["conv_igemm_kernel<128,128,2,2,true,5>[f16x1]"], 2],
    "lean_cm_two_sources": [["conv_igemm_kernel<128,128,2,2,true,5>"], ["conv_igemm_kernel<128,128,2,2,true,5>[f16x1]"], ["conv_igemm_kernel<128,128,2,2,true,5>"], 2, ["conv_igemm_kernel<128,128,2,2,true,5>[f16x1]"], 2],
    "lean_non_pow2_channels": [["conv_igemm_kernel<128,128,2,2,true,4>"], ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], ["conv_igemm_kernel<128,128,2,2,true,4>"], 2, ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], 2],
    "lean_odd_chunk_count": [["conv_igemm_kernel<128,128,2,2,true,4>"], ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], ["conv_igemm_kernel<128,128,2,2,true,4>"], 2, ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], 2],
    "patch_and_ring_disabled": [["conv_igemm_kernel<128,64,2,2,true,4>"], ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], ["conv_igemm_kernel<128,64,2,2,true,4>"], 64, ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], 64],
    "patch_resident_c32": [["conv3x3_patch_kernel<1,1,16,1>"], ["conv_igemm_kernel<256,32,4,1,true,4>[f16x1]"], ["conv3x3_patch_kernel<1,1,16,1>"], 0, ["conv_igemm_kernel<256,32,4,1,true,4>[f16x1]"], 64],
    "patch_resident_c8": [["conv3x3_patch_kernel<1,1,16,1>"], ["conv_igemm_kernel<256,32,4,1,true,0>[f16x1]"], ["conv3x3_patch_kernel<1,1,16,1>"], 0, ["conv_igemm_kernel<256,32,4,1,true,0>[f16x1]"], 0],
    "patch_resident_cout64": [["conv3x3_patch_kernel<2,2,16,1>"], ["conv_igemm_kernel<128,64,2,2,true,0>[f16x1]"], ["conv3x3_patch_kernel<2,2,16,1>"], 0, ["conv_igemm_kernel<128,64,2,2,true,0>[f16x1]"], 0],
    "patch_streamed_ring_off": [["conv3x3_patch_stream_kernel"], ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], ["conv3x3_patch_stream_kernel"], 0, ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], 64],
    "patch_streamed_two_sources": [["conv3x3_patch_stream_kernel"], ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], ["conv3x3_patch_stream_kernel"], 0, ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], 64],
    "pingpong_default": [["conv_pp_kernel<3>[256x128,8w,3stage]"], ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], ["conv_pp_kernel<3>[256x128,8w,3stage]"], 0, ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], 16],
    "pingpong_halo_off": [["conv_pp_kernel<3>[256x128,8w,3stage]"], ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], ["conv_pp_kernel<3>[256x128,8w,3stage]"], 0, ["conv_igemm_kernel<128,128,2,2,true,4>[f16x1]"], 20],
    "ring_cout32_two_sources": [["conv3x3_ring_kernel<1>[16x16patch,ring]"], ["conv_igemm_kernel<256,32,4,1,true,4>[f16x1]"], ["conv3x3_ring_kernel<1>[16x16patch,ring]"], 64, ["conv_igemm_kernel<256,32,4,1,true,4>[f16x1]"], 64],
    "ring_cout64": [["conv3x3_ring_kernel<2>[16x16patch,ring]"], ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], ["conv3x3_ring_kernel<2>[16x16patch,ring]"], 64, ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], 64],
    "tile_128x64": [["conv_igemm_kernel<128,64,2,2,true,4>"], ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], ["conv_igemm_kernel<128,64,2,2,true,4>"], 2, ["conv_igemm_kernel<128,64,2,2,true,4>[f16x1]"], 2],
    "tile_256x32": [["conv_igemm_kernel<256,32,4,1,true,4>"], ["conv_igemm_kernel<256,32,4,1,true,4>[f16x1]"], ["conv_igemm_kernel<256,32,4,1,true,4>"], 4, ["conv_igemm_kernel<256,32,4,1,true,4>[f16x1]"], 4],
}
EXPECTED_F32 = {
    "f32_1x1_c40": ["conv_igemm_kernel<128,128,2,2,false,2>"],
    "f32_3x3_c8": ["conv_igemm_kernel<256,32,4,1,false,0>"],
    "f32_3x3_whole_chunks": ["conv_igemm_kernel<128,128,2,2,false,1>"],
}


def _desc(L, shape, convt):
    B, H, W, C0, C1, Cout, k = shape
    d = L.SmirkConvDesc()
    d.B, d.H, d.W, d.C0, d.C1, d.Cout, d.KH, d.KW, d.stride = B, H, W, C0, C1, Cout, k, k, 1
    d.pad_t = d.pad_l = (k - 1) // 2
    d.Ho, d.Wo, d.pad_mode, d.act = H, W, L.PAD_ZERO, L.ACT_NONE
    d.out_mode = L.OUT_CONVT2X2 if convt else L.OUT_NHWC
    return d


def _operands(L, shape, convt, split):
    """random operands; the split-fp16 format has the footprint of fp32, so one conversion launch per tensor gives valid split tensors of the same shapes"""
    B, H, W, C0, C1, Cout, k = shape
    g = torch.Generator().manual_seed(C0 * 131 + C1 * 17 + Cout + k)
    n = Cout * (4 if convt else 1)
    ts = [torch.randn(B, H, W, C0, generator=g).cuda(), torch.randn(B, H, W, C1, generator=g).cuda() if C1 else None,
          (torch.randn(n, k * k * (C0 + C1), generator=g) * 0.05).cuda()]
    if split:
        for i, t in enumerate(ts):
            if t is not None:
                o = torch.empty_like(t)
                L.check(L.lib().smirk_f32_to_split16(L.ptr(t), L.ptr(o), t.numel(), L.stream_ptr()))
                ts[i] = o
    out = torch.empty(B, H * (2 if convt else 1), W * (2 if convt else 1), Cout, device="cuda")
    return ts + [out]


def _launches(L, env, call):
    """kernel names of the launches `call` makes with the switches of `env` set around it"""
    os.environ.update(env)
    try:
        L.profile_start()
        try:
            rc = call()
        finally:
            recs = L.profile_stop()
    finally:
        for k in env:
            del os.environ[k]
    L.check(rc)
    return [r[0] for r in recs]


def observe_split(shape, env, convt):
    """-> [f16x3 names, f16x1 names, stats names (x1 = 0), rows, stats names (x1 = 1), rows]"""
    import ctypes as C
    from smirk_amd import _lib as L
    lib, P = L.lib(), L.ptr
    d = _desc(L, shape, convt)
    x0, x1, w, out = _operands(L, shape, convt, True)
    rows_max = lib.smirk_conv_stats_rows_max(d)
    part = torch.empty(rows_max, shape[5], 2, device="cuda")
    got = []
    for fn in (lib.smirk_conv_igemm_f16x3, lib.smirk_conv_igemm_f16x1):
        got.append(_launches(L, env, lambda: fn(d, P(x0), P(x1, allow_none=True), P(w), None, None, None, P(out), L.stream_ptr())))
    for one in (0, 1):
        rows = C.c_int(-1)
        got.append(_launches(L, env, lambda: lib.smirk_conv_igemm_stats_split16(d, P(x0), P(x1, allow_none=True), P(w), P(out), P(part), C.byref(rows), one,
                                                                                  L.stream_ptr())))
        assert 0 <= rows.value <= rows_max
        got.append(rows.value)
    torch.cuda.synchronize()
    return got


def observe_f32(shape):
    from smirk_amd import _lib as L
    P = L.ptr
    d = _desc(L, shape, False)
    x0, x1, w, out = _operands(L, shape, False, False)
    got = _launches(L, {}, lambda: L.lib().smirk_conv_igemm_f32(d, P(x0), P(x1, allow_none=True), P(w), None, None, None, P(out), L.stream_ptr()))
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("case", sorted(SPLIT_CASES))
def test_split_entries_launch_the_recorded_kernels_and_report_the_recorded_rows(case):
    got = observe_split(*SPLIT_CASES[case])
    assert got == EXPECTED_SPLIT[case]
    assert all(len(names) == 1 for names in got[0:3] + got[4:5]), "one launch per layer at these sizes"


@pytest.mark.parametrize("case", sorted(F32_CASES))
def test_f32_entry_launches_the_recorded_kernel(case):
    assert observe_f32(F32_CASES[case]) == EXPECTED_F32[case]
