"""Which kernels the weight-gradient dispatcher launches for a layer (csrc/wgrad.hip: wgrad_plan / conv_wgrad_impl).

For every layer of tests/wgrad_cases.py, every mode {0 exact fp32, 1 and 2 split-fp16 with one / two chunks per barrier} set through smirk_conv_wgrad_set_mode, and
the entries smirk_conv_wgrad_f32, smirk_conv_wgrad_f16x1 and smirk_conv_wgrad_param (layout 0) with x1 = 0 and x1 = 1, the return code, the launch names between
profile_start() and profile_stop() and the movement of smirk_conv_wgrad_x1_fallbacks() must equal EXPECTED.  EXPECTED was recorded by running this same table on the
commit BEFORE the dispatch was rewritten around WgradPlan: the rewrite must choose what that commit chose, and label its launches as that commit did.  A refused call
(f16x1 under mode 0) launches nothing and must leave no pending profile label: the smirk_colsum_split16 launch that follows it carries its own kernel's name.
The >= 2 GiB fallback to the exact-fp32 kernels cannot be reached with tiny layers; tests/test_train_scale_gpu.py keeps covering it."""
import pytest
import torch

import wgrad_cases as WC

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)
ENTRIES = ("f32", "f16x1", "param_x1=0", "param_x1=1")
UNSUPPORTED = -4

# Recorded on the parent commit (see the module docstring).  Per (case, mode): [return code, launch names, movement of the x1 fallback counter] for each of ENTRIES,
# then the launch names of the smirk_colsum_split16 call that follows the f16x1 call.
EXPECTED = {
    ('1x1_convtranspose', 0): [[0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('1x1_convtranspose', 1): [[0, ["wgrad_f16_kernel<64,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('1x1_convtranspose', 2): [[0, ["wgrad_f16_kernel<64,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('1x1_final', 0): [[0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('1x1_final', 1): [[0, ["wgrad_f16_kernel<32,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('1x1_final', 2): [[0, ["wgrad_f16_kernel<32,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_32_32', 0): [[0, ["wgrad3x3_halo_kernel<32,32>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad3x3_halo_kernel<32,32>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_kernel<32,32>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_32_32', 1): [[0, ["wgrad3x3_halo_f16_kernel<32,32,3,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,32,3,2,true,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,32,3,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,32,3,2,true,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_32_32', 2): [[0, ["wgrad3x3_halo_f16_kernel<32,32,3,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,32,3,2,true,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,32,3,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,32,3,2,true,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_32_64', 0): [[0, ["wgrad3x3_halo_kernel<32,64>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad3x3_halo_kernel<32,64>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_kernel<32,64>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_32_64', 1): [[0, ["wgrad3x3_halo_f16_kernel<32,64,6,1,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,64,6,1,false,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,64,6,1,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,64,6,1,false,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_32_64', 2): [[0, ["wgrad3x3_halo_f16_kernel<32,64,6,1,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,64,6,1,false,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,64,6,1,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<32,64,6,1,false,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_64_32', 0): [[0, ["wgrad3x3_halo_kernel<64,32>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad3x3_halo_kernel<64,32>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_kernel<64,32>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_64_32', 1): [[0, ["wgrad3x3_halo_f16_kernel<64,32,6,2,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,32,6,2,false,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,32,6,2,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,32,6,2,false,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_64_32', 2): [[0, ["wgrad3x3_halo_f16_kernel<64,32,6,2,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,32,6,2,false,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,32,6,2,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,32,6,2,false,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_64_64', 0): [[0, ["wgrad3x3_halo_kernel<64,64>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad3x3_halo_kernel<64,64>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_kernel<64,64>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_64_64', 1): [[0, ["wgrad3x3_halo_f16_kernel<64,64,12,1,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,64,12,1,false,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,64,12,1,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,64,12,1,false,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_64_64', 2): [[0, ["wgrad3x3_halo_f16_kernel<64,64,12,1,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,64,12,1,false,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,64,12,1,false>", "wgrad_reduce_kernel"], 0], [0, ["wgrad3x3_halo_f16_kernel<64,64,12,1,false,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_split_tiled_1x1_n288', 0): [[0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_split_tiled_1x1_n288', 1): [[0, ["wgrad_f16_kernel<32,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_split_tiled_1x1_n288', 2): [[0, ["wgrad_f16_kernel<32,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_split_tiled_w8', 0): [[0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_split_tiled_w8', 1): [[0, ["wgrad_f16_kernel<32,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('halo_split_tiled_w8', 2): [[0, ["wgrad_f16_kernel<32,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('reflect', 0): [[0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('reflect', 1): [[0, ["wgrad_f16_kernel<64,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('reflect', 2): [[0, ["wgrad_f16_kernel<64,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile128', 0): [[0, ["wgrad_kernel<128>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<128>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<128>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile128', 1): [[0, ["wgrad_f16_kernel<128,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile128', 2): [[0, ["wgrad_f16_kernel<128,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile128_ragged', 0): [[0, ["wgrad_kernel<128>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<128>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<128>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile128_ragged', 1): [[0, ["wgrad_f16_kernel<128,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile128_ragged', 2): [[0, ["wgrad_f16_kernel<128,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<128,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile32', 0): [[0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<32>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile32', 1): [[0, ["wgrad_f16_kernel<32,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile32', 2): [[0, ["wgrad_f16_kernel<32,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<32,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile64', 0): [[0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile64', 1): [[0, ["wgrad_f16_kernel<64,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile64', 2): [[0, ["wgrad_f16_kernel<64,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile64_ragged', 0): [[0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 0], [-4, [], 0], [0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_kernel<64>", "wgrad_reduce_kernel"], 1], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile64_ragged', 1): [[0, ["wgrad_f16_kernel<64,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,1>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
    ('tile64_ragged', 2): [[0, ["wgrad_f16_kernel<64,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2>", "wgrad_reduce_kernel"], 0], [0, ["wgrad_f16_kernel<64,2,true>", "wgrad_reduce_kernel"], 0], ["colsum_stage1<0>", "colsum_stage2"]],
}


def _split(L, t):
    o = torch.empty_like(t)
    L.check(L.lib().smirk_f32_to_split16(L.ptr(t), L.ptr(o), t.numel(), L.stream_ptr()))
    return o


def observe(shape, mode):
    from smirk_amd import _lib as L
    lib, P = L.lib(), L.ptr
    B, H, W, Cout, Cin, k, reflect = shape
    g = torch.Generator().manual_seed(Cout * 131 + Cin * 17 + k)
    dz = _split(L, torch.randn(B, H, W, Cout, generator=g).cuda())
    x = _split(L, torch.randn(B, H, W, Cin, generator=g).cuda())
    dw = torch.empty(Cout, k * k * Cin, device="cuda")
    nws = lib.smirk_conv_wgrad_workspace_bytes(B, H, W, Cout, Cin, k)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    sums = torch.empty(Cout, device="cuda")
    nred = lib.smirk_train_reduce_workspace_bytes(Cout)
    red = torch.empty(nred, dtype=torch.uint8, device="cuda")
    head = (P(dz), P(x), P(dw), B, H, W, Cout, Cin, k, reflect)
    tail = (P(ws, torch.uint8), nws, L.stream_ptr())
    calls = {
        "f32": lambda: lib.smirk_conv_wgrad_f32(*head, *tail),
        "f16x1": lambda: lib.smirk_conv_wgrad_f16x1(*head, *tail),
        "param_x1=0": lambda: lib.smirk_conv_wgrad_param(*head, 0, 0, 0, 0, 0, *tail),
        "param_x1=1": lambda: lib.smirk_conv_wgrad_param(*head, 0, 0, 0, 0, 1, *tail),
    }
    got = []
    prev = lib.smirk_conv_wgrad_set_mode(mode)
    try:
        for e in ENTRIES:
            before = lib.smirk_conv_wgrad_x1_fallbacks()
            L.profile_start()
            try:
                rc = calls[e]()
            finally:
                names = [r[0] for r in L.profile_stop()]
            got.append([rc, names, lib.smirk_conv_wgrad_x1_fallbacks() - before])
            if e == "f16x1":                                     # whatever that call left behind must not label the next launch of this thread
                L.profile_start()
                try:
                    L.check(lib.smirk_colsum_split16(P(dz), B * H * W, Cout, P(sums), P(red, torch.uint8), nred, L.stream_ptr()))
                finally:
                    after = [r[0] for r in L.profile_stop()]
    finally:
        lib.smirk_conv_wgrad_set_mode(prev)
    torch.cuda.synchronize()
    return got + [after]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(WC.CASES))
def test_entries_launch_the_recorded_kernels(case, mode):
    got = observe(WC.CASES[case], mode)
    assert got == EXPECTED[case, mode]
    for e, (rc, names, moved) in zip(ENTRIES, got):
        if e == "f16x1" and mode == 0:
            assert rc == UNSUPPORTED and names == [], "refused before anything is launched"
        else:
            assert rc == 0 and len(names) == 2 and names[1] == "wgrad_reduce_kernel", "kernel, then reduce"
        assert moved == (1 if e == "param_x1=1" and mode == 0 else 0)
    assert got[-1] == ["colsum_stage1<0>", "colsum_stage2"], "no stale label survives a refused call"
