"""What every branch of the convolution dispatch COMPUTES (csrc/conv.hip conv_dispatch_one / igemm_plan and the four kernel families in front of it), against float64.

tests/test_conv_dispatch_gpu.py pins which kernel a layer reaches; this file runs the table of tests/conv_cases.py through every public entry and checks the numbers:
the f16x3 entry must launch the case's kernel, every entry must equal conv_cases.conv_ref64 on the exactly representable values of the converted operands to the
project's bound for this data path (TOL of tests/test_train_ops_gpu.py), every output pixel must have been written and nothing around the output touched.  Outputs
live in the middle of a larger buffer filled with fp16 NaNs: a pixel a ragged tile skips decodes to NaN, a store past either end changes a guard word."""
import ctypes as C
import os

import pytest
import torch

import conv_cases as CC

pytestmark = pytest.mark.gpu

TOL = 3e-6              # max|out - ref| / max|ref|: tests/test_train_ops_gpu.py TOL, the split-fp16 x3 / fp32 data path against exactly representable operands
OUT_TOL = 2e-5          # absolute, on the sigmoid output of the fused tail: tests/test_generator_gpu.py OUT_TOL
NAN_WORD = 0x7E007E00   # two fp16 quiet NaNs per 32-bit word: whichever of hi / lo a half becomes, an unwritten element decodes to NaN
NAN_WORD_F32 = 0x7FC00000


def _L():
    from smirk_amd import _lib as L
    return L


def _desc(c, B=None):
    L = _L()
    d = L.SmirkConvDesc()
    d.B, d.H, d.W, d.C0, d.C1, d.Cout, d.KH, d.KW, d.stride = (c.B if B is None else B), c.H, c.W, c.C0, c.C1, c.Cout, c.k, c.k, c.stride
    d.pad_t, d.pad_l, d.Ho, d.Wo = c.pad_t, c.pad_l, c.Ho, c.Wo
    d.pad_mode = L.PAD_REFLECT if c.reflect else L.PAD_ZERO
    d.act = L.ACT_RELU if CC.EPILOGUES[c.epi][3] else L.ACT_NONE
    d.out_mode = L.OUT_CONVT2X2 if c.convt else L.OUT_NHWC
    return d


class Guarded:
    """a tensor of `shape` in the middle of a buffer of NaN words, with `guard` words on either side"""

    def __init__(self, shape, guard, word=NAN_WORD):
        n = 1
        for s in shape:
            n *= s
        guard = (guard + 7) // 8 * 8                                 # keeps the 32-byte alignment of an 8-channel group
        self.word, self.n, self.g = word, n, guard
        self.buf = torch.full((guard + n + guard,), word, dtype=torch.int32, device="cuda")
        self.t = self.buf[guard:guard + n].view(torch.float32).view(*shape)

    def guards_intact(self):
        return bool((self.buf[:self.g] == self.word).all()) and bool((self.buf[self.g + self.n:] == self.word).all())

    def untouched(self):
        return bool((self.buf == self.word).all())


def _guard_words(c):
    return 256 * c.Cout * (4 if c.convt else 1)                      # one output row of one 256-row tile, all N columns


def _launches(env, call):
    """kernel names of the launches `call` makes with the switches of `env` set around it (as tests/test_conv_dispatch_gpu.py observes them)"""
    L = _L()
    env = dict(env)
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


def _where(bad):
    """which (b, y, x, c) index sets are wrong: names a broken index map at a glance"""
    idx = bad.nonzero()
    return {n: sorted(set(idx[:, k].tolist()))[:40] for k, n in enumerate(("b", "y", "x", "c"))}


def _assert_close(got, ref, what, tol=TOL):
    """got: float64 NHWC values (NaN where nothing was stored); the issue's bound, with the wrong index sets in the message"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = torch.isfinite(got)
    assert bool(fin.all()), f"{what}: output elements never written (or not finite) at {_where(~fin)}"
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs()
    print(f"{what}: max|out - ref| / max|ref| = {err.max().item() / scale:.3e}")
    assert err.max().item() / scale < tol, f"{what}: rel {err.max().item() / scale:.3e} >= {tol}; wrong at {_where(err >= tol * scale)}"


def _cuda(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("cid", [c.id for c in CC.CASES])
def test_every_entry_on_every_branch_equals_float64_and_stays_inside_its_output(cid):
    """one case of tests/conv_cases.py through smirk_conv_igemm_f16x3 (which must launch the case's kernel), _f16x1 (reference on the hi halves), _f32 and, for a raw
    epilogue, _stats_split16 with one and three MFMAs per product: each within TOL of float64, every output element written, the guard words on both sides intact;
    the statistics entries bit-identical to the plain ones, their rows within smirk_conv_stats_rows_max, untouched beyond the reported count, and summing to the
    column sums of the stored tensor.  First run on the MI355X: no case of any family failed."""
    L = _L()
    lib, P, c = L.lib(), L.ptr, CC.BY_ID[cid]
    ops = CC.operands_of(cid)
    x0, x1, w, scale, shift, res = (_cuda(t) for t in ops)
    d, shape, gw = _desc(c), CC.out_shape(c), _guard_words(c)
    ref3 = CC.reference_of(cid)
    raw = c.epi == "raw"

    def run_split(fn):
        out = Guarded(shape, gw)
        names = _launches(c.env, lambda: fn(d, P(x0), P(x1, allow_none=True), P(w), P(scale, allow_none=True), P(shift, allow_none=True), P(res, allow_none=True),
                                            P(out.t), L.stream_ptr()))
        torch.cuda.synchronize()
        return out, names

    # ---- f16x3: the case's branch, its values, its stores ----
    o3, n3 = run_split(lib.smirk_conv_igemm_f16x3)
    assert len(n3) == 1 and n3[0].startswith(c.prefix), f"{cid}: f16x3 launched {n3}, the case is meant for {c.prefix}"
    _assert_close(CC.decode(o3.t.cpu()).double(), ref3, f"{cid} f16x3 {n3[0]}")
    assert o3.guards_intact(), f"{cid}: {n3[0]} stored outside its output"

    # ---- f16x1: the hi halves only ----
    o1, n1 = run_split(lib.smirk_conv_igemm_f16x1)
    # (the kernels tests/test_conv_dispatch_gpu.py records for the family: halo has a one-MFMA kernel of its own, everything else is on the implicit GEMM)
    assert len(n1) == 1 and n1[0].startswith(CC.x1_prefix(c)) and n1[0].endswith("f16x1]"), (n1, CC.x1_prefix(c))
    assert c.family not in ("igemm", "convt") or n1[0] == n3[0] + "[f16x1]"
    _assert_close(CC.decode(o1.t.cpu()).double(), CC.reference_of(cid, True), f"{cid} f16x1 {n1[0]}")
    assert o1.guards_intact(), f"{cid}: {n1[0]} stored outside its output"

    # ---- exact fp32 on the same values ----
    f0, f1, fw, fres = (None if t is None else CC.decode(t).cuda() for t in (ops.x0, ops.x1, ops.w, ops.res))
    o32 = Guarded(shape, gw, NAN_WORD_F32)
    n32 = _launches(c.env, lambda: lib.smirk_conv_igemm_f32(d, P(f0), P(f1, allow_none=True), P(fw), P(scale, allow_none=True), P(shift, allow_none=True),
                                                            P(fres, allow_none=True), P(o32.t), L.stream_ptr()))
    torch.cuda.synchronize()
    assert n32 == [CC.igemm_name(c, False)] and n32[0].startswith(c.f32_prefix or ""), n32      # (only the split-fp16 entries have specialised families)
    _assert_close(o32.t.cpu().double(), ref3, f"{cid} f32 {n32[0]}")
    assert o32.guards_intact(), f"{cid}: {n32[0]} stored outside its output"

    # ---- raw epilogue: the statistics entry, one and three MFMAs per product ----
    if not raw:
        return
    rows_max = lib.smirk_conv_stats_rows_max(d)
    for one, plain, nplain in ((0, o3, n3), (1, o1, n1)):
        out, part, rows = Guarded(shape, gw), Guarded((rows_max, c.Cout, 2), 2 * c.Cout, NAN_WORD_F32), C.c_int(-1)
        ns = _launches(c.env, lambda: lib.smirk_conv_igemm_stats_split16(d, P(x0), P(x1, allow_none=True), P(w), P(out.t), P(part.t), C.byref(rows), one,
                                                                           L.stream_ptr()))
        torch.cuda.synchronize()
        assert ns == nplain, (ns, nplain)                           # the statistics epilogue is a property of the launch, not another kernel family
        assert torch.equal(out.t, plain.t), f"{cid}: statistics entry (x1 = {one}) differs from the plain entry"
        assert out.guards_intact() and part.guards_intact()
        assert 0 <= rows.value <= rows_max
        assert bool(torch.isnan(part.t[rows.value:]).all()), "partial rows beyond the reported count were written"
        if rows.value == 0:
            continue                                                # (this family leaves no partial sums: the caller reduces the stored tensor)
        p = part.t[:rows.value].double().sum(0).cpu()               # [Cout][2]
        assert bool(torch.isfinite(p).all()), "a reported partial row was not written"
        zv = CC.decode(out.t.cpu()).double().reshape(-1, c.Cout)
        s1, s2 = zv.sum(0), (zv * zv).sum(0)
        # the two bounds of test_conv_epilogue_statistics_equal_the_sums_of_the_stored_output (tests/test_train_ops_gpu.py)
        e1, e2 = (p[:, 0] - s1).abs().max().item(), (p[:, 1] - s2).abs().max().item()
        print(f"{cid} stats x1={one}: |sum - s1| = {e1:.3e}, |sumsq - s2| = {e2:.3e}, rows = {rows.value}")
        assert e1 <= 2e-6 * zv.abs().sum(0).max().item() + 1e-6
        assert e2 <= 4e-6 * s2.max().item() + 1e-9


@pytest.mark.parametrize("cid", CC.BATCH_INVARIANT)
def test_an_image_of_a_batch_equals_the_same_image_run_alone(cid):
    """patch -> workgroup and row -> tile assignments change with B; a frame's result must not: bit for bit, on the same kernel"""
    L = _L()
    lib, P, c = L.lib(), L.ptr, CC.BY_ID[cid]
    ops = CC.operands_of(cid)

    def run(sel):
        x0, x1, res = (None if t is None else t[sel].contiguous().cuda() for t in (ops.x0, ops.x1, ops.res))
        w, scale, shift = _cuda(ops.w), _cuda(ops.scale), _cuda(ops.shift)
        d = _desc(c, B=x0.shape[0])
        out = Guarded((x0.shape[0],) + CC.out_shape(c)[1:], _guard_words(c))
        names = _launches(c.env, lambda: lib.smirk_conv_igemm_f16x3(d, P(x0), P(x1, allow_none=True), P(w), P(scale, allow_none=True), P(shift, allow_none=True),
                                                                    P(res, allow_none=True), P(out.t), L.stream_ptr()))
        torch.cuda.synchronize()
        assert len(names) == 1 and names[0].startswith(c.prefix), names
        assert out.guards_intact()
        return out.t

    whole = run(slice(None))
    for b in (0, c.B - 1):
        alone = run(slice(b, b + 1))
        same = alone[0].view(torch.int32) == whole[b].view(torch.int32)
        assert bool(same.all()), f"{cid}: image {b} differs from the same image alone at {_where(~same[None])}"


@pytest.mark.parametrize("B,H,W,C0,C1", CC.POOL_CASES)
def test_pool_entry_on_non_square_images(B, H, W, C0, C1):
    """smirk_conv3x3_pool_f16x3: the conv output is bit-identical to smirk_conv_igemm_f16x3's, the pooled output to smirk_maxpool2x2_split16 of it, both equal float64,
    every pixel of both is written and nothing outside them; a shape without a fused-pool kernel stays a refusal that launches and writes nothing"""
    L = _L()
    lib, P = L.lib(), L.ptr
    c = CC.Case(f"pool-{B}x{H}x{W}-{C0}+{C1}", "ring", B, H, W, C0, C1, 64, 3, 1, 1, 1, H, W, False, False, "bn_relu", (), "conv3x3_ring_kernel<2,pool>", None)
    ops = CC.make_operands(c)
    x0, x1, w, scale, shift, _ = (_cuda(t) for t in ops)
    d, gw = _desc(c), _guard_words(c)
    o0, o1 = Guarded((B, H, W, 64), gw), Guarded((B, H, W, 64), gw)
    p0, p1 = Guarded((B, H // 2, W // 2, 64), gw), Guarded((B, H // 2, W // 2, 64), gw)
    L.check(lib.smirk_conv_igemm_f16x3(d, P(x0), P(x1, allow_none=True), P(w), P(scale), P(shift), None, P(o0.t), L.stream_ptr()))
    L.check(lib.smirk_maxpool2x2_split16(P(o0.t), P(p0.t), B, H, W, 64, L.stream_ptr()))
    names = _launches((), lambda: lib.smirk_conv3x3_pool_f16x3(d, P(x0), P(x1, allow_none=True), P(w), P(scale), P(shift), P(o1.t), P(p1.t), L.stream_ptr()))
    torch.cuda.synchronize()
    assert len(names) == 1 and names[0].startswith(c.prefix), names
    ref = CC.reference(c, ops)
    _assert_close(CC.decode(o1.t.cpu()).double(), ref, f"{c.id} conv")
    _assert_close(CC.decode(p1.t.cpu()).double(), CC.maxpool_ref64(ref), f"{c.id} pooled")
    assert all(g.guards_intact() for g in (o0, o1, p0, p1))
    eq_o, eq_p = o0.t.view(torch.int32) == o1.t.view(torch.int32), p0.t.view(torch.int32) == p1.t.view(torch.int32)
    assert bool(eq_o.all()), _where(~eq_o)
    assert bool(eq_p.all()), _where(~eq_p)
    # refusals: 32 output channels; a height that is no multiple of 16; nothing is launched, nothing written
    o2, p2 = Guarded((B, H, W, 64), gw), Guarded((B, H // 2, W // 2, 64), gw)
    d32 = _desc(c._replace(Cout=32))
    dh = _desc(c._replace(H=H - 8, Ho=H - 8))
    for bad in (d32, dh):
        L.profile_start()
        rc = lib.smirk_conv3x3_pool_f16x3(bad, P(x0), P(x1, allow_none=True), P(w), P(scale), P(shift), P(o2.t), P(p2.t), L.stream_ptr())
        assert rc == -4 and L.profile_stop() == []                  # SMIRK_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert o2.untouched() and p2.untouched()


@pytest.mark.parametrize("B,H,W,C0,C1,fcout", CC.TAIL_CASES)
def test_tail_entry_equals_float64(B, H, W, C0, C1, fcout):
    """smirk_conv3x3_tail_f16x3 on its own: conv + BatchNorm + ReLU + 1 x 1 conv + bias + sigmoid -> NCHW fp32, within the generator's output tolerance of float64 on
    the exactly representable operands; every output pixel of every one of the fcout planes written, nothing outside them"""
    L = _L()
    lib, P = L.lib(), L.ptr
    c = CC.Case(f"tail-{B}x{H}x{W}-{C0}+{C1}-f{fcout}", "patch_resident", B, H, W, C0, C1, 32, 3, 1, 1, 1, H, W, False, False, "bn_relu", (),
                "conv3x3_patch_kernel<1,", None)
    ops = CC.make_operands(c)
    g = torch.Generator().manual_seed(CC.case_seed(c) + 1)
    fw, fb = torch.randn(fcout, 32, generator=g) * 0.3, torch.randn(fcout, generator=g) * 0.3
    x0, x1, w, scale, shift, _ = (_cuda(t) for t in ops)
    fwd, fbd = fw.cuda(), fb.cuda()
    out = Guarded((B, fcout, H, W), 256 * 32, NAN_WORD_F32)
    names = _launches((), lambda: lib.smirk_conv3x3_tail_f16x3(_desc(c), P(x0), P(x1, allow_none=True), P(w), P(scale), P(shift), P(fwd), P(fbd), P(out.t),
                                                               fcout, L.stream_ptr()))
    torch.cuda.synchronize()
    assert len(names) == 1 and names[0].startswith(c.prefix), names
    ref = CC.tail_ref64(CC.reference(c, ops), fw, fb)
    got = out.t.cpu().double()
    fin = torch.isfinite(got)
    assert bool(fin.all()), f"never written: { {n: v for n, v in zip(('b', 'o', 'y', 'x'), _where(~fin).values())} }"
    err = (got - ref).abs()
    print(f"{c.id}: max|out - ref| = {err.max().item():.3e}")
    assert err.max().item() < OUT_TOL, {n: v for n, v in zip(("b", "o", "y", "x"), _where(err >= OUT_TOL).values())}
    assert out.guards_intact()
