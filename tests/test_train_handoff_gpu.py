"""masking.train_masked_image_packed (include/smirk_train_handoff.h) against the utilities it stands for: with $SMIRK_DISABLE_TRAIN_HANDOFF set and unset, under
one pinned PhiloxStream, masked, the generator's packed input, the returned coords and the stream's final offset must be the same.  Exact equality, no tolerance:
a quantised pixel flips if a multiply-add of the fused sampler rounds differently from the separate gather.  The shapes are the smallest at which the kernels
can go wrong; H <= W everywhere because the points are quantised with S = H."""
import os

import pytest
import torch

from oracle.flame_ref import FlameRef

pytestmark = pytest.mark.gpu

SWITCH = "SMIRK_DISABLE_TRAIN_HANDOFF"
# (B, Ke, H, W, rendered-mask rule, probability of a patch centre, hull mask).  Ke == 1 with the "nonzero" rule is the first path (no target vertices: every
# sampled pixel is transferred onto itself); the others are the second path.  The hull masks hold 0 and 1 only, so that a pixel of `masked` that is neither 0 nor
# its own img value can only be a transferred one.
CASES = [(2, 1, 32, 32, "nonzero", 0.01, "blocks"),      # first path; the 10-row halo lies wholly outside the image
         (2, 2, 32, 32, "positive", 0.005, "blocks"),    # Ke by index
         (1, 3, 40, 48, "positive", 0.005, "blocks"),    # kb % B always 0; a ragged last band (40 = 2 x 16 + 8)
         (3, 2, 37, 45, "positive", 0.05, "shared"),     # W no multiple of 4; ONE [1,H,W] hull mask for every frame
         (2, 1, 224, 224, "nonzero", 0.01, "blocks")]    # the workload's own size


@pytest.fixture(scope="module")
def mesh(sandbox):
    from smirk_amd import masking as M
    cwd = os.getcwd(); os.chdir(sandbox)
    try:
        prob = M.load_probabilities_per_FLAME_triangle().cuda()
    finally:
        os.chdir(cwd)
    return M, prob, torch.from_numpy(FlameRef(sandbox).faces).cuda()


def _hull(kind, B, H, W):
    """1 = keep the photo.  The zero (face) regions reach all four borders and the corners."""
    h = torch.ones(1 if kind == "shared" else B, 1, H, W)
    for b in range(h.shape[0]):
        o = b % 2
        h[b, :, : max(1, H // 3), W // 4 + o: W // 2] = 0
        h[b, :, H // 2:, : max(1, W // 5) + o] = 0
        h[b, :, H // 4: H // 2 + 1, W - max(1, W // 6):] = 0
        h[b, :, H - 1, W // 2:] = 0
        h[b, :, 0, 0] = 0
    return h[:, 0] if kind == "shared" else h                              # "shared": [1,H,W]


def _inputs(B, Ke, H, W, rule, kind, seed):
    g = torch.Generator().manual_seed(seed)
    KB = Ke * B
    img = torch.rand(B, 3, H, W, generator=g)
    img[:, :, ::7, ::5] = 0.0                                              # exact zeros and a few negative values: `extra > 0` must fail there
    img[:, 1, 3::11, 2::9] *= -1.0
    rendered = torch.rand(KB, 3, H, W, generator=g)
    rendered[:, :, : H // 2, : (2 * W) // 3] = 0.0                         # background of the rendering (all three channels zero), up to two borders
    rendered[:, 0, H // 2:, ::3] = 0.0                                     # one zero channel: covered under "nonzero", not under "positive"
    if rule == "positive":
        rendered[:, 2, H // 2:, 1::4] *= -1.0                              # a negative channel: nonzero, but not positive
    tv_src = torch.randn(B, 5023, 3, generator=g) * 0.9                    # points land all over the image; those beyond it are clamped onto its borders
    tv_dst = None if (Ke == 1 and rule == "nonzero") else torch.randn(KB, 5023, 3, generator=g) * 0.9
    return img.cuda(), rendered.cuda(), _hull(kind, B, H, W).cuda(), tv_src.cuda(), None if tv_dst is None else tv_dst.cuda()


def _run(mesh, inputs, monkeypatch, off, Ke, H, rule, p_field):
    M, prob, faces = mesh
    img, rendered, hull, tv_src, tv_dst = inputs
    if off:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    rng = M.PhiloxStream(0x5EED, 12345)
    masked, packed, coords = M.train_masked_image_packed(img, hull, rendered, tv_src, faces, prob, trans_verts_dst=tv_dst, Ke=Ke,
                                                         mask_ratio=0.01 if H == 224 else 0.2, rendered_rule=rule, random_mask=p_field, rng=rng, want_coords=True)
    return masked, packed, coords, rng.offset


def _pack(rendered, masked):
    from smirk_amd import _lib as L
    B, _, H, W = rendered.shape
    out = torch.empty(B, H, W, 8, device=rendered.device)
    L.check(L.lib().smirk_pack_generator_input_split16(L.ptr(rendered), 3, L.ptr(masked), 3, L.ptr(out), B, H, W, L.stream_ptr()))
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("B,Ke,H,W,rule,p_field,kind", CASES)
def test_two_launches_equal_the_separate_utilities_bit_for_bit(mesh, monkeypatch, B, Ke, H, W, rule, p_field, kind):
    M = mesh[0]
    inputs = _inputs(B, Ke, H, W, rule, kind, seed=300 + H + W + Ke)
    img, rendered, hull, tv_src, tv_dst = inputs
    m_off, p_off, c_off, end_off = _run(mesh, inputs, monkeypatch, True, Ke, H, rule, p_field)
    m_on, p_on, c_on, end_on = _run(mesh, inputs, monkeypatch, False, Ke, H, rule, p_field)
    KB, N = Ke * B, int((0.01 if H == 224 else 0.2) * H * H)
    assert p_off is None and p_on is not None and p_on.shape == (KB, H, W, 8) and m_on.shape == (KB, 3, H, W)
    assert end_on == end_off == 12345 + B * N + (KB * H * W + 3) // 4 + KB * 3 * H * W     # points, field, noise: later draws of the stream do not move
    torch.cuda.synchronize()
    assert sorted(c_on) == sorted(c_off) == ["barycentric_coords", "points1", "points2", "sampled_faces_indices"]
    for k in c_off:
        assert c_on[k].dtype == c_off[k].dtype and torch.equal(c_on[k], c_off[k]), k
    assert c_on["points1"].shape == (B, N, 3) and c_on["points2"].shape == (KB, N, 3) and c_on["sampled_faces_indices"].shape == (B, N)
    assert _same_bits(m_on, m_off)
    assert _same_bits(p_on, _pack(rendered, m_off))
    # ---- what the inputs must provide for the comparison to see anything (conditions of the inputs, checked on the separate utilities' results) ----
    img_k, p1, p2 = img.repeat(Ke, 1, 1, 1), c_off["points1"].repeat(Ke, 1, 1), c_off["points2"]
    assert bool((p2[..., 0] == 0).any()) and bool((p2[..., 1] == H - 1).any())             # points clamped onto borders
    if tv_dst is not None:
        # a pixel that is the target of two or more points whose SOURCE pixels differ: only there does "the highest index wins" decide the value (in the
        # first path every point is its own source, so points that share a target share the source too)
        tgt = (torch.arange(KB, device="cuda")[:, None] * H + p2[..., 1]) * W + p2[..., 0]
        src = p1[..., 1] * W + p1[..., 0]
        order = torch.argsort(tgt.flatten(), stable=True)
        t_sorted, s_sorted = tgt.flatten()[order], src.flatten()[order]
        contested = (t_sorted[1:] == t_sorted[:-1]) & (s_sorted[1:] != s_sorted[:-1])
        assert int(contested.sum()) > 0
    extra = M.transfer_pixels(img_k, p1, p2)
    took = (extra > 0) & (m_off != 0) & (m_off != img_k)                                   # hull of 0 / 1: an untransferred pixel is 0 or its own img value
    assert int(took.sum()) > 0                                                             # a sampled value, with its noise, survives into masked
    assert bool((m_off == 0).any())                                                        # and so does the other outcome of the composition
    if Ke > 1:
        assert not torch.equal(m_off[:B], m_off[B:2 * B])                                  # the Ke copies of a frame are different frames


P, Q, R, S, T, U, V_, X = (0x10000 * i for i in range(1, 9))                               # never dereferenced
BAD_ARG, UNSUPPORTED = -1, -4


def test_every_documented_refusal_comes_before_a_pointer_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()

    def sample(weights=P, tv_src=Q, tv_dst=R, faces=S, B=2, Ke=2, V=5023, F=9976, num=100, size=32, psrc=T, pdst=U, idx=None, bary=None, np1=None, np2=None):
        return lib.smirk_sample_transfer_points(weights, tv_src, tv_dst, faces, B, Ke, V, F, num, size, 1, 0, psrc, pdst, idx, bary, np1, np2, None)
    for name in ("weights", "tv_src", "faces", "psrc", "pdst"):
        assert sample(**{name: None}) == BAD_ARG, name
    for bad in (dict(B=0), dict(Ke=0), dict(V=0), dict(F=0), dict(num=0), dict(size=0), dict(B=-1), dict(F=38001), dict(size=32769)):
        assert sample(**bad) == BAD_ARG, bad
    # first path (no target vertices): Ke must be 1 and there is nothing to write for the targets
    for bad in (dict(Ke=2, pdst=None), dict(Ke=1, pdst=U), dict(Ke=1, pdst=None, np2=X)):
        assert sample(tv_dst=None, **bad) == BAD_ARG, bad

    def handoff(img=P, rendered=Q, hull=R, stride=32 * 48, psrc=S, pdst=T, B=2, Ke=2, N=100, H=32, W=48, rule=1, p=0.05, masked=U, packed=V_):
        return lib.smirk_train_masking_handoff(img, rendered, hull, stride, psrc, pdst, B, Ke, N, H, W, rule, p, 1, 0, 0, masked, packed, None)
    for name in ("img", "rendered", "hull", "psrc", "pdst", "masked", "packed"):
        assert handoff(**{name: None}) == BAD_ARG, name
    for bad in (dict(B=0), dict(Ke=0), dict(N=0), dict(H=0), dict(W=-1), dict(stride=48), dict(stride=-1), dict(p=0.0), dict(p=-0.5), dict(p=float("nan")),
                dict(rule=2), dict(rule=-1)):
        assert handoff(**bad) == BAD_ARG, bad
    # rows too wide for two workgroups per CU: the caller keeps the separate launches
    assert handoff(W=1024, stride=32 * 1024) == UNSUPPORTED and handoff(W=1024, stride=0) == UNSUPPORTED
    assert handoff(W=248, stride=0) == UNSUPPORTED                                         # 244 is the widest row whose band fits 80 KB
