"""masking_handoff_kernel (include/smirk_handoff.h) against the six launches it stands for: with $SMIRK_DISABLE_MASKING_HANDOFF set and unset, under one pinned
PhiloxStream, masked_img and the generator's packed input must be the same bits.  The shapes are the smallest at which the kernel can go wrong: one band with the
halo wholly outside the image, a ragged second band, a width that is no multiple of 4, a height below the radius, and the demo's 224 x 224."""
import os

import pytest
import torch

from oracle.flame_ref import FlameRef

pytestmark = pytest.mark.gpu

SWITCH = "SMIRK_DISABLE_MASKING_HANDOFF"
# The kernel works in bands of 16 rows.  (B, H, W, hull mask, probability of a patch centre): at 0.05 the 11 x 11 patches overlap every border and cover all but
# 0.2 % of the pixels; at 0.01 they leave 30 % uncovered, so sampled points survive and their noise reaches the output
CASES = [(2, 32, 32, "blocks", 0.05),    # the 10-row halo lies wholly outside the image above the first band and below the last
         (3, 48, 48, "shared", 0.05),    # three bands; ONE [1,H,W] hull mask for the whole batch (batch stride 0)
         (2, 40, 48, "blocks", 0.01),    # a ragged last band (40 = 2 x 16 + 8)
         (2, 37, 45, "values", 0.05),    # W no multiple of 4, odd sizes, a hull mask of arbitrary values
         (1, 8, 224, "blocks", 0.05),    # one band; H smaller than either radius
         (2, 224, 224, "blocks", 0.01)]
RATIO = 0.04                             # x 5 = 0.2 H^2 sampled points per image: enough of them at 32 x 32 too


@pytest.fixture(scope="module")
def mesh(sandbox):
    from smirk_amd import masking as M
    cwd = os.getcwd(); os.chdir(sandbox)
    try:
        prob = M.load_probabilities_per_FLAME_triangle().cuda()
    finally:
        os.chdir(cwd)
    return M, prob, torch.from_numpy(FlameRef(sandbox).faces).cuda()


def _hull(kind, B, H, W, g):
    """1 = keep the photo.  The zero (face) regions reach all four borders and the corners."""
    if kind == "values":
        return torch.rand(B, 1, H, W, generator=g)
    h = torch.ones(1 if kind == "shared" else B, 1, H, W)
    for b in range(h.shape[0]):
        o = b % 2
        h[b, :, : max(1, H // 3), W // 4 + o: W // 2] = 0                  # top border
        h[b, :, H // 2:, : max(1, W // 5) + o] = 0                         # left border and the bottom-left corner
        h[b, :, H // 4: H // 2 + 1, W - max(1, W // 6):] = 0               # right border
        h[b, :, H - 1, W // 2:] = 0                                        # bottom border and the bottom-right corner
        h[b, :, 0, 0] = 0
    return h[:, 0] if kind == "shared" else h                              # "shared": the reference's own call shape, [1,H,W]


def _inputs(B, H, W, kind, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, W, generator=g)
    img[:, :, ::7, ::5] = 0.0                                              # exact zeros and a few negative values: `extra > 0` must fail there
    img[:, 1, 3::11, 2::9] *= -1.0
    rendered = torch.rand(B, 3, H, W, generator=g)
    rendered[:, :, : H // 2, : (2 * W) // 3] = 0.0                         # background of the rendering (all three channels zero), up to two borders
    rendered[:, 0, H // 2:, ::3] = 0.0                                     # one zero channel is not background
    tv = torch.randn(B, 5023, 3, generator=g) * 0.9                        # sampled points land all over the image; those beyond it are clamped onto its borders
    return img.cuda(), rendered.cuda(), _hull(kind, B, H, W, g).cuda(), tv.cuda()


def _run(mesh, inputs, monkeypatch, off, p_field):
    M, prob, faces = mesh
    img, rendered, hull, tv = inputs
    if off:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    rng = M.PhiloxStream(0x5EED, 12345)
    masked, packed = M.demo_masked_image_packed(img, hull, rendered, tv, faces, prob, mask_ratio=RATIO, rng=rng, random_mask=p_field)
    return masked, packed, rng.offset


def _pack(rendered, masked):
    from smirk_amd import _lib as L
    B, _, H, W = rendered.shape
    out = torch.empty(B, H, W, 8, device=rendered.device)
    L.check(L.lib().smirk_pack_generator_input_split16(L.ptr(rendered), 3, L.ptr(masked), 3, L.ptr(out), B, H, W, L.stream_ptr()))
    return out


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("B,H,W,kind,p_field", CASES)
def test_one_launch_equals_the_six_bit_for_bit(mesh, monkeypatch, B, H, W, kind, p_field):
    inputs = _inputs(B, H, W, kind, seed=100 + H + W)
    m_off, p_off, end_off = _run(mesh, inputs, monkeypatch, True, p_field)
    m_on, p_on, end_on = _run(mesh, inputs, monkeypatch, False, p_field)
    assert p_off is None and p_on is not None and p_on.shape == (B, H, W, 8)
    assert end_on == end_off                                               # the same Philox counters were consumed: later draws of the stream do not move
    torch.cuda.synchronize()
    assert _same_bits(m_on, m_off)
    assert _same_bits(p_on, _pack(inputs[1], m_off))
    if H == 224:                                                           # what the inputs promise where there are enough points to promise it
        M, prob, faces = mesh
        pm = M._demo_points_mask(inputs[0], inputs[3], faces, prob, RATIO, 5, M.PhiloxStream(0x5EED, 12345))
        assert bool(pm[:, :, 0, :].any()) and bool(pm[:, :, :, 0].any())  # sampled points on border pixels
        took = (pm != 0).expand_as(m_on) & (m_on > 0) & (m_on != inputs[0])
        assert int(took.sum()) > 100 and bool((m_on == 0).any())           # both outcomes of the composition, the first with its noise


def test_zero_extra_points_skip_the_noise_and_the_rest_still_draws_it(mesh, monkeypatch):
    """Where pmask == 0 the output is img * mask_d * (1 - rendered_mask) exactly, whichever path computed it; where pmask != 0 some pixels differ from it."""
    M, prob, faces = mesh
    B, H, W = 2, 224, 224
    img, rendered, hull, tv = _inputs(B, H, W, "blocks", seed=7)
    rng = M.PhiloxStream(99, 0)
    npts, _ = M.mesh_based_mask_uniform_faces(tv, faces, prob, mask_ratio=0.05, IMAGE_SIZE=H, _rng_stream=rng)
    pmask = M.points_mask(npts, H, W)
    rmask = M.rendered_mask_of(rendered)
    mask_d = 1 - torch.nn.functional.max_pool2d(1 - hull, 21, 1, 10)
    want = img * (mask_d * (1 - rmask))
    out = M.masking(img, hull, None, 10, rendered_mask=rmask, _pmask=pmask, _rng_stream=M.PhiloxStream(99, 1 << 20))        # masking_compose_kernel
    monkeypatch.delenv(SWITCH, raising=False)
    fused, packed = M.demo_masked_image_packed(img, hull, rendered, tv, faces, prob, rng=M.PhiloxStream(99, 0))                # masking_handoff_kernel
    assert packed is not None
    torch.cuda.synchronize()
    pm_fused = M._demo_points_mask(img, tv, faces, prob, 0.01, 5, M.PhiloxStream(99, 0))      # the points the fused call sampled: the same stream from its start
    for got, pm in ((out, pmask), (fused, pm_fused)):
        zero = (pm == 0).expand_as(got)
        assert _same_bits(got[zero], want[zero])
        assert bool((got[~zero] != want[~zero]).any())
    hit = (pmask != 0).expand_as(out) & (out != want)
    ratio = out[hit] / img[hit]                                            # the kept extra points carry N(1, 0.05) noise
    assert ratio.numel() > 100 and abs(float(ratio.mean()) - 1) < 0.02 and 0.03 < float(ratio.std()) < 0.07
