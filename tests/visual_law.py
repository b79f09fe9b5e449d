"""The law of smirk_amd.visualize (csrc/visual.hip): the reference's visualisation sheet restated in numpy, float32 operation for operation.

cv2 and torchvision are not available where this suite runs, so parity with them is UNPINNED: `make_grid` restates torchvision.utils.make_grid from its
documented geometry and `draw_keypoints` restates cv2.circle(image, centre, 1, colour, -1) as the five pixels with dx^2 + dy^2 <= 1, clipped to the image.
Everything else follows the reference line by line (file:line beside each function).  The kernel is held to this file byte for byte.

Stated deviations (the same list as smirk_amd/visualize.py): on the landmark panel a value outside [0, 1] saturates where numpy's astype('uint8') wraps; a NaN pixel
becomes 0; a non-finite landmark is skipped where int() raises; columns whose grids differ in height raise ValueError.
"""
import math

import numpy as np

F = np.float32
PADDING = 2
IMAGE_KEYS = ('img_mica', 'rendered_img_base', 'rendered_img', 'overlap_image', 'overlap_image_pixels', 'rendered_img_mica_zero', 'rendered_img_zero',
              'masked_1st_path', 'reconstructed_img', 'loss_img', '2nd_path')                        # base_trainer.py:147-151
# base_trainer.py:138-141 in drawing order; the colours are cv2 BGR tuples on an image flipped to BGR (utils.py:73) and flipped back (utils.py:86): RGB here
LAYERS = (('landmarks_mp', None, (0, 255, 0)), ('landmarks_mp_gt', None, (255, 0, 0)), ('landmarks_fan', 17, (255, 0, 255)),
          ('landmarks_fan_gt', 17, (255, 255, 255)))


def make_grid(tensor, nrow=8, padding=PADDING, pad_value=0.0):
    """torchvision.utils.make_grid (normalize=False): float32 [N, C, H, W] -> [3, ymaps (H + p) + p, xmaps (W + p) + p]; a single image comes back unpadded."""
    t = np.asarray(tensor, F)
    assert t.ndim == 4 and t.shape[1] in (1, 3)
    if t.shape[1] == 1:
        t = np.concatenate([t, t, t], 1)
    N, _, H, W = t.shape
    if N == 1:
        return t[0].copy()
    xmaps = min(nrow, N)
    ymaps = int(math.ceil(float(N) / xmaps))
    h, w = H + padding, W + padding
    grid = np.full((3, h * ymaps + padding, w * xmaps + padding), pad_value, F)
    for k in range(N):
        y0, x0 = (k // xmaps) * h + padding, (k % xmaps) * w + padding
        grid[:, y0:y0 + H, x0:x0 + W] = t[k]
    return grid


def to_uint8_saturating(x):
    """utils.py:72  (images * 255).astype('uint8'): the product in float32, truncated; saturating outside [0, 255] and 0 for NaN (the stated deviations)."""
    with np.errstate(invalid="ignore"):
        t = np.asarray(x, F) * F(255)
        t = np.where(np.isnan(t), F(0), np.minimum(np.maximum(t, F(0)), F(255)))
    return t.astype(np.uint8)


def draw_keypoints(images_u8, landmarks, colour, centre=112.0):
    """utils.py:65-81 on uint8 [N, H, W, 3] RGB images (in place): points = lm * centre + centre in float32 (utils.py:68, centre = 112), int() toward zero,
    a filled radius-1 disc clipped to the image; non-finite points are skipped."""
    pts = np.asarray(landmarks, F) * F(centre) + F(centre)
    N, H, W, _ = images_u8.shape
    for img, lm in zip(images_u8, pts):
        for px, py in lm:
            if not (np.isfinite(px) and np.isfinite(py)) or abs(float(px)) >= 1.0e9 or abs(float(py)) >= 1.0e9:
                continue
            cx, cy = int(px), int(py)
            for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
                x, y = cx + dx, cy + dy
                if 0 <= x < W and 0 <= y < H:
                    img[y, x] = colour
    return images_u8


def landmark_panel(img, vis, centre=112.0):
    """base_trainer.py:138-142: the four layers in order on (img * 255).astype(uint8), then make_grid_from_opencv_images' float()/255. (utils.py:88)."""
    u8 = np.ascontiguousarray(to_uint8_saturating(img).transpose(0, 2, 3, 1))
    if u8.shape[-1] == 1:
        u8 = np.repeat(u8, 3, -1)
    for key, first, colour in LAYERS:
        lm = np.asarray(vis[key], F)
        draw_keypoints(u8, lm if first is None else lm[:, :first], colour, centre)
    return u8.transpose(0, 3, 1, 2).astype(F) / F(255)


def blend(img, other, w_img=0.7, w_other=0.3):
    """base_trainer.py:134-135: img * 0.7 + other * 0.3, the scalars as float32, both products and the sum rounded (no fma)."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.asarray(img, F) * F(w_img)
        b = np.asarray(other, F) * F(w_other)
        return a + b


def interleave_second_path(panels, Ke):
    """smirk_trainer.py:327-330: four [Ke * B, C, H, W] batches -> [B * Ke * 4, C, H, W] in the order (b, ke, which of the four)."""
    out = []
    for p in panels:
        p = np.asarray(p, F)
        KB, C, H, W = p.shape
        out.append(p.reshape(Ke, KB // Ke, C, H, W).transpose(1, 0, 2, 3, 4).reshape(-1, C, H, W))
    C, H, W = out[0].shape[1:]
    return np.stack(out, 1).reshape(-1, C, H, W)


def interpolate_nearest(x, size):
    """F.interpolate(x, size) with its default mode 'nearest' (base_trainer.py:211): source index floor(dst * float32(in / out)), clamped to in - 1."""
    x = np.asarray(x, F)
    Hs, Ws = x.shape[2:]

    def index(n_in, n_out):
        scale = F(n_in) / F(n_out)
        return np.minimum(np.floor(np.arange(n_out, dtype=F) * scale).astype(np.int64), n_in - 1)
    return x[:, :, index(Hs, size)][:, :, :, index(Ws, size)]


def quantise(grid, bgr=True):
    """base_trainer.py:157-160: permute, * 255.0, clip, astype(uint8), RGB -> BGR; NaN -> 0."""
    with np.errstate(invalid="ignore"):
        g = np.asarray(grid, F).transpose(1, 2, 0) * F(255)
        g = np.where(np.isnan(g), F(0), np.clip(g, F(0), F(255)))
    g = g.astype(np.uint8)
    return np.ascontiguousarray(g[..., ::-1]) if bgr else g


def round_trip_table():
    """trunc(float32(k / 255) * 255) for k = 0 .. 255: what a uint8 level of the landmark panel becomes on the sheet.  Computed as written, never assumed to be
    the identity: it is one with a correctly rounded float32 quotient, and a quotient one ulp low drops levels by one (tests/test_visual_cpu.py)."""
    k = np.arange(256, dtype=F)
    return (k / F(255) * F(255)).astype(np.uint8)


def sheet(vis, show_landmarks=False, Ke=1, bgr=True, centre=112.0):
    """base_trainer.py:130-160 on host arrays: `vis` maps the keys of create_visualizations to numpy arrays ('2nd_path': the four batches).  -> uint8 [H, W, 3]."""
    img = np.asarray(vis['img'], F)
    S = img.shape[2]
    panels = dict(vis)
    if all(k in vis for k in ('img', 'rendered_img', 'masked_1st_path')):
        panels['overlap_image'] = blend(img, vis['rendered_img'])
        panels['overlap_image_pixels'] = blend(img, vis['masked_1st_path'])
    if '2nd_path' in vis:
        panels['2nd_path'] = interleave_second_path(vis['2nd_path'], Ke)
    grids = [make_grid(landmark_panel(img, vis, centre) if show_landmarks else img, nrow=1)]
    for key in IMAGE_KEYS:
        if key in panels:
            p = np.asarray(panels[key], F)
            if p.shape[2:] != (S, S):
                p = interpolate_nearest(p, S)                                                      # img_mica, base_trainer.py:210-211
            grids.append(make_grid(p, nrow=4 * Ke if key == '2nd_path' else 1))
    if len({g.shape[1] for g in grids}) != 1:
        raise ValueError("grids of unequal height")                                                # torch.cat(dim=2) raises
    return quantise(np.concatenate(grids, 2), bgr)
