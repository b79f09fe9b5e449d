"""The law of the batch preparation (smirk_amd.data; reference: datasets/base_dataset.py:124-215 prepare_data) — helper module, no tests.

What smirk_amd/csrc/data.hip computes, restated function by function in numpy integers / float64 from the Philox words up (counter layout:
smirk_amd/csrc/data_rng.h).  The kernels are compiled with floating-point contraction off and every expression below is written in the order the kernel evaluates
it, so the two sides agree bit for bit except where a libm function (pow, cbrt, log, cos, sin) differs in its last place AND the result sits on a rounding
boundary.

PARITY UNPINNED: the reference does this arithmetic with cv2, skimage and albumentations, none of which is on disk.  The law is this project's own; it follows the
documented behaviour of albumentations 1.3.0, OpenCV 4.9 and skimage 0.22, with the deviations listed in smirk_amd/data.py.  The self-checks of
tests/test_data_cpu.py keep the restatement honest without those sources (train with every p = 0 equals test, zero ShiftScaleRotate is the identity, crop / hull /
similarity against oracle.video_ref, CLAHE of a constant image, blur of a constant image).
"""
import numpy as np

from augment_law import _normal2, philox

STREAM_FRAME, STREAM_PIXEL, FRAME_COUNTERS = 6, 7, 8
MICA = 112
ARCFACE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], dtype=np.float32).astype(np.float64)
TRANSFORMS = ("brightness_contrast", "gamma", "color_jitter", "clahe", "rgb_shift", "blur", "gauss_noise", "shift_scale_rotate")
f32 = np.float32


def n_counters(N, S):
    return N * max(S * S, FRAME_COUNTERS)


def _u01(x):
    return float(int(x) >> 8) / 16777216.0


def _uniform(x, lo, hi):
    return lo + (hi - lo) * _u01(x)


# ---- per-frame parameters ----------------------------------------------------------------------------------------------------------------------------------------
def crop_similarity(lm_mp, scale, S):
    """crop_face in closed form -> (fwd, inv) 2x3 row-major lists: frame (x, y) -> crop, crop (col, row) -> frame"""
    lm = np.asarray(lm_mp, np.float64)
    left, right, top, bottom = lm[:, 0].min(), lm[:, 0].max(), lm[:, 1].min(), lm[:, 1].max()
    old_size = (right - left + bottom - top) / 2
    cx, cy = right - (right - left) / 2.0, bottom - (bottom - top) / 2.0
    size = float(max(int(old_size * scale), 1))
    s, si = (S - 1) / size, size / (S - 1)
    x0, y0 = cx - size / 2.0, cy - size / 2.0
    return [s, 0.0, -s * x0, 0.0, s, -s * y0], [si, 0.0, x0, 0.0, si, y0]


def ssr_matrices(S, angle, zoom, dx, dy):
    """cv2.getRotationMatrix2D(((S-1)/2, (S-1)/2), angle, zoom) with (dx S, dy S) added to the translation, and its inverse"""
    rad, c = angle * (3.141592653589793 / 180.0), (S - 1) / 2.0
    a, b = zoom * np.cos(rad), zoom * np.sin(rad)
    m = [a, b, ((1.0 - a) * c - b * c) + dx * float(S), -b, a, (b * c + (1.0 - a) * c) + dy * float(S)]
    det = a * a + b * b
    ia, ib = a / det, b / det
    mi = [ia, -ib, 0.0, ib, ia, 0.0]
    mi[2] = -(mi[0] * m[2] + mi[1] * m[5])
    mi[5] = -(mi[3] * m[2] + mi[4] * m[5])
    return [float(v) for v in m], [float(v) for v in mi]


IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def arcface_points(fan):
    fan = np.asarray(fan, np.float64)
    return np.stack([(fan[36] + fan[39]) / 2, (fan[42] + fan[45]) / 2, fan[32], fan[48], fan[54]])


def similarity_closed_form(src, dst):
    """least-squares similarity dst ~ [[a, -b], [b, a]] src + t about the centroids -> (a, b, tx, ty)"""
    seq = lambda v: ((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) / 5.0
    msx, msy, mdx, mdy = seq(src[:, 0]), seq(src[:, 1]), seq(dst[:, 0]), seq(dst[:, 1])
    na = nb = den = 0.0
    for i in range(5):
        xs, ys, xd, yd = src[i, 0] - msx, src[i, 1] - msy, dst[i, 0] - mdx, dst[i, 1] - mdy
        na += xs * xd + ys * yd
        nb += xs * yd - ys * xd
        den += xs * xs + ys * ys
    a, b = na / den, nb / den
    return a, b, mdx - (a * msx - b * msy), mdy - (b * msx + a * msy)


def arcface_inverse(fan):
    """output (col, row) of the 112 x 112 MICA image -> frame (x, y)"""
    a, b, tx, ty = similarity_closed_form(arcface_points(fan), ARCFACE)
    det = a * a + b * b
    ia, ib = a / det, b / det
    return [ia, ib, -(ia * tx + ib * ty), -ib, ia, -(-ib * tx + ia * ty)]


def draw_frame(cfg, scale, S, seed, offset, f):
    """every draw and coin of frame f (cfg: an AugmentConfig) -> dict; `used` lists the local counter indices touched"""
    base = offset + FRAME_COUNTERS * f
    w = [[int(v[0]) for v in philox(np.array([base + j], dtype=np.uint64), STREAM_FRAME, seed)] for j in range(7)]
    p = cfg.probabilities()
    P = dict(used=[FRAME_COUNTERS * f + j for j in range(7)])
    coins = 0
    P["scale"] = _uniform(w[0][0], scale[0], scale[1])
    coins |= (_u01(w[0][1]) < p[0]) << 0
    P["bc_alpha"] = 1.0 + _uniform(w[0][2], -cfg.contrast_limit, cfg.contrast_limit)
    P["bc_beta"] = _uniform(w[0][3], -cfg.brightness_limit, cfg.brightness_limit)
    coins |= (_u01(w[1][0]) < p[1]) << 1
    P["gamma"] = _uniform(w[1][1], float(cfg.gamma_limit[0]), float(cfg.gamma_limit[1])) / 100.0
    coins |= (_u01(w[1][2]) < p[2]) << 2
    P["cj"] = [1.0 + _uniform(w[1][3], -cfg.jitter_brightness, cfg.jitter_brightness), 1.0 + _uniform(w[2][0], -cfg.jitter_contrast, cfg.jitter_contrast),
               1.0 + _uniform(w[2][1], -cfg.jitter_saturation, cfg.jitter_saturation), _uniform(w[2][2], -cfg.jitter_hue, cfg.jitter_hue)]
    coins |= (_u01(w[2][3]) < p[3]) << 3
    P["clahe_clip"] = _uniform(w[3][0], float(cfg.clahe_clip_limit[0]), float(cfg.clahe_clip_limit[1]))
    coins |= (_u01(w[3][1]) < p[4]) << 4
    P["rgb_shift"] = [_uniform(w[3][2], -float(cfg.rgb_shift_limit), float(cfg.rgb_shift_limit)), _uniform(w[3][3], -float(cfg.rgb_shift_limit), float(cfg.rgb_shift_limit)),
                      _uniform(w[4][0], -float(cfg.rgb_shift_limit), float(cfg.rgb_shift_limit))]
    coins |= (_u01(w[4][1]) < p[5]) << 5
    P["blur_k"] = 3 + 2 * ((w[4][2] * ((int(cfg.blur_limit) - 1) // 2)) >> 32)
    coins |= (_u01(w[4][3]) < p[6]) << 6
    P["noise_sigma"] = float(np.sqrt(_uniform(w[5][0], float(cfg.noise_var_limit[0]), float(cfg.noise_var_limit[1]))))
    coins |= (_u01(w[5][1]) < p[7]) << 7
    P["ssr_angle"] = _uniform(w[5][2], -float(cfg.rotate_limit), float(cfg.rotate_limit))
    P["ssr_scale"] = 1.0 + _uniform(w[5][3], -cfg.scale_limit, cfg.scale_limit)
    P["ssr_dx"] = _uniform(w[6][0], -cfg.shift_limit, cfg.shift_limit)
    P["ssr_dy"] = _uniform(w[6][1], -cfg.shift_limit, cfg.shift_limit)
    P["coins"] = int(coins)
    P["ssr_fwd"], P["ssr_inv"] = ssr_matrices(S, P["ssr_angle"], P["ssr_scale"], P["ssr_dx"], P["ssr_dy"]) if coins >> 7 & 1 else (IDENTITY, IDENTITY)
    return P


def neutral_params(scale):
    return dict(scale=scale, coins=0, ssr_fwd=IDENTITY, ssr_inv=IDENTITY, used=[])


# ---- landmarks ------------------------------------------------------------------------------------------------------------------------------------------------------
def crop_points(pts, fwd):
    pts = np.asarray(pts, np.float64)[:, :2]
    return np.stack([fwd[0] * pts[:, 0] + fwd[2], fwd[4] * pts[:, 1] + fwd[5]], 1)


def landmarks_out(pts, fwd, m, S):
    """float64 crop -> ShiftScaleRotate -> cast to float32 -> / S, * 2, - 1, each rounded in float32 (base_dataset.py:173-174)"""
    c = crop_points(pts, fwd)
    x, y = c[:, 0], c[:, 1]
    a = np.stack([(m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5]], 1).astype(f32)
    a = (a / f32(S)).astype(f32)
    a = (a * f32(2)).astype(f32)
    return (a - f32(1)).astype(f32)


def hull_points(lm_mp, fwd):
    """create_mask's landmarks.astype(np.int32): ALL cropped points, truncated toward zero"""
    return crop_points(lm_mp, fwd).astype(np.int32)


def hull_mask(points, S):
    """1 outside / 0 inside the convex hull of integer points [L, 2]: gift wrapping, then per row the span [floor(x_left + .5), floor(x_right + .5)] of the closed
    polygon (cv2.fillConvexPoly's rounding; its outline pass is not restated, as in oracle.video_ref.hull_mask)"""
    pts = sorted(set(map(tuple, np.asarray(points, np.int64).tolist())))
    hull = [pts[0]]                                           # smallest (x, y): a vertex
    while True:
        cx, cy = hull[-1]
        q = None
        for p in pts:
            if p == (cx, cy):
                continue
            if q is None:
                q = p
                continue
            cr = (q[0] - cx) * (p[1] - cy) - (q[1] - cy) * (p[0] - cx)
            if cr < 0 or (cr == 0 and (p[0] - cx) ** 2 + (p[1] - cy) ** 2 > (q[0] - cx) ** 2 + (q[1] - cy) ** 2):
                q = p
        if q is None or q == hull[0] or len(hull) > len(pts):
            break
        hull.append(q)
    mask = np.ones((S, S), np.uint8)
    h = np.array(hull, np.int64)
    n = len(h)
    for y in range(max(int(h[:, 1].min()), 0), min(int(h[:, 1].max()), S - 1) + 1):
        xl, xr = np.inf, -np.inf
        for i in range(n):
            (x0, y0), (x1, y1) = h[i], h[(i + 1) % n]
            if min(y0, y1) <= y <= max(y0, y1):
                if y0 == y1:
                    xl, xr = min(xl, float(min(x0, x1))), max(xr, float(max(x0, x1)))
                else:
                    xx = x0 + float(x1 - x0) * float(y - y0) / float(y1 - y0)
                    xl, xr = min(xl, xx), max(xr, xx)
        if n == 1:
            xl = xr = float(h[0, 0])
        a, b = max(int(np.floor(xl + 0.5)), 0), min(int(np.floor(xr + 0.5)), S - 1)
        if a <= b:
            mask[y, a:b + 1] = 0
    return mask


# ---- warps ------------------------------------------------------------------------------------------------------------------------------------------------------------
def _grid(n):
    cc, rr = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64))
    return cc, rr


def _px(img, r, c):
    """img [H, W, C] float64 at float64 integer-valued (r, c); 0 outside"""
    H, W = img.shape[:2]
    ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
    v = img[np.clip(r, 0, H - 1).astype(np.int64), np.clip(c, 0, W - 1).astype(np.int64)]
    return np.where(ok[..., None], v, 0.0)


def warp_crop(frame_bgr, inv, S):
    """skimage.transform.warp(order=1, mode='constant', preserve_range=True).astype(uint8) of the BGR -> RGB frame: float64 bilinear over floor / ceil neighbours"""
    img = np.asarray(frame_bgr)[..., ::-1].astype(np.float64)
    cc, rr = _grid(S)
    x = inv[0] * cc + inv[1] * rr + inv[2]
    y = inv[3] * cc + inv[4] * rr + inv[5]
    minr, minc, maxr, maxc = np.floor(y), np.floor(x), np.ceil(y), np.ceil(x)
    dr, dc = (y - minr)[..., None], (x - minc)[..., None]
    top = (1 - dc) * _px(img, minr, minc) + dc * _px(img, minr, maxc)
    bot = (1 - dc) * _px(img, maxr, minc) + dc * _px(img, maxr, maxc)
    return ((1 - dr) * top + dr * bot).astype(np.uint8)


def warp_mica(frame_bgr, q):
    """cv2.warpAffine(image / 255., M, (112, 112), borderValue=0.0) through the inverse q: float64 bilinear, floor neighbours -> float32 [3, 112, 112] RGB"""
    img = np.asarray(frame_bgr)[..., ::-1].astype(np.float64)
    cc, rr = _grid(MICA)
    x = q[0] * cc + q[1] * rr + q[2]
    y = q[3] * cc + q[4] * rr + q[5]
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    p00, p01, p10, p11 = _px(img, y0, x0) / 255.0, _px(img, y0, x0 + 1) / 255.0, _px(img, y0 + 1, x0) / 255.0, _px(img, y0 + 1, x0 + 1) / 255.0
    v = (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11)
    return v.astype(f32).transpose(2, 0, 1)


def resample(img_u8, hull, mi):
    """ShiftScaleRotate: image by float64 bilinear through the inverse with the constant 0 border taking part and round-half-even; mask by nearest
    (floor(coord + 0.5)) on 1 - hull with border 0, returned as 1 - that"""
    S = img_u8.shape[0]
    img = img_u8.astype(np.float64)
    cc, rr = _grid(S)
    x = (mi[0] * cc + mi[1] * rr) + mi[2]
    y = (mi[3] * cc + mi[4] * rr) + mi[5]
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    v = (1 - fy) * ((1 - fx) * _px(img, y0, x0) + fx * _px(img, y0, x0 + 1)) + fy * ((1 - fx) * _px(img, y0 + 1, x0) + fx * _px(img, y0 + 1, x0 + 1))
    out = np.rint(np.clip(v, 0.0, 255.0)).astype(np.uint8)
    sx, sy = np.floor(x + 0.5), np.floor(y + 0.5)
    inside = (sx >= 0) & (sx < S) & (sy >= 0) & (sy < S)
    m = np.where(inside, hull[np.clip(sy, 0, S - 1).astype(np.int64), np.clip(sx, 0, S - 1).astype(np.int64)], 1)
    return out, m.astype(np.uint8)


# ---- colour, all on integer levels ----------------------------------------------------------------------------------------------------------------------------------
def _trunc(v):
    return np.clip(v, 0.0, 255.0).astype(np.int64)


def _rint(v):
    return np.rint(np.clip(v, 0.0, 255.0)).astype(np.int64)


def grey(img):
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14


def lut_brightness_contrast(alpha, beta):
    return _trunc(np.arange(256) * alpha + beta * 255.0)


def lut_gamma(g):
    return _trunc(np.power(np.arange(256) / 255.0, g) * 255.0)


def lut_jitter(fb, fc, mean):
    v = _trunc(np.arange(256) * fb)
    return _trunc(v * fc + (1.0 - fc) * mean)


def saturation_hue(img, fs, hue):
    img = np.asarray(img, np.int64)
    gr = grey(img).astype(np.float64)[..., None]
    img = _rint(fs * img + (1.0 - fs) * gr)
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    v, mn = img.max(-1), img.min(-1)
    d = v - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        s8 = np.where(v > 0, np.rint(255.0 * d / v.astype(np.float64)), 0.0).astype(np.int64)
        dd = d.astype(np.float64)
        h = np.where(v == r, 60.0 * (g - b) / dd, np.where(v == g, 120.0 + 60.0 * (b - r) / dd, 240.0 + 60.0 * (r - g) / dd))
    h = np.where(d != 0, h, 0.0)
    h = np.where(h < 0.0, h + 360.0, h)
    h8 = np.rint(h / 2.0).astype(np.int64)
    h8 = np.where(h8 >= 180, h8 - 180, h8)
    t = h8 + hue * 180.0
    t = t - 180.0 * np.floor(t / 180.0)
    t = np.where(t >= 180.0, t - 180.0, t)
    h8 = t.astype(np.int64)
    hh = (2 * h8) / 60.0
    sec = np.floor(hh)
    f, s, vv = hh - sec, s8 / 255.0, v.astype(np.float64)
    p, q, u = vv * (1.0 - s), vv * (1.0 - s * f), vv * (1.0 - s * (1.0 - f))
    k = sec.astype(np.int64)
    rr = np.where((k == 0) | (k == 5), vv, np.where(k == 1, q, np.where(k == 4, u, p)))
    gg = np.where((k == 1) | (k == 2), vv, np.where(k == 0, u, np.where(k == 3, q, p)))
    bb = np.where((k == 3) | (k == 4), vv, np.where(k == 2, u, np.where(k == 5, q, p)))
    return np.stack([_rint(rr), _rint(gg), _rint(bb)], -1)


def _srgb_to_linear():
    u = np.arange(256) / 255.0
    return np.where(u <= 0.04045, u / 12.92, np.power((u + 0.055) / 1.055, 2.4))


def _lab_f(t):
    return np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)


def _lab_finv(t):
    t3 = t * t * t
    return np.where(t3 > 0.008856, t3, (t - 16.0 / 116.0) / 7.787)


def _linear_to_srgb(c):
    with np.errstate(invalid="ignore"):
        return np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(np.maximum(c, 0.0031308), 1.0 / 2.4) - 0.055)


def rgb_to_lab8(img):
    lin = _srgb_to_linear()
    R, G, B = lin[img[..., 0]], lin[img[..., 1]], lin[img[..., 2]]
    X = ((0.412453 * R + 0.357580 * G) + 0.180423 * B) / 0.950456
    Y = 0.212671 * R + 0.715160 * G + 0.072169 * B
    Z = ((0.019334 * R + 0.119193 * G) + 0.950227 * B) / 1.088754
    fy = _lab_f(Y)
    l8 = _rint(2.55 * np.where(Y > 0.008856, 116.0 * fy - 16.0, 903.3 * Y))
    return l8, _rint(500.0 * (_lab_f(X) - fy) + 128.0), _rint(200.0 * (fy - _lab_f(Z)) + 128.0)


def lab8_to_rgb(l8, a8, b8):
    Lv, av, bv = l8 / 2.55, a8 - 128.0, b8 - 128.0
    big = Lv > 7.9996248
    gy_big = (Lv + 16.0) / 116.0
    Y = np.where(big, gy_big * gy_big * gy_big, Lv / 903.3)
    gy = np.where(big, gy_big, 7.787 * Y + 16.0 / 116.0)
    Xn, Zn = _lab_finv(gy + av / 500.0) * 0.950456, _lab_finv(gy - bv / 200.0) * 1.088754
    Rl = (3.240479 * Xn - 1.53715 * Y) - 0.498535 * Zn
    Gl = (-0.969256 * Xn + 1.875991 * Y) + 0.041556 * Zn
    Bl = (0.055648 * Xn - 0.204043 * Y) + 1.057311 * Zn
    return np.stack([_rint(255.0 * _linear_to_srgb(Rl)), _rint(255.0 * _linear_to_srgb(Gl)), _rint(255.0 * _linear_to_srgb(Bl))], -1)


def clahe_tables(l8, clip_limit, T=8):
    """cv::CLAHE on an 8-bit plane: per tile histogram, clip at max(int(clip * area / 256), 1), excess redistributed as excess / 256 per bin plus the strided
    residual walk, table = rint(cdf * 255 / area) -> uint8-valued [T, T, 256]"""
    S = l8.shape[0]
    th = S // T
    area = th * th
    clip = max(int(clip_limit * area / 256.0), 1)
    out = np.zeros((T, T, 256), np.int64)
    for ty in range(T):
        for tx in range(T):
            h = np.bincount(l8[ty * th:(ty + 1) * th, tx * th:(tx + 1) * th].ravel(), minlength=256).astype(np.int64)
            clipped = int(np.maximum(h - clip, 0).sum())
            h = np.minimum(h, clip)
            batch = clipped // 256
            resid = clipped - batch * 256
            h += batch
            if resid:
                step = max(256 // resid, 1)
                i = 0
                while i < 256 and resid > 0:
                    h[i] += 1
                    i += step
                    resid -= 1
            out[ty, tx] = _rint(np.cumsum(h) * 255.0 / float(area))
    return out


def clahe_apply(l8, tables, T=8):
    S = l8.shape[0]
    th = S // T
    rows, cols = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    tyf, txf = rows / float(th) - 0.5, cols / float(th) - 0.5
    ty0, tx0 = np.floor(tyf), np.floor(txf)
    ya, xa = tyf - ty0, txf - tx0
    ty1, ty2 = np.maximum(ty0.astype(np.int64), 0), np.minimum(ty0.astype(np.int64) + 1, T - 1)
    tx1, tx2 = np.maximum(tx0.astype(np.int64), 0), np.minimum(tx0.astype(np.int64) + 1, T - 1)
    v11, v12, v21, v22 = (tables[a, b, l8].astype(np.float64) for a, b in ((ty1, tx1), (ty1, tx2), (ty2, tx1), (ty2, tx2)))
    return _rint((v11 * (1.0 - xa) + v12 * xa) * (1.0 - ya) + (v21 * (1.0 - xa) + v22 * xa) * ya)


def clahe(img, clip_limit):
    l8, a8, b8 = rgb_to_lab8(img)
    return lab8_to_rgb(clahe_apply(l8, clahe_tables(l8, clip_limit)), a8, b8)


def rgb_shift(img, shifts):
    return np.stack([_trunc(img[..., c] + shifts[c]) for c in range(3)], -1)


def blur(img, k):
    """cv2.blur: integer box sum over k x k with BORDER_REFLECT_101, rint(sum / k^2)"""
    h = k // 2
    pad = np.pad(np.asarray(img, np.int64), ((h, h), (h, h), (0, 0)), mode="reflect")
    S0, S1 = img.shape[:2]
    acc = np.zeros(img.shape, np.int64)
    for dy in range(k):
        for dx in range(k):
            acc += pad[dy:dy + S0, dx:dx + S1]
    return _rint(acc / float(k * k))


def gauss_noise(img, sigma, seed, offset, f, used=None):
    S = img.shape[0]
    local = f * S * S + np.arange(S * S, dtype=np.int64)
    if used is not None:
        used.extend((int(local[0]), int(local[-1])))
    x0, x1, x2, x3 = philox((np.uint64(offset) + local.astype(np.uint64)), STREAM_PIXEL, seed)
    (zr, zg), (zb, _) = _normal2(x0, x1), _normal2(x2, x3)
    z = np.stack([zr, zg, zb], -1).reshape(S, S, 3)
    return _trunc(img + sigma * z)


def colour_chain(crop_rgb, P, seed, offset, f):
    """the seven colour / filter transforms in the reference's order on integer levels [S, S, 3]"""
    img = np.asarray(crop_rgb, np.int64)
    c = P["coins"]
    if c >> 0 & 1:
        img = lut_brightness_contrast(P["bc_alpha"], P["bc_beta"])[img]
    if c >> 1 & 1:
        img = lut_gamma(P["gamma"])[img]
    if c >> 2 & 1:
        mean = int(float(grey(img).sum()) / float(img.shape[0] * img.shape[1]) + 0.5)
        img = lut_jitter(P["cj"][0], P["cj"][1], mean)[img]
        img = saturation_hue(img, P["cj"][2], P["cj"][3])
    if c >> 3 & 1:
        img = clahe(img, P["clahe_clip"])
    if c >> 4 & 1:
        img = rgb_shift(img, P["rgb_shift"])
    if c >> 5 & 1:
        img = blur(img, P["blur_k"])
    if c >> 6 & 1:
        img = gauss_noise(img, P["noise_sigma"], seed, offset, f, P["used_pixels"])
    return img


# ---- one batch ------------------------------------------------------------------------------------------------------------------------------------------------------
def prepare(frames, landmarks_fan, landmarks_mp, mp_indices, S, scale, cfg=None, seed=0, offset=0, cache=None):
    """cfg None: the deterministic path at scale (a float); else the training path with scale = (lo, hi).  -> dict of stacked numpy arrays: img levels uint8
    [N, 3, S, S] (img = levels / 255 in float32), mask uint8 [N, 1, S, S], landmarks float32, flag bool, img_mica float32, plus `params` (list of dicts) and
    `counters_used` (the largest local counter index touched + 1, or 0).  `cache`: a dict that keeps (crop, hull) per (frame index, scale, S) between calls
    on the same inputs."""
    out = dict(img_levels=[], mask=[], landmarks_fan=[], landmarks_mp=[], flag_landmarks_fan=[], img_mica=[], params=[])
    top = -1
    for f, (frame, fan, mp) in enumerate(zip(frames, landmarks_fan, landmarks_mp)):
        P = neutral_params(float(scale)) if cfg is None else draw_frame(cfg, scale, S, seed, offset, f)
        P["used_pixels"] = []
        flag = fan is not None
        fan_pts = np.zeros((68, 2)) if fan is None else np.asarray(fan, np.float64)[:, :2]
        fwd, inv = crop_similarity(mp, P["scale"], S)
        P["crop_fwd"], P["crop_inv"] = fwd, inv
        key = (f, P["scale"], S)
        if cache is None or key not in cache:
            made = (warp_crop(frame, inv, S).astype(np.int64), hull_mask(hull_points(mp, fwd), S))
            if cache is not None:
                cache[key] = made
        img, hull = cache[key] if cache is not None else made
        if cfg is not None:
            img = colour_chain(img, P, seed, offset, f)
            img, hull = resample(img.astype(np.uint8), hull, P["ssr_inv"])
        P["mica_inv"] = arcface_inverse(fan_pts) if flag else [0.0] * 6
        out["img_levels"].append(np.asarray(img, np.uint8).transpose(2, 0, 1))
        out["mask"].append(hull[None])
        out["landmarks_fan"].append(landmarks_out(fan_pts, fwd, P["ssr_fwd"], S))
        out["landmarks_mp"].append(landmarks_out(np.asarray(mp, np.float64)[np.asarray(mp_indices), :2], fwd, P["ssr_fwd"], S))
        out["flag_landmarks_fan"].append(flag)
        out["img_mica"].append(warp_mica(frame, P["mica_inv"]) if flag else np.zeros((3, MICA, MICA), f32))
        out["params"].append(P)
        top = max([top] + P["used"] + P["used_pixels"])
    res = {k: np.stack(v) for k, v in out.items() if k != "params"}
    res["params"] = out["params"]
    res["counters_used"] = top + 1
    return res


# ---- synthetic inputs of the tests ----------------------------------------------------------------------------------------------------------------------------------
SIZES = ((96, 80), (131, 157), (224, 224), (300, 211), (64, 64))         # (H, W): mixed resolutions, one below and one above the crop size


def synth_frame(H, W, seed):
    """smooth-plus-noise content of synthdata.synth_images at [H, W], uint8 BGR"""
    import torch
    import torch.nn.functional as F
    import synthdata
    img = synthdata.synth_images(1, seed=seed)
    if (H, W) != (224, 224):
        img = F.interpolate(img, size=(H, W), mode="bilinear", align_corners=False)
    return np.ascontiguousarray((img[0].permute(1, 2, 0).numpy()[..., ::-1] * 255.0).astype(np.uint8))


def synth_landmarks(H, W, seed, L=478, overhang=False):
    """L mediapipe points and 68 FAN points spread over a face-sized box of an [H, W] frame (x, y, and a third column that must be ignored); `overhang` pushes the
    box over the frame's right / bottom edge so that the crop reads the constant border"""
    r = np.random.default_rng(seed)
    cx, cy, half = (0.78 * W, 0.8 * H, 0.3 * min(H, W)) if overhang else (0.5 * W + r.uniform(-3, 3), 0.52 * H + r.uniform(-3, 3), 0.27 * min(H, W))
    ang = r.uniform(0, 2 * np.pi, L)
    rad = half * np.sqrt(r.uniform(0, 1, L))
    mp = np.stack([cx + rad * np.cos(ang), cy + 1.15 * rad * np.sin(ang), r.standard_normal(L)], 1)
    fan = np.stack([cx + half * r.uniform(-0.9, 0.9, 68), cy + half * r.uniform(-0.9, 0.9, 68)], 1)
    # eyes left / right of the nose, mouth corners below: the ArcFace template's order, so that the fitted similarity is a proper rotation
    fan[36], fan[39], fan[42], fan[45] = (cx - 0.5 * half, cy - 0.3 * half), (cx - 0.25 * half, cy - 0.3 * half), (cx + 0.25 * half, cy - 0.3 * half), (cx + 0.5 * half, cy - 0.3 * half)
    fan[32], fan[48], fan[54] = (cx + 0.02 * half, cy + 0.1 * half), (cx - 0.3 * half, cy + 0.5 * half), (cx + 0.3 * half, cy + 0.5 * half)
    fan += r.uniform(-0.03, 0.03, fan.shape) * half
    return fan, mp


def synth_batch(seed=0, L=478, sizes=SIZES, none_at=1, overhang_at=3):
    """the mixed-size batch of the tests: (frames, landmarks_fan with one None, landmarks_mp)"""
    frames, fans, mps = [], [], []
    for i, (H, W) in enumerate(sizes):
        frames.append(synth_frame(H, W, seed + 10 * i))
        fan, mp = synth_landmarks(H, W, seed + 100 + i, L=L, overhang=(i == overhang_at))
        fans.append(None if i == none_at else fan)
        mps.append(mp)
    return frames, fans, mps
