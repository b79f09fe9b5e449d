"""smirk_amd.data without a GPU: the extension table of include/smirk_data.h against its header, every refusal of every entry (raw ctypes, dummy pointers that
are never dereferenced: a refusal comes before anything touches the device), the Python refusals (numpy only), and the self-checks that keep the law of
tests/data_law.py honest without the third-party sources it restates."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import data_law as LAW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, R, S_, T, U, V, W, X = (0x10000 * k for k in range(1, 10))         # never dereferenced
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def _indices():
    import synthdata
    return np.asarray(synthdata.load_bundle()["mp_landmark_indices"]).astype(np.int64).ravel()


# ---- the table --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_extension_table_equals_the_header():
    from smirk_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "smirk_data.h")).read()
    declared = set(re.findall(r"\b(smirk_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.DATA_EXPORTS), declared ^ set(L.DATA_EXPORTS)
    assert L.DATA_EXPORTS == tuple(L.DATA_SIGS) and len(L.DATA_EXPORTS) == 9
    others = (L.EXPORTS, L.MICA_EXPORTS, L.EMOTION_EXPORTS, L.OPTIM_EXPORTS, L.HANDOFF_EXPORTS, L.GENPLAN_EXPORTS, L.GENARITH_EXPORTS)
    for other in others:
        assert not set(L.DATA_EXPORTS) & set(other)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    version = int(re.search(r"#define\s+SMIRK_DATA_ABI_VERSION\s+(\d+)", hdr).group(1))
    lib = L.lib()
    assert lib.smirk_data_abi_version() == L.DATA_ABI_VERSION == version == 1
    assert "smirk_data.h" in open(os.path.join(REPO, "README.md")).read()
    build_py = open(os.path.join(REPO, "smirk_amd", "build.py")).read()
    assert '"smirk_data.h"' in build_py and re.search(r'"data\.hip":\s*\["-ffp-contract=off"\]', build_py)
    # the other tables and their versions did not move, and none of their headers declares the new entries
    assert lib.smirk_abi_version() == L.ABI_VERSION == 17 and len(L.EXPORTS) == 116
    assert (lib.smirk_mica_abi_version(), lib.smirk_emotion_abi_version(), lib.smirk_optim_abi_version(), lib.smirk_handoff_abi_version(),
            lib.smirk_genplan_abi_version(), lib.smirk_genarith_abi_version()) == (1, 1, 1, 1, 1, 1)
    for name in os.listdir(os.path.join(REPO, "include")):
        if name != "smirk_data.h":
            text = open(os.path.join(REPO, "include", name)).read()
            assert not any(e in text for e in L.DATA_EXPORTS), name
    # the constants and records _lib.py mirrors
    for macro, value in (("MAX_POINTS", L.DATA_MAX_POINTS), ("FAN_POINTS", L.DATA_FAN_POINTS), ("MICA_SIZE", L.DATA_MICA_SIZE), ("MAX_SIZE", L.DATA_MAX_SIZE)):
        assert int(re.search(rf"#define\s+SMIRK_DATA_{macro}\s+(\d+)", hdr).group(1)) == value
    assert C.sizeof(L.SmirkDataParams) == 49 * 8 and C.sizeof(L.SmirkDataAugment) == 25 * 8 and C.sizeof(L.SmirkDataFrame) == 16
    rng_h = open(os.path.join(REPO, "smirk_amd", "csrc", "data_rng.h")).read()
    assert (int(re.search(r"#define DATA_STREAM_FRAME (\d+)u", rng_h).group(1)), int(re.search(r"#define DATA_STREAM_PIXEL (\d+)u", rng_h).group(1)),
            int(re.search(r"#define DATA_FRAME_COUNTERS (\d+)", rng_h).group(1))) == (LAW.STREAM_FRAME, LAW.STREAM_PIXEL, LAW.FRAME_COUNTERS)


def test_exported_from_the_package():
    import smirk_amd
    from smirk_amd import data
    assert smirk_amd.BatchPreparer is data.BatchPreparer and smirk_amd.AugmentConfig is data.AugmentConfig and smirk_amd.data is data
    assert {"data", "BatchPreparer", "AugmentConfig"} <= set(smirk_amd.__all__)
    assert data.n_counters(5, 224) == LAW.n_counters(5, 224) == 5 * 224 * 224 and data.n_counters(3, 2) == 24
    cfg = data.AugmentConfig()                                   # the reference's A.Compose at albumentations 1.3.0 defaults
    assert cfg.probabilities() == (0.5, 0.5, 0.25, 0.255, 0.25, 0.1, 0.5, 0.9)
    a = cfg.struct()
    assert (a.brightness_limit, a.contrast_limit, a.gamma_lo, a.gamma_hi, a.cj_brightness, a.cj_contrast, a.cj_saturation, a.cj_hue, a.clahe_lo, a.clahe_hi,
            a.rgb_shift, a.noise_var_lo, a.noise_var_hi, a.shift_limit, a.scale_limit, a.rotate_limit, a.blur_max) == \
        (0.2, 0.2, 80.0, 120.0, 0.05, 0.05, 0.05, 0.05, 1.0, 4.0, 20.0, 10.0, 50.0, 0.05, 0.1, 10.0, 7)


# ---- refusals of the library ----------------------------------------------------------------------------------------------------------------------------------------
def _aug(**kw):
    from smirk_amd import data
    a = data.AugmentConfig().struct()
    for k, v in kw.items():
        if k.startswith("p") and k[1:].isdigit():
            a.p[int(k[1:])] = v
        else:
            setattr(a, k, v)
    return a


def test_workspace_bytes():
    from smirk_amd import _lib as L
    lib = L.lib()
    for train in (0, 1):
        assert lib.smirk_data_workspace_bytes(5, 224, train) >= 5 * C.sizeof(L.SmirkDataParams) + 5 * 1024 * 8
        for bad in ((0, 224), (-1, 224), (5, 0), (5, -8), (5, 220), (5, 2048)):
            assert lib.smirk_data_workspace_bytes(*bad, train) == 0, bad
        assert 0 < lib.smirk_data_hull_points_offset(5, 224, train) < lib.smirk_data_workspace_bytes(5, 224, train)
    assert lib.smirk_data_workspace_bytes(5, 224, 1) >= lib.smirk_data_workspace_bytes(5, 224, 0) + 5 * 224 * 224 * (3 * 3 + 4) + 5 * 65 * 256
    assert 0 < lib.smirk_data_hull_offset(5, 224, 1) < lib.smirk_data_workspace_bytes(5, 224, 1)
    assert lib.smirk_data_workspace_bytes(3, 64, 1) > lib.smirk_data_workspace_bytes(2, 64, 1)


def test_params_refuses_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    need = {t: lib.smirk_data_workspace_bytes(4, 224, t) for t in (0, 1)}

    def call(mp=P, n_mp=Q, Lmax=478, fan=R, flag=S_, index=T, n_index=105, N=4, S=224, lo=1.2, hi=1.8, aug="default", of=U, om=V, ofl=W, ws=X, ws_bytes=None):
        a = _aug() if aug == "default" else aug
        if ws_bytes is None:
            ws_bytes = lib.smirk_data_workspace_bytes(N, S, int(a is not None)) or need[1]
        return lib.smirk_data_params(mp, n_mp, Lmax, fan, flag, index, n_index, N, S, lo, hi, None if a is None else C.byref(a), 1, 0, of, om, ofl, ws, ws_bytes, None)
    for name in ("mp", "n_mp", "fan", "flag", "index", "of", "om", "ofl", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    for bad in (dict(N=0), dict(N=-3), dict(S=0), dict(S=-8), dict(Lmax=0), dict(Lmax=1025), dict(n_index=0), dict(n_index=1025), dict(lo=0.0), dict(lo=-1.0),
                dict(lo=2.0, hi=1.0), dict(lo=float("nan")), dict(hi=float("nan")), dict(hi=float("inf"))):
        assert call(**bad) == BAD_ARG, bad
    assert call(S=220) == UNSUPPORTED and call(S=4) == UNSUPPORTED and call(S=2048) == UNSUPPORTED
    assert call(ws_bytes=0) == WORKSPACE and call(ws_bytes=need[1] - 1) == WORKSPACE
    assert call(aug=None, lo=1.6, hi=1.6, ws_bytes=need[0] - 1) == WORKSPACE
    assert call(ws_bytes=need[0]) == WORKSPACE                   # the training path needs the larger workspace
    for t in range(8):                                           # probabilities outside [0, 1] or NaN
        for v in (-0.01, 1.01, float("nan"), float("inf")):
            assert call(aug=_aug(**{f"p{t}": v})) == BAD_ARG, (t, v)
    reversed_or_out_of_range = (dict(gamma_lo=120.0, gamma_hi=80.0), dict(gamma_lo=0.0), dict(gamma_lo=float("nan")), dict(clahe_lo=4.0, clahe_hi=1.0), dict(clahe_lo=0.5),
                                dict(noise_var_lo=50.0, noise_var_hi=10.0), dict(noise_var_lo=-1.0), dict(noise_var_hi=float("inf")), dict(brightness_limit=-0.2),
                                dict(contrast_limit=-0.2), dict(contrast_limit=float("nan")), dict(cj_brightness=-0.05), dict(cj_contrast=1.5), dict(cj_saturation=-0.05),
                                dict(cj_hue=0.6), dict(cj_hue=-0.05), dict(rgb_shift=-20.0), dict(rgb_shift=300.0), dict(shift_limit=-0.05), dict(scale_limit=-0.1),
                                dict(scale_limit=1.0), dict(rotate_limit=-10.0), dict(rotate_limit=float("nan")), dict(blur_max=4), dict(blur_max=9), dict(blur_max=1))
    for bad in reversed_or_out_of_range:
        assert call(aug=_aug(**bad)) == BAD_ARG, bad


def test_pixel_entries_refuse_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    need = {t: lib.smirk_data_workspace_bytes(4, 224, t) for t in (0, 1)}

    def crop(frames=P, nbytes=1 << 20, table=Q, N=4, S=224, train=1, img=R, mica=S_, ws=T, ws_bytes=None):
        return lib.smirk_data_crop(frames, nbytes, table, N, S, train, img, mica, ws, need[train] if ws_bytes is None else ws_bytes, None)
    for name in ("frames", "table", "mica", "ws"):
        assert crop(**{name: None}) == BAD_ARG, name
    assert crop(img=None, train=0) == BAD_ARG and crop(nbytes=0) == BAD_ARG
    for bad in (dict(N=0), dict(N=-1), dict(S=0), dict(S=-8)):
        assert crop(**bad) == BAD_ARG, bad
    assert crop(S=100) == UNSUPPORTED and crop(S=2048) == UNSUPPORTED
    assert crop(ws_bytes=need[1] - 1) == WORKSPACE and crop(train=0, ws_bytes=need[0] - 1) == WORKSPACE and crop(ws_bytes=0) == WORKSPACE

    entries = dict(stats=lambda N=4, S=224, ws=T, b=need[1]: lib.smirk_data_stats(N, S, ws, b, None),
                   colour=lambda N=4, S=224, ws=T, b=need[1]: lib.smirk_data_colour(N, S, ws, b, None),
                   finish=lambda N=4, S=224, ws=T, b=need[1], img=R, mask=S_: lib.smirk_data_finish(N, S, 1, 0, img, mask, ws, b, None))
    for name, fn in entries.items():
        assert fn(ws=None) == BAD_ARG, name
        for bad in (dict(N=0), dict(N=-1), dict(S=0), dict(S=-8)):
            assert fn(**bad) == BAD_ARG, (name, bad)
        assert fn(S=100) == UNSUPPORTED and fn(S=2048) == UNSUPPORTED, name
        assert fn(b=need[1] - 1) == WORKSPACE and fn(b=need[0]) == WORKSPACE and fn(b=0) == WORKSPACE, name
    assert entries["finish"](img=None) == BAD_ARG and entries["finish"](mask=None) == BAD_ARG


# ---- refusals of the Python surface (numpy only: nothing is uploaded) ------------------------------------------------------------------------------------------------
def test_python_refusals():
    from smirk_amd import data
    from smirk_amd import SmirkHipError
    idx = _indices()
    prep = data.BatchPreparer(mp_indices=idx)
    frames, fans, mps = LAW.synth_batch(seed=3)

    def refused(match, f=frames, a=fans, m=mps, p=prep):
        with pytest.raises(ValueError, match=match):
            p(f, a, m)
    refused("uint8", f=[frames[0].astype(np.float32)] + frames[1:])
    refused("uint8", f=[frames[0][..., :2]] + frames[1:])
    refused("uint8", f=[frames[0][..., 0]] + frames[1:])
    refused("lengths", f=frames[:4])
    refused("lengths", a=fans[:3])
    refused("lengths", m=mps + mps[:1])
    refused("empty", f=[], a=[], m=[])
    nan_mp = mps[2].copy(); nan_mp[7, 1] = np.nan
    refused("non-finite", m=mps[:2] + [nan_mp] + mps[3:])
    inf_fan = fans[0].copy(); inf_fan[3, 0] = np.inf
    refused("non-finite", a=[inf_fan] + fans[1:])
    refused("degenerate", m=[np.full_like(mps[0], 5.0)] + mps[1:])
    refused("degenerate", m=[mps[0] * 1e-3] + mps[1:])
    refused("points", m=[mps[0][:400]] + mps[1:])                 # fewer than the largest mediapipe index + 1
    refused("points", m=[mps[0][:int(idx.max())]] + mps[1:])
    refused("points", m=[np.concatenate([mps[0]] * 3)[:1025]] + mps[1:])
    refused("expected", m=[mps[0][:, :1]] + mps[1:])
    refused("68", a=[fans[0][:67]] + fans[1:])
    refused("coincide", a=[np.full((68, 2), 9.0)] + fans[1:])
    for kw in (dict(image_size=220), dict(image_size=0), dict(scale=1.6), dict(scale=(1.8, 1.2)), dict(scale=(0.0, 1.0)), dict(test=True, scale=(1.2, 1.8)),
               dict(augment=data.AugmentConfig(p_blur=1.5)), dict(augment=data.AugmentConfig(p_gamma=float("nan"))), dict(augment=data.AugmentConfig(gamma_limit=(120, 80))),
               dict(augment=data.AugmentConfig(blur_limit=4)), dict(mp_indices=[1024]), dict(mp_indices=[])):
        with pytest.raises(ValueError):
            data.BatchPreparer(**{**dict(mp_indices=idx), **kw})
    with pytest.raises(SmirkHipError):
        data.BatchPreparer(mp_indices=idx, device="cpu")


# ---- the law's self-checks ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    return LAW.synth_batch(seed=0)


def _zero_cfg(**kw):
    from smirk_amd import data
    base = dict(p_brightness_contrast=0.0, p_gamma=0.0, p_color_jitter=0.0, p_clahe=0.0, p_rgb_shift=0.0, p_blur=0.0, p_gauss_noise=0.0, p_shift_scale_rotate=0.0)
    base.update(kw)
    return data.AugmentConfig(**base)


def test_train_with_every_probability_zero_is_the_test_path(batch):
    frames, fans, mps = batch
    idx = _indices()
    a = LAW.prepare(frames, fans, mps, idx, 64, (1.6, 1.6), _zero_cfg(), seed=9, offset=5)
    b = LAW.prepare(frames, fans, mps, idx, 64, 1.6)
    for k in ("img_levels", "mask", "landmarks_fan", "landmarks_mp", "flag_landmarks_fan", "img_mica"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert b["flag_landmarks_fan"].tolist() == [True, False, True, True, True] and not b["img_mica"][1].any() and b["img_mica"][0].any()


def test_shift_scale_rotate_with_zero_draws_is_the_identity(batch):
    m, mi = LAW.ssr_matrices(64, 0.0, 1.0, 0.0, 0.0)
    assert m == LAW.IDENTITY and mi == LAW.IDENTITY
    frames, fans, mps = batch
    fwd, inv = LAW.crop_similarity(mps[0], 1.6, 64)
    img = LAW.warp_crop(frames[0], inv, 64)
    hull = LAW.hull_mask(LAW.hull_points(mps[0], fwd), 64)
    out, mask = LAW.resample(img, hull, mi)
    assert np.array_equal(out, img) and np.array_equal(mask, hull)
    assert np.array_equal(LAW.landmarks_out(fans[0], fwd, m, 64), LAW.landmarks_out(fans[0], fwd, LAW.IDENTITY, 64))
    # and a pure shift by whole pixels moves image, mask and key points by exactly that much, with 1 in the mask where the frame ends
    m, mi = LAW.ssr_matrices(64, 0.0, 1.0, 4 / 64, -2 / 64)
    out, mask = LAW.resample(img, hull, mi)
    assert np.array_equal(out[:-2, 4:], img[2:, :-4]) and not out[-2:].any() and not out[:, :4].any()
    assert np.array_equal(mask[:-2, 4:], hull[2:, :-4]) and mask[-2:].all() and mask[:, :4].all()


def test_crop_hull_and_similarity_equal_the_oracle(batch):
    from oracle import video_ref as VR
    frames, fans, mps = batch
    for i, (frame, mp) in enumerate(zip(frames, mps)):
        for S, scale in ((64, 1.6), (224, 1.25)):
            fwd, inv = LAW.crop_similarity(mp, scale, S)
            T = VR.crop_transform(mp, scale=scale, image_size=S)
            assert np.abs(np.array(fwd).reshape(2, 3) - T[:2]).max() < 1e-9 * max(1.0, np.abs(T).max())
            M = np.array([inv[:3], inv[3:], [0.0, 0.0, 1.0]])
            assert np.abs(M @ T - np.eye(3)).max() < 1e-9
            assert np.array_equal(LAW.warp_crop(frame, inv, S), VR.warp_u8(frame[..., ::-1], M, (S, S))), (i, S)
            pts = LAW.hull_points(mp, fwd)
            ref = (T @ np.hstack([mp[:, :2], np.ones((len(mp), 1))]).T).T[:, :2]        # prepare_data:150-151; truncation moves a point by less than 1
            assert np.abs(pts - ref).max() < 1.0 + 1e-9 and (np.abs(pts) <= np.abs(ref) + 1e-9).all()
            assert np.array_equal(LAW.hull_mask(pts, S), VR.hull_mask(pts, (S, S))), (i, S)
    # the crop box of sample 3 hangs over the frame: the constant border is part of its crop
    fwd, inv = LAW.crop_similarity(mps[3], 1.6, 64)
    assert not LAW.warp_crop(frames[3], inv, 64)[-1].any()
    for fan in (f for f in fans if f is not None):
        a, b, tx, ty = LAW.similarity_closed_form(LAW.arcface_points(fan), LAW.ARCFACE)
        U = VR.umeyama(LAW.arcface_points(fan), LAW.ARCFACE)
        assert np.abs(np.array([[a, -b, tx], [b, a, ty]]) - U[:2]).max() < 1e-9
        q = LAW.arcface_inverse(fan)
        assert np.abs(np.array([q[:3], q[3:], [0, 0, 1]]) @ U - np.eye(3)).max() < 1e-9


def test_clahe_of_a_constant_image_is_that_image_up_to_the_lab_round_trip():
    S, clip_limit = 224, 2.0
    area = (S // 8) ** 2
    clip = max(int(clip_limit * area / 256.0), 1)
    for rgb in ((120, 90, 60), (10, 200, 30), (255, 255, 255), (0, 0, 0), (37, 37, 37), (200, 200, 200)):
        img = np.tile(np.array(rgb, np.int64), (S, S, 1))
        l8, a8, b8 = LAW.rgb_to_lab8(img)
        v = int(l8[0, 0])
        assert np.ptp(l8) == 0 and np.ptp(a8) == 0 and np.ptp(b8) == 0
        tables = LAW.clahe_tables(l8, clip_limit)
        # one full bin: `clip` stays, area - clip is spread as batch per bin + a strided residual of < 256, so the cumulative count at v is within
        # residual + clip of the uniform ramp's (v + 1) area / 256, i.e. the level moves by at most that many counts * 255 / area (+ 0.5 for rint)
        resid = (area - clip) % 256
        assert np.ptp(tables.reshape(64, 256), axis=0).max() == 0
        assert abs(int(tables[0, 0, v]) - (v + 1) * 255.0 / 256.0) <= (resid + clip) * 255.0 / area + 0.5
        assert (np.diff(tables, axis=-1) >= 0).all() and tables[0, 0, 255] == 255
        out = LAW.clahe(img, clip_limit)
        assert np.ptp(out.reshape(-1, 3), axis=0).max() == 0                        # still constant: the blend of equal tables is that table
        assert np.array_equal(out, LAW.lab8_to_rgb(np.full((S, S), tables[0, 0, v]), a8, b8))
        if rgb[0] == rgb[1] == rgb[2]:
            # a grey has a8 = b8 = 128 and the round trip only quantises L: half an L8 step is at most 0.72 of a grey level (the linear toe, 0.27 L* a level)
            assert a8[0, 0] == 128 and b8[0, 0] == 128
            assert np.abs(LAW.lab8_to_rgb(l8, a8, b8) - img).max() <= 1


def test_blur_and_the_point_transforms_at_their_neutral_values():
    r = np.random.default_rng(0)
    img = r.integers(0, 256, (16, 24, 3)).astype(np.int64)
    const = np.tile(np.array([13, 200, 77], np.int64), (16, 16, 1))
    for k in (3, 5, 7):
        assert np.array_equal(LAW.blur(const, k), const)                           # k = 1-equivalent: a box mean leaves a constant image alone
        b = LAW.blur(img, k)
        h = k // 2
        assert b[8, 9, 0] == int(np.rint(img[8 - h:9 + h, 9 - h:10 + h, 0].sum() / (k * k)))
        col = [abs(j) if j < 24 else 2 * 23 - j for j in range(-h, h + 1)]         # reflect-101 at the corner
        row = [abs(j) for j in range(-h, h + 1)]
        assert b[0, 0, 1] == int(np.rint(img[np.ix_(row, col)][..., 1].sum() / (k * k)))
    ident = np.arange(256)
    assert np.array_equal(LAW.lut_brightness_contrast(1.0, 0.0), ident) and np.array_equal(LAW.lut_gamma(1.0), ident)
    assert np.array_equal(LAW.lut_jitter(1.0, 1.0, 99), ident) and np.array_equal(LAW.rgb_shift(img, [0.0, 0.0, 0.0]), img)
    assert np.array_equal(LAW.lut_brightness_contrast(1.0, 0.1), np.minimum(ident + 25, 255))          # beta * 255 = 25.5, truncated
    greys = np.stack([ident] * 3, -1)[None]
    assert np.array_equal(LAW.saturation_hue(greys, 1.0, 0.0), greys) and np.array_equal(LAW.saturation_hue(greys, 1.03, 0.05), greys)      # grey has no hue
    prim = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.int64)
    assert np.array_equal(LAW.saturation_hue(prim, 1.0, 0.0), prim)
    assert np.array_equal(LAW.saturation_hue(prim, 1.0, 1.0 / 3.0), prim[:, [1, 2, 0]])                # a third of a turn: R -> G -> B -> R
    assert np.array_equal(LAW.grey(greys), greys[..., 0])


def test_the_draw_layout_consumes_exactly_n_counters(batch):
    from smirk_amd import data
    frames, fans, mps = batch
    cfg = _zero_cfg(p_gauss_noise=1.0)
    res = LAW.prepare(frames, fans, mps, _indices(), 64, (1.2, 1.8), cfg, seed=11, offset=1000)
    assert res["counters_used"] == LAW.n_counters(5, 64) == data.n_counters(5, 64)
    assert all(p["coins"] == 1 << 6 for p in res["params"])
    # without the per-pixel draws only the per-frame counters are touched, and they fit in front
    res = LAW.prepare(frames, fans, mps, _indices(), 64, (1.2, 1.8), _zero_cfg(), seed=11, offset=1000)
    assert res["counters_used"] == 5 * LAW.FRAME_COUNTERS - 1 <= LAW.n_counters(5, 64)
    # a frame's draws depend on (seed, offset, frame index) only
    a = LAW.draw_frame(data.AugmentConfig(), (1.2, 1.8), 64, 11, 1000, 3)
    b = LAW.draw_frame(data.AugmentConfig(), (1.2, 1.8), 64, 11, 1000 + 8, 2)
    assert {k: v for k, v in a.items() if k != "used"} == {k: v for k, v in b.items() if k != "used"}
    assert 1.2 <= a["scale"] < 1.8 and a["blur_k"] in (3, 5, 7)
