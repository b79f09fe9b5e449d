"""smirk_amd.data on the MI355X against the law of tests/data_law.py (and oracle.video_ref where it has the function): five frames of mixed sizes, one without FAN
landmarks, one whose crop box hangs over the frame edge.

The condition on every image (img, img_mica): integer levels rint(255 x) differ from the law's by at most one level in at most 4 elements of an image.  Both sides
compute in float64 with contraction off, so a difference needs a value within ~1e-13 of a rounding boundary (a last-place pow / cbrt / log / cos difference): zero
is expected, and the cap is far below what any real defect produces.  mask and flags are exact; landmarks are within one float32 ulp of the restated value (the
double-rounding margin of casting a float64 result)."""
import ctypes as C

import numpy as np
import pytest
import torch

import data_law as LAW

pytestmark = pytest.mark.gpu
SEED, OFFSET = 0x5EEDDA7A, 4096


def _indices():
    import synthdata
    return np.asarray(synthdata.load_bundle()["mp_landmark_indices"]).astype(np.int64).ravel()


@pytest.fixture(scope="module")
def batch():
    return LAW.synth_batch(seed=0)


@pytest.fixture(scope="module")
def law_cache():
    return {}


def _cfg(**kw):
    from smirk_amd import data
    base = dict(p_brightness_contrast=0.0, p_gamma=0.0, p_color_jitter=0.0, p_clahe=0.0, p_rgb_shift=0.0, p_blur=0.0, p_gauss_noise=0.0, p_shift_scale_rotate=0.0)
    base.update(kw)
    return data.AugmentConfig(**base)


def _levels(x):
    return np.rint(255.0 * x.detach().cpu().numpy().astype(np.float64)).astype(np.int64)


def _assert_images(name, got, want):
    """the condition of the module docstring, per image; prints the figures before it asserts"""
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    for i in range(got.shape[0]):
        d = np.abs(got[i] - want[i])
        print(f"{name}[{i}]: {int((d != 0).sum())} of {d.size} elements differ, max {int(d.max())} levels")
        assert d.max() <= 1 and (d != 0).sum() <= 4, (name, i, int(d.max()), int((d != 0).sum()))


def _assert_within_one_ulp(name, got, want):
    got, want = got.detach().cpu().numpy(), np.asarray(want, np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{name}: max |got - law| = {err.max():.3g} ({(err / np.spacing(np.abs(want)).astype(np.float64)).max():.2f} ulp)")
    assert (err <= np.spacing(np.abs(want)).astype(np.float64)).all(), name


def _assert_batch(out, law, S):
    assert set(out) == {"img", "landmarks_fan", "flag_landmarks_fan", "landmarks_mp", "mask", "img_mica"}
    N = law["img_levels"].shape[0]
    assert out["img"].shape == (N, 3, S, S) and out["mask"].shape == (N, 1, S, S) and out["img_mica"].shape == (N, 3, 112, 112)
    assert out["flag_landmarks_fan"].dtype == torch.bool and out["flag_landmarks_fan"].cpu().tolist() == law["flag_landmarks_fan"].tolist()
    _assert_images("img", _levels(out["img"]), law["img_levels"])
    img = out["img"].cpu().numpy()
    assert np.array_equal(img, (_levels(out["img"]).astype(np.float32) / np.float32(255.0)))          # img IS level / 255 in float32
    assert np.array_equal(out["mask"].cpu().numpy(), law["mask"].astype(np.float32))
    _assert_within_one_ulp("landmarks_fan", out["landmarks_fan"], law["landmarks_fan"])
    _assert_within_one_ulp("landmarks_mp", out["landmarks_mp"], law["landmarks_mp"])
    _assert_images("img_mica", _levels(out["img_mica"]), np.rint(255.0 * law["img_mica"].astype(np.float64)).astype(np.int64))


# ---- 1. the deterministic path ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [224, 64])
def test_test_mode_equals_the_oracle_and_the_law(batch, S):
    from oracle import video_ref as VR
    from smirk_amd import data, _lib as L
    frames, fans, mps = batch
    idx = _indices()
    prep = data.BatchPreparer(image_size=S, scale=1.6, test=True, mp_indices=idx)
    L.profile_start()
    out = prep(frames, fans, mps)
    launches = L.profile_stop()
    assert len(launches) <= 3, [k for k, *_ in launches]
    law = LAW.prepare(frames, fans, mps, idx, S, 1.6)
    got_img, got_mask = _levels(out["img"]), out["mask"].cpu().numpy()
    for i, (frame, mp) in enumerate(zip(frames, mps)):                    # exactly the oracle's warp and hull on the law's transform
        fwd, inv = LAW.crop_similarity(mp, 1.6, S)
        M = np.array([inv[:3], inv[3:], [0.0, 0.0, 1.0]])
        assert np.array_equal(got_img[i], VR.warp_u8(frame[..., ::-1], M, (S, S)).transpose(2, 0, 1).astype(np.int64)), i
        assert np.array_equal(got_mask[i, 0], VR.hull_mask(LAW.hull_points(mp, fwd), (S, S)).astype(np.float32)), i
    assert np.array_equal(got_img, law["img_levels"].astype(np.int64))
    _assert_batch(out, law, S)
    assert not out["img_mica"][1].any() and not got_img[3][:, -1].any()     # no FAN landmarks: zeros; the overhanging box reads the constant border


# ---- 2. each transform alone, then the default config ----------------------------------------------------------------------------------------------------------------
ALONE = ("p_brightness_contrast", "p_gamma", "p_color_jitter", "p_clahe", "p_rgb_shift", "p_blur", "p_gauss_noise", "p_shift_scale_rotate")


@pytest.mark.parametrize("which", ALONE + ("default",))
def test_training_path_equals_the_law(batch, law_cache, which):
    from smirk_amd import data, _lib as L
    from smirk_amd.masking import PhiloxStream
    frames, fans, mps = batch
    idx, S = _indices(), 224
    cfg = data.AugmentConfig() if which == "default" else _cfg(**{which: 1.0})
    prep = data.BatchPreparer(image_size=S, scale=(1.2, 1.8), augment=cfg, mp_indices=idx)
    rng = PhiloxStream(SEED, OFFSET)
    L.profile_start()
    out = prep(frames, fans, mps, rng=rng)
    launches = L.profile_stop()
    assert len(launches) <= 8, [k for k, *_ in launches]
    assert rng.offset == OFFSET + data.n_counters(len(frames), S)
    law = LAW.prepare(frames, fans, mps, idx, S, (1.2, 1.8), cfg, seed=SEED, offset=OFFSET, cache=law_cache)
    coins = [p["coins"] for p in law["params"]]
    print(which, "coins", coins)
    if which != "default":
        assert coins == [1 << ALONE.index(which)] * len(frames)
        plain = LAW.prepare(frames, fans, mps, idx, S, (1.2, 1.8), _cfg(), seed=SEED, offset=OFFSET, cache=law_cache)
        assert not np.array_equal(plain["img_levels"], law["img_levels"])                             # the transform does something to compare
    _assert_batch(out, law, S)


# ---- 3. geometry, independent of the law --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,H", [(224, 160), (64, 64)])                     # frame sizes at which the crop enlarges the dot (the warp does not prefilter)
def test_a_dot_lands_on_its_landmark_and_the_mask_is_one_outside_the_frame(S, H):
    from smirk_amd import data
    from smirk_amd.masking import PhiloxStream
    idx, N = _indices(), 4
    frames, fans, mps, dots = [], [], [], []
    for i in range(N):
        fan, mp = LAW.synth_landmarks(H, H, 50 + i)
        k = (36, 54, 48, 45)[i]                                              # the landmark that carries the dot (eye and mouth corners), on a whole pixel
        fan[k] = np.rint(fan[k])
        x, y = int(fan[k, 0]), int(fan[k, 1])
        f = np.zeros((H, H, 3), np.uint8)
        f[y - 1:y + 2, x - 1:x + 2] = 255
        frames.append(f); fans.append(fan); mps.append(mp); dots.append(k)
    cfg = _cfg(p_shift_scale_rotate=1.0)
    out = data.BatchPreparer(image_size=S, scale=(1.2, 1.8), augment=cfg, mp_indices=idx)(frames, fans, mps, rng=PhiloxStream(77, 0))
    img, lm = out["img"].cpu().numpy().astype(np.float64), out["landmarks_fan"].cpu().numpy().astype(np.float64)
    rows, cols = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    for i in range(N):
        w = img[i].sum(0)
        assert w.sum() > 1.0, i
        cx, cy = (w * cols).sum() / w.sum(), (w * rows).sum() / w.sum()
        px, py = (lm[i, dots[i]] + 1.0) / 2.0 * S
        print(f"frame {i}: dot centroid ({cx:.2f}, {cy:.2f}), landmark ({px:.2f}, {py:.2f})")
        assert abs(cx - px) <= 1.0 and abs(cy - py) <= 1.0, (i, cx, cy, px, py)
    # white frames whose crop is white everywhere: after ShiftScaleRotate a pixel is 0 only where all its neighbours are outside the frame, and there mask == 1
    white = [np.full((640, 640, 3), 255, np.uint8) for _ in range(N)]
    wl = [tuple(np.concatenate([p[:, :2] + 120.0, p[:, 2:]], 1) for p in LAW.synth_landmarks(400, 400, 60 + i)) for i in range(N)]      # box well inside the frame
    plain = data.BatchPreparer(image_size=S, scale=(1.2, 1.8), augment=_cfg(), mp_indices=idx)([f for f in white], [a for a, _ in wl], [m for _, m in wl],
                                                                                                    rng=PhiloxStream(78, 0))
    assert (plain["img"] == 1.0).all()
    out = data.BatchPreparer(image_size=S, scale=(1.2, 1.8), augment=cfg, mp_indices=idx)([f for f in white], [a for a, _ in wl], [m for _, m in wl], rng=PhiloxStream(78, 0))
    outside = (out["img"] == 0.0).all(1, keepdim=True)
    assert int(outside.sum()) > 0
    assert (out["mask"][outside] == 1.0).all()
    assert ((out["mask"] == 0.0) | (out["mask"] == 1.0)).all() and int((out["mask"] == 0.0).sum()) > 0


# ---- 4. the draw law ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_draws_are_inside_their_limits_and_coins_fall_at_their_rates():
    from smirk_amd import data, _lib as L
    N, S, Lm = 4096, 64, 478
    idx = _indices()
    dev = torch.device("cuda")
    fan, mp = LAW.synth_landmarks(200, 200, 5)
    d_mp = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(mp[None, :, :2], (N, Lm, 2)))).to(dev)
    d_fan = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(fan[None], (N, 68, 2)))).to(dev)
    d_n = torch.full((N,), Lm, dtype=torch.int32, device=dev)
    d_flag = torch.ones(N, dtype=torch.uint8, device=dev)
    d_idx = torch.from_numpy(idx.astype(np.int32)).to(dev)
    o_fan, o_mp, o_flag = torch.empty(N, 68, 2, device=dev), torch.empty(N, idx.size, 2, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
    lib = L.lib()
    cfg = data.AugmentConfig()
    aug = cfg.struct()
    ws = torch.empty(lib.smirk_data_workspace_bytes(N, S, 1), dtype=torch.uint8, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.smirk_data_params(P(d_mp), P(d_n), Lm, P(d_fan), P(d_flag), P(d_idx), idx.size, N, S, 1.2, 1.8, C.byref(aug), SEED, OFFSET, P(o_fan), P(o_mp), P(o_flag),
                                  P(ws), ws.numel(), L.stream_ptr()))
    raw = ws[:N * C.sizeof(L.SmirkDataParams)].cpu().numpy().tobytes()
    rec = (L.SmirkDataParams * N).from_buffer_copy(raw)
    col = lambda get: np.array([get(r) for r in rec], np.float64)
    uniforms = dict(scale=(col(lambda r: r.scale), 1.2, 1.8), bc_alpha=(col(lambda r: r.bc_alpha), 0.8, 1.2), bc_beta=(col(lambda r: r.bc_beta), -0.2, 0.2),
                    gamma=(col(lambda r: r.gamma), 0.8, 1.2), clahe_clip=(col(lambda r: r.clahe_clip), 1.0, 4.0),
                    noise_var=(col(lambda r: r.noise_sigma) ** 2, 10.0, 50.0), ssr_angle=(col(lambda r: r.ssr_angle), -10.0, 10.0),
                    ssr_scale=(col(lambda r: r.ssr_scale), 0.9, 1.1), ssr_dx=(col(lambda r: r.ssr_dx), -0.05, 0.05), ssr_dy=(col(lambda r: r.ssr_dy), -0.05, 0.05))
    for j, (lo, hi) in enumerate(((0.95, 1.05), (0.95, 1.05), (0.95, 1.05), (-0.05, 0.05))):
        uniforms[f"cj{j}"] = (col(lambda r: r.cj[j]), lo, hi)
    for j in range(3):
        uniforms[f"rgb_shift{j}"] = (col(lambda r: r.rgb_shift[j]), -20.0, 20.0)
    for name, (v, lo, hi) in uniforms.items():
        eps = 1e-12 * max(abs(lo), abs(hi))                                   # noise_var is sigma squared again: a rounding of the square root, not of the draw
        se = (hi - lo) / np.sqrt(12.0 * N)
        print(f"{name}: [{v.min():.6g}, {v.max():.6g}] mean {v.mean():.6g} (midpoint {(lo + hi) / 2:.6g}, 4 se = {4 * se:.3g})")
        assert v.min() >= lo - eps and v.max() <= hi + eps, name
        assert abs(v.mean() - (lo + hi) / 2) <= 4 * se, name
    coins = col(lambda r: r.coins).astype(np.int64)
    for t, p in enumerate(cfg.probabilities()):
        rate = ((coins >> t) & 1).mean()
        print(f"coin {L.DATA_TRANSFORMS[t]}: rate {rate:.4f} (p {p}, 4 sd = {4 * np.sqrt(p * (1 - p) / N):.4f})")
        assert abs(rate - p) <= 4 * np.sqrt(p * (1 - p) / N), t
    k = col(lambda r: r.blur_k).astype(np.int64)
    assert set(np.unique(k).tolist()) == {3, 5, 7}
    assert (col(lambda r: r.flag_fan) == 1).all() and (o_flag.cpu().numpy() == 1).all()
    # the records agree with the law's restatement of the same counters (first frames)
    for f in range(4):
        want = LAW.draw_frame(cfg, (1.2, 1.8), S, SEED, OFFSET, f)
        r = rec[f]
        assert r.coins == want["coins"] and r.blur_k == want["blur_k"] and r.scale == want["scale"] and r.bc_alpha == want["bc_alpha"] and r.gamma == want["gamma"]
        assert list(r.cj) == want["cj"] and list(r.rgb_shift) == want["rgb_shift"] and r.noise_sigma == want["noise_sigma"] and r.ssr_dy == want["ssr_dy"]
        assert np.allclose(list(r.ssr_inv), want["ssr_inv"], rtol=1e-14, atol=1e-12)


# ---- 5. the contract ------------------------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


def test_contract(batch):
    import smirk_amd
    from smirk_amd import data, _lib as L
    from smirk_amd.masking import PhiloxStream
    frames, fans, mps = batch
    idx, S = _indices(), 64
    prep = data.BatchPreparer(image_size=S, scale=(1.2, 1.8), mp_indices=idx)       # the default augmentation
    a, b = prep(frames, fans, mps, rng=PhiloxStream(SEED, 7)), prep(frames, fans, mps, rng=PhiloxStream(SEED, 7))
    assert _same(a, b)                                                               # the same stream gives the same bits
    rng = PhiloxStream(SEED, 7)
    c = prep(frames, fans, mps, rng=rng)
    assert rng.offset == 7 + data.n_counters(5, S) and _same(a, c)
    d = prep(frames, fans, mps, rng=rng)                                             # the stream moved on: other draws
    assert rng.offset == 7 + 2 * data.n_counters(5, S) and not torch.equal(a["img"], d["img"])
    head = prep(frames[:3], fans[:3], mps[:3], rng=PhiloxStream(SEED, 7))            # frame i does not change when frames are appended after it
    assert all(torch.equal(head[k], a[k][:3]) for k in a)
    torch.manual_seed(5)
    e = prep(frames, fans, mps)
    torch.manual_seed(5)
    assert _same(e, prep(frames, fans, mps)) and not torch.equal(e["img"], prep(frames, fans, mps)["img"])      # keyed by torch.manual_seed; successive calls differ
    # run(): 11 samples at batch 4 -> 4 + 4 + 3, the bits of three direct calls
    samples = [(frames[i % 5], fans[i % 5], mps[i % 5]) for i in range(11)]
    got = list(data.BatchPreparer(image_size=S, scale=(1.2, 1.8), mp_indices=idx).run(iter(samples), batch_size=4, rng=PhiloxStream(3, 0)))
    assert [g["img"].shape[0] for g in got] == [4, 4, 3]
    rng = PhiloxStream(3, 0)
    for j, g in enumerate(got):
        part = samples[4 * j:4 * j + 4]
        assert _same(g, prep([s[0] for s in part], [s[1] for s in part], [s[2] for s in part], rng=rng)), j
    # the deterministic path draws nothing
    rng = PhiloxStream(1, 11)
    t = data.BatchPreparer(image_size=S, scale=1.6, test=True, mp_indices=idx)
    assert _same(t(frames, fans, mps, rng=rng), t(frames, fans, mps)) and rng.offset == 11
    # what first_path reads, without a copy: float32, contiguous, on the device, 16-byte aligned
    for k, shape in (("img", (5, 3, S, S)), ("mask", (5, 1, S, S)), ("landmarks_fan", (5, 68, 2)), ("landmarks_mp", (5, 105, 2)), ("img_mica", (5, 3, 112, 112))):
        v = a[k]
        assert tuple(v.shape) == shape and v.dtype == torch.float32 and v.is_cuda and v.is_contiguous()
        assert L.aligned16(v).data_ptr() == v.data_ptr() and L.as_f32c(v) is v
    assert a["flag_landmarks_fan"].dtype == torch.bool and tuple(a["flag_landmarks_fan"].shape) == (5,)
    assert float(a["img"].min()) >= 0.0 and float(a["img"].max()) <= 1.0
    smirk_amd.check_numerics()
