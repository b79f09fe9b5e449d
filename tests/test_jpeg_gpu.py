"""smirk_amd.jpeg on the GPU: the files and the span table equal tests/jpeg_law.py's byte for byte (the law is integer arithmetic, so there is no tolerance),
over sizes that are no multiple of the MCU, more MCUs than a wave has lanes, every restart-interval branch, both pixel orders, the ends of the quality scale, and
contents chosen for one entropy-coding branch each."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import jpeg_law as LAW

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _noise(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _constant(B, H, W):
    return np.broadcast_to(np.array([200, 90, 31], np.uint8), (B, H, W, 3)).copy()


def _checkerboard(B, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], (B, H, W, 3)).copy()


def _lone_63(B, H, W):
    """grey pictures whose luminance blocks are 128 + 100 c7(x) c7(y): after the forward DCT and quantisation at quality 50 only coefficient 63 survives (4 A / 99)"""
    c7 = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    blk = np.rint(128 + 100 * np.outer(c7, c7))
    img = np.tile(blk, (-(-H // 8), -(-W // 8)))[:H, :W]
    return np.broadcast_to(np.clip(img, 0, 255).astype(np.uint8)[None, :, :, None], (B, H, W, 3)).copy()


def _raw_encode(images, quality=95, bgr=False, R=1, qt=None):
    """the C entry on a sentinel-filled output buffer: -> (the whole buffer, spans [(offset, length)])"""
    from smirk_amd import _lib as L
    lib = L.lib()
    B, H, W, _ = images.shape
    dev = torch.from_numpy(images).cuda()
    tables = L.JpegQuantTables()
    L.check(lib.smirk_jpeg_quant_tables(quality, C.byref(tables)))
    ws_bytes, bound = lib.smirk_jpeg_workspace_bytes(B, H, W, R), lib.smirk_jpeg_max_bytes(B, H, W, R)
    assert ws_bytes > 0 and bound > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.full((bound + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    spans = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    L.check(lib.smirk_jpeg_encode_u8(L.ptr(dev, torch.uint8), B, H, W, int(bgr), C.byref(tables), R, C.c_void_p(ws.data_ptr()), ws_bytes,
                                     C.c_void_p(out.data_ptr()), bound, C.c_void_p(spans.data_ptr()), L.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), [tuple(int(v) for v in row) for row in spans.cpu().numpy()]


def _check(images, quality, bgr, R):
    """-> the law's stream; asserts bytes, spans and the untouched tail"""
    want, spans = LAW.encode_batch(images, quality, bgr, R)
    got, got_spans = _raw_encode(images, quality, bgr, R)
    assert got_spans == spans
    assert got[:len(want)].tobytes() == want
    assert (got[len(want):] == SENTINEL).all()                                        # nothing past the last file
    return want


CASES = [  # id, picture, B, H, W, quality, bgr, R
    ("1x1", _noise, 1, 1, 1, 95, False, 1),
    ("8x8", _noise, 1, 8, 8, 50, False, 2),
    ("16x16-bgr", _noise, 1, 16, 16, 95, True, 1),
    ("17x23-B2-R3", _noise, 2, 17, 23, 95, False, 3),                                 # 4 MCUs: intervals of 3 and 1
    ("17x23-B2-R65", _noise, 2, 17, 23, 1, False, 65),                                # R above the MCU count: one interval, DRI states 4
    ("48x32-B3-R2-q1", _noise, 3, 48, 32, 1, False, 2),
    ("48x32-B3-R1-q100-bgr", _noise, 3, 48, 32, 100, True, 1),
    ("16x1040-R1", _noise, 1, 16, 1040, 95, False, 1),                                # 65 MCUs, 65 intervals: one more than a wave, RSTm wraps eight times
    ("16x1040-R2-q50", _noise, 1, 16, 1040, 50, False, 2),                            # 33 intervals, the last of one MCU
    ("16x1040-R65-q100", _noise, 1, 16, 1040, 100, False, 65),                        # one interval of 65 MCUs
    ("16x1040-R3-bgr", _noise, 1, 16, 1040, 95, True, 3),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_noise_equals_the_law(case):
    _, make, B, H, W, quality, bgr, R = case
    images = make(B, H, W, seed=H * 1000 + W + B)
    want = _check(images, quality, bgr, R)
    if H * W >= 16 * 1040 and quality >= 95:
        assert b"\xff\x00" in want[LAW.HEADER_BYTES:]                                 # the stuffing branch is really taken


def test_constant_picture_is_eob_only():
    images = _constant(2, 17, 23)
    want = _check(images, 95, False, 1)
    c = LAW.coefficients(images[0], LAW.quant_tables(95))
    assert not c[:, :, 1:].any() and c[:, :, 0].any()


def test_checkerboard_reaches_the_largest_categories():
    images = _checkerboard(1, 48, 32)
    _check(images, 100, False, 2)
    c = LAW.coefficients(images[0], LAW.quant_tables(100))
    assert np.abs(c[:, :4, 1:]).max() >= 512                                          # AC category 10
    _check(np.concatenate([np.zeros((1, 16, 16, 3), np.uint8), np.full((1, 16, 16, 3), 255, np.uint8)]), 100, False, 1)     # DC -1024 and 1016


def test_lone_coefficient_63_codes_zrl_and_no_eob():
    images = _lone_63(1, 48, 32)
    c = LAW.coefficients(images[0], LAW.quant_tables(50))
    assert (c[:, :4, 63] != 0).all() and not c[:, :4, 1:63].any() and LAW.has_zrl(c)  # three ZRLs, then coefficient 63: the block ends without EOB
    _check(images, 50, False, 3)


def test_two_runs_are_bitwise_equal_and_a_frame_does_not_depend_on_its_batch():
    images = _noise(3, 48, 32, seed=7)
    a, sa = _raw_encode(images, 95, False, 2)
    b, sb = _raw_encode(images, 95, False, 2)
    assert sa == sb and np.array_equal(a, b)
    for i in range(3):
        alone, s1 = _raw_encode(images[i:i + 1], 95, False, 2)
        assert s1[0][0] == 0 and alone[:s1[0][1]].tobytes() == a[sa[i][0]:sa[i][0] + sa[i][1]].tobytes()


def test_encode_jpeg_does_not_synchronise_and_to_host_returns_the_files():
    import smirk_amd
    images = _noise(2, 17, 23, seed=3)
    dev = torch.from_numpy(images).cuda()
    smirk_amd.encode_jpeg(dev, quality=75, restart_interval=3)                          # allocations and the first launch of the unit, outside the guarded call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batch = smirk_amd.encode_jpeg(dev, quality=75, restart_interval=3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    files = batch.to_host()
    assert len(batch) == 2 and files == [LAW.encode(im, 75, False, 3) for im in images]
    # [H, W, 3], BGR, an offset view, and the defaults
    one = smirk_amd.encode_jpeg(dev[1], bgr=True).to_host()
    assert one == [LAW.encode(images[1], 95, True, smirk_amd.jpeg.DEFAULT_RESTART_INTERVAL)]
    view = smirk_amd.encode_jpeg(dev[:, 1:, 2:], quality=50).to_host()                # not contiguous
    assert view == [LAW.encode(im[1:, 2:], 50, False, smirk_amd.jpeg.DEFAULT_RESTART_INTERVAL) for im in images]


def test_refusals():
    import smirk_amd
    from smirk_amd import SmirkHipError
    good = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device="cuda")
    for bad in (good.float(), good[..., :2], good[0, 0], good.unsqueeze(0), good.cpu().numpy()):
        with pytest.raises(ValueError):
            smirk_amd.encode_jpeg(bad)
    for kw in (dict(quality=0), dict(quality=101), dict(restart_interval=0), dict(restart_interval=-3)):
        with pytest.raises(ValueError):
            smirk_amd.encode_jpeg(good, **kw)
    with pytest.raises(ValueError):
        smirk_amd.encode_jpeg(good[:0])
    with pytest.raises(SmirkHipError, match="CPU"):
        smirk_amd.encode_jpeg(good.cpu())


def test_save_visualizations_hip_encoder(tmp_path):
    from smirk_amd import visualize
    r = np.random.default_rng(11)
    B, S = 2, 32
    rnd = lambda *s: torch.from_numpy(r.random(s, dtype=np.float32)).cuda()
    vis = dict(img=rnd(B, 3, S, S), rendered_img=rnd(B, 3, S, S), masked_1st_path=rnd(B, 3, S, S), loss_img=rnd(B, 1, S, S))
    for key, n in (('landmarks_mp', 105), ('landmarks_mp_gt', 105), ('landmarks_fan', 68), ('landmarks_fan_gt', 68)):
        vis[key] = 2 * rnd(B, n, 2) - 1
    path = str(tmp_path / "sheet.jpg")
    sheet = visualize.save_visualizations(vis, path, show_landmarks=True, encoder="hip")
    assert sheet.dtype == np.uint8 and sheet.shape[2] == 3 and np.array_equal(sheet, visualize.save_visualizations(vis, None, show_landmarks=True))
    data = open(path, "rb").read()
    assert data == LAW.encode(sheet, 95, True, visualize_default_interval())
    path2 = str(tmp_path / "rgb.JPEG")
    assert visualize.save_visualizations(vis, path2, show_landmarks=True, bgr=False, encoder="hip", return_sheet=False, quality=60) is None
    assert open(path2, "rb").read() == LAW.encode(sheet[..., ::-1], 60, False, visualize_default_interval())
    for kw in (dict(save_path=str(tmp_path / "x.png"), encoder="hip"), dict(save_path=None, encoder="hip"), dict(save_path=path, encoder="cv2"),
               dict(save_path=path, return_sheet=False), dict(save_path=path, quality=50)):
        with pytest.raises(ValueError):
            visualize.save_visualizations(vis, **kw)


def visualize_default_interval():
    from smirk_amd import jpeg
    return jpeg.DEFAULT_RESTART_INTERVAL


@pytest.fixture(scope="module")
def modules(sandbox):
    from oracle import mobilenet_ref as M
    from smirk_amd import FLAME, Renderer, SmirkEncoder
    cwd = os.getcwd(); os.chdir(sandbox)
    try:
        fl, rn = FLAME().cuda(), Renderer().cuda()
    finally:
        os.chdir(cwd)
    enc = SmirkEncoder(); enc.load_state_dict(M.synth_encoder_state_dict()); enc = enc.cuda().eval()
    return enc, fl, rn


def test_video_pipeline_yields_the_laws_files(modules, tmp_path):
    from smirk_amd import VideoPipeline, jpeg
    from smirk_amd.video import MjpegWriter
    enc, fl, rn = modules
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:48, 0:64]
    base = np.sin(xx / 7.0)[..., None] * np.array([60, 80, 40]) + np.cos(yy / 5.0)[..., None] * np.array([50, 30, 70]) + 128
    frames = [np.clip(base + rng.integers(-40, 40, (48, 64, 3)), 0, 255).astype(np.uint8) for _ in range(4)]
    vp = VideoPipeline(enc, fl, rn, batch_size=3)                                     # 4 frames in batches of 3: a ragged second batch
    arrays = list(vp.run(frames))
    files = list(vp.run(frames, jpeg=dict(quality=80)))
    assert len(files) == 4 and all(isinstance(f, bytes) for f in files)
    assert files == [LAW.encode(a, 80, True, jpeg.DEFAULT_RESTART_INTERVAL) for a in arrays]
    again = list(vp.run(frames))                                                      # and the default is back on the next run
    assert all(np.array_equal(a, b) for a, b in zip(arrays, again))
    with pytest.raises(ValueError):
        list(vp.run(frames, jpeg=dict(bgr=False)))
    with MjpegWriter(str(tmp_path / "out.avi"), 25, arrays[0].shape[1], arrays[0].shape[0]) as w:
        for f in files:
            w.write(f)
    assert os.path.getsize(str(tmp_path / "out.avi")) > sum(len(f) for f in files)
