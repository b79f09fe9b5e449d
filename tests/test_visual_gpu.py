"""smirk_amd.visualize on the MI355X: the sheet kernel, the landmark overlay and the Python surface against tests/visual_law.py.  Every comparison is byte for byte:
law and kernel produce integers from the same float32 operations in the same order, so there is no tolerance to choose."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import visual_law as LAW

pytestmark = pytest.mark.gpu

F = np.float32


def _host(vis):
    return {k: ([t.cpu().numpy() for t in v] if isinstance(v, (tuple, list)) else v.cpu().numpy()) for k, v in vis.items() if k != 'encoder_output'}


def _levels():
    """every k / 255 with its two float32 neighbours: 768 values, one 3 x 16 x 16 image"""
    k = np.arange(256, dtype=F) / F(255)
    return np.stack([np.nextafter(k, F(-1)), k, np.nextafter(k, F(2))], 1).ravel()


def _panels(B, S, Ke, seed):
    """the columns of the issue's sheet: plain 3-channel (img, rendered_img, masked_1st_path), 1-channel (loss_img), both blends, a panel resampled 8 -> 16
    (img_mica) and the four-source interleave; pixel values: every level with its neighbours, values below 0 and above 1, NaN, random"""
    r = np.random.default_rng(seed)
    rnd = lambda *s: r.random(s, dtype=F)

    def spiced(x):
        flat = x.reshape(-1)
        at = r.choice(flat.size, size=max(flat.size // 8, 6), replace=False)
        flat[at] = np.resize(np.array([-0.25, -1e-8, -3.0, 1.0000001, 1.5, 260.0, np.nan, -np.inf, np.inf, -0.0, 1.0, 0.0], F), at.size)
        return x
    img = rnd(B, 3, S, S)
    if S == 16:
        img[0] = _levels().reshape(3, S, S)
        if B > 1:
            img[1:] = spiced(img[1:])
    vis = dict(img=img, rendered_img=spiced(rnd(B, 3, S, S)), masked_1st_path=spiced(rnd(B, 3, S, S)), loss_img=spiced(rnd(B, 1, S, S)),
               img_mica=spiced(rnd(B, 3, S // 2, S // 2)), reconstructed_img=rnd(B, 3, S, S))
    vis['2nd_path'] = tuple(spiced(rnd(Ke * B, 3, S, S)) for _ in range(4))
    vis['rendered_img'][0] = _levels()[::-1].reshape(3, S, S) if S == 16 else vis['rendered_img'][0]
    for key, n in (('landmarks_mp', 105), ('landmarks_mp_gt', 105), ('landmarks_fan', 68), ('landmarks_fan_gt', 68)):
        vis[key] = (2 * rnd(B, n, 2) - 1).astype(F)
    return vis


def _device(vis):
    return {k: (tuple(torch.from_numpy(t).cuda() for t in v) if isinstance(v, tuple) else torch.from_numpy(v).cuda()) for k, v in vis.items()}


# ---- the sheet against the law ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [True, False], ids=["bgr", "rgb"])
@pytest.mark.parametrize("Ke", [1, 2])
def test_sheet_equals_the_law(Ke, bgr):
    from smirk_amd import save_visualizations
    B, S = 2, 16
    vis = _panels(B, S, Ke, seed=10 + Ke)
    want = LAW.sheet(vis, Ke=Ke, bgr=bgr)
    got = save_visualizations(_device(vis), Ke=Ke, bgr=bgr)
    assert got.dtype == np.uint8 and got.shape == want.shape == (B * (S + 2) + 2, 8 * (S + 4) + 4 * Ke * (S + 2) + 2, 3)
    diff = np.argwhere(got != want)
    print(f"Ke = {Ke}, bgr = {bgr}: sheet {got.shape}, {len(diff)} differing bytes")
    assert len(diff) == 0, diff[:10]
    # the level image came through as itself: below a level truncates to the level under it
    lv = got[2:2 + S, 2:2 + S][..., ::-1] if bgr else got[2:2 + S, 2:2 + S]
    lv = lv.transpose(2, 0, 1).reshape(256, 3)
    assert np.array_equal(lv[:, 1], np.arange(256)) and np.array_equal(lv[1:, 0], np.arange(255)) and np.array_equal(lv[:, 2], np.arange(256))


def test_tail_alignment_and_every_byte_written():
    """Byte counts that are no multiple of 16: the sentinels behind the rounded count stay, everything before them is written once, padding and tail included (the
    buffer starts as 0xAB, which no padding byte may keep)."""
    from smirk_amd import _lib as L, visualize
    lib = L.lib()
    for B, S, keys in ((2, 16, ('img',)), (3, 10, ('img', 'loss_img', 'rendered_img', 'masked_1st_path')), (5, 9, ('img', 'loss_img'))):
        vis = {k: v for k, v in _panels(B, S, 1, seed=S).items() if k in keys or k.startswith('landmarks')}
        dev = _device(vis)
        arr, keep, b, s, H, W, nbytes = visualize.plan_sheet(dev)
        assert (b, s) == (B, S) and H * W * 3 % 16 != 0 and nbytes == H * W * 3 + (-H * W * 3) % 16
        buf = torch.full((nbytes + 512,), 0xAB, dtype=torch.uint8, device="cuda")
        L.check(lib.smirk_visual_sheet(arr, len(arr), B, S, 1, None, 0, C.c_void_p(buf.data_ptr()), nbytes, L.stream_ptr()))
        out = buf.cpu().numpy()
        want = LAW.sheet(vis)
        assert want.shape == (H, W, 3)
        assert np.array_equal(out[:H * W * 3].reshape(H, W, 3), want), (B, S)
        assert not out[H * W * 3:nbytes].any() and (out[nbytes:] == 0xAB).all()
        pad = np.ones((H, W), bool)
        for c in range(len(arr)):
            for k in range(B):
                pad[k * (S + 2) + 2:k * (S + 2) + 2 + S, c * (S + 4) + 2:c * (S + 4) + 2 + S] = False
        assert pad.sum() == H * W - len(arr) * B * S * S and not out[:H * W * 3].reshape(H, W, 3)[pad].any()


# ---- landmarks ---------------------------------------------------------------------------------------------------------------------------------------------
def _points(S, centre):
    """pixel positions -> landmark coordinates; the kernel and the law both compute lm * centre + centre in float32"""
    e = S - 1
    mp = [(-0.4, -0.4), (0, 5), (e, 6), (7, 0), (9, e), (0, 0), (0, e), (e, 0), (e, e), (-1, 3), (S, 11), (4, -1), (12, S), (-2, 8), (S + 1, 8), (-40, -40),
          (3 * S, 2), (np.nan, 4), (4, np.inf), (-np.inf, np.nan), (5.99, 5.01), (6.0, 9.0)]
    mp_gt = [(5, 5), (6, 10), (7, 9), (2.5, 12.5), (-0.9, 14.2), (np.inf, np.inf), (10, 4)]        # coincident with, and adjacent to, points of layer 0
    fan = [(5, 5), (10, 5), (11, 4), (e - 0.5, e - 0.5), (8, 8)] + [(8, 8)] * 12                   # coincident with layers 0 and 1; 17 rows
    fan_gt = [(10, 5), (8, 9), (13, 13), (np.nan, np.nan)] + [(13, 12)] * 13
    unused = [(k % S, (3 * k) % S) for k in range(68 - 17)]                                        # rows 17 .. 67: would draw all over the cell
    to_lm = lambda pts: ((np.array(pts, np.float64) - centre) / centre).astype(F)
    return to_lm(mp), to_lm(mp_gt), to_lm(fan + unused), to_lm(fan_gt + unused)


def _landmark_vis(B, S, centre, seed):
    vis = {k: v for k, v in _panels(B, S, 1, seed).items() if k in ('img', 'loss_img')}
    layers = _points(S, centre)
    for (key, _, _), lm in zip(LAW.LAYERS, layers):
        per_frame = [lm if b == 0 else np.roll(lm, b, 0)[::-1] * F(0.9) for b in range(B)]
        vis[key] = np.ascontiguousarray(np.stack(per_frame))
    return vis


def test_landmarks_small():
    from smirk_amd import visualize
    B, S, centre = 2, 16, 8.0
    vis = _landmark_vis(B, S, centre, seed=4)
    want = LAW.sheet(vis, show_landmarks=True, centre=centre)
    plain = LAW.sheet(vis, show_landmarks=False)
    every = dict(vis)
    every['landmarks_fan'], every['landmarks_fan_gt'] = vis['landmarks_fan'][:, :17], vis['landmarks_fan_gt'][:, :17]
    assert np.array_equal(LAW.sheet(every, show_landmarks=True, centre=centre), want)              # the law draws the first 17 rows only ...
    assert (want != plain).any() and tuple((k, n) for k, n, _ in LAW.LAYERS) == visualize.LANDMARK_LAYERS
    dev = _device(vis)
    runs = []
    for _ in range(2):
        sheet, H, W = visualize.render_sheet(dev, show_landmarks=True, landmark_centre=centre)
        runs.append(visualize.download_sheet(sheet, H, W).copy())
    assert np.array_equal(runs[0], runs[1])
    diff = np.argwhere(runs[0] != want)
    print(f"landmarks S = {S}: {int((want != plain).any(-1).sum())} overlay pixels, {len(diff)} differing bytes")
    assert len(diff) == 0, diff[:10]
    cell = want[2:2 + S, 2:2 + S, ::-1]                                                            # frame 0, RGB
    assert tuple(cell[0, 0]) == (0, 255, 0)                                                        # (-0.4, -0.4) truncates to pixel (0, 0)
    assert tuple(cell[5, 5]) == (255, 0, 255) and tuple(cell[5, 10]) == (255, 255, 255)            # coincident centres: the later layer wins
    assert tuple(cell[10, 6]) == (255, 0, 0) and tuple(cell[9, 6]) == (255, 0, 0) and tuple(cell[4, 11]) == (255, 0, 255)      # and so does a later neighbour's disc
    assert tuple(cell[3, 0]) == (0, 255, 0) and tuple(cell[11, S - 1]) == (0, 255, 0)              # centres one pixel outside still reach the border
    # rows 17 .. 67 of the fan layers are not drawn: they would have reached pixels the sheet leaves as they were
    drawn = np.zeros((1, S, S, 3), np.uint8)
    LAW.draw_keypoints(drawn, vis['landmarks_fan'][:1, 17:], (1, 1, 1), centre)
    painted = (want[2:2 + S, 2:2 + S] != plain[2:2 + S, 2:2 + S]).any(-1)
    assert ((drawn[0, :, :, 0] != 0) & ~painted).any()


def test_landmarks_full_size_single_frame():
    """B = 1, S = 224 at the reference's centre of 112: no padding, and the same point classes at full size"""
    from smirk_amd import save_visualizations
    B, S = 1, 224
    vis = _landmark_vis(B, S, 112.0, seed=6)
    want = LAW.sheet(vis, show_landmarks=True)
    dev = _device(vis)
    got = save_visualizations(dev, show_landmarks=True)
    again = save_visualizations(dev, show_landmarks=True)
    assert got.shape == want.shape == (S, 2 * S, 3) and np.array_equal(got, again)
    diff = np.argwhere(got != want)
    print(f"landmarks S = {S}: {len(diff)} differing bytes")
    assert len(diff) == 0, diff[:10]
    assert tuple(want[0, 0, ::-1]) == (0, 255, 0) and tuple(want[5, 5, ::-1]) == (255, 0, 255)


def test_single_frame_has_no_padding():
    from smirk_amd import save_visualizations
    B, S = 1, 16
    vis = {k: v for k, v in _panels(B, S, 1, seed=8).items() if k != '2nd_path'}
    want = LAW.sheet(vis, bgr=False)
    got = save_visualizations(_device(vis), bgr=False)
    assert got.shape == want.shape == (S, 8 * S, 3) and np.array_equal(got, want)
    assert np.array_equal(got[:, :S], LAW.quantise(vis['img'][0], bgr=False))
    with pytest.raises(ValueError, match="differ in height"):
        save_visualizations(_device(_panels(B, S, 1, seed=8)))


# ---- the Python surface over the modules ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def modules(sandbox):
    from oracle import generator_ref as G
    from oracle import mobilenet_ref as M
    from smirk_amd import FLAME, Renderer, SmirkEncoder, SmirkGenerator, masking
    cwd = os.getcwd(); os.chdir(sandbox)
    try:
        fl, rn = FLAME().cuda(), Renderer().cuda()
        prob = masking.load_probabilities_per_FLAME_triangle().cuda()
    finally:
        os.chdir(cwd)
    enc = SmirkEncoder(); enc.load_state_dict(M.synth_encoder_state_dict()); enc = enc.cuda().eval()
    gen = SmirkGenerator(6, 3, 32, 5); gen.load_state_dict(G.synth_state_dict()); gen = gen.cuda().eval()
    return fl, rn, enc, gen, prob


def _batch(B):
    from loss_law import synth_first_path_inputs
    from oracle import assets as A
    batch = synth_first_path_inputs(B, seed=31, device="cuda")[3]
    batch["img"] = A.synth_images(B, seed=81).cuda()
    yy, xx = torch.meshgrid(torch.arange(224.0), torch.arange(224.0), indexing="ij")
    batch["mask"] = (((yy - 112) ** 2 + (xx - 112) ** 2) > 80 ** 2).float()[None, None].repeat(B, 1, 1, 1).cuda()
    batch["img_mica"] = torch.rand(B, 3, 112, 112, generator=torch.Generator().manual_seed(5)).cuda()
    return batch


def test_create_visualizations(modules):
    import mica_law as ML
    from smirk_amd import MICA, create_visualizations
    fl, rn, enc, gen, prob = modules
    mica = MICA(ML.synth_checkpoint((1, 1, 1, 1), 1), layers=(1, 1, 1, 1)).cuda()
    B = 2
    batch = _batch(B)
    with torch.no_grad():
        encoder_output = enc(batch["img"])
        encoder_output["shape_params"] = encoder_output["shape_params"] + 0.25               # not the base model's output
        fo = fl.forward(encoder_output)
        ro = rn.forward(fo["vertices"], encoder_output["cam"], landmarks_fan=fo["landmarks_fan"], landmarks_mp=fo["landmarks_mp"])
    g = torch.Generator().manual_seed(3)
    outputs = dict(encoder_output=encoder_output, rendered_img=ro["rendered_img"], landmarks_fan=ro["landmarks_fan"], landmarks_mp=ro["landmarks_mp"],
                   landmarks_fan_gt=batch["landmarks_fan"], landmarks_mp_gt=batch["landmarks_mp"], reconstructed_img=torch.rand(B, 3, 224, 224, generator=g).cuda(),
                   masked_1st_path=torch.rand(B, 3, 224, 224, generator=g).cuda(), loss_img=torch.rand(B, 1, 224, 224, generator=g).cuda(), vertices=fo["vertices"])
    second = tuple(torch.rand(B, 3, 224, 224, generator=g).cuda() for _ in range(4))
    mods = dict(flame=fl, renderer=rn, encoder=enc, mica=mica)
    state = {n: {k: v.clone() for k, v in m.state_dict().items()} for n, m in mods.items()}
    modes = {n: m.training for n, m in mods.items()}
    vis = create_visualizations(batch, outputs, fl, rn, base_encoder=enc, mica=mica, num_shape=300, second_path=second + (1,))
    for n, m in mods.items():
        assert m.training == modes[n] and all(torch.equal(v, state[n][k]) for k, v in m.state_dict().items()), n
    assert set(vis) == {'img', 'rendered_img', 'rendered_img_base', 'rendered_img_zero', 'reconstructed_img', 'masked_1st_path', 'loss_img', 'rendered_img_mica_zero',
                        'img_mica', '2nd_path', 'landmarks_mp', 'landmarks_mp_gt', 'landmarks_fan', 'landmarks_fan_gt'}
    for k, v in vis.items():
        for t in (v if isinstance(v, tuple) else (v,)):
            assert t.is_cuda and not t.requires_grad, k
    # the direct module calls of base_trainer.py:165-224
    with torch.no_grad():
        cam0 = torch.tensor([7.0, 0.0, 0.0], device="cuda").repeat(B, 1)
        base = enc(batch["img"])
        want = dict(rendered_img_base=rn.forward(fl.forward(base)["vertices"], base["cam"])["rendered_img"],
                    rendered_img_zero=rn.forward(fl.forward(encoder_output, zero_expression=True, zero_pose=True)["vertices"], cam0)["rendered_img"])
        mo = dict(base); mo["shape_params"] = mica(batch["img_mica"])["shape_params"]
        want["rendered_img_mica_zero"] = rn.forward(fl.forward(mo, zero_expression=True, zero_pose=True)["vertices"], cam0)["rendered_img"]
    for k, v in want.items():
        assert torch.equal(vis[k], v) and v.abs().sum() > 0, k
    assert not torch.equal(want["rendered_img_zero"], want["rendered_img_mica_zero"]) and not torch.equal(want["rendered_img_zero"], want["rendered_img_base"])
    for k in ('rendered_img', 'reconstructed_img', 'masked_1st_path', 'loss_img', 'landmarks_mp', 'landmarks_fan'):
        assert torch.equal(vis[k], outputs[k]), k
    assert vis['img'] is batch['img'] and torch.equal(vis['landmarks_mp_gt'], batch['landmarks_mp']) and torch.equal(vis['landmarks_fan_gt'], batch['landmarks_fan'])
    assert tuple(vis['img_mica'].shape) == (B, 3, 112, 112) and torch.equal(vis['img_mica'], batch['img_mica'])      # stays at 112: the sheet resamples it
    assert all(torch.equal(a, b) for a, b in zip(vis['2nd_path'], second))
    # the num_shape cut (base_trainer.py:202-204), and what is left out without the optional modules
    cut = create_visualizations(batch, outputs, fl, rn, base_encoder=enc, mica=mica, num_shape=100)
    with torch.no_grad():
        mo["shape_params"] = mica(batch["img_mica"])["shape_params"][:, :100]
        assert torch.equal(cut["rendered_img_mica_zero"], rn.forward(fl.forward(mo, zero_expression=True, zero_pose=True)["vertices"], cam0)["rendered_img"])
    bare = create_visualizations(batch, outputs, fl, rn)
    assert not {'rendered_img_base', 'rendered_img_mica_zero', 'img_mica', '2nd_path'} & set(bare) and torch.equal(bare['rendered_img_zero'], want['rendered_img_zero'])
    with pytest.raises(ValueError, match="Ke \\* B"):
        create_visualizations(batch, outputs, fl, rn, second_path=second + (2,))


def test_end_to_end_sheet(modules):
    """first_path + the second path at B = 2, S = 224, Ke = 1 -> create_visualizations -> save_visualizations, against the law applied to the same tensors on the host"""
    from augment_law import synth_templates
    from loss_law import WEIGHTS_TRAIN
    from smirk_amd import FirstPathLoss, TemplateBank, create_visualizations, masking, save_visualizations
    from smirk_amd.cycle import second_path
    from smirk_amd.first_path import first_path
    fl, rn, enc, gen, prob = modules
    B, Ke = 2, 1
    batch = _batch(B)
    with torch.no_grad():
        loss, terms, out = first_path(enc, fl, rn, gen, FirstPathLoss(WEIGHTS_TRAIN), batch, prob, _rng_stream=masking.PhiloxStream(7))
        bank = TemplateBank(synth_templates(width=50), num_expression=50).cuda()
        torch.manual_seed(11)
        feats, rendered, masked = second_path(fl, rn, out['encoder_output'], bank, batch['img'], batch['mask'], prob, masking, Ke=Ke)
        recon = gen(torch.cat([rendered, masked], dim=1))
        again = enc(recon)
        rendered_2 = rn.forward(fl.forward(again)['vertices'], again['cam'])['rendered_img']
    vis = create_visualizations(batch, out, fl, rn, base_encoder=enc, second_path=(rendered, masked, recon, rendered_2, Ke))
    host = _host(vis)
    assert 'loss_img' in host and host['loss_img'].shape == (B, 1, 224, 224) and len(host['2nd_path']) == 4
    for show in (True, False):
        got = save_visualizations(vis, show_landmarks=show, Ke=Ke)
        want = LAW.sheet(host, show_landmarks=show, Ke=Ke)
        diff = np.argwhere(got != want)
        print(f"end to end, landmarks {show}: sheet {got.shape}, {len(diff)} differing bytes")
        assert got.shape == want.shape == (2 * 226 + 2, 9 * 228 + 4 * 226 + 2, 3) and len(diff) == 0, diff[:10]
    assert got.any(axis=2).mean() > 0.3                                                            # a sheet with content


def test_file_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from smirk_amd import save_visualizations
    vis = _device(_panels(2, 16, 1, seed=2))
    path = str(tmp_path / "sheet.png")
    got = save_visualizations(vis, save_path=path, show_landmarks=True)
    back = np.asarray(Image.open(path))
    assert back.shape == got.shape and np.array_equal(back[..., ::-1], got)                        # the file is RGB, the returned array BGR like the reference's
    path = str(tmp_path / "rgb.png")
    rgb = save_visualizations(vis, save_path=path, bgr=False)
    assert np.array_equal(np.asarray(Image.open(path)), rgb)
