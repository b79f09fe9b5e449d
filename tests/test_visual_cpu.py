"""smirk_amd.visualize without a GPU: the extension table of include/smirk_visual.h against its header, every refusal of every entry (raw ctypes, dummy pointers
that are never dereferenced: a refusal comes before anything touches the device), the Python refusals (shapes only: nothing is launched), and the self-checks that
keep the law of tests/visual_law.py honest without torchvision."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import visual_law as LAW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, R, S_, T, U = (0x10000 * k for k in range(1, 7))              # never dereferenced; all 256-byte aligned
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


# ---- the table --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_extension_table_equals_the_header():
    from smirk_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "smirk_visual.h")).read()
    declared = set(re.findall(r"\b(smirk_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.VISUAL_EXPORTS), declared ^ set(L.VISUAL_EXPORTS)
    assert L.VISUAL_EXPORTS == tuple(L.VISUAL_SIGS) and len(L.VISUAL_EXPORTS) == 5
    others = (L.EXPORTS, L.MICA_EXPORTS, L.EMOTION_EXPORTS, L.OPTIM_EXPORTS, L.HANDOFF_EXPORTS, L.GENPLAN_EXPORTS, L.GENARITH_EXPORTS, L.DATA_EXPORTS)
    for other in others:
        assert not set(L.VISUAL_EXPORTS) & set(other)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    version = int(re.search(r"#define\s+SMIRK_VISUAL_ABI_VERSION\s+(\d+)", hdr).group(1))
    lib = L.lib()
    assert lib.smirk_visual_abi_version() == L.VISUAL_ABI_VERSION == version == 1
    assert "smirk_visual.h" in open(os.path.join(REPO, "README.md")).read()
    build_py = open(os.path.join(REPO, "smirk_amd", "build.py")).read()
    assert '"smirk_visual.h"' in build_py and re.search(r'"visual\.hip":\s*\["-ffp-contract=off"\]', build_py)
    # the other tables and their versions did not move, none of their headers names the new entries, and the new header names none of theirs
    assert lib.smirk_abi_version() == L.ABI_VERSION == 17 and len(L.EXPORTS) == 116
    assert (lib.smirk_mica_abi_version(), lib.smirk_emotion_abi_version(), lib.smirk_optim_abi_version(), lib.smirk_handoff_abi_version(),
            lib.smirk_genplan_abi_version(), lib.smirk_genarith_abi_version(), lib.smirk_data_abi_version()) == (1, 1, 1, 1, 1, 1, 1)
    for name in os.listdir(os.path.join(REPO, "include")):
        if name != "smirk_visual.h":
            text = open(os.path.join(REPO, "include", name)).read()
            assert not any(e in text for e in L.VISUAL_EXPORTS), name
    for other in others:
        assert not any(re.search(rf"\b{e}\b(?!\.h)", hdr) for e in other)      # the file names smirk_generator_plan.h / _arith.h are not entries
    # the constants and records _lib.py mirrors
    for macro, value in (("MAX_COLUMNS", L.VISUAL_MAX_COLUMNS), ("MAX_POINTS", L.VISUAL_MAX_POINTS), ("LAYERS", L.VISUAL_LAYERS), ("MIN_SIZE", L.VISUAL_MIN_SIZE),
                         ("MAX_SIZE", L.VISUAL_MAX_SIZE), ("PADDING", L.VISUAL_PADDING)):
        assert int(re.search(rf"#define\s+SMIRK_VISUAL_{macro}\s+(\d+)", hdr).group(1)) == value
    assert (L.VISUAL_MAX_COLUMNS, L.VISUAL_MAX_POINTS, L.VISUAL_PADDING) == (16, 1024, LAW.PADDING)
    assert C.sizeof(L.SmirkVisualColumn) == 72 and C.sizeof(L.SmirkVisualDots) == 64
    assert L.SmirkVisualColumn.blend.offset == 32 and L.SmirkVisualColumn.nsrc.offset == 48 and L.SmirkVisualColumn.landmarks.offset == 68


def test_exported_from_the_package():
    import smirk_amd
    from smirk_amd import visualize
    assert smirk_amd.visualize is visualize and smirk_amd.create_visualizations is visualize.create_visualizations
    assert smirk_amd.save_visualizations is visualize.save_visualizations
    assert {"visualize", "create_visualizations", "save_visualizations"} <= set(smirk_amd.__all__)
    assert visualize.IMAGE_KEYS == LAW.IMAGE_KEYS and visualize.LANDMARK_CENTRE == 112.0 and visualize.OVERLAP_WEIGHTS == (0.7, 0.3)
    assert tuple((k, n) for k, n, _ in LAW.LAYERS) == visualize.LANDMARK_LAYERS


# ---- refusals of the library ----------------------------------------------------------------------------------------------------------------------------------------
def _col(src=(P,), blend=None, w=(0.0, 0.0), channels=3, Hs=16, Ws=16, nrow=1, landmarks=0, nsrc=None):
    from smirk_amd import _lib as L
    c = L.SmirkVisualColumn()
    for k, s in enumerate(src):
        c.src[k] = s
    c.blend, c.w_src, c.w_blend = blend, w[0], w[1]
    c.nsrc, c.channels, c.Hs, c.Ws, c.nrow, c.landmarks = len(src) if nsrc is None else nsrc, channels, Hs, Ws, nrow, landmarks
    return c


def _arr(cols):
    from smirk_amd import _lib as L
    return (L.SmirkVisualColumn * len(cols))(*cols)


def test_sheet_size_and_its_refusals():
    from smirk_amd import _lib as L
    lib = L.lib()

    def size(cols, B=2, S=16, n=None, out=(True, True, True)):
        H, W, nb = C.c_int32(-7), C.c_int32(-7), C.c_size_t(7)
        rc = lib.smirk_visual_sheet_size(_arr(cols) if cols is not None else None, len(cols) if n is None else n, B, S,
                                         C.byref(H) if out[0] else None, C.byref(W) if out[1] else None, C.byref(nb) if out[2] else None)
        return rc, H.value, W.value, nb.value
    # geometry: the byte count is H * W * 3 rounded up to 16
    assert size([_col()]) == (0, 38, 20, 38 * 20 * 3 + (-38 * 20 * 3) % 16)
    assert size([_col()], B=1) == (0, 16, 16, 768)
    assert size([_col(), _col(channels=1), _col(src=(P, Q, R, S_), nrow=8)], B=3) == (0, 56, 20 + 20 + 8 * 18 + 2, 56 * 186 * 3)
    assert size([_col(nrow=2)], B=5) == (0, 3 * 18 + 2, 2 * 18 + 2, 56 * 38 * 3)
    assert size([_col()] * 16)[0] == 0
    assert size([_col()], S=8)[0] == 0 and size([_col()], S=4096, B=1)[0] == 0
    # refusals
    assert size(None, n=1)[0] == BAD_ARG
    for out in ((False, True, True), (True, False, True), (True, True, False)):
        assert size([_col()], out=out)[0] == BAD_ARG
    assert size([_col()], n=0)[0] == BAD_ARG and size([_col()] * 17)[0] == BAD_ARG and size([_col()], n=-1)[0] == BAD_ARG
    assert size([_col()], B=0)[0] == BAD_ARG and size([_col()], B=-2)[0] == BAD_ARG
    for bad in (dict(channels=2), dict(channels=0), dict(channels=4), dict(nsrc=2), dict(nsrc=0), dict(nsrc=3), dict(Hs=0), dict(Ws=-1), dict(nrow=0),
                dict(src=(P, Q, R, S_), nrow=6), dict(src=(P, Q, R, S_), nrow=4, landmarks=1)):
        assert size([_col(), _col(**bad)])[0] == BAD_ARG, bad
    assert size([_col(landmarks=1), _col(landmarks=1)])[0] == BAD_ARG
    for S in (0, -16, 7, 4097):
        assert size([_col()], S=S)[0] == UNSUPPORTED, S
    assert size([_col(), _col(nrow=2)], B=4)[0] == UNSUPPORTED                       # 4 rows of 1 against 2 rows of 2
    assert size([_col(), _col(src=(P, Q, R, S_), nrow=4)], B=1)[0] == UNSUPPORTED    # B == 1: unpadded panel beside a padded one
    assert size([_col()] * 16, B=40, S=4096)[0] == UNSUPPORTED                       # 2^31 bytes and more
    assert size([_col()], B=300, S=4096)[0] == UNSUPPORTED                           # higher than 2^20 rows
    assert size([_col()], B=1)[1:] == (16, 16, 768) and size([_col(), _col(nrow=2)], B=4)[1:] == (-7, -7, 7)       # a refusal writes nothing


def test_workspace_bytes():
    from smirk_amd import _lib as L
    lib = L.lib()
    assert lib.smirk_visual_workspace_bytes(2, 16) == 512 and lib.smirk_visual_workspace_bytes(1, 224) == 224 * 224
    assert lib.smirk_visual_workspace_bytes(3, 10) == 512 and lib.smirk_visual_workspace_bytes(64, 224) == 64 * 224 * 224
    for bad in ((0, 16), (-1, 16), (2, 0), (2, 7), (2, 4097), (2, -16)):
        assert lib.smirk_visual_workspace_bytes(*bad) == 0, bad


def test_dots_refuses_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    need = lib.smirk_visual_workspace_bytes(2, 16)

    def dots(lm=(P, Q, R, S_), rows=(105, 105, 68, 68), npts=(105, 105, 17, 17), B=2, S=16, centre=8.0, ws=T, ws_bytes=need, null=False):
        d = L.SmirkVisualDots()
        for l in range(4):
            d.lm[l], d.rows[l], d.npts[l] = lm[l], rows[l], npts[l]
        return lib.smirk_visual_dots(None if null else C.byref(d), B, S, centre, ws, ws_bytes, None)
    assert dots(null=True) == BAD_ARG and dots(ws=None) == BAD_ARG and dots(ws=T + 16) == BAD_ARG
    assert dots(lm=(P + 2, Q, R, S_)) == BAD_ARG and dots(lm=(P, Q, R, S_ + 1)) == BAD_ARG
    assert dots(B=0) == BAD_ARG and dots(B=-1) == BAD_ARG
    assert dots(rows=(105, -1, 68, 68)) == BAD_ARG and dots(npts=(105, 105, -1, 17)) == BAD_ARG and dots(npts=(106, 105, 17, 17)) == BAD_ARG
    assert dots(centre=float("nan")) == BAD_ARG and dots(centre=float("inf")) == BAD_ARG
    for S in (0, 7, 4097, -16):
        assert dots(S=S) == UNSUPPORTED, S
    assert dots(rows=(1025, 105, 68, 68), npts=(1025, 105, 17, 17)) == UNSUPPORTED
    assert dots(ws_bytes=need - 1) == WORKSPACE and dots(ws_bytes=0) == WORKSPACE
    assert dots(B=3, ws_bytes=need) == WORKSPACE


def test_sheet_refuses_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()

    def sheet(cols, B=2, S=16, n=None, ws=None, ws_bytes=0, out=U, out_bytes=1 << 24):
        return lib.smirk_visual_sheet(_arr(cols) if cols is not None else None, len(cols) if n is None else n, B, S, 1, ws, ws_bytes, out, out_bytes, None)
    # everything the size entry refuses
    assert sheet(None, n=1) == BAD_ARG and sheet([_col()], n=0) == BAD_ARG and sheet([_col()] * 17) == BAD_ARG and sheet([_col()], B=0) == BAD_ARG
    for bad in (dict(channels=2), dict(nsrc=2), dict(Hs=0), dict(Ws=0), dict(nrow=0), dict(src=(P, Q, R, S_), nrow=6), dict(src=(P, Q, R, S_), nrow=4, landmarks=1)):
        assert sheet([_col(), _col(**bad)]) == BAD_ARG, bad
    assert sheet([_col(landmarks=1), _col(landmarks=1)], ws=T, ws_bytes=512) == BAD_ARG
    assert sheet([_col()], S=7) == UNSUPPORTED and sheet([_col()], S=4097) == UNSUPPORTED
    assert sheet([_col(), _col(nrow=2)], B=4) == UNSUPPORTED and sheet([_col(), _col(src=(P, Q, R, S_), nrow=4)], B=1) == UNSUPPORTED
    # and its own
    assert sheet([_col()], out=None) == BAD_ARG and sheet([_col()], out=U + 16) == BAD_ARG and sheet([_col()], out=U + 128) == BAD_ARG
    assert sheet([_col(src=(None,), nsrc=1)]) == BAD_ARG and sheet([_col(src=(P + 2,))]) == BAD_ARG
    assert sheet([_col(src=(P, Q, None, S_), nrow=4)]) == BAD_ARG and sheet([_col(src=(P, Q, R, S_ + 1), nrow=4)]) == BAD_ARG
    assert sheet([_col(blend=Q + 1, w=(0.7, 0.3))]) == BAD_ARG
    assert sheet([_col(src=(P, Q, R, S_), nrow=4, blend=T, w=(0.7, 0.3))]) == BAD_ARG
    assert sheet([_col(blend=Q, w=(0.7, 0.3), landmarks=1)], ws=T, ws_bytes=512) == BAD_ARG
    assert sheet([_col(blend=Q, w=(float("nan"), 0.3))]) == BAD_ARG and sheet([_col(blend=Q, w=(0.7, float("inf")))]) == BAD_ARG
    assert sheet([_col(landmarks=1)], ws=None, ws_bytes=512) == BAD_ARG and sheet([_col(landmarks=1)], ws=T + 64, ws_bytes=512) == BAD_ARG
    need = 38 * 20 * 3 + (-38 * 20 * 3) % 16
    assert sheet([_col()], out_bytes=need - 1) == WORKSPACE and sheet([_col()], out_bytes=38 * 20 * 3) == WORKSPACE and sheet([_col()], out_bytes=0) == WORKSPACE
    assert sheet([_col(landmarks=1)], ws=T, ws_bytes=511) == WORKSPACE and sheet([_col(landmarks=1)], ws=T, ws_bytes=0) == WORKSPACE


# ---- refusals of the Python surface (shapes only: nothing is launched) ------------------------------------------------------------------------------------------------
def _vis(B=2, S=16, Ke=1, second=True):
    z = lambda *s: torch.zeros(*s)
    vis = dict(img=z(B, 3, S, S), rendered_img=z(B, 3, S, S), masked_1st_path=z(B, 3, S, S), loss_img=z(B, 1, S, S), img_mica=z(B, 3, 8, 8),
               landmarks_mp=z(B, 105, 2), landmarks_mp_gt=z(B, 105, 2), landmarks_fan=z(B, 68, 2), landmarks_fan_gt=z(B, 68, 2))
    if second:
        vis['2nd_path'] = tuple(z(Ke * B, 3, S, S) for _ in range(4))
    return vis


def test_python_refusals():
    from smirk_amd import SmirkHipError, visualize
    cols, B, S, H = visualize.sheet_layout(_vis(Ke=2), show_landmarks=True, Ke=2)
    assert (B, S, H) == (2, 16, 38) and [len(c[0]) for c in cols] == [1, 1, 1, 1, 1, 1, 1, 4] and cols[0][3] and cols[-1][2] == 8
    assert [c[1] is not None for c in cols] == [False, False, False, True, True, False, False, False]      # the two overlap panels are blend columns

    def refused(match, vis, **kw):
        with pytest.raises(ValueError, match=match):
            visualize.save_visualizations(vis, **kw)
    refused("differ in height", _vis(B=1))                                            # B == 1 with a second-path panel
    refused("differ in height", _vis(B=1, Ke=3), Ke=3)
    v = _vis(second=False); v['rendered_img_zero'] = torch.zeros(2, 3, 8, 16)         # a panel that is not square resamples to the cell: same height, accepted
    assert visualize.sheet_layout(v)[3] == 38
    refused("Ke \\* B", _vis(Ke=2), Ke=1)
    refused("Ke \\* B", _vis(Ke=1), Ke=2)
    refused("at least 1", _vis(), Ke=0)
    v = _vis(); v['2nd_path'] = torch.zeros(8, 3, 16, 16)
    refused("four", v)
    v = _vis(); v['2nd_path'] = v['2nd_path'][:3]
    refused("four", v)
    v = _vis(); v['2nd_path'] = v['2nd_path'][:3] + (torch.zeros(2, 3, 8, 8),)
    refused("one shape", v)
    v = _vis(); v['loss_img'] = torch.zeros(2, 2, 16, 16)
    refused("1 or 3", v)
    v = _vis(); v['loss_img'] = torch.zeros(2, 16, 16)
    refused("1 or 3", v)
    v = _vis(); v['loss_img'] = torch.zeros(3, 1, 16, 16)
    refused("holds 3 images", v)
    v = _vis(); v['rendered_img'] = torch.zeros(2, 1, 16, 16)
    refused("another shape", v)
    v = _vis(); v['img'] = torch.zeros(2, 3, 16, 12)
    refused("square", v)
    refused("outside", _vis(S=4))
    v = _vis(); v['landmarks_fan'] = torch.zeros(2, 68, 3)
    refused("landmarks_fan", v, show_landmarks=True)
    visualize.sheet_layout(v)                                                         # without the overlay the landmark arrays are not looked at
    v = _vis(); v['landmarks_mp_gt'] = torch.zeros(3, 105, 2)
    refused("landmarks_mp_gt", v, show_landmarks=True)
    v = _vis(); v['landmarks_mp'] = torch.zeros(2, 1025, 2)
    refused("at most 1024", v, show_landmarks=True)
    v = _vis(); v['landmarks_fan'] = torch.zeros(2, 2000, 2)                          # only the first 17 are drawn
    visualize.sheet_layout(v, show_landmarks=True)
    # and a well-formed sheet of CPU tensors is refused as everywhere else
    with pytest.raises(SmirkHipError, match="CPU"):
        visualize.save_visualizations(_vis())
    with pytest.raises(SmirkHipError, match="CPU"):
        visualize.create_visualizations(dict(img=torch.zeros(2, 3, 16, 16)), {}, None, None)
    with pytest.raises(ValueError):
        LAW.sheet({k: t.numpy() if torch.is_tensor(t) else [x.numpy() for x in t] for k, t in _vis(B=1).items()})


# ---- the law's self-checks ------------------------------------------------------------------------------------------------------------------------------------------
def _grid_by_pad_and_cat(t, nrow):
    """make_grid restated independently: every image padded on its top and left, the cells of a row joined along the width, the rows along the height, and the
    right and bottom border added last"""
    F = torch.nn.functional
    t = torch.as_tensor(t)
    if t.shape[1] == 1:
        t = t.expand(-1, 3, -1, -1)
    N = t.shape[0]
    if N == 1:
        return t[0]
    xmaps = min(nrow, N)
    cells = [F.pad(img, (2, 0, 2, 0)) for img in t]
    cells += [torch.zeros_like(cells[0])] * (-N % xmaps)
    rows = [torch.cat(cells[i:i + xmaps], dim=2) for i in range(0, len(cells), xmaps)]
    return F.pad(torch.cat(rows, dim=1), (0, 2, 0, 2))


@pytest.mark.parametrize("N,C,H,W,nrow", [(1, 3, 5, 7, 1), (1, 1, 4, 4, 8), (2, 3, 5, 7, 1), (5, 1, 4, 6, 2), (8, 3, 3, 3, 4), (7, 3, 3, 5, 4), (3, 3, 6, 2, 8), (6, 1, 2, 2, 3)])
def test_grid_geometry_equals_pad_and_cat(N, C, H, W, nrow):
    x = np.random.default_rng(N * 100 + nrow).random((N, C, H, W), dtype=np.float32) + np.float32(0.25)       # no zeros: padding is told apart from content
    g = LAW.make_grid(x, nrow)
    assert g.dtype == np.float32 and np.array_equal(g, _grid_by_pad_and_cat(x, nrow).numpy())
    if N > 1:
        xmaps = min(nrow, N)
        assert g.shape == (3, -(-N // xmaps) * (H + 2) + 2, xmaps * (W + 2) + 2)
        for k in range(N):
            y0, x0 = (k // xmaps) * (H + 2) + 2, (k % xmaps) * (W + 2) + 2
            assert np.array_equal(g[:, y0:y0 + H, x0:x0 + W], np.broadcast_to(x[k], (3, H, W)))
    else:
        assert g.shape == (3, H, W)


def test_round_trip_table():
    """trunc(float32(k / 255) * 255), the law's 256 values, against exact rational arithmetic rounded to float32 after the division and after the product."""
    from fractions import Fraction
    table = LAW.round_trip_table()
    assert table.dtype == np.uint8 and table.shape == (256,)

    def f32(q):                                                                      # round-to-nearest-even of an exact rational to float32
        if q == 0:
            return Fraction(0)
        e = 0
        while q >= 2 ** (e + 1):
            e += 1
        while q < 2 ** e:
            e -= 1
        ulp = Fraction(2) ** (e - 23)
        n = q / ulp
        lo = n.numerator // n.denominator
        r = n - lo
        if r > Fraction(1, 2) or (r == Fraction(1, 2) and lo % 2 == 1):
            lo += 1
        return lo * ulp
    exact = [int(f32(f32(Fraction(k, 255)) * 255)) for k in range(256)]
    assert table.tolist() == exact
    # with a correctly rounded float32 division and product every level survives (in float64 arithmetic truncated the same way, or with a quotient rounded down,
    # levels drop by one: 1/255 is not representable); law and kernel compute the two operations as written all the same and never assume the identity
    assert exact == list(range(256))
    down = [int(np.nextafter(np.float32(k) / np.float32(255), np.float32(0)) * np.float32(255)) for k in range(256)]
    assert down != exact
    k = np.arange(256, dtype=np.float32)
    # and through the whole landmark panel: to_uint8 -> / 255 -> quantise goes through the table
    x = (k / np.float32(255)).reshape(1, 1, 16, 16)
    panel = LAW.landmark_panel(x, {key: np.zeros((1, 0, 2), np.float32) for key, _, _ in LAW.LAYERS})
    assert np.array_equal(LAW.quantise(panel[0], bgr=False)[..., 0].ravel(), table[LAW.to_uint8_saturating(x).ravel()])


def test_law_pieces():
    r = np.random.default_rng(5)
    # the interleave of smirk_trainer.py:327-330, restated with torch exactly as written there
    Ke, B = 3, 2
    four = [r.random((Ke * B, 3, 4, 4), dtype=np.float32) for _ in range(4)]
    want = torch.stack([torch.from_numpy(p).view(Ke, B, 3, 4, 4).permute(1, 0, 2, 3, 4).reshape(-1, 3, 4, 4) for p in four], dim=1).reshape(-1, 3, 4, 4)
    got = LAW.interleave_second_path(four, Ke)
    assert np.array_equal(got, want.numpy())
    for b in range(B):
        for ke in range(Ke):
            for which in range(4):
                assert np.array_equal(got[(b * Ke + ke) * 4 + which], four[which][ke * B + b])
    # nearest resampling against torch's own
    for n_in, n_out in ((8, 16), (112, 224), (5, 16), (16, 16), (7, 3), (224, 112)):
        x = r.random((2, 3, n_in, n_in), dtype=np.float32)
        assert np.array_equal(LAW.interpolate_nearest(x, n_out), torch.nn.functional.interpolate(torch.from_numpy(x), n_out).numpy()), (n_in, n_out)
    # the blends against torch's scalar arithmetic
    a, b = r.random((2, 3, 8, 8), dtype=np.float32), r.random((2, 3, 8, 8), dtype=np.float32)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    assert np.array_equal(LAW.blend(a, b), (ta * 0.7 + tb * 0.3).numpy()) and np.array_equal(LAW.blend(a, b), (ta * 0.7 + 0.3 * tb).numpy())
    # truncation toward zero, clipping of the disc, later layers on top
    img = np.zeros((1, 5, 5, 3), np.uint8)
    LAW.draw_keypoints(img, np.array([[[-0.4 / 2 - 1, -0.4 / 2 - 1]]], np.float32), (9, 9, 9), centre=2.0)        # lands at (-0.4, -0.4): pixel (0, 0), not (-1, -1)
    assert sorted(zip(*np.nonzero(img[0, :, :, 0]))) == [(0, 0), (0, 1), (1, 0)]
    LAW.draw_keypoints(img, np.array([[[1.0, 0.0], [np.nan, 0.0], [0.0, np.inf], [40.0, 0.0]]], np.float32), (7, 7, 7), centre=2.0)     # (4, 2) on the right border
    assert sorted(zip(*np.nonzero(img[0, :, :, 0] == 7))) == [(1, 4), (2, 3), (2, 4), (3, 4)]
    assert LAW.to_uint8_saturating(np.array([-0.5, 0.0, 0.999, 1.0, 1.7, np.nan], np.float32)).tolist() == [0, 0, 254, 255, 255, 0]
    assert LAW.quantise(np.array([-0.5, 0.5, 1.7, np.nan], np.float32).reshape(1, 2, 2).repeat(3, 0), bgr=False)[..., 0].ravel().tolist() == [0, 127, 255, 0]
