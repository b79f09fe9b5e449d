"""smirk_amd.jpeg without a GPU: the law of tests/jpeg_law.py against itself (entropy round trip) and against PIL (tables, quality rule, decodability, the quality
cap), the extension table of include/smirk_jpeg.h against its header with every refusal (raw ctypes, dummy pointers that are never dereferenced: a refusal comes
before anything touches the device), the Python refusals that need no device, and video.MjpegWriter."""
import ctypes as C
import io
import os
import re
import struct

import numpy as np
import pytest
import torch

import jpeg_law as LAW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, R_, S_ = (0x10000 * k for k in range(1, 5))                   # never dereferenced; all 256-byte aligned
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def _smooth(noise=0.0, H=77, W=93, seed=2):
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([128 + 100 * np.sin(xx / 17 + yy / 29), 128 + 90 * np.cos(xx / 23 - yy / 13), 128 + 80 * np.sin(xx / 9) * np.cos(yy / 11)], -1)
    if noise:
        img = img + np.random.default_rng(seed).normal(0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _pil():
    Image = pytest.importorskip("PIL.Image")
    try:
        Image.new("RGB", (8, 8)).save(io.BytesIO(), "JPEG")
    except Exception:                                                # noqa: BLE001
        pytest.skip("PIL without its JPEG codec")
    return Image


def _segments(data):
    """[(marker, payload)] of a JPEG file up to and including SOS"""
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return out


# ---- the law against itself -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,R,quality", [(1, 1, 1, 95), (8, 8, 2, 50), (17, 23, 3, 95), (48, 32, 1, 100), (48, 32, 100, 1), (16, 160, 1, 75)])
def test_stream_decodes_back_to_its_coefficients(H, W, R, quality):
    img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    data = LAW.encode(img, quality, restart_interval=R)
    c = LAW.coefficients(img, LAW.quant_tables(quality))
    assert np.array_equal(LAW.decode_coefficients(data), c)
    h, w, qt, r, scan = LAW.parse(data)
    assert (h, w, r) == (H, W, LAW.effective_interval(H, W, R)) and np.array_equal(qt, LAW.quant_tables(quality))
    assert data[:LAW.HEADER_BYTES] == LAW.header(H, W, LAW.quant_tables(quality), r) and len(LAW.header(H, W, qt, r)) == LAW.HEADER_BYTES
    n = -(-len(c) // r)
    assert sum(scan.count(bytes([0xFF, 0xD0 + m])) >= 1 for m in range(8)) == min(n - 1, 8)          # RSTm cyclic
    assert np.abs(c[:, :, 1:]).max() <= 1023 and np.abs(c[:, :, 0]).max() <= 1024
    assert len(data) - LAW.HEADER_BYTES <= n * (2 * r * 1245 + 2)                                   # the bound of include/smirk_jpeg.h


def test_law_pieces():
    T = LAW.dct_matrix()
    exact = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)]) * 8192
    assert np.abs(T - exact).max() <= 0.5 and set(np.abs(T).ravel()) <= set(LAW.DCT_K) and np.abs(T).sum(1).max() == 46344
    assert sorted(LAW.ZIGZAG) == list(range(64)) and LAW.MAX_INTERVAL_MCU_BITS == 1245 * 8
    for table, longest in ((LAW.DC_LUMA, 9), (LAW.DC_CHROMA, 11), (LAW.AC_LUMA, 16), (LAW.AC_CHROMA, 16)):
        codes = LAW.huffman_codes(table)
        assert len(codes) == sum(table[0]) == len(table[1]) and max(n for _, n in codes.values()) == longest
    assert LAW.huffman_codes(LAW.AC_LUMA)[0xF0][1] == 11 and LAW.huffman_codes(LAW.AC_LUMA)[0][1] == 4 and LAW.huffman_codes(LAW.AC_CHROMA)[0][1] == 2
    # the colour law on the corners of the cube: Y of a grey is the grey, its chroma 128
    g = np.arange(256, dtype=np.uint8)[None, :, None].repeat(3, 2)
    c = LAW.coefficients(np.full((16, 16, 3), 77, np.uint8), LAW.quant_tables(100))
    assert c[0, 0, 0] == round((77 - 128) * 8) and not c[0, 4:].any() and not c[0, :, 1:].any() and g.shape == (1, 256, 3)
    assert not LAW.has_zrl(np.zeros((1, 64), int)) and LAW.has_zrl(np.eye(64, dtype=int)[63:]) and not LAW.has_zrl(np.eye(64, dtype=int)[16:17])
    assert LAW.has_zrl(np.eye(64, dtype=int)[17:18])
    with pytest.raises(ValueError):
        LAW.encode(np.zeros((4, 4, 3), np.uint8), restart_interval=0)
    with pytest.raises(ValueError):
        LAW.quant_tables(0)


# ---- the law against PIL ------------------------------------------------------------------------------------------------------------------------------------------
def test_tables_and_quality_rule_equal_pil():
    Image = _pil()
    for q in (1, 25, 50, 75, 95, 100):
        b = io.BytesIO()
        Image.fromarray(_smooth(H=32, W=32)).save(b, "JPEG", quality=q, subsampling=2, optimize=False)
        seg = _segments(b.getvalue())
        dqt = b"".join(p for m, p in seg if m == 0xDB)
        assert len(dqt) == 130 and dqt[0] == 0 and dqt[65] == 1
        want = LAW.quant_tables(q)
        assert list(dqt[1:65]) == [want[0][z] for z in LAW.ZIGZAG] and list(dqt[66:130]) == [want[1][z] for z in LAW.ZIGZAG], q
        dht = b"".join(p for m, p in seg if m == 0xC4)
        found, i = {}, 0
        while i < len(dht):
            n = sum(dht[i + 1:i + 17])
            found[dht[i]] = (tuple(dht[i + 1:i + 17]), tuple(dht[i + 17:i + 17 + n]))
            i += 17 + n
        assert found == {0x00: LAW.DC_LUMA, 0x10: LAW.AC_LUMA, 0x01: LAW.DC_CHROMA, 0x11: LAW.AC_CHROMA}
    assert np.array_equal(LAW.quant_tables(50), [LAW.BASE_LUMA, LAW.BASE_CHROMA])


@pytest.mark.parametrize("H,W", [(1, 1), (8, 8), (17, 23), (48, 32), (93, 77)])
def test_pil_loads_the_laws_files(H, W):
    Image = _pil()
    img = _smooth(3.0, H, W)
    mcus = -(-H // 16) * -(-W // 16)
    for R in (1, 3, mcus + 5, max(1, mcus // 9)):                    # the last: more than 8 intervals where the picture has that many MCUs
        data = LAW.encode(img, restart_interval=R)
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (W, H) and im.mode == "RGB"
        assert np.abs(np.asarray(im).astype(int) - img).mean() < 6.0                                # and it is the picture
    assert H * W < 93 * 77 or mcus // max(1, mcus // 9) > 8
    bgr = Image.open(io.BytesIO(LAW.encode(img[..., ::-1], bgr=True)))
    assert np.array_equal(np.asarray(bgr), np.asarray(Image.open(io.BytesIO(LAW.encode(img)))))


def _mae(Image, data, img):
    return float(np.abs(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(int) - img).mean())


@pytest.mark.parametrize("noise", [0.0, 6.0], ids=["smooth", "noisy"])
@pytest.mark.parametrize("q", [50, 75, 95])
def test_quality_cap(q, noise):
    """The error of the PIL-decoded law stream is at most that of PIL's own file at quality q - 10.  Measured (smooth / sigma 6), law vs PIL at q vs PIL at q - 10:
    q 50: 2.622 2.605 2.982 / 5.371 5.363 5.545;  q 75: 1.730 1.714 2.123 / 4.958 4.948 5.129;  q 95: 0.896 0.879 1.305 / 4.287 4.298 4.755."""
    Image = _pil()
    img = _smooth(noise, seed=1)

    def pil(quality):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling=2)
        return _mae(Image, b.getvalue(), img)
    law, own, cap = _mae(Image, LAW.encode(img, q, restart_interval=3), img), pil(q), pil(q - 10)
    print(f"q={q} noise={noise}: law {law:.4f}  PIL(q) {own:.4f}  ratio {law / own:.4f}  PIL(q-10) {cap:.4f}")
    assert own < cap                                                # PIL's own monotonicity on this input
    assert law <= cap


# ---- the extension table ------------------------------------------------------------------------------------------------------------------------------------------
def test_extension_table_equals_the_header():
    from smirk_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "smirk_jpeg.h")).read()
    declared = set(re.findall(r"\b(smirk_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.JPEG_EXPORTS), declared ^ set(L.JPEG_EXPORTS)
    assert L.JPEG_EXPORTS == tuple(L.JPEG_SIGS) and len(L.JPEG_EXPORTS) == 5
    others = (L.EXPORTS, L.MICA_EXPORTS, L.EMOTION_EXPORTS, L.OPTIM_EXPORTS, L.HANDOFF_EXPORTS, L.GENPLAN_EXPORTS, L.GENARITH_EXPORTS, L.DATA_EXPORTS,
              L.VISUAL_EXPORTS)
    for other in others:
        assert not set(L.JPEG_EXPORTS) & set(other)
    dll = C.CDLL(L.LIB_PATH)
    for name in declared:
        getattr(dll, name)
    version = int(re.search(r"#define\s+SMIRK_JPEG_ABI_VERSION\s+(\d+)", hdr).group(1))
    lib = L.lib()
    assert lib.smirk_jpeg_abi_version() == L.JPEG_ABI_VERSION == version == 1
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "smirk_jpeg.h" in readme and re.search(r"smirk_jpeg\.h[^\n]*\b5 entries", readme)
    build_py = open(os.path.join(REPO, "smirk_amd", "build.py")).read()
    assert '"smirk_jpeg.h"' in build_py and '"jpeg.hip"' not in build_py                           # the unit has the common flags alone
    # the other tables and their versions did not move, none of their headers names the new entries, and the new header names none of theirs
    assert lib.smirk_abi_version() == L.ABI_VERSION == 17 and len(L.EXPORTS) == 116
    assert (lib.smirk_mica_abi_version(), lib.smirk_emotion_abi_version(), lib.smirk_optim_abi_version(), lib.smirk_handoff_abi_version(),
            lib.smirk_genplan_abi_version(), lib.smirk_genarith_abi_version(), lib.smirk_data_abi_version(), lib.smirk_visual_abi_version()) == (1,) * 8
    for name in os.listdir(os.path.join(REPO, "include")):
        if name != "smirk_jpeg.h":
            text = open(os.path.join(REPO, "include", name)).read()
            assert not any(e in text for e in L.JPEG_EXPORTS), name
    for other in others:
        assert not any(re.search(rf"\b{e}\b(?!\.h)", hdr) for e in other)
    for macro, value in (("HEADER_BYTES", L.JPEG_HEADER_BYTES), ("MCU_MAX_BYTES", L.JPEG_MCU_MAX_BYTES), ("MAX_DIM", L.JPEG_MAX_DIM)):
        assert int(re.search(rf"#define\s+SMIRK_JPEG_{macro}\s+(\d+)", hdr).group(1)) == value
    assert (L.JPEG_HEADER_BYTES, L.JPEG_MCU_MAX_BYTES * 8) == (LAW.HEADER_BYTES, LAW.MAX_INTERVAL_MCU_BITS) and C.sizeof(L.JpegQuantTables) == 128
    # the kernel's constants are the law's: the literals stand in the unit
    unit = open(os.path.join(REPO, "smirk_amd", "csrc", "jpeg.hip")).read()
    assert "{" + ", ".join(str(k) for k in LAW.DCT_K) + "}" in unit and f"#define JPEG_PASS1_SHIFT {LAW.PASS1_SHIFT}" in unit
    assert "getenv" not in unit and "smirk_switch" not in unit and "smirk_split" not in unit and "smirk_range" not in unit


def test_exported_from_the_package():
    import smirk_amd
    from smirk_amd import jpeg, video
    assert smirk_amd.jpeg is jpeg and smirk_amd.encode_jpeg is jpeg.encode_jpeg and smirk_amd.JpegBatch is jpeg.JpegBatch
    assert {"jpeg", "encode_jpeg", "JpegBatch"} <= set(smirk_amd.__all__)
    assert jpeg.DEFAULT_QUALITY == LAW.DEFAULT_QUALITY == 95 and jpeg.DEFAULT_RESTART_INTERVAL >= 1 and callable(video.MjpegWriter)


def test_quant_tables_entry():
    from smirk_amd import _lib as L, jpeg
    lib = L.lib()
    for q in (1, 2, 25, 49, 50, 51, 75, 95, 99, 100):
        assert np.array_equal(jpeg.quant_tables(q), LAW.quant_tables(q)), q
    qt = L.JpegQuantTables()
    assert lib.smirk_jpeg_quant_tables(0, C.byref(qt)) == BAD_ARG and lib.smirk_jpeg_quant_tables(101, C.byref(qt)) == BAD_ARG
    assert lib.smirk_jpeg_quant_tables(-5, C.byref(qt)) == BAD_ARG and lib.smirk_jpeg_quant_tables(95, None) == BAD_ARG


def test_workspace_and_bound_queries():
    from smirk_amd import _lib as L
    lib = L.lib()
    up = lambda n: -(-n // 256) * 256
    assert lib.smirk_jpeg_workspace_bytes(1, 1, 1, 1) == up(768) + 2 * 256
    assert lib.smirk_jpeg_workspace_bytes(2, 17, 23, 1) == up(2 * 4 * 768) + 2 * up(2 * 4 * 4)
    assert lib.smirk_jpeg_workspace_bytes(3, 16, 1040, 2) == up(3 * 65 * 768) + 2 * up(3 * 33 * 4)
    assert lib.smirk_jpeg_max_bytes(1, 1, 1, 1) == 629 + 2 * 1245 + 2
    assert lib.smirk_jpeg_max_bytes(2, 17, 23, 3) == 2 * (629 + 2 * (2 * 3 * 1245 + 2))
    assert lib.smirk_jpeg_max_bytes(2, 17, 23, 1000) == 2 * (629 + 2 * 4 * 1245 + 2)                # R capped at the MCU count
    assert lib.smirk_jpeg_max_bytes(1, 4096, 4096, 1 << 20) == 629 + 2 * (2 * 65535 * 1245 + 2)     # and at DRI's 16 bits: 65536 MCUs, two intervals
    assert lib.smirk_jpeg_max_bytes(64, 720, 3840, 1) == 64 * (629 + 10800 * 2492)
    for bad in ((0, 16, 16, 1), (-1, 16, 16, 1), (1, 0, 16, 1), (1, 16, 0, 1), (1, 65536, 16, 1), (1, 16, 65536, 1), (1, 16, 16, 0), (1, 16, 16, -2)):
        assert lib.smirk_jpeg_workspace_bytes(*bad) == 0 and lib.smirk_jpeg_max_bytes(*bad) == 0, bad
    assert lib.smirk_jpeg_max_bytes(1, 65535, 65535, 1) > 1 << 31 and lib.smirk_jpeg_workspace_bytes(1, 65535, 65535, 1) == 0
    assert lib.smirk_jpeg_workspace_bytes(1, 65535, 16, 1) > 0


def test_encode_refuses_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    good = L.JpegQuantTables()
    assert lib.smirk_jpeg_quant_tables(95, C.byref(good)) == 0

    def enc(img=P, B=2, H=17, W=23, bgr=0, qt=good, R=1, ws=Q, ws_bytes=None, out=R_, out_bytes=None, spans=S_):
        need, bound = lib.smirk_jpeg_workspace_bytes(B, H, W, R), lib.smirk_jpeg_max_bytes(B, H, W, R)
        return lib.smirk_jpeg_encode_u8(img, B, H, W, bgr, None if qt is None else C.byref(qt), R, ws, need if ws_bytes is None else ws_bytes, out,
                                        bound if out_bytes is None else out_bytes, spans, None)
    for kw in (dict(img=None), dict(qt=None), dict(ws=None), dict(out=None), dict(spans=None)):
        assert enc(**kw) == BAD_ARG, kw
    for kw in (dict(img=P + 8), dict(img=P + 1), dict(out=R_ + 4), dict(ws=Q + 128), dict(ws=Q + 16), dict(spans=S_ + 4)):
        assert enc(**kw) == BAD_ARG, kw
    for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=65536), dict(W=65536), dict(H=-4), dict(R=0), dict(R=-1)):
        assert enc(ws_bytes=1 << 30, out_bytes=1 << 30, **kw) == BAD_ARG, kw
    for t, i in ((0, 0), (0, 63), (1, 17)):
        zero = L.JpegQuantTables()
        lib.smirk_jpeg_quant_tables(95, C.byref(zero))
        zero[t][i] = 0
        assert enc(qt=zero) == BAD_ARG
    huge = 1 << 40
    assert enc(B=1, H=65535, W=65535, ws_bytes=huge, out_bytes=huge) == UNSUPPORTED                 # 12.9 GB of pixels
    assert enc(B=48, H=4096, W=4096, ws_bytes=huge, out_bytes=huge) == UNSUPPORTED                  # 2.4 GB of pixels
    assert enc(B=100, H=720, W=3840, ws_bytes=huge, out_bytes=huge) == UNSUPPORTED                  # 0.83 GB of pixels, a bound of 2.7 GB
    need, bound = lib.smirk_jpeg_workspace_bytes(2, 17, 23, 1), lib.smirk_jpeg_max_bytes(2, 17, 23, 1)
    assert enc(ws_bytes=need - 1) == WORKSPACE and enc(ws_bytes=0) == WORKSPACE and enc(out_bytes=bound - 1) == WORKSPACE and enc(out_bytes=0) == WORKSPACE


def test_python_refusals_without_a_device():
    import smirk_amd
    from smirk_amd import SmirkHipError
    good = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    for bad in (good.float(), good[..., :2], good[0, 0], good.unsqueeze(0), good.numpy(), good[:0], torch.zeros(1, 0, 4, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            smirk_amd.encode_jpeg(bad)
    for kw in (dict(quality=0), dict(quality=101), dict(restart_interval=0)):
        with pytest.raises(ValueError):
            smirk_amd.encode_jpeg(good, **kw)
    with pytest.raises(ValueError, match="in parts"):
        smirk_amd.encode_jpeg(torch.zeros(1, 1, 1, 3, dtype=torch.uint8).expand(100, 720, 3840, 3))
    with pytest.raises(SmirkHipError, match="CPU"):
        smirk_amd.encode_jpeg(good)
    with pytest.raises(SmirkHipError, match="CPU"):
        smirk_amd.encode_jpeg(good[0], quality=50, bgr=True, restart_interval=4)


# ---- the AVI writer -----------------------------------------------------------------------------------------------------------------------------------------------
def _chunks(data, at, end):
    while at < end:
        fourcc, n = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        yield fourcc, at, data[at + 8:at + 8 + n]
        at += 8 + n + (n & 1)


def test_mjpeg_writer_reparses(tmp_path):
    from smirk_amd.video import MjpegWriter
    frames = [LAW.encode(_smooth(2.0, 24, 40, seed=k), 60 + k) for k in range(5)]
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)                  # both parities: the pad byte is exercised
    path = str(tmp_path / "clip.avi")
    with MjpegWriter(path, 25, 40, 24) as w:
        for f in frames:
            w.write(f)
    with pytest.raises(ValueError):
        w.write(frames[0])
    w.close()                                                        # a second close is harmless
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and data[8:12] == b"AVI "
    top = list(_chunks(data, 12, len(data)))
    assert [c[0] for c in top] == [b"LIST", b"LIST", b"idx1"] and top[0][2][:4] == b"hdrl" and top[1][2][:4] == b"movi"
    hdrl = list(_chunks(top[0][2], 4, len(top[0][2])))
    assert [c[0] for c in hdrl] == [b"avih", b"LIST"]
    avih = struct.unpack("<14I", hdrl[0][2])
    assert avih[0] == 40000 and avih[3] & 0x10 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (40, 24) and avih[7] == max(len(f) for f in frames)
    strl = list(_chunks(hdrl[1][2], 4, len(hdrl[1][2])))
    assert hdrl[1][2][:4] == b"strl" and [c[0] for c in strl] == [b"strh", b"strf"]
    strh = struct.unpack("<4s4sIHHIIIIIIIIhhhh", strl[0][2])
    assert strh[:2] == (b"vids", b"MJPG") and strh[6:8] == (1, 25) and strh[9] == 5
    strf = struct.unpack("<IiiHH4sIiiII", strl[1][2])
    assert strf[:6] == (40, 40, 24, 1, 24, b"MJPG")
    movi_at = top[1][1] + 8                                          # position of the 'movi' fourcc
    movi = list(_chunks(data, movi_at + 4, top[1][1] + 8 + len(top[1][2])))
    assert [c[0] for c in movi] == [b"00dc"] * 5 and [c[2] for c in movi] == frames
    idx = [struct.unpack("<4sIII", top[2][2][k:k + 16]) for k in range(0, len(top[2][2]), 16)]
    assert len(idx) == 5
    for (fourcc, flags, off, n), (_, at, payload) in zip(idx, movi):
        assert fourcc == b"00dc" and flags == 0x10 and movi_at + off == at and n == len(payload)
    with MjpegWriter(str(tmp_path / "ntsc.avi"), 29.97, 8, 8) as w2:
        pass
    head = open(str(tmp_path / "ntsc.avi"), "rb").read()
    assert struct.unpack("<I", head[4:8])[0] == len(head) - 8 and b"idx1" in head
    for bad in ((0, 8, 8), (25, 0, 8), (25, 8, -1)):
        with pytest.raises(ValueError):
            MjpegWriter(str(tmp_path / "bad.avi"), *bad)
