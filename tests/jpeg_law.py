"""The law of smirk_amd.jpeg (csrc/jpeg.hip, include/smirk_jpeg.h): one picture uint8 [H][W][3] -> one complete baseline JFIF file (sequential DCT,
8 bit, YCbCr 4:2:0, 16 x 16 MCUs, the Annex K "typical" Huffman tables, restart intervals), in numpy and Python integers: no floating point after the constants.
The kernels reproduce every step below bit for bit, so parity on the GPU is byte equality.

  pad        H and W up to multiples of 16 by edge replication
  colour     BT.601 in 16-bit fixed point: (a R + b G + c B + 32768) >> 16 (arithmetic shift); Cb, Cr get + 128 and a clip to 0 .. 255
  chroma     (a + b + c + d + 2) >> 2 over each 2 x 2 of the clipped Cb / Cr; every sample - 128
  DCT        T[u][x] = +-K[.] (K = the eight cos(k pi / 16) * 2^13, row 0 uses K[4]); a true 1-D DCT is T x / 2^14.  Pass 1 along x: P[y][u] = (sum_x T[u][x] X[y][x]
             + 256) >> 9; pass 2 along y: C[v][u] = sum_y T[v][y] P[y][u].  C is the DCT at scale 2^19 and every intermediate fits int32
             (|pass 1 sum| <= 128 * 46344, |P| <= 11586, |C| <= 11586 * 46344 < 2^29.01)
  quantise   round half away from zero of C / (Q 2^19): sign(C) * (((|C| >> 18) + Q) // (2 Q)), which is floor((|C| + Q 2^18) / (Q 2^19)); AC clipped to +-1023
  entropy    DC difference (category code + magnitude bits), AC run/size with ZRL and EOB, MSB first, 0x00 after every 0xFF; every restart interval of R MCUs coded on
             its own (predictors 0), padded with 1-bits, followed by RSTm (m cyclic 0 .. 7) except after the last
  file       SOI, APP0 JFIF 1.01, DQT x 2, SOF0, DHT x 4, DRI, SOS, scan, EOI
"""
import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
          15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)          # zigzag position -> natural (row-major) index

# ITU-T T.81 Annex K.1, natural order
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# Annex K.3: (BITS, HUFFVAL) of the DC luminance, AC luminance, DC chrominance and AC chrominance tables
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
           (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22,
            23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103,
            104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164,
            165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
            217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
             (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36,
              52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101,
              102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
              162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213,
              214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250))

DCT_K = (8192, 8035, 7568, 6811, 5793, 4551, 3135, 1598)            # round(2^13 cos(k pi / 16)), k = 0 .. 7
PASS1_SHIFT = 9
DEFAULT_QUALITY = 95
MAX_INTERVAL_MCU_BITS = 6 * (22 + 63 * 26)                          # include/smirk_jpeg.h: the longest codes of the tables


def dct_matrix():
    """int64 [8][8]: T[u][x] = 2^14 * (C(u) / 2) cos((2 x + 1) u pi / 16) rounded through DCT_K"""
    T = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            a = (2 * x + 1) * u % 32
            a = 32 - a if a > 16 else a
            T[u, x] = DCT_K[4] if u == 0 else (DCT_K[a] if a < 8 else -DCT_K[16 - a])
    return T


def quant_tables(quality=DEFAULT_QUALITY):
    """-> int64 [2][64], natural order: the Annex K base tables under the IJG quality rule"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality outside 1 .. 100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([[min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (BASE_LUMA, BASE_CHROMA)], np.int64)


def huffman_codes(table):
    """(BITS, HUFFVAL) -> {symbol: (code, length)}, Annex C"""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def mcu_grid(H, W):
    return (H + 15) // 16, (W + 15) // 16


def coefficients(img, qt, bgr=False):
    """uint8 [H][W][3] -> int64 [mcus][6][64], quantised, in zigzag order; blocks Y00 Y01 Y10 Y11 Cb Cr; MCUs row-major"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("picture must be uint8 [H][W][3]")
    H, W = img.shape[:2]
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("H, W outside 1 .. 65535")
    my, mx = mcu_grid(H, W)
    p = np.pad(img, ((0, my * 16 - H), (0, mx * 16 - W), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = (p[..., 2], p[..., 1], p[..., 0]) if bgr else (p[..., 0], p[..., 1], p[..., 2])
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = np.clip(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128, 0, 255)
    cr = np.clip(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128, 0, 255)
    mean = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    y, cb, cr = y - 128, mean(cb) - 128, mean(cr) - 128
    T = dct_matrix()
    qt = np.asarray(qt, np.int64).reshape(2, 8, 8)
    zz = np.array(ZIGZAG)
    out = np.zeros((my * mx, 6, 64), np.int64)
    for m in range(my * mx):
        j, i = divmod(m, mx)
        blocks = [y[16 * j + 8 * (k >> 1):16 * j + 8 * (k >> 1) + 8, 16 * i + 8 * (k & 1):16 * i + 8 * (k & 1) + 8] for k in range(4)]
        blocks += [cb[8 * j:8 * j + 8, 8 * i:8 * i + 8], cr[8 * j:8 * j + 8, 8 * i:8 * i + 8]]
        for k, X in enumerate(blocks):
            P = (X @ T.T + (1 << (PASS1_SHIFT - 1))) >> PASS1_SHIFT           # P[y][u]
            Cf = T @ P                                                       # C[v][u]
            assert np.abs(X @ T.T).max() < 2 ** 31 and np.abs(Cf).max() < 2 ** 31
            Q = qt[0 if k < 4 else 1]
            n = np.sign(Cf) * (((np.abs(Cf) >> 18) + Q) // (2 * Q))
            n = n.reshape(64)
            n[1:] = np.clip(n[1:], -1023, 1023)
            out[m, k] = n[zz]
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _category(v):
    return int(abs(int(v))).bit_length()


def encode_interval(coefs):
    """int [n][6][64] (the MCUs of one restart interval) -> its bytes, padded to a byte boundary, without the marker"""
    dc = (huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA))
    ac = (huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA))
    w, pred = _Bits(), [0, 0, 0]
    for mcu in coefs:
        for k in range(6):
            comp = 0 if k < 4 else k - 3
            t = 0 if k < 4 else 1
            blk = [int(v) for v in mcu[k]]
            d = blk[0] - pred[comp]
            pred[comp] = blk[0]
            s = _category(d)
            code, length = dc[t][s]
            w.put((code << s) | ((d if d >= 0 else d - 1) & ((1 << s) - 1)), length + s)
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    w.put(*ac[t][0xF0])
                    run -= 16
                s = _category(v)
                code, length = ac[t][(run << 4) | s]
                w.put((code << s) | ((v if v >= 0 else v - 1) & ((1 << s) - 1)), length + s)
                run = 0
            if run:
                w.put(*ac[t][0x00])
    w.flush()
    return bytes(w.out)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(H, W, qt, R):
    qt = np.asarray(qt, np.int64).reshape(2, 64)
    h = bytes([0xFF, 0xD8]) + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2):
        h += _segment(0xDB, bytes([t]) + bytes(int(qt[t][z]) for z in ZIGZAG))
    h += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        h += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    h += _segment(0xDD, R.to_bytes(2, "big"))
    h += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return h


HEADER_BYTES = 629


def effective_interval(H, W, R):
    """the interval the file is coded with and DRI states: R capped at the MCU count (one interval either way) and at DRI's 16 bits"""
    my, mx = mcu_grid(H, W)
    if R < 1:
        raise ValueError("restart interval below 1")
    return min(int(R), my * mx, 65535)


def encode(img, quality=DEFAULT_QUALITY, bgr=False, restart_interval=1, qt=None):
    """-> the file's bytes"""
    img = np.asarray(img)
    qt = quant_tables(quality) if qt is None else np.asarray(qt, np.int64).reshape(2, 64)
    c = coefficients(img, qt, bgr)
    H, W = img.shape[:2]
    R = effective_interval(H, W, restart_interval)
    out = bytearray(header(H, W, qt, R))
    n = -(-len(c) // R)
    for i in range(n):
        out += encode_interval(c[i * R:(i + 1) * R])
        out += bytes([0xFF, 0xD0 + (i & 7)]) if i + 1 < n else bytes([0xFF, 0xD9])
    return bytes(out)


def encode_batch(images, quality=DEFAULT_QUALITY, bgr=False, restart_interval=1):
    """[B][H][W][3] -> (the files back to back, [(offset, length)])"""
    files = [encode(im, quality, bgr, restart_interval) for im in images]
    spans, at = [], 0
    for f in files:
        spans.append((at, len(f)))
        at += len(f)
    return b"".join(files), spans


# ---- the entropy decoder of the law's own streams ---------------------------------------------------------------------------------------------------------------------
def parse(data):
    """a file of this law -> (H, W, qt [2][64] natural order, R, scan bytes without EOI)"""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    i, H, W, R, qt = 2, None, None, 0, np.zeros((2, 64), np.int64)
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        seg = data[i + 4:i + 2 + n]
        if m == 0xDB:
            for k, z in enumerate(ZIGZAG):
                qt[seg[0]][z] = seg[1 + k]
        elif m == 0xC0:
            H, W = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
        elif m == 0xDD:
            R = int.from_bytes(seg, "big")
        i += 2 + n
        if m == 0xDA:
            return H, W, qt, R, data[i:-2]


def decode_coefficients(data):
    """a file of this law -> int64 [mcus][6][64], zigzag order: what `coefficients` returned"""
    H, W, _, R, scan = parse(data)
    my, mx = mcu_grid(H, W)
    total = my * mx
    inv = [{(c, n): s for s, (c, n) in huffman_codes(t).items()} for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)]
    # split at the RST markers (a stuffed FF 00 is data), then undo the stuffing
    parts, cur, i = [], bytearray(), 0
    while i < len(scan):
        if scan[i] == 0xFF:
            nxt = scan[i + 1]
            if nxt == 0:
                cur.append(0xFF)
            else:
                assert nxt == 0xD0 + (len(parts) & 7), "restart markers out of order"
                parts.append(bytes(cur))
                cur = bytearray()
            i += 2
        else:
            cur.append(scan[i])
            i += 1
    parts.append(bytes(cur))
    assert len(parts) == -(-total // R)
    out = np.zeros((total, 6, 64), np.int64)
    for p, part in enumerate(parts):
        bits = "".join(format(b, "08b") for b in part)
        at, pred = 0, [0, 0, 0]

        def symbol(table):
            nonlocal at
            code, n = 0, 0
            while True:
                code, n = (code << 1) | int(bits[at]), n + 1
                at += 1
                if (code, n) in table:
                    return table[(code, n)]
                assert n < 16

        def magnitude(s):
            nonlocal at
            if s == 0:
                return 0
            v = int(bits[at:at + s], 2)
            at += s
            return v if v >> (s - 1) else v - (1 << s) + 1
        for m in range(p * R, min((p + 1) * R, total)):
            for k in range(6):
                comp, t = (0, 0) if k < 4 else (k - 3, 1)
                pred[comp] += magnitude(symbol(inv[2 * t]))
                out[m, k, 0] = pred[comp]
                z = 1
                while z < 64:
                    rs = symbol(inv[2 * t + 1])
                    if rs == 0:
                        break
                    z += rs >> 4
                    if rs & 15:
                        out[m, k, z] = magnitude(rs & 15)
                    z += 1
        assert len(bits) - at < 8 and set(bits[at:]) <= {"1"}, "interval not padded with 1-bits"
    return out


def has_zrl(coefs):
    """does any block of int [..][64] code a ZRL: a run of 16 or more zeros before a non-zero AC coefficient"""
    for blk in np.asarray(coefs).reshape(-1, 64):
        nz = np.nonzero(blk[1:])[0] + 1
        prev = 0
        for z in nz:
            if z - prev - 1 >= 16:
                return True
            prev = z
    return False
