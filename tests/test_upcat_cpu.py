"""conv_upcat.hip on the CPU: (1) the composition identity — a 3x3 convolution over cat(ConvTranspose2d(d), e) equals a 3x3 convolution over e plus a
2x2-tap convolution over the coarse tensor d with one weight set per output sub-position, plus a bias that depends on the sub-position and the image border —
in float64 against torch.nn.functional; (2) the kernel's two LDS halo layouts restated lane by lane: the DMA's slot / piece map and the A-fragment reads
must agree on which pixel and which 16-byte piece a lane gets, and every read must be conflict-free in the gfx950 bank model (tools/lds_bank_model.py).
A layout change in the kernel has to be mirrored here, which is the point."""
import pytest
import torch
import torch.nn.functional as F

from tools.lds_bank_model import read_b128_cycles


# ---- (1) the arithmetic ---------------------------------------------------------------------------------------------------------------------------------
def compose(Wup, bup, W3, c):
    """Weff[dy][dx][co][ai][bi][ci] (coarse tap a = dy - 1 + ai, b = dx - 1 + bi) and Beff[dy][dx][row edge][col edge][co], as upcat_compose_kernel builds them."""
    Weff = torch.zeros(2, 2, c, 2, 2, 2 * c, dtype=W3.dtype)
    Beff = torch.zeros(2, 2, 2, 2, c, dtype=W3.dtype)
    for dy in range(2):
        for dx in range(2):
            for ty in (-1, 0, 1):
                for tx in (-1, 0, 1):
                    a, b = (dy + ty) // 2, (dx + tx) // 2
                    py, px = (dy + ty) % 2, (dx + tx) % 2
                    w3 = W3[:, :c, ty + 1, tx + 1]                                     # [co][cu]
                    Weff[dy, dx, :, a - (dy - 1), b - (dx - 1), :] += w3 @ Wup[:, :, py, px].T    # Wup [ci][cu] -> [cu][ci]
                    for re in range(2):
                        for ce in range(2):
                            if (re and ty == (1 if dy else -1)) or (ce and tx == (1 if dx else -1)):
                                continue                                              # this tap's fine pixel lies in the zero padding
                            Beff[dy, dx, re, ce] += w3 @ bup
    return Weff, Beff


def composed_forward(d, e, Wup, bup, W3, c):
    B, _, h, w = d.shape
    H, W = 2 * h, 2 * w
    Weff, Beff = compose(Wup, bup, W3, c)
    out = F.conv2d(e, W3[:, c:], padding=1)
    dp = F.pad(d, (1, 1, 1, 1))
    for dy in range(2):
        for dx in range(2):
            acc = torch.zeros(B, c, h, w, dtype=d.dtype)
            for ai in range(2):
                for bi in range(2):
                    a, b = dy - 1 + ai, dx - 1 + bi
                    win = dp[:, :, 1 + a:1 + a + h, 1 + b:1 + b + w]
                    acc += torch.einsum("oc,bcyx->boyx", Weff[dy, dx, :, ai, bi], win)
            Y = torch.arange(h) * 2 + dy
            X = torch.arange(w) * 2 + dx
            re = (Y == (H - 1 if dy else 0)).long()
            ce = (X == (W - 1 if dx else 0)).long()
            bias = Beff[dy, dx][re][:, ce]                                            # [h][w][co]
            out[:, :, dy::2, dx::2] += acc + bias.permute(2, 0, 1)
    return out


@pytest.mark.parametrize("c,h,w,B", [(4, 3, 5, 2), (8, 1, 1, 1), (8, 2, 1, 1), (32, 8, 8, 1)])
def test_composition_identity_float64(c, h, w, B):
    g = torch.Generator().manual_seed(7 + c + h)
    d = torch.randn(B, 2 * c, h, w, generator=g, dtype=torch.float64)
    e = torch.randn(B, c, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    Wup = torch.randn(2 * c, c, 2, 2, generator=g, dtype=torch.float64)
    bup = torch.randn(c, generator=g, dtype=torch.float64)
    W3 = torch.randn(c, 2 * c, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(torch.cat([F.conv_transpose2d(d, Wup, bup, stride=2), e], 1), W3, padding=1)
    got = composed_forward(d, e, Wup, bup, W3, c)
    # float64 sums of 18 c products of N(0,1) values (|ref| up to ~1e2): 1e-13 observed, 1e-11 is 2^-53 * terms * magnitude with two orders of slack
    assert (got - ref).abs().max() < 1e-11 * max(1.0, ref.abs().max().item())


# ---- (2) the LDS layouts ------------------------------------------------------------------------------------------------------------------------------------
PLANE, CP, CSLOTS = 81, 11, 112


def swz(row, col):
    return ((row & 3) << 1) | ((col >> 1) & 1)


def fine_dma():
    """slot -> (halo pixel (hy, hx) of the 18 x 18 fine halo or None, {position: logical piece}) as dmaE issues it."""
    m = {}
    for s in range(328):
        pl, rem = divmod(s, PLANE)
        py, px = divmod(rem, 9)
        pix = (2 * py + (pl >> 1), 2 * px + (pl & 1)) if pl < 4 else None
        m[s] = (pix, {pos: pos ^ swz(py, px) for pos in range(8)})
    return m


def coarse_dma():
    m = {}
    for t in range(CSLOTS):
        hy, hx = divmod(t, CP)
        pix = (hy, hx) if hy < 10 and hx < 10 else None
        m[t] = (pix, {pos: pos ^ swz(hy, hx) for pos in range(8)})
    return m


def a_base(lane, sbase, r0, c0, pitch):
    """byte address (relative to the halo area) of the kernel's a_base, then ^ (s << 6), | 16 for lo, + i * 4 * pitch * 128 for tile i"""
    r, cx = (lane >> 3) & 3, lane & 7
    return (sbase + (r0 + r) * pitch + c0 + cx) * 128 + ((swz(r0 + r, c0 + cx) << 4) ^ ((lane >> 5) << 5))


def reads(sbase, r0, c0, pitch):
    for i in range(2):
        for s in range(2):
            for lo in range(2):
                yield i, s, lo, (lambda lane, i=i, s=s, lo=lo: (a_base(lane, sbase, r0, c0, pitch) ^ (s << 6) ^ (lo << 4)) + i * 4 * pitch * 128)


def test_fine_halo_planes_cover_the_halo_once():
    pix = [p for p, _ in fine_dma().values() if p is not None]
    assert sorted(pix) == [(y, x) for y in range(18) for x in range(18)]


@pytest.mark.parametrize("cls", range(4))
def test_skip_half_reads_get_the_right_piece_and_are_conflict_free(cls):
    dy, dx = cls >> 1, cls & 1
    dma = fine_dma()
    for ky in range(3):
        for kx in range(3):
            sy, sx = dy + ky, dx + kx
            for i, s, lo, addr in reads(((sy & 1) * 2 + (sx & 1)) * PLANE, sy >> 1, sx >> 1, 9):
                for lane in range(64):
                    fr, hb = lane & 31, lane >> 5
                    cy, cx = 4 * i + (fr >> 3), fr & 7
                    a = addr(lane)
                    pix, pieces = dma[a // 128]
                    assert pix == (2 * cy + dy + ky, 2 * cx + dx + kx)                 # the input pixel under tap (ky, kx) of output pixel (2 cy + dy, 2 cx + dx)
                    assert pieces[(a % 128) // 16] == 2 * (2 * s + hb) + lo            # channels 16 s + 8 hb .., hi / lo halves
                assert read_b128_cycles(lambda lane: addr(lane) // 4) == 4, (cls, ky, kx, i, s, lo)


@pytest.mark.parametrize("cls", range(4))
def test_composed_reads_get_the_right_piece_and_are_conflict_free(cls):
    dy, dx = cls >> 1, cls & 1
    dma = coarse_dma()
    for kc in range(2):
        for ai in range(2):
            for bi in range(2):
                for i, s, lo, addr in reads(kc * CSLOTS, dy + ai, dx + bi, CP):
                    for lane in range(64):
                        fr, hb = lane & 31, lane >> 5
                        cy, cx = 4 * i + (fr >> 3), fr & 7
                        a = addr(lane)
                        assert kc * CSLOTS <= a // 128 < (kc + 1) * CSLOTS
                        pix, pieces = dma[a // 128 - kc * CSLOTS]
                        assert pix == (cy + dy + ai, cx + dx + bi)                     # coarse pixel (y + a, x + b), a = dy - 1 + ai, in a halo that starts at (y0 - 1, x0 - 1)
                        assert pieces[(a % 128) // 16] == 2 * (2 * s + hb) + lo
                    assert read_b128_cycles(lambda lane: addr(lane) // 4) == 4, (cls, kc, ai, bi, i, s, lo)


def test_a_swizzle_of_the_column_alone_would_conflict():
    """why the ring kernel's (x >> 1) & 7 was not kept: with an odd row pitch, (row i, column 2m) and (row i + 1, column 2m + 1) share their banks"""
    def addr(lane):
        r, cx = (lane >> 3) & 3, lane & 7
        return ((r * 9 + cx) * 128 + ((((cx >> 1) & 7) << 4) ^ ((lane >> 5) << 5))) // 4
    assert read_b128_cycles(addr) > 4
