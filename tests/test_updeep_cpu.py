"""Decoder levels 3 / 4 with the ConvTranspose2d composed into the level's first convolution as TWO launches (conv_halo.hip), on the CPU in float64:

    partial'(2y+dy, 2x+dx, co) = s[co] * ( sum over a in {dy-1, dy}, b in {dx-1, dx}, ci < 2c of Weff[dy,dx][co][a,b][ci] * d[y+a][x+b][ci] + Beff[dy,dx][row edge][col edge][co] )
    out = ReLU( s * conv3x3_zero_pad(e ; W3[:, c:]) + t + partial' )

against conv2d(cat(conv_transpose2d(d), e)) + BatchNorm + ReLU, and the three tables updeep_compose_kernel writes, restated index by index:

    weff   [class = 2 dy + dx][co][tap * 2c + ci]      tap = 2 ta + tb reads the coarse pixel (y + dy - 1 + ta, x + dx - 1 + tb)
    shift16[class][row edge][column edge][co]          = s[co] * Beff
    wskip  [co][(3 ky + kx) * c + ci]                  = W3[co][c + ci][ky][kx]

The two launches are then evaluated FROM those rows the way the kernels walk them (launch 1: GEMM rows = coarse raster pixels of one class, out-of-image taps
read zeros, store at the fine pixel; launch 2: an ordinary 3x3 convolution whose residual is partial').  A layout change in the kernels has to be mirrored here."""
import pytest
import torch
import torch.nn.functional as F

SIZES = [(1, 1), (1, 3), (2, 2), (3, 5), (4, 4)]          # coarse h x w: every class meets every edge combination (1 x 1: all four edges at once)


def tables(Wup, bup, W3, s, c):
    """weff, shift16, wskip as updeep_compose_kernel lays them out"""
    weff = torch.zeros(4, c, 4 * 2 * c, dtype=W3.dtype)
    shift16 = torch.zeros(4, 2, 2, c, dtype=W3.dtype)
    for dy in range(2):
        for dx in range(2):
            cls = 2 * dy + dx
            for fy in (-1, 0, 1):
                for fx in (-1, 0, 1):
                    ca, cb = (dy + fy) // 2, (dx + fx) // 2                            # coarse offset of the fine tap
                    sub = ((dy + fy) % 2, (dx + fx) % 2)                              # which ConvTranspose tap produced that fine pixel
                    tap = 2 * (ca - (dy - 1)) + (cb - (dx - 1))
                    w3 = W3[:, :c, fy + 1, fx + 1]                                     # [co][cu]
                    weff[cls, :, tap * 2 * c:(tap + 1) * 2 * c] += w3 @ Wup[:, :, sub[0], sub[1]].T    # [co][cu] @ [cu][ci]
                    for re in range(2):
                        for ce in range(2):
                            if (re and fy == (1 if dy else -1)) or (ce and fx == (1 if dx else -1)):
                                continue                                              # the fine tap lies in the zero padding: no bias through it
                            shift16[cls, re, ce] += w3 @ bup
    shift16 *= s
    wskip = W3[:, c:].permute(0, 2, 3, 1).reshape(c, 9 * c)
    return weff, shift16, wskip


def launch1(d, weff, shift16, s, c):
    """partial' [B][2h][2w][c] (NHWC), one class per GEMM, rows = coarse raster pixels"""
    B, _, h, w = d.shape
    dn = d.permute(0, 2, 3, 1)                                                        # NHWC
    out = torch.zeros(B, 2 * h, 2 * w, c, dtype=d.dtype)
    for cls in range(4):
        dy, dx = cls >> 1, cls & 1
        for b in range(B):
            for y in range(h):
                for x in range(w):
                    arow = torch.zeros(4 * 2 * c, dtype=d.dtype)                      # the im2col row: 4 taps x 2c channels, zeros outside the image
                    for tap in range(4):
                        ay, ax = y + dy - 1 + (tap >> 1), x + dx - 1 + (tap & 1)
                        if 0 <= ay < h and 0 <= ax < w:
                            arow[tap * 2 * c:(tap + 1) * 2 * c] = dn[b, ay, ax]
                    re = int(y == (h - 1 if dy else 0))
                    ce = int(x == (w - 1 if dx else 0))
                    out[b, 2 * y + dy, 2 * x + dx] = s * (weff[cls] @ arow) + shift16[cls, re, ce]
    return out


def launch2(e, wskip, s, t, partial, c):
    """ReLU(s * conv3x3(e; wskip) + t + partial'), NCHW out"""
    w = wskip.reshape(c, 3, 3, c).permute(0, 3, 1, 2)
    z = F.conv2d(e, w, padding=1) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1) + partial.permute(0, 3, 1, 2)
    return torch.relu(z)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("c,B", [(4, 2), (8, 1)])
def test_two_launch_identity_float64(c, B, h, w):
    g = torch.Generator().manual_seed(100 * c + 10 * h + w)
    d = torch.randn(B, 2 * c, h, w, generator=g, dtype=torch.float64)
    e = torch.randn(B, c, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    Wup = torch.randn(2 * c, c, 2, 2, generator=g, dtype=torch.float64)
    bup = torch.randn(c, generator=g, dtype=torch.float64)                           # ConvTranspose bias N(0, 1)
    W3 = torch.randn(c, 2 * c, 3, 3, generator=g, dtype=torch.float64)
    s = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    t = torch.randn(c, generator=g, dtype=torch.float64)
    z = F.conv2d(torch.cat([F.conv_transpose2d(d, Wup, bup, stride=2), e], 1), W3, padding=1)
    ref = torch.relu(z * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1))
    weff, shift16, wskip = tables(Wup, bup, W3, s, c)
    got = launch2(e, wskip, s, t, launch1(d, weff, shift16, s, c), c)
    # float64 sums of 18 c products of N(0, 1) values scaled by <= 1.5 (|z| up to ~1e2): 2^-53 * terms * magnitude with two orders of slack
    assert (got - ref).abs().max() < 1e-11 * max(1.0, z.abs().max().item())
    assert (ref > 0).any() and (ref == 0).any()                                       # the ReLU is exercised on both sides


def test_table_rows_index_by_index():
    """every entry of the three tables from the definition, element by element (small c: 4 classes x c x 8c + 16 c + 9 c^2 entries)"""
    c = 3
    g = torch.Generator().manual_seed(5)
    Wup = torch.randn(2 * c, c, 2, 2, generator=g, dtype=torch.float64)
    bup = torch.randn(c, generator=g, dtype=torch.float64)
    W3 = torch.randn(c, 2 * c, 3, 3, generator=g, dtype=torch.float64)
    s = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    weff, shift16, wskip = tables(Wup, bup, W3, s, c)
    for cls in range(4):
        dy, dx = cls >> 1, cls & 1
        for co in range(c):
            for tap in range(4):
                a, b = dy - 1 + (tap >> 1), dx - 1 + (tap & 1)
                for ci in range(2 * c):
                    v = 0.0
                    for ty in (-1, 0, 1):
                        for tx in (-1, 0, 1):
                            if (dy + ty) // 2 == a and (dx + tx) // 2 == b:
                                for cu in range(c):
                                    v += W3[co, cu, ty + 1, tx + 1].item() * Wup[ci, cu, (dy + ty) % 2, (dx + tx) % 2].item()
                    assert abs(weff[cls, co, tap * 2 * c + ci].item() - v) < 1e-12
            for re in range(2):
                for ce in range(2):
                    v = 0.0
                    for ty in (-1, 0, 1):
                        for tx in (-1, 0, 1):
                            inside_y = not (re and ty == (1 if dy else -1))
                            inside_x = not (ce and tx == (1 if dx else -1))
                            if inside_y and inside_x:
                                for cu in range(c):
                                    v += W3[co, cu, ty + 1, tx + 1].item() * bup[cu].item()
                    assert abs(shift16[cls, re, ce, co].item() - s[co].item() * v) < 1e-12
    for co in range(c):
        for ky in range(3):
            for kx in range(3):
                for ci in range(c):
                    assert wskip[co, (3 * ky + kx) * c + ci] == W3[co, c + ci, ky, kx]
    # each class's four taps cover the nine fine taps exactly once: 1 + 2 + 2 + 4
    for dy in range(2):
        for dx in range(2):
            n = [0, 0, 0, 0]
            for ty in (-1, 0, 1):
                for tx in (-1, 0, 1):
                    n[2 * ((dy + ty) // 2 - (dy - 1)) + ((dx + tx) // 2 - (dx - 1))] += 1
            assert sorted(n) == [1, 2, 2, 4]
