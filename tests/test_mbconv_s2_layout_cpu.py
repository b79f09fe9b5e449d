"""The wave-private E region of csrc/mbconv_s2.hip against the gfx950 LDS bank model (tools/lds_bank_model.py), in the style of tests/test_lds_layouts_cpu.py: the
address arithmetic of the kernel (`s2w_idx`, `s2w_pix`, `s2w_out_px`, the XOR swizzle of a cell's eight 16-byte slots) is restated here lane by lane.  The 16 lanes of
every ds_read_b128 group of every depthwise tap must hit 16 distinct 16-byte slots, the 32 lanes of every expand store group 32 distinct banks, and the cell map must be a
bijection between the 153 halo pixels and 153 cells.  A layout change in the kernel has to be mirrored here, which is the point."""
import numpy as np

from tools.lds_bank_model import B32_GROUPS, READ_B128_GROUPS, read_b128_cycles

NH, HI, WI = 153, 9, 17


def s2w_idx(hy, hx):
    R, J = hy >> 1, hx >> 1
    if not hx & 1:
        return (85 if hy & 1 else 0) + (R >> 1) * 18 + 2 * J + (R & 1)
    if hy & 1:
        return 121 + (R >> 1) * 16 + 2 * J + (R & 1)
    return 53 + (R >> 1) * 16 + 2 * J + (R & 1) if R < 4 else 37 + 2 * J


def s2w_pix(p):
    if p < 53:
        if p < 36 or not p & 1:
            pr, rem = divmod(p, 18)
            rp, cp, R, J = 0, 0, 2 * pr + (rem & 1), rem >> 1
        else:
            rp, cp, R, J = 0, 1, 4, (p - 37) >> 1
    elif p < 85:
        u = p - 53
        rp, cp, R, J = 0, 1, 2 * (u >> 4) + (u & 1), (u & 15) >> 1
    elif p < 121:
        pr, rem = divmod(p - 85, 18)
        rp, cp, R, J = 1, 0, 2 * pr + (rem & 1), rem >> 1
    else:
        u = p - 121
        rp, cp, R, J = 1, 1, 2 * (u >> 4) + (u & 1), (u & 15) >> 1
    return 2 * R + rp, 2 * J + cp


def s2w_out_px(m):
    k = m >> 2
    return (0xD728 >> (2 * k)) & 3, ((k >> 1) & 1) * 4 + (m & 3)


def e_dword(cell, ch):
    """dword address of channel ch of a cell inside a wave's region"""
    return cell * 32 + ((((ch >> 2) ^ (cell >> 1)) & 7) << 2) + (ch & 3)


def test_the_cell_map_is_a_bijection_and_s2w_pix_is_its_inverse():
    cells = np.array([[s2w_idx(hy, hx) for hx in range(WI)] for hy in range(HI)])
    assert sorted(cells.flatten().tolist()) == list(range(NH))
    for p in range(NH):
        hy, hx = s2w_pix(p)
        assert 0 <= hy < HI and 0 <= hx < WI and cells[hy, hx] == p, p
    # the channels of a cell fill its 32 dwords
    for cell in (0, 1, 2, 37, 152):
        assert sorted(e_dword(cell, ch) for ch in range(32)) == list(range(cell * 32, cell * 32 + 32))


def test_the_output_pixel_map_deals_two_output_rows_to_each_read_group():
    assert sorted(s2w_out_px(m) for m in range(32)) == [(oy, ox) for oy in range(4) for ox in range(8)]
    for g in READ_B128_GROUPS:
        px = sorted(s2w_out_px(lane & 31) for lane in g)
        rows = sorted({oy for oy, _ in px})
        assert len(rows) == 2 and rows[1] == rows[0] + 1 and px == [(oy, ox) for oy in rows for ox in range(8)]


def test_depthwise_tap_reads_are_conflict_free():
    """lane (fr, hb): output pixel s2w_out_px(fr), channels 8 (2 s + hb) .. + 7 as two ds_read_b128 (h = 0, 1) per tap"""
    for region in (0, NH * 32, 3 * NH * 32):               # the regions of waves 0, 1, 3 (a multiple of 32 dwords: the banks do not move)
        for ky in range(3):
            for kx in range(3):
                for s in range(2):
                    for h in range(2):
                        def addr(lane):
                            fr, hb = lane & 31, lane >> 5
                            oy, ox = s2w_out_px(fr)
                            return region + e_dword(s2w_idx(2 * oy + ky, 2 * ox + kx), 8 * (2 * s + hb) + 4 * h)
                        assert read_b128_cycles(addr) == 4, (ky, kx, s, h)
                        for g in READ_B128_GROUPS:           # said directly: 16 distinct 16-byte slots of the 16 a 64-bank row holds
                            assert len({(addr(lane) // 4) % 16 for lane in g}) == 16, (ky, kx, s, h)


def test_the_kernel_s_xor_form_of_the_tap_address_equals_the_plain_one():
    """ta[k] = cell * 128 + (((cell >> 1) ^ 2 hb) & 7) << 4, then ^ ((4 s + h) << 4) per read (bytes)"""
    for fr in range(32):
        oy, ox = s2w_out_px(fr)
        for hb in range(2):
            for ky in range(3):
                for kx in range(3):
                    cell = s2w_idx(2 * oy + ky, 2 * ox + kx)
                    ta = cell * 128 + ((((cell >> 1) ^ (2 * hb)) & 7) << 4)
                    for s in range(2):
                        for h in range(2):
                            assert (ta ^ ((4 * s + h) << 4)) == 4 * e_dword(cell, 8 * (2 * s + hb) + 4 * h)


def test_expand_stores_are_conflict_free_and_land_on_their_cells():
    """accumulator register r of row block t, lane (fr, hb): cell 32 t + (r & 3) + 8 (r >> 2) + 4 hb, channel fr, one ds_write_b32;
    kernel form: (est ^ (cr << 4)) + (32 t + ro) * 128 with est = hb * 512 + (((fr >> 2) ^ (hb << 1)) << 4) + (fr & 3) * 4"""
    for t in range(5):
        for r in range(16):
            ro, cr = (r & 3) + 8 * (r >> 2), ((r >> 1) & 1) | (((r >> 2) & 1) << 2)

            def byte(lane):
                fr, hb = lane & 31, lane >> 5
                est = hb * 512 + (((fr >> 2) ^ (hb << 1)) << 4) + (fr & 3) * 4
                return (est ^ (cr << 4)) + (32 * t + ro) * 128
            for lane in range(64):
                fr, hb = lane & 31, lane >> 5
                assert byte(lane) == 4 * e_dword(32 * t + ro + 4 * hb, fr), (t, r, lane)
            for g in B32_GROUPS:
                assert len({(byte(lane) // 4) % 32 for lane in g}) == 32, (t, r)
    # the rows the last block must not store are exactly the cells that do not exist
    assert [ro4 for ro4 in range(32) if 128 + ro4 >= NH] == list(range(25, 32))
