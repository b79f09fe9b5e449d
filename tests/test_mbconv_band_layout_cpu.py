"""The wave-private E region of the halo-tile mode of csrc/mbconv_image.hip (mbi_band_body) against the gfx950 LDS bank model (tools/lds_bank_model.py), in the
style of tests/test_mbconv_s2_layout_cpu.py: the address arithmetic of the kernel (the cell map 16 hy + hx, `mbb_out_px`, the XOR swizzle of a cell's eight 16-byte
slots, the XOR forms of the tap and store addresses) is restated here lane by lane.  Every lane of every depthwise tap must read the cell of ITS halo pixel, the 16 lanes
of every ds_read_b128 group must hit 16 distinct 16-byte slots for all nine taps, and the 32 lanes of every expand store group 32 distinct banks.  A layout change
in the kernel has to be mirrored here, which is the point."""
from tools.lds_bank_model import B32_GROUPS, READ_B128_GROUPS, read_b128_cycles

HH, HW, NCELL = 4, 16, 64       # E halo of a 2 x 14 band: 4 rows x 16 columns = two 32-row expand blocks
REGION = NCELL * 32             # dwords of a wave's region (8 KB)


def cell_of(hy, hx):
    return 16 * hy + hx


def mbb_out_px(m):
    k = m >> 2
    return (0x96 >> k) & 1, (k >> 1) * 4 + (m & 3)


def e_dword(cell, ch):
    """dword address of channel ch of a cell inside a wave's region"""
    return cell * 32 + ((((ch >> 2) ^ (cell >> 1)) & 7) << 2) + (ch & 3)


def tap_cell(fr, ky, kx):
    """the kernel's form: rows 28 - 31 of the project block are no pixel (ox = 14, 15), their cells wrap inside the region"""
    oy, ox = mbb_out_px(fr)
    return ((oy + ky) * 16 + ox + kx) & 63


def test_the_cell_map_is_a_bijection_and_expand_row_p_is_cell_p():
    cells = [cell_of(hy, hx) for hy in range(HH) for hx in range(HW)]
    assert cells == list(range(NCELL))
    # lane fr of expand block t loads halo pixel (2 t + (fr >> 4), fr & 15): row 32 t + fr of the expand GEMM is cell 32 t + fr
    for t in range(2):
        for fr in range(32):
            assert cell_of(2 * t + (fr >> 4), fr & 15) == 32 * t + fr
    for cell in (0, 1, 2, 37, 63):                          # the channels of a cell fill its 32 dwords
        assert sorted(e_dword(cell, ch) for ch in range(32)) == list(range(cell * 32, cell * 32 + 32))


def test_the_output_pixel_map_deals_one_output_row_to_each_read_group():
    px = [mbb_out_px(m) for m in range(32)]
    assert sorted(p for p in px if p[1] < 14) == [(oy, ox) for oy in range(2) for ox in range(14)]       # 28 pixels, each once
    assert sorted(p for p in px if p[1] >= 14) == [(0, 14), (0, 15), (1, 14), (1, 15)]                    # 4 rows of the project block that are no pixel
    for g in READ_B128_GROUPS:
        got = sorted(mbb_out_px(lane & 31) for lane in g)
        assert got == [(got[0][0], ox) for ox in range(16)], g


def test_every_pixel_lane_reads_the_cell_of_its_tap_inside_the_region():
    for fr in range(32):
        oy, ox = mbb_out_px(fr)
        for ky in range(3):
            for kx in range(3):
                c = tap_cell(fr, ky, kx)
                assert 0 <= c < NCELL
                if ox < 14:                                 # output (oy, ox) of the band reads halo pixel (oy + ky, ox + kx): the halo starts one pixel up and left
                    assert oy + ky < HH and ox + kx < HW and c == cell_of(oy + ky, ox + kx), (fr, ky, kx)


def test_depthwise_tap_reads_are_conflict_free():
    """lane (fr, hb): output pixel mbb_out_px(fr), channels 8 (2 s + hb) .. + 7 as two ds_read_b128 (h = 0, 1) per tap"""
    for region in (0, REGION, 3 * REGION):                 # the regions of waves 0, 1, 3 (a multiple of 64 dwords: the banks do not move)
        for ky in range(3):
            for kx in range(3):
                for s in range(2):
                    for h in range(2):
                        def addr(lane):
                            fr, hb = lane & 31, lane >> 5
                            return region + e_dword(tap_cell(fr, ky, kx), 8 * (2 * s + hb) + 4 * h)
                        assert read_b128_cycles(addr) == 4, (ky, kx, s, h)
                        for g in READ_B128_GROUPS:           # said directly: 16 distinct 16-byte slots of the 16 a 64-bank row holds
                            assert len({(addr(lane) // 4) % 16 for lane in g}) == 16, (ky, kx, s, h)


def test_the_kernel_s_xor_form_of_the_tap_address_equals_the_plain_one():
    """ta[k] = cell * 128 + (((cell >> 1) ^ 2 hb) & 7) << 4, then ^ ((4 s + h) << 4) per read (bytes)"""
    for fr in range(32):
        for hb in range(2):
            for ky in range(3):
                for kx in range(3):
                    cell = tap_cell(fr, ky, kx)
                    ta = cell * 128 + ((((cell >> 1) ^ (2 * hb)) & 7) << 4)
                    for s in range(2):
                        for h in range(2):
                            assert (ta ^ ((4 * s + h) << 4)) == 4 * e_dword(cell, 8 * (2 * s + hb) + 4 * h)


def test_expand_stores_are_conflict_free_and_land_on_their_cells():
    """accumulator register r of row block t, lane (fr, hb): cell 32 t + (r & 3) + 8 (r >> 2) + 4 hb, channel fr, one ds_write_b32;
    kernel form: (est ^ (cr << 4)) + (32 t + ro) * 128 with est = hb * 512 + (((fr >> 2) ^ (hb << 1)) << 4) + (fr & 3) * 4"""
    seen = set()
    for t in range(2):
        for r in range(16):
            ro, cr = (r & 3) + 8 * (r >> 2), ((r >> 1) & 1) | (((r >> 2) & 1) << 2)

            def byte(lane):
                fr, hb = lane & 31, lane >> 5
                est = hb * 512 + (((fr >> 2) ^ (hb << 1)) << 4) + (fr & 3) * 4
                return (est ^ (cr << 4)) + (32 * t + ro) * 128
            for lane in range(64):
                fr, hb = lane & 31, lane >> 5
                assert byte(lane) == 4 * e_dword(32 * t + ro + 4 * hb, fr), (t, r, lane)
                seen.add(byte(lane) // 4)
            for g in B32_GROUPS:
                assert len({(byte(lane) // 4) % 32 for lane in g}) == 32, (t, r)
    assert seen == set(range(REGION))                       # the two blocks write every dword of the region, each once


def test_the_epilogue_transpose_fits_the_region():
    assert 32 * 36 * 4 <= NCELL * 128                       # 32 rows x 36 floats
