/* smirk_jpeg.h — extension table of libsmirk_hip.so for baseline JPEG encoding of finished uint8 pictures on the device (reference: base_trainer.py:162
 * cv2.imwrite of the visualisation sheet, demo_video.py:211-214 cv2.VideoWriter of every grid):
 *   B pictures uint8 [B][H][W][3] on the device  ->  B complete JFIF files back to back on the device, and their (offset, length) table.
 * Sequential DCT, 8 bit, YCbCr 4:2:0, 16 x 16 MCUs, the Annex K "typical" Huffman tables, restart intervals.  The arithmetic is integer throughout and is
 * restated step by step in tests/jpeg_law.py: the output equals the law's byte for byte.  Kernels: csrc/jpeg.hip; design and measurements: DESIGN.md §34.
 *
 * It is versioned on its own (the version function below): the tables of smirk_hip.h, smirk_mica.h, smirk_emotion.h, smirk_optim.h, smirk_handoff.h,
 * smirk_train_handoff.h, smirk_generator_plan.h, smirk_generator_arith.h, smirk_data.h and smirk_visual.h and their versions do not move when an entry is added
 * here.  Conventions of smirk_hip.h: device pointers, caller-owned workspace, no allocation, copy or synchronisation inside, work enqueued on `stream`,
 * 0 = SMIRK_OK or a negative SMIRK_ERR_*; every refusal comes before the device is touched.
 *
 * Four launches: coefficients (colour, chroma mean, DCT, quantisation); the byte count of every restart interval; one scan that turns the counts into
 * offsets; the bytes themselves, with every file's header and EOI.  Every output byte is written exactly once.
 *
 * The interval a file is coded with is min(R, MCUs of a picture, 65535) (DRI holds 16 bits); below, Re is that number and
 * intervals = ceil(MCUs / Re), MCUs = ceil(H / 16) * ceil(W / 16).
 *
 * The bound.  The longest codes of the tables: DC 11 bits (chrominance, category 11) + 11 magnitude bits = 22; AC 16 bits + 10 magnitude bits = 26 per
 * non-zero coefficient; a zero coefficient never costs more than a non-zero one in its place (k >= 1 zeros of a block cost at most one EOB of 4 bits and
 * floor(k / 16) ZRLs of 11 bits, and 26 k >= 4 + 11 k / 16).  So a block is at most 22 + 63 * 26 = 1660 bits, an MCU of six blocks 9960 bits = 1245 bytes, and an
 * interval ceil(Re * 1245) bytes after its padding; stuffing at most doubles that (every byte 0xFF), and the RSTm or EOI after it adds 2:
 *   max_bytes = B * (SMIRK_JPEG_HEADER_BYTES + intervals * (2 * Re * 1245 + 2))
 */
#ifndef SMIRK_JPEG_H
#define SMIRK_JPEG_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_JPEG_ABI_VERSION 1
#define SMIRK_JPEG_HEADER_BYTES 629       /* SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14 */
#define SMIRK_JPEG_MCU_MAX_BYTES 1245     /* 6 * (22 + 63 * 26) / 8, before stuffing */
#define SMIRK_JPEG_MAX_DIM 65535

int smirk_jpeg_abi_version(void);

/* Bytes of the workspace: int16 zigzag coefficients [B][MCUs][6][64], uint32 sizes [B * intervals], uint32 offsets [B * intervals], each part rounded up to 256.
 * 0 for arguments the encode entry refuses. */
size_t smirk_jpeg_workspace_bytes(int B, int H, int W, int R);

/* The bound derived above; 0 for arguments the encode entry refuses with SMIRK_ERR_BAD_ARG.  May reach 2^31 and more: the encode entry refuses such a batch. */
size_t smirk_jpeg_max_bytes(int B, int H, int W, int R);

/* Host only.  qt[0] luminance, qt[1] chrominance, natural (row-major) order: the Annex K base tables under the IJG quality rule, s = 5000 / quality below 50 and
 * 200 - 2 quality from there on, entry = clip((base * s + 50) / 100, 1, 255), integer divisions.  SMIRK_ERR_BAD_ARG: NULL qt, quality outside 1 .. 100. */
int smirk_jpeg_quant_tables(int quality, uint8_t qt[2][64]);

/* img: uint8 [B][H][W][3] on the device, RGB or (bgr != 0) BGR; qt: HOST memory, as the entry above fills it (it travels in the kernel arguments, like the header
 * built from it); out: the files back to back from out[0]; spans: uint32 [B][2] on the device, (offset, length) of every file.  Nothing past the last file is
 * written.
 * SMIRK_ERR_BAD_ARG: NULL img, qt, ws, out or spans; img or out off 16 bytes, ws off 256, spans off 8; B <= 0; H or W outside 1 .. SMIRK_JPEG_MAX_DIM; R < 1; a
 * quantisation entry of 0.  SMIRK_ERR_UNSUPPORTED: B * H * W * 3 or smirk_jpeg_max_bytes at 2^31 or above.  SMIRK_ERR_WORKSPACE: ws_bytes below
 * smirk_jpeg_workspace_bytes, out_bytes below smirk_jpeg_max_bytes. */
int smirk_jpeg_encode_u8(const uint8_t* img, int B, int H, int W, int bgr, const uint8_t qt[2][64], int R, void* ws, size_t ws_bytes, uint8_t* out,
                         size_t out_bytes, uint32_t* spans, void* stream);

#ifdef __cplusplus
}
#endif
#endif
