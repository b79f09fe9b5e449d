/* smirk_visual.h — extension table of libsmirk_hip.so for the trainer's visualisation sheet (reference: base_trainer.py:130-162 save_visualizations,
 * utils.py:65-90 batch_draw_keypoints / make_grid_from_opencv_images, torchvision's make_grid):
 *   fp32 NCHW panels on the device  ->  one uint8 [H][W][3] sheet on the device, every column a make_grid of its panel, the columns side by side.
 * Kernels: csrc/visual.hip; the law, function by function: tests/visual_law.py; design: DESIGN.md §32.
 *
 * It is versioned on its own (the version function below): the tables of smirk_hip.h, smirk_mica.h, smirk_emotion.h, smirk_optim.h, smirk_handoff.h,
 * smirk_generator_plan.h, smirk_generator_arith.h and smirk_data.h and their versions do not move when an entry is added here.  Conventions of smirk_hip.h:
 * device pointers, caller-owned workspace, no allocation, copy or synchronisation inside, work enqueued on `stream`, 0 = SMIRK_OK or a negative SMIRK_ERR_*;
 * every refusal comes before the device is touched.
 *
 * A sheet without landmarks is one launch; with them it is three: clear the overlay map, scatter the dots, write the sheet.
 */
#ifndef SMIRK_VISUAL_H
#define SMIRK_VISUAL_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_VISUAL_ABI_VERSION 1
#define SMIRK_VISUAL_MAX_COLUMNS 16
#define SMIRK_VISUAL_MAX_POINTS 1024      /* points per landmark layer and frame */
#define SMIRK_VISUAL_LAYERS 4             /* landmark layers, drawn in order: a later one overwrites an earlier one */
#define SMIRK_VISUAL_MIN_SIZE 8           /* cell size S outside MIN_SIZE .. MAX_SIZE: SMIRK_ERR_UNSUPPORTED */
#define SMIRK_VISUAL_MAX_SIZE 4096
#define SMIRK_VISUAL_PADDING 2            /* make_grid's padding; its pad value is 0 */

/* One column of the sheet: make_grid(panel, nrow) of a panel of N images, every image resampled nearest (F.interpolate's default: source index
 * floor(dst * float32(Hs / S)), clamped) to the S x S cell.
 *   nsrc == 1: N = B images, src[0] = float32 [B][channels][Hs][Ws]; with `blend` (same shape) a pixel is  src * w_src + blend * w_blend, the two products and
 *              the sum each rounded to float32, never contracted.
 *   nsrc == 4: the second-path panel (smirk_trainer.py:327-330): N = B * nrow images with nrow = 4 Ke; src[which] = float32 [Ke * B][channels][Hs][Ws];
 *              image (b, ke, which) is src[which][ke * B + b].  `blend` must be NULL.
 * N == 1 is shown without padding (S x S); otherwise xmaps = min(nrow, N), ymaps = ceil(N / xmaps) and the grid is ymaps (S + 2) + 2 high, xmaps (S + 2) + 2 wide.
 * channels == 1 repeats the plane to three channels.  `landmarks` != 0 (nsrc == 1, no blend; at most one column): the panel goes through uint8 (x * 255
 * truncated, saturating; NaN -> 0), takes the overlay of the dots entry below, and returns as u8 / 255. */
typedef struct SmirkVisualColumn {
    const float* src[4];
    const float* blend;
    float w_src, w_blend;
    int32_t nsrc, channels;
    int32_t Hs, Ws;
    int32_t nrow;
    int32_t landmarks;
} SmirkVisualColumn;

/* The landmark layers (base_trainer.py:138-141): layer l holds float32 [B][rows[l]][2] of which the first npts[l] rows of every frame are drawn; lm[l] == NULL
 * skips the layer.  Colours in RGB: layer 0 (0,255,0), 1 (255,0,0), 2 (255,0,255), 3 (255,255,255). */
typedef struct SmirkVisualDots {
    const float* lm[SMIRK_VISUAL_LAYERS];
    int32_t rows[SMIRK_VISUAL_LAYERS];
    int32_t npts[SMIRK_VISUAL_LAYERS];
} SmirkVisualDots;

int smirk_visual_abi_version(void);

/* Height, width and byte count (H * W * 3 rounded up to 16: what the sheet entry writes) of the sheet of these columns (host memory; pointers unread).
 * SMIRK_ERR_BAD_ARG: a NULL argument, ncols outside 1 .. SMIRK_VISUAL_MAX_COLUMNS, B <= 0, channels other than 1 or 3, nsrc other than 1 or 4, Hs, Ws or nrow
 * <= 0, nsrc == 4 with nrow % 4 != 0, more than one landmark column or one with nsrc == 4.  SMIRK_ERR_UNSUPPORTED: S outside
 * SMIRK_VISUAL_MIN_SIZE .. SMIRK_VISUAL_MAX_SIZE, columns whose grids differ in height, a sheet of 2^31 bytes or more. */
int smirk_visual_sheet_size(const SmirkVisualColumn* cols, int ncols, int B, int S, int32_t* H, int32_t* W, size_t* bytes);

/* Bytes of the overlay map uint8 [B][S][S] (bit l of a byte: a dot of layer l covers the pixel), rounded up to 256.  0 when B <= 0 or S is out of range. */
size_t smirk_visual_workspace_bytes(int B, int S);

/* Two launches: clear the map; one lane per (layer, frame, point): p = lm * centre + centre in float32 (the reference has centre = 112), truncated toward zero
 * (-0.4 is pixel 0), a filled radius-1 disc (the five pixels with dx^2 + dy^2 <= 1) clipped to the cell, each pixel an atomic OR of bit `layer` into its byte
 * inside the aligned 32-bit word: the map does not depend on execution order.  A non-finite point is skipped.
 * SMIRK_ERR_BAD_ARG: NULL dots or ws, a layer pointer off 4 bytes, B <= 0, rows or npts < 0, npts > rows, centre not finite, ws off 256 bytes;
 * SMIRK_ERR_UNSUPPORTED: S out of range, npts above SMIRK_VISUAL_MAX_POINTS; SMIRK_ERR_WORKSPACE: ws_bytes below smirk_visual_workspace_bytes(B, S). */
int smirk_visual_dots(const SmirkVisualDots* dots, int B, int S, float centre, void* ws, size_t ws_bytes, void* stream);

/* One launch writes every byte of sheet[0 .. bytes) exactly once, padding and the tail after H * W * 3 (zeros) included: a lane produces 16 consecutive bytes and
 * stores them as one vector.  Per byte: v * 255, clipped to [0, 255] (NaN -> 0), truncated; channel order RGB, or BGR when bgr != 0.  A landmark column paints
 * the colour of the highest bit set in the map (ws, as the dots entry left it).  The descriptors travel in the kernel arguments: nothing has to stay alive.
 * Refusals of the size entry, and SMIRK_ERR_BAD_ARG: NULL sheet, a sheet off 256 bytes, a NULL or 4-byte-unaligned src, a blend with nsrc == 4 or on a landmark
 * column, a landmark column with ws NULL or off 256 bytes; SMIRK_ERR_WORKSPACE: sheet_bytes below the size entry's byte count, or (landmark column) ws_bytes below
 * smirk_visual_workspace_bytes(B, S). */
int smirk_visual_sheet(const SmirkVisualColumn* cols, int ncols, int B, int S, int bgr, const void* ws, size_t ws_bytes, uint8_t* sheet, size_t sheet_bytes,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
