/* smirk_data.h — extension table of libsmirk_hip.so for the trainer's batch preparation (reference: datasets/base_dataset.py:124-215 prepare_data):
 *   decoded uint8 BGR frames of any mix of resolutions + their landmark arrays  ->  the `batch` dict on the device
 *   (img, landmarks_fan, flag_landmarks_fan, landmarks_mp, mask, img_mica), training path (random crop scale + the eight-transform augmentation) and
 *   deterministic path.  Kernels: csrc/data.hip; draws: csrc/data_rng.h; the law, function by function: tests/data_law.py; design: DESIGN.md §31.
 *
 * It is versioned on its own (the version function below): the tables of smirk_hip.h, smirk_mica.h, smirk_emotion.h, smirk_optim.h, smirk_handoff.h,
 * smirk_generator_plan.h and smirk_generator_arith.h and their versions do not move when an entry is added here.  Conventions of smirk_hip.h: device
 * pointers, caller-owned workspace, no allocation, copy or synchronisation inside, work enqueued on `stream`, 0 = SMIRK_OK or a negative SMIRK_ERR_*; every
 * refusal comes before the device is touched.
 *
 * One batch is  params -> crop -> the hull mask entry of smirk_hip.h on the truncated points params wrote [-> stats -> colour -> finish]:
 * three launches on the deterministic path, seven on the training path (finish is two), whatever N.
 */
#ifndef SMIRK_DATA_H
#define SMIRK_DATA_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_DATA_ABI_VERSION 1
#define SMIRK_DATA_MAX_POINTS 1024        /* mediapipe points per frame (the limit of smirk_hull_mask) */
#define SMIRK_DATA_FAN_POINTS 68
#define SMIRK_DATA_MICA_SIZE 112
#define SMIRK_DATA_CLAHE_TILES 8          /* 8 x 8 tiles: S must be a multiple of 8 */
#define SMIRK_DATA_MAX_SIZE 2040          /* S above this: SMIRK_ERR_UNSUPPORTED (tile histograms and the grey sum are 32-bit) */

/* the eight transforms, in the order they are applied; also the bit of SmirkDataParams.coins */
enum SmirkDataTransform {
    SMIRK_DATA_BRIGHTNESS_CONTRAST = 0, SMIRK_DATA_GAMMA = 1, SMIRK_DATA_COLOR_JITTER = 2, SMIRK_DATA_CLAHE = 3, SMIRK_DATA_RGB_SHIFT = 4, SMIRK_DATA_BLUR = 5,
    SMIRK_DATA_GAUSS_NOISE = 6, SMIRK_DATA_SHIFT_SCALE_ROTATE = 7, SMIRK_DATA_TRANSFORMS = 8
};

/* Probabilities and limits of the augmentation (host memory).  Every p in [0, 1]; every symmetric limit >= 0; every lo <= hi. */
typedef struct SmirkDataAugment {
    double p[SMIRK_DATA_TRANSFORMS];
    double brightness_limit, contrast_limit;                    /* beta in +-limit (x 255, "by max"), alpha in 1 +- limit */
    double gamma_lo, gamma_hi;                                  /* gamma = U(lo, hi) / 100; lo > 0 */
    double cj_brightness, cj_contrast, cj_saturation, cj_hue;   /* factors in 1 +- limit (limit <= 1), hue shift in +-limit (limit <= 0.5) */
    double clahe_lo, clahe_hi;                                  /* clip limit = U(lo, hi); lo >= 1 */
    double rgb_shift;                                           /* each channel in +-limit */
    double noise_var_lo, noise_var_hi;                          /* variance = U(lo, hi); lo >= 0 */
    double shift_limit, scale_limit, rotate_limit;              /* dx, dy in +-shift (fractions of S), scale in 1 +- limit (limit < 1), angle in +-rotate degrees */
    int32_t blur_max;                                           /* k uniform over the odd numbers 3 .. blur_max; blur_max in {3, 5, 7} */
    int32_t _pad;
} SmirkDataAugment;

/* where frame i lies in the packed byte buffer: uint8 [H][W][3] BGR at `offset` */
typedef struct SmirkDataFrame {
    uint64_t offset;
    int32_t H, W;
} SmirkDataFrame;

/* What smirk_data_params decides per frame, all float64.  2 x 3 matrices are row-major (m0 m1 m2 / m3 m4 m5): x' = m0 x + m1 y + m2, y' = m3 x + m4 y + m5. */
typedef struct SmirkDataParams {
    double crop_fwd[6];          /* frame (x, y) -> crop (x, y): crop_face's similarity in closed form (scale + translation) */
    double crop_inv[6];          /* crop (col, row) -> frame (x, y) */
    double ssr_fwd[6];           /* ShiftScaleRotate on key points; the identity when its coin is off (and on the deterministic path) */
    double ssr_inv[6];           /* output (col, row) -> source pixel */
    double mica_inv[6];          /* 112 x 112 output (col, row) -> frame (x, y): inverse of the 5-point ArcFace similarity; zeros when flag_fan is 0 */
    double scale;                /* crop scale */
    double bc_alpha, bc_beta;    /* RandomBrightnessContrast */
    double gamma;                /* RandomGamma exponent */
    double cj[4];                /* ColorJitter: brightness, contrast, saturation factors and the hue shift */
    double clahe_clip;
    double rgb_shift[3];
    double noise_sigma;          /* sqrt(variance) */
    double ssr_angle, ssr_scale, ssr_dx, ssr_dy;
    int32_t coins;               /* bit t: transform t (enum SmirkDataTransform) is applied */
    int32_t blur_k;              /* 3, 5 or 7 */
    int32_t flag_fan;
    int32_t _pad;
} SmirkDataParams;

int smirk_data_abi_version(void);

/* Bytes of the workspace one batch needs.  Its head is the SmirkDataParams [N] array (smirk_data_params writes it, every other entry reads it), followed by
 * the truncated hull points float32 [N][Lmax][2] (byte offset smirk_data_hull_points_offset; room for Lmax = SMIRK_DATA_MAX_POINTS) and, on the training path, the uint8 staging
 * images, the float32 hull masks (smirk_data_hull_offset: [N][S][S], where smirk_hull_mask is told to write) and the per-frame tables.
 * 0 when N <= 0, S <= 0, S % 8 != 0 or S > SMIRK_DATA_MAX_SIZE. */
size_t smirk_data_workspace_bytes(int N, int S, int train);
size_t smirk_data_hull_points_offset(int N, int S, int train);
size_t smirk_data_hull_offset(int N, int S, int train);

/* Per frame, one workgroup, float64 throughout:
 *   the crop similarity (random scale = scale_lo + (scale_hi - scale_lo) u; scale_lo == scale_hi on the deterministic path), every augmentation coin and draw
 *   (aug != NULL: training path), the ShiftScaleRotate matrix and inverse, the ArcFace similarity, and the landmark outputs
 *       landmarks_fan_out [N][68][2], landmarks_mp_out [N][n_index][2]   float32: crop -> ShiftScaleRotate -> cast -> / S, * 2, - 1 each rounded in float32
 *       flag_fan_out [N] bytes
 *       hull points (workspace): all n_mp[i] cropped points truncated toward zero; rows n_mp[i] .. Lmax - 1 repeat point 0
 * lmk_mp [N][Lmax][2] float64 (rows past n_mp[i] unread), n_mp [N] int32 with mp_index[] < n_mp[i] <= Lmax (validated by the caller: device memory),
 * lmk_fan [N][68][2] float64 (zeros where flag_fan[i] == 0), mp_index [n_index] int32.
 * SMIRK_ERR_BAD_ARG: a NULL pointer, N <= 0, S <= 0, Lmax or n_index outside 1 .. SMIRK_DATA_MAX_POINTS, a scale that is not finite and positive or
 * scale_lo > scale_hi, a probability outside [0, 1] or NaN, a reversed or out-of-range limit.  SMIRK_ERR_UNSUPPORTED: S % 8 != 0 or S > SMIRK_DATA_MAX_SIZE.
 * SMIRK_ERR_WORKSPACE: ws_bytes below smirk_data_workspace_bytes(N, S, aug != NULL). */
int smirk_data_params(const double* lmk_mp, const int32_t* n_mp, int Lmax, const double* lmk_fan, const uint8_t* flag_fan, const int32_t* mp_index,
                      int n_index, int N, int S, double scale_lo, double scale_hi, const SmirkDataAugment* aug, uint64_t seed, uint64_t offset,
                      float* landmarks_fan_out, float* landmarks_mp_out, uint8_t* flag_fan_out, void* ws, size_t ws_bytes, void* stream);

/* From the descriptor table (device, [N]) and the packed frames (device, frames_bytes bytes; a descriptor that reaches past them reads as a black frame):
 *   the crop: arithmetic of the affine warp entry of smirk_hip.h: float64 bilinear over floor / ceil neighbours, constant 0 outside, truncation to uint8, BGR -> RGB;
 *             training path (train != 0): uint8 [N][S][S][3] into the workspace, img unused (may be NULL);  deterministic path: img [N][3][S][S] = v / 255
 *   img_mica [N][3][112][112]: float64 bilinear of frame / 255 through mica_inv, constant 0 outside, BGR -> RGB; zeros where flag_fan is 0.
 * Same refusals as smirk_data_params for N, S and the workspace; NULL frames, table, img_mica (or img with train == 0), frames_bytes == 0: SMIRK_ERR_BAD_ARG. */
int smirk_data_crop(const uint8_t* frames, size_t frames_bytes, const SmirkDataFrame* table, int N, int S, int train, float* img, float* img_mica,
                    void* ws, size_t ws_bytes, void* stream);

/* Training path.  One workgroup per frame: the point-wise lookup table of RandomBrightnessContrast -> RandomGamma -> ColorJitter brightness / contrast
 * (the contrast pivots on the mean grey of the image entering ColorJitter, which is summed here), then CLAHE's 8 x 8 tile histograms of the 8-bit L channel
 * in LDS (two halves of 32 tiles), clip + redistribute, CDF -> 64 x 256 table bytes.  A frame without the CLAHE coin leaves after its lookup table. */
int smirk_data_stats(int N, int S, void* ws, size_t ws_bytes, void* stream);
/* Training path.  The point-wise chain on the crop: lookup table, ColorJitter saturation and hue, CLAHE apply, RGBShift -> uint8 staging image. */
int smirk_data_colour(int N, int S, void* ws, size_t ws_bytes, void* stream);
/* Training path, two launches: box blur (reflect-101) + per-pixel per-channel Gaussian noise (counters seed / offset, stream id DATA_STREAM_PIXEL) into a
 * second staging image; then the ShiftScaleRotate resample of image (float64 bilinear, constant 0 taking part, round-half-even) and mask (nearest on
 * 1 - hull, border 0) -> img [N][3][S][S] = v / 255, mask [N][1][S][S] (1 outside the hull and outside the frame). */
int smirk_data_finish(int N, int S, uint64_t seed, uint64_t offset, float* img, float* mask, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
