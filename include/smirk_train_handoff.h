/* smirk_train_handoff.h — extension table of libsmirk_hip.so for the hand-off from the masking utilities to SmirkGenerator in the two TRAINING paths
 * (reference: smirk_trainer.py:76-94 — first path; :262-295 — second path with its Ke repeated frames):
 *   one launch that samples the mesh points and quantises them for the source frame and for each of its Ke target frames, and one launch that transfers the
 *   sampled pixels, composes masked_img and stores the generator's packed split-fp16 input beside it.  The Ke copies of the batch exist as index arithmetic only.
 *
 * It is versioned on its own (the version function below): the tables of smirk_hip.h, smirk_handoff.h and the other extension headers and their versions do not
 * move when an entry is added here.  Conventions of smirk_hip.h: device pointers, caller-owned memory, no allocation, copy or synchronisation inside, work
 * enqueued on `stream`, 0 = SMIRK_OK or a negative SMIRK_ERR_*; every refusal comes before the device is touched.
 */
#ifndef SMIRK_TRAIN_HANDOFF_H
#define SMIRK_TRAIN_HANDOFF_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_TRAIN_HANDOFF_ABI_VERSION 1

/* how the rendering's coverage mask is read off rendered_img [.][3][H][W] */
#define SMIRK_RENDERED_RULE_NONZERO 0    /* 1 - (r == 0).all(1)    first path, smirk_trainer.py:79   */
#define SMIRK_RENDERED_RULE_POSITIVE 1   /* (r > 0).all(1)         second path, smirk_trainer.py:290 */

int smirk_train_handoff_abi_version(void);

/* What smirk_sample_faces -> smirk_vertices2landmarks + smirk_points_to_pixels on tv_src -> the same two on each of the Ke target frames compute, in one launch
 * (one workgroup per source frame).  `weights` [B][F] are the face weights of smirk_mask_face_weights on tv_src; the draws are those of smirk_sample_faces under
 * the same (seed, offset): counter offset + b * num + t of stream 0.
 *     points_src  [B][num][2] int32        (x, y) pixel of point t on source frame b: .5 * (1 + p) * image_size, truncated, clamped to [0, image_size - 1]
 *     points_dst  [Ke * B][num][2] int32   the same point on target frame k * B + b, gathered from tv_dst[k * B + b]
 * and, each behind a pointer that may be NULL, the tensors of the separate launches, bit for bit:
 *     faces_idx   [B][num] int64           sampled face of every point
 *     bary        [B][num][3] fp32         its folded barycentric coordinates
 *     npoints_src [B][num][3] int64, npoints_dst [Ke * B][num][3] int64     (x, y, z) as smirk_points_to_pixels writes them
 * tv_src [B][V][3], tv_dst [Ke * B][V][3], faces [F][3] int32 with vertex indices below V.
 * tv_dst == NULL is the first path: the targets are the sources; Ke must be 1 and points_dst and npoints_dst NULL.
 * SMIRK_ERR_BAD_ARG: weights, tv_src, faces or points_src NULL; tv_dst given and points_dst NULL; tv_dst NULL and Ke != 1, points_dst or npoints_dst given;
 * B, Ke, V, F, num or image_size <= 0; F > 38000 (the CDF must fit the LDS); image_size > 32768. */
int smirk_sample_transfer_points(const float* weights, const float* tv_src, const float* tv_dst, const int32_t* faces, int B, int Ke, int V, int F, int num,
                                 int image_size, uint64_t seed, uint64_t offset, int32_t* points_src, int32_t* points_dst, int64_t* faces_idx, float* bary,
                                 int64_t* npoints_src, int64_t* npoints_dst, void* stream);

/* What the chain transfer_pixels(img.repeat(Ke), points1.repeat(Ke), points2) -> rendered mask -> masking(img.repeat(Ke), hull.repeat(Ke), extra, 10, rendered_mask,
 * extra_noise) -> pack of cat(rendered_img, masked_img) computes, in one launch over the Ke * B output frames.  Output frame kb reads img[kb % B], the hull of
 * kb % B, rendered_img[kb], points_dst[kb] and the sources points_src[kb % B]:
 *     masked_img [Ke * B][3][H][W] fp32       bit for bit the tensor of the separate launches (field_offset and noise_offset are the offsets the Bernoulli field over
 *                                             [Ke * B][H][W] and the composition over [Ke * B][3][H][W] would have been handed)
 *     packed     [Ke * B][H][W][8] split-fp16 channels 0-2 rendered_img, 3-5 masked_img, 6-7 zero: bit for bit what the generator's own pack writes
 * img [B][3][H][W]; rendered_img [Ke * B][3][H][W]; hull_mask [B][H][W] with hull_batch_stride = H * W, or ONE [H][W] mask with stride 0; points_src [B][N][2]
 * and points_dst [Ke * B][N][2] as above (the same pointer twice in the first path).  Where several points land on one pixel the highest point index wins; a
 * target outside the image is dropped, and a winner whose source lies outside the image contributes nothing.
 * SMIRK_ERR_BAD_ARG: a NULL pointer; B, Ke, N, H or W <= 0; another stride; random_mask <= 0 or NaN; rendered_rule not one of the two above.
 * SMIRK_ERR_UNSUPPORTED: rows too wide for two workgroups per CU (W above 244), or a grid beyond 2^31 - 1: the caller keeps the separate launches. */
int smirk_train_masking_handoff(const float* img, const float* rendered_img, const float* hull_mask, long long hull_batch_stride, const int32_t* points_src,
                                const int32_t* points_dst, int B, int Ke, int N, int H, int W, int rendered_rule, float random_mask, uint64_t seed,
                                uint64_t field_offset, uint64_t noise_offset, float* masked_img, void* packed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
