/* smirk_emotion.h — extension table of libsmirk_hip.so for the first path's emotion term: EMOCA's frozen ResNet-50
 *   conv 7x7/2 -> BatchNorm -> ReLU -> MaxPool(3, 2, 1) -> Bottleneck x (3, 4, 6, 3) -> AvgPool(7) -> l2 / l1 / cos distance of two feature rows
 *   (reference: src/losses/ExpressionLoss.py, src/losses/resnet.py with emoca_specific=True, include_top=False; smirk_trainer.py:108-119)
 *
 * The 1x1 and 3x3 convolutions of the network, forward and data gradient, are the entries of smirk_hip.h (smirk_conv_igemm_f16x3 with BatchNorm as the
 * epilogue's scale / shift, the residual and the ReLU; smirk_relu_scale_backward_split16 for the masks); this header declares the parts of a Bottleneck
 * ResNet that no entry there serves.  It is versioned on its own (smirk_emotion_abi_version): the tables of smirk_hip.h and smirk_mica.h and their versions
 * do not move when an entry is added here.  Conventions of smirk_hip.h: device pointers, caller-owned buffers, work enqueued on `stream`, 0 = SMIRK_OK.
 * Every pointer must be 16-byte aligned; NULL (where not stated nullable), a misaligned pointer, a channel count that is no multiple of 8 and non-positive
 * sizes return SMIRK_ERR_BAD_ARG before the device is touched, a tensor of 2 GiB or more SMIRK_ERR_UNSUPPORTED.  No entry uses scratch memory or float
 * atomics: every sum has one order, fixed by the shapes, so two runs agree bit for bit.  Every kernel that writes split16 audits the range of what it stores.
 */
#ifndef SMIRK_EMOTION_H
#define SMIRK_EMOTION_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_EMOTION_ABI_VERSION 1
#define SMIRK_EMOTION_STEM_COUT 64   /* output channels of the stem */
#define SMIRK_EMOTION_STEM_K 147     /* 7 * 7 * 3 products per output */
#define SMIRK_EMOTION_STEM_KPAD 160  /* the same padded to ten 16-wide MFMA steps */
enum { SMIRK_EMOTION_L2 = 0, SMIRK_EMOTION_L1 = 1, SMIRK_EMOTION_COS = 2 };

int smirk_emotion_abi_version(void);

/* resnet.py:95-97,138-140: relu(conv(img, w) + shift), Conv2d(3, 64, 7, stride 2, pad 3) with the BatchNorm scale folded into w by the caller.
 * gen, tar: fp32 NCHW [B][3][H][W]; they form one batch of 2B (gen rows first).  w: fp32 [64][SMIRK_EMOTION_STEM_KPAD], k = (ky * 7 + kx) * 3 + c,
 * zeros from k = 147 on.  shift fp32 [64].  out: split16 NHWC [2B][ceil(H/2)][ceil(W/2)][64].  Implicit GEMM on the fp16 matrix pipe, f16x3.
 * The images and the weights come from outside the library: a non-finite value (or one of magnitude >= 65520) sets the range flag. */
int smirk_emotion_stem_split16(const float* gen, const float* tar, const float* w, const float* shift, void* out, int B, int H, int W, void* stream);

/* its data gradient for the gen rows: dimg[b][c][iy][ix] = gup[b] * inv_lift * sum_{ky,kx,co} dz[b][(iy+3-ky)/2][(ix+3-kx)/2][co] * wd[ky][kx][c][co]
 * over the taps whose (iy+3-ky, ix+3-kx) are even and inside the output.  dz split16 [B][ceil(H/2)][ceil(W/2)][64]; wd fp32 [7][7][3][64]
 * (= w[co][c][ky][kx] * the BatchNorm scale); gup fp32 [B], the upstream gradient per sample; dimg fp32 NCHW [B][3][H][W].  Gather form, fp32 FMA. */
int smirk_emotion_stem_dgrad_split16(const void* dz, const float* wd, const float* gup, float inv_lift, float* dimg, int B, int H, int W, void* stream);

/* MaxPool2d(3, stride 2, pad 1) (resnet.py:100): x split16 [N][H][W][C] -> y [N][ceil(H/2)][ceil(W/2)][C]. */
int smirk_emotion_maxpool_split16(const void* x, void* y, int N, int H, int W, int C, void* stream);
/* its backward as a gather: dx[p] = sum over the <= 4 windows that contain p of dy[window] where p is the window's first maximum in row-major order;
 * with relu_mask != 0 multiplied by [x[p] > 0] (x is then the output of a ReLU whose backward is fused in). */
int smirk_emotion_maxpool_backward_split16(const void* x, const void* dy, void* dx, int N, int H, int W, int C, int relu_mask, void* stream);

/* The adjoint of a stride-2 subsampling: out[n][iy][ix][c] = (iy, ix both even ? dz[n][iy/2][ix/2][c] * s[c] * [y[n][iy/2][ix/2][c] > 0] : 0) + add[n][iy][ix][c].
 * dz, y split16 [N][Hl][Wl][C]; add, out split16 [N][H][W][C] with Hl = ceil(H/2), Wl = ceil(W/2); s fp32 [C].  s, y and add are nullable (1 / 1 / 0).
 * Each product and the sum are rounded to fp32 on their own (no fused multiply-add). */
int smirk_emotion_dilate2_split16(const void* dz, const void* y, const float* s, const void* add, void* out, int N, int Hl, int Wl, int H, int W, int C,
                                  void* stream);

/* AvgPool2d(HW) and the loss (ExpressionLoss.py:50-65): feat split16 [2B][HW][C] (gen rows first) -> pooled fp32 [2B][C]; loss fp32 [B]:
 * L2 mean_c (g - t)^2, L1 mean_c |g - t|, COS 1 - sum_c g t / (max(|g|, 1e-8) max(|t|, 1e-8)); mean (nullable) fp32 [1] = mean_b loss[b];
 * aux fp32 [B][4] = (g . t, |g|, |t|, 0) for the backward.  Two launches. */
int smirk_emotion_head_forward_split16(const void* feat, float* pooled, float* aux, float* loss, float* mean, int B, int HW, int C, int metric, void* stream);
/* g[b][p][c] = lift / HW * d loss[b] / d pooled[b][c] * [feat[b][p][c] > 0]: the gradient of the per-sample loss at the input of the last ReLU, times
 * `lift` (a power of two chosen by the caller so that the values sit in fp16's normal range; smirk_emotion_stem_dgrad_split16 divides it out).
 * feat: the gen rows [B][HW][C]; pooled [2B][C] and aux as the forward wrote them; g split16 [B][HW][C]. */
int smirk_emotion_head_backward_split16(const void* feat, const float* pooled, const float* aux, void* g, int B, int HW, int C, int metric, float lift,
                                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
