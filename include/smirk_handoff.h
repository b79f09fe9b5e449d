/* smirk_handoff.h — extension table of libsmirk_hip.so for the hand-off from the masking utilities to SmirkGenerator in the inference path
 * (reference: demo.py:138-169 — rendered mask, masking(), torch.cat([rendered_img, masked_img], 1), the generator):
 *   one launch that produces masked_img AND the generator's packed split-fp16 input, and a generator entry that starts from that packed tensor.
 *
 * It is versioned on its own (the version function below): the tables of smirk_hip.h, smirk_mica.h, smirk_emotion.h and smirk_optim.h and their versions do
 * not move when an entry is added here.  Conventions of smirk_hip.h: device pointers, caller-owned memory, no allocation, copy or synchronisation inside, work
 * enqueued on `stream`, 0 = SMIRK_OK or a negative SMIRK_ERR_*; every refusal comes before the device is touched.
 */
#ifndef SMIRK_HANDOFF_H
#define SMIRK_HANDOFF_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_HANDOFF_ABI_VERSION 1

int smirk_handoff_abi_version(void);

/* What the chain rendered mask -> masking(img, hull_mask, None, 10, rendered_mask, _pmask=pmask) -> pack of cat(rendered_img, masked_img) computes, in one launch:
 *     masked_img [B][3][H][W] fp32            bit for bit the tensor of the separate launches (max pools of radius 10 and 5, patch centres and point noise drawn
 *                                             from the same Philox counters: field_offset and noise_offset are the offsets the Bernoulli field and the composition
 *                                             would have been handed)
 *     packed     [B][H][W][8] split-fp16      channels 0-2 rendered_img, 3-5 masked_img, 6-7 zero: bit for bit what the generator's own pack writes (32 bytes a pixel)
 * img, rendered_img [B][3][H][W]; pmask [B][H][W]; hull_mask [B][H][W] with hull_batch_stride = H * W, or ONE [H][W] mask shared by the batch with stride 0.
 * random_mask > 0 (the probability of a patch centre).  SMIRK_ERR_BAD_ARG: a NULL pointer, B, H or W <= 0, another stride, random_mask <= 0 or NaN.
 * SMIRK_ERR_UNSUPPORTED: rows too wide for two workgroups per CU (W above about 300), or a grid beyond 2^31 - 1: the caller keeps the separate launches. */
int smirk_masking_handoff(const float* img, const float* rendered_img, const float* hull_mask, long long hull_batch_stride, const float* pmask,
                          int B, int H, int W, float random_mask, uint64_t seed, uint64_t field_offset, uint64_t noise_offset, float* masked_img,
                          void* packed, void* stream);

/* The whole-network generator entry of smirk_hip.h with the packed tensor [B][H][W][8] (above) as its input and without the pack step: same schedule, same
 * workspace size, same output bits.  Split-fp16 weights only: SMIRK_ERR_BAD_ARG for any other precision, a NULL pointer or a shape the entry of smirk_hip.h
 * refuses; SMIRK_ERR_WORKSPACE as there.  `packed` is only read, and must stay untouched until the work enqueued here has run. */
int smirk_generator_forward_packed(const SmirkGeneratorWeights* w, const void* packed, float* y, int B, int H, int W, void* const* taps, void* ws,
                                   size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
