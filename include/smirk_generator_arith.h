/* smirk_generator_arith.h — extension table of libsmirk_hip.so for ONE query: which arithmetic every level of a whole-network generator entry
 * (smirk_generator_forward of smirk_hip.h, smirk_generator_forward_packed of smirk_handoff.h) runs in under the weights' precision.  It is answered by the
 * function the forward itself asks for every convolution it launches (gen_level_arith, csrc/network.hip), without touching device memory.
 * It is for tests and tools; nothing on the hot path calls it.
 *
 * It is versioned on its own (the version function below): the tables of smirk_hip.h, smirk_mica.h, smirk_emotion.h, smirk_optim.h, smirk_handoff.h and
 * smirk_generator_plan.h and their versions do not move when an entry is added here.
 */
#ifndef SMIRK_GENERATOR_ARITH_H
#define SMIRK_GENERATOR_ARITH_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_GENARITH_ABI_VERSION 1

int smirk_genarith_abi_version(void);

/* The arithmetic of every convolution of the generator, as SMIRK_PRECISION_* values.  Levels are indexed as in smirk_generator_plan.h: level l = 0..3 works at
 * H >> l x W >> l with features << l channels and holds both encoder convolutions, the ConvTranspose2d (or its composed form) and both decoder convolutions of
 * encoder l + 1 / decoder l + 1; `deep_arith` is the bottleneck and the ResNet blocks.  The arithmetic of a layer depends on its level and the weights' precision
 * only: never on the batch, the image size, the chain count, taps or a kernel switch.
 *   SMIRK_PRECISION_F32     every level F32
 *   SMIRK_PRECISION_F16X3   every level F16X3
 *   SMIRK_PRECISION_F16X1   levels l >= *x1_from and deep_arith F16X1 (one fp16 MFMA per product block on the hi halves, fp32 accumulation, the output written as
 *                           a full (hi, lo) pair); levels below F16X3, with exactly the launches of SMIRK_PRECISION_F16X3.  The final 1 x 1 convolution + sigmoid
 *                           belongs to level 0.
 * *x1_from is the library's compile-time constant (1) whatever the precision.  Only w->precision is read; no pointer of `w` is followed.
 * SMIRK_ERR_BAD_ARG for a NULL argument or a precision that is none of the three. */
int smirk_generator_arith(const SmirkGeneratorWeights* w, int32_t* x1_from, int32_t level_arith[4], int32_t* deep_arith);

#ifdef __cplusplus
}
#endif
#endif
