/* smirk_optim.h — extension table of libsmirk_hip.so for the trainer's optimiser stage (reference: smirk_trainer.py:378-382, base_trainer.py:51,62,123-127):
 *   torch.nn.utils.clip_grad_norm_(parameters, max_norm)   the global L2 norm of a list of gradients and the clip by coef = min(1, max_norm / (norm + 1e-6))
 *   torch.optim.Adam.step()                                torch's non-capturable Adam (no weight decay, no amsgrad), element-wise in fp32
 *
 * All four kernels are multi-tensor: ONE launch walks a whole list of tensors.  The list is two device tables of n rows, a static one (SmirkOptimTensor: what
 * stays the same from step to step) and a per-step one (SmirkOptimStep: the gradient pointers, which autograd re-allocates after zero_grad(), and Adam's two
 * per-tensor scalars), plus a chunk map: one workgroup of 256 threads handles one chunk of SMIRK_OPTIM_CHUNK consecutive elements of one tensor, and
 * chunk_map[chunk] is that tensor's row.  The chunk layout depends on the element counts alone (smirk_optim_plan), never on the device.
 *
 * It is versioned on its own (smirk_optim_abi_version): the tables of smirk_hip.h, smirk_mica.h and smirk_emotion.h and their versions do not move when an
 * entry is added here.  Conventions of smirk_hip.h: device pointers (the *_host arguments excepted), caller-owned memory, no allocation, copy or
 * synchronisation inside, work enqueued on `stream`, 0 = SMIRK_OK or a negative SMIRK_ERR_*; every refusal comes before the device is touched.  The tables
 * live on the device, so the launch entries cannot see the tensor pointers: smirk_optim_plan validates them on the host copy.
 *
 * Alignment: fp32 tensors are 4-byte aligned and nothing more is required.  A tensor whose pointers (those the kernel uses) are all 16-byte aligned is
 * streamed with 16-byte loads and stores; any other tensor — a view at an odd storage offset, restored optimiser state — runs a 4-byte path as a whole.
 * The choice is made per tensor from its table row, in workgroup-uniform control flow.  Tails (numel % 4, the last partial chunk) are scalar and bounds-checked.
 * No entry uses scratch memory or float atomics; every sum has one order, fixed by the element counts, so two runs agree bit for bit.  No entry writes the
 * split-fp16 format or touches its range flag.
 */
#ifndef SMIRK_OPTIM_H
#define SMIRK_OPTIM_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_OPTIM_ABI_VERSION 1
#define SMIRK_OPTIM_CHUNK 4096       /* elements per workgroup; a multiple of 4 (1024 would be the smallest that keeps a 16-byte access per lane) */
enum { SMIRK_OPTIM_KIND_NORM = 1, SMIRK_OPTIM_KIND_SCALE = 2, SMIRK_OPTIM_KIND_ADAM = 4 };   /* `kinds` of smirk_optim_plan: which entries the tables will be handed to */

typedef struct SmirkOptimTensor {    /* static row: 40 bytes */
    float* param;                    /* fp32 [numel]; ADAM only */
    float* exp_avg;                  /* fp32 [numel]; ADAM only */
    float* exp_avg_sq;               /* fp32 [numel]; ADAM only */
    long long numel;                 /* 0 is legal: the tensor owns no chunk */
    int first_chunk;                 /* filled by smirk_optim_plan: the tensor owns chunks [first_chunk, first_chunk + ceil(numel / SMIRK_OPTIM_CHUNK)) */
    int _pad;
} SmirkOptimTensor;

typedef struct SmirkOptimStep {      /* per-step row: 16 bytes */
    float* grad;                     /* fp32 [numel]; read by NORM and ADAM, scaled in place by SCALE */
    float step_size;                 /* ADAM: lr / (1 - beta1^t), computed in double precision from the tensor's OWN step count t and rounded to fp32 */
    float bias_correction2_sqrt;     /* ADAM: sqrt(1 - beta2^t), likewise */
} SmirkOptimStep;

int smirk_optim_abi_version(void);

/* Pure host: validates host copies of the two tables and fills first_chunk; never touches the device.  steps_host may be NULL when the gradient pointers are
 * not known yet (only the static rows are checked then).  SMIRK_ERR_BAD_ARG: tensors_host or total_chunks NULL, n <= 0, kinds 0 or with unknown bits, a
 * negative numel, a pointer that `kinds` needs (ADAM: param, exp_avg, exp_avg_sq; any kind: grad when steps_host is given) NULL on a tensor with elements or
 * not 4-byte aligned; under ADAM with steps_host, a step_size that is negative or not finite, a bias_correction2_sqrt that is not finite and positive.  SMIRK_ERR_UNSUPPORTED: a tensor of 2^31 elements or
 * more, more than 2^31 - 1 chunks. */
int smirk_optim_plan(SmirkOptimTensor* tensors_host, const SmirkOptimStep* steps_host, int n, int kinds, long long* total_chunks);
/* Pure host: map_host[c] = row of the tensor that owns chunk c, for the first_chunk values smirk_optim_plan filled; total_chunks as it returned them
 * (anything else is SMIRK_ERR_BAD_ARG). */
int smirk_optim_chunk_map(const SmirkOptimTensor* tensors_host, int n, int* map_host, long long total_chunks);

/* clip_grad_norm_, first half.  optim_sumsq_partials: one float64 partial sum of g^2 per chunk (per lane in element order, a fixed butterfly across the wave,
 * the four waves in wave order).  optim_norm_finalise: one workgroup adds the partials in float64 (thread t takes partials t, t + 256, ... in index order,
 * then the same tree), and writes norm_coef_out[0] = norm (the float64 sum's square root, rounded once to fp32) and norm_coef_out[1] = coef =
 * min(1, max_norm / (norm + 1e-6)) in fp32: one add, one division, one clamp; a NaN norm gives a NaN coef, like torch.clamp.  Two launches (one when
 * total_chunks is 0: norm 0, coef 1).  partials_ws: 8-byte aligned, smirk_optim_grad_norm_workspace_bytes(total_chunks) bytes (SMIRK_ERR_WORKSPACE below).
 * max_norm must be finite and >= 0. */
size_t smirk_optim_grad_norm_workspace_bytes(long long total_chunks);
int smirk_optim_grad_norm(const SmirkOptimTensor* tensors_device, const SmirkOptimStep* steps_device, const int* chunk_map_device, int n, long long total_chunks,
                          float max_norm, void* partials_ws, size_t ws_bytes, float* norm_coef_out, void* stream);
/* clip_grad_norm_, second half: g *= *coef_device in place (one rounding per element).  One launch, none when total_chunks is 0. */
int smirk_optim_scale_grads(const SmirkOptimTensor* tensors_device, const SmirkOptimStep* steps_device, const int* chunk_map_device, int n, long long total_chunks,
                            const float* coef_device, void* stream);

/* One Adam step of every tensor of the tables (one parameter group), per element in fp32, operation for operation what torch's fp32 kernels compute
 * (w = 1 - beta1):
 *     g       = grad * *grad_scale_device           only when grad_scale_device != NULL; the gradient in memory is not rewritten (the fused clip)
 *     exp_avg     = w < 0.5 ? fma(w, g - exp_avg, exp_avg) : fma(-(g - exp_avg), 1 - w, g)          ATen's lerp
 *     exp_avg_sq  = fma((1 - beta2) * g, g, exp_avg_sq * beta2)                                     mul_ and addcmul_
 *     denom   = sqrt(exp_avg_sq) / bias_correction2_sqrt + eps          a true division, as torch's CPU kernels do it (torch's GPU kernels multiply by the
 *     param  += (-step_size * exp_avg) / denom                          fp32 reciprocal of the scalar: one more rounding)
 * Every other product, quotient and sum is rounded on its own: the two fused multiply-adds are the ones torch's kernels have, and with them the result equals
 * torch.optim.Adam(foreach=False) on the CPU bit for bit on the test inputs (tests/optim_law.py).  1 - beta1, beta2, 1 - beta2 and eps are taken in double
 * precision and rounded to fp32 once, as torch rounds the Python scalars it is handed.
 * SMIRK_ERR_BAD_ARG: beta1 or beta2 outside [0, 1), eps < 0, any of them not finite.  One launch, none when total_chunks is 0. */
int smirk_optim_adam_step(const SmirkOptimTensor* tensors_device, const SmirkOptimStep* steps_device, const int* chunk_map_device, int n, long long total_chunks,
                          double beta1, double beta2, double eps, const float* grad_scale_device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
