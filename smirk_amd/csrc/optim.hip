// The trainer's optimiser stage for MI355X (gfx950): clip_grad_norm_ (smirk_trainer.py:379) and the Adam steps (base_trainer.py:123-127) as four multi-tensor
// streaming kernels over two device tables and a chunk map (include/smirk_optim.h).  One workgroup of 256 threads = one chunk of SMIRK_OPTIM_CHUNK consecutive
// elements of one tensor; the workgroup reads its tensor's rows through scalar loads, so everything decided from them is uniform control flow.
//   optim_sumsq_partials   one float64 partial of sum g^2 per chunk: per lane in element order, a fixed butterfly across the wave, the four waves in wave order
//   optim_norm_finalise    one workgroup: the partials in float64 (thread t: t, t + 256, ... in index order, then the same tree); norm and coef in fp32
//   optim_scale            g *= coef
//   optim_adam             torch's non-capturable Adam; with grad_scale the clip rides in registers and the gradient in memory stays as it is
// A tensor whose pointers are all 16-byte aligned takes the vector path: four f32x4 per lane and array, every load of the chunk issued before the first use
// (16 loads in flight per lane in optim_adam).  Any other tensor takes the 4-byte path as a whole.  A chunk starts at a multiple of SMIRK_OPTIM_CHUNK elements
// of its tensor, so an aligned tensor's chunks are aligned.  The arithmetic is written per component on purpose: fp32 vector-typed expressions are what hipcc
// turns into packed-FP32 instructions (build.py).  This file is compiled with -ffp-contract=off: the only fused multiply-adds are the two torch has (optim_adam1).  The per-lane arithmetic of
// an element does not depend on the path it takes or on its neighbours, so one multi-tensor launch and one launch per tensor give the same bits.
// No scratch, no atomics, LDS for the reductions only; no kernel here writes split-fp16, and the launches do not bind the range flag.
#include <math.h>

#include "../../include/smirk_optim.h"
#include "common.h"

#define OPTIM_BLOCK 256
#define OPTIM_VECS (SMIRK_OPTIM_CHUNK / (4 * OPTIM_BLOCK))                          // f32x4 per lane, array and chunk
#define OPTIM_ITEMS (SMIRK_OPTIM_CHUNK / OPTIM_BLOCK)                               // elements per lane and chunk
static_assert(SMIRK_OPTIM_CHUNK % (4 * OPTIM_BLOCK) == 0 && OPTIM_VECS >= 1, "a chunk is a whole number of 16-byte vectors per lane");
static_assert(sizeof(SmirkOptimTensor) == 40 && sizeof(SmirkOptimStep) == 16, "table rows as include/smirk_optim.h states them");

// like SMIRK_LAUNCH without the range-flag binding: these kernels store no split-fp16
#define OPTIM_LAUNCH(kernel, grid, block, st, ...)                                        \
    do {                                                                                  \
        SmirkLaunchScope smirk_launch_scope_(#kernel, (hipStream_t)(st));                 \
        hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);                      \
    } while (0)

// The table rows are read from memory, so the compiler cannot know that the pointers in them are global: said here, or every access is a flat one.
typedef __attribute__((address_space(1))) float optim_gf32;
typedef __attribute__((address_space(1))) f32x4 optim_gf32x4;
__device__ __forceinline__ f32x4 optim_ld4(const float* p) { return *(const optim_gf32x4*)p; }
__device__ __forceinline__ void optim_st4(float* p, f32x4 v) { *(optim_gf32x4*)p = v; }
__device__ __forceinline__ float optim_ld1(const float* p) { return *(const optim_gf32*)p; }
__device__ __forceinline__ void optim_st1(float* p, float v) { *(optim_gf32*)p = v; }

__device__ __forceinline__ bool optim_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15u) == 0;
}

// What a workgroup owns: elements [e0, e0 + len) of its tensor, len >= 1 (a tensor without elements owns no chunk); nvec whole f32x4 of them, then
// len - 4 nvec < 4 scalar ones (only a tensor's last chunk has any).  Loads are never predicated: a lane whose item lies past the end reads the LAST item
// of the span instead (index clamped, inside the tensor) and drops it, so every load of the chunk is issued back to back; stores are predicated.
struct OptimSpan {
    long long e0;
    int len, nvec;
};
__device__ __forceinline__ OptimSpan optim_span(const SmirkOptimTensor& T, int chunk) {
    OptimSpan s;
    s.e0 = (long long)(chunk - T.first_chunk) * SMIRK_OPTIM_CHUNK;
    const long long left = T.numel - s.e0;
    s.len = left < SMIRK_OPTIM_CHUNK ? (int)(left > 0 ? left : 0) : SMIRK_OPTIM_CHUNK;
    s.nvec = s.len >> 2;
    return s;
}

// sum over the workgroup in a fixed order; valid in thread 0
__device__ __forceinline__ double optim_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(OPTIM_BLOCK) void optim_sumsq_partials(const SmirkOptimTensor* __restrict__ tensors, const SmirkOptimStep* __restrict__ steps,
                                                                     const int* __restrict__ chunk_map, double* __restrict__ partials) {
    __shared__ double red[OPTIM_BLOCK / 64];
    const int chunk = blockIdx.x, t = chunk_map[chunk];
    const SmirkOptimTensor T = tensors[t];
    const OptimSpan s = optim_span(T, chunk);
    const float* g = steps[t].grad + s.e0;
    const int tid = threadIdx.x;
    double acc = 0.0;
    if (s.len > 0) {
        if (optim_aligned16(g)) {
            if (s.nvec > 0) {
                f32x4 v[OPTIM_VECS];
#pragma unroll
                for (int i = 0; i < OPTIM_VECS; ++i) v[i] = optim_ld4(g + 4 * min(i * OPTIM_BLOCK + tid, s.nvec - 1));
#pragma unroll
                for (int i = 0; i < OPTIM_VECS; ++i) {
                    const double k = i * OPTIM_BLOCK + tid < s.nvec ? 1.0 : 0.0;       // an exact factor: a dropped item adds +0
                    acc += k * ((double)v[i].x * (double)v[i].x); acc += k * ((double)v[i].y * (double)v[i].y);
                    acc += k * ((double)v[i].z * (double)v[i].z); acc += k * ((double)v[i].w * (double)v[i].w);
                }
            }
            const int e = 4 * s.nvec + tid;
            if (e < s.len && tid < 4) { const double x = (double)optim_ld1(g + e); acc += x * x; }
        } else {
            float v[OPTIM_ITEMS];
#pragma unroll
            for (int i = 0; i < OPTIM_ITEMS; ++i) v[i] = optim_ld1(g + min(i * OPTIM_BLOCK + tid, s.len - 1));
#pragma unroll
            for (int i = 0; i < OPTIM_ITEMS; ++i) acc += (i * OPTIM_BLOCK + tid < s.len ? 1.0 : 0.0) * ((double)v[i] * (double)v[i]);
        }
    }
    const double sum = optim_block_sum(acc, red);
    if (tid == 0) partials[chunk] = sum;
}

__global__ __launch_bounds__(OPTIM_BLOCK) void optim_norm_finalise(const double* __restrict__ partials, int n_partials, float max_norm, float* __restrict__ norm_coef) {
    __shared__ double red[OPTIM_BLOCK / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += OPTIM_BLOCK) acc += partials[i];
    const double sum = optim_block_sum(acc, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(sum);
        const float c = max_norm / (norm + 1e-6f);
        norm_coef[0] = norm;
        norm_coef[1] = c > 1.0f ? 1.0f : c;                                        // a NaN stays a NaN, as in torch.clamp(max=1.0)
    }
}

__global__ __launch_bounds__(OPTIM_BLOCK) void optim_scale(const SmirkOptimTensor* __restrict__ tensors, const SmirkOptimStep* __restrict__ steps,
                                                            const int* __restrict__ chunk_map, const float* __restrict__ coef_ptr) {
    const int chunk = blockIdx.x, t = chunk_map[chunk];
    const SmirkOptimTensor T = tensors[t];
    const OptimSpan s = optim_span(T, chunk);
    float* g = steps[t].grad + s.e0;
    const float coef = *coef_ptr;
    const int tid = threadIdx.x;
    if (s.len <= 0) return;
    if (optim_aligned16(g)) {
        if (s.nvec > 0) {
            f32x4 v[OPTIM_VECS];
#pragma unroll
            for (int i = 0; i < OPTIM_VECS; ++i) v[i] = optim_ld4(g + 4 * min(i * OPTIM_BLOCK + tid, s.nvec - 1));
#pragma unroll
            for (int i = 0; i < OPTIM_VECS; ++i) {
                const int q = i * OPTIM_BLOCK + tid;
                f32x4 o;
                o.x = v[i].x * coef; o.y = v[i].y * coef; o.z = v[i].z * coef; o.w = v[i].w * coef;
                if (q < s.nvec) optim_st4(g + 4 * q, o);
            }
        }
        const int e = 4 * s.nvec + tid;
        if (e < s.len && tid < 4) optim_st1(g + e, optim_ld1(g + e) * coef);
    } else {
        float v[OPTIM_ITEMS];
#pragma unroll
        for (int i = 0; i < OPTIM_ITEMS; ++i) v[i] = optim_ld1(g + min(i * OPTIM_BLOCK + tid, s.len - 1));
#pragma unroll
        for (int i = 0; i < OPTIM_ITEMS; ++i) {
            const int e = i * OPTIM_BLOCK + tid;
            if (e < s.len) optim_st1(g + e, v[i] * coef);
        }
    }
}

struct OptimAdamArgs {
    float w1, one_minus_w1, beta2, w2, eps;                                        // 1 - beta1, beta2, 1 - beta2, eps: each rounded once from double precision
};

// One element, operation for operation what torch's fp32 kernels compute (checked bit for bit against torch.optim.Adam(foreach=False) on the CPU, tests/optim_law.py):
//   exp_avg.lerp_(g, w)               w < 0.5 ? fma(w, g - m, m) : fma(-(g - m), 1 - w, g)      ATen's lerp, both forms fused
//   exp_avg_sq.mul_(b2).addcmul_      fma(w2 * g, g, v * b2)                                    the product (w2 g) g fused into the sum
//   denom = sqrt(v) / bc2_sqrt + eps  a true division and a correctly rounded square root (hipcc's defaults; HIP's __fsqrt_rn is the approximate one)
//   param.addcdiv_(m, denom, -ss)     p + (-ss * m) / denom
// The two fused multiply-adds are written out; this file is compiled with -ffp-contract=off, so the compiler fuses nothing else.  Without them (every product
// rounded on its own) exp_avg_sq sits 1.8 x and exp_avg 1.1 x the tests' bound away from the float64 law: the reference itself rounds once there.
__device__ __forceinline__ void optim_adam1(float& p, float g, float& m, float& v, const OptimAdamArgs a, float neg_step_size, float bc2_sqrt) {
    const float d = g - m;
    m = a.w1 < 0.5f ? fmaf(a.w1, d, m) : fmaf(-d, a.one_minus_w1, g);
    v = fmaf(a.w2 * g, g, v * a.beta2);
    const float denom = sqrtf(v) / bc2_sqrt + a.eps;
    p = p + (neg_step_size * m) / denom;
}

__global__ __launch_bounds__(OPTIM_BLOCK) void optim_adam(const SmirkOptimTensor* __restrict__ tensors, const SmirkOptimStep* __restrict__ steps,
                                                           const int* __restrict__ chunk_map, OptimAdamArgs a, const float* __restrict__ grad_scale) {
    const int chunk = blockIdx.x, t = chunk_map[chunk];
    const SmirkOptimTensor T = tensors[t];
    const SmirkOptimStep S = steps[t];
    const OptimSpan s = optim_span(T, chunk);
    float* P = T.param + s.e0;
    float* M = T.exp_avg + s.e0;
    float* V = T.exp_avg_sq + s.e0;
    const float* G = S.grad + s.e0;
    const float gs = grad_scale ? *grad_scale : 1.0f;                              // g * 1.0f is g: one kernel serves both forms with the same bits
    const float nss = -S.step_size, bc = S.bias_correction2_sqrt;
    const int tid = threadIdx.x;
    if (s.len <= 0) return;
    if (optim_aligned16(P, M, V, G)) {
        if (s.nvec > 0) {
            f32x4 p[OPTIM_VECS], g[OPTIM_VECS], m[OPTIM_VECS], v[OPTIM_VECS];
#pragma unroll
            for (int i = 0; i < OPTIM_VECS; ++i) {
                const int q = 4 * min(i * OPTIM_BLOCK + tid, s.nvec - 1);
                g[i] = optim_ld4(G + q); m[i] = optim_ld4(M + q); v[i] = optim_ld4(V + q); p[i] = optim_ld4(P + q);
            }
#pragma unroll
            for (int i = 0; i < OPTIM_VECS; ++i) {
                const int q = i * OPTIM_BLOCK + tid;
                float px = p[i].x, py = p[i].y, pz = p[i].z, pw = p[i].w, mx = m[i].x, my = m[i].y, mz = m[i].z, mw = m[i].w;
                float vx = v[i].x, vy = v[i].y, vz = v[i].z, vw = v[i].w;
                optim_adam1(px, g[i].x * gs, mx, vx, a, nss, bc); optim_adam1(py, g[i].y * gs, my, vy, a, nss, bc);
                optim_adam1(pz, g[i].z * gs, mz, vz, a, nss, bc); optim_adam1(pw, g[i].w * gs, mw, vw, a, nss, bc);
                if (q < s.nvec) {
                    optim_st4(M + 4 * q, f32x4{mx, my, mz, mw});
                    optim_st4(V + 4 * q, f32x4{vx, vy, vz, vw});
                    optim_st4(P + 4 * q, f32x4{px, py, pz, pw});
                }
            }
        }
        const int e = 4 * s.nvec + tid;
        if (e < s.len && tid < 4) {
            float pp = optim_ld1(P + e), mm = optim_ld1(M + e), vv = optim_ld1(V + e);
            optim_adam1(pp, optim_ld1(G + e) * gs, mm, vv, a, nss, bc);
            optim_st1(M + e, mm); optim_st1(V + e, vv); optim_st1(P + e, pp);
        }
    } else {
        // four elements per lane at a time (16 loads in flight): the 4-byte path is for the odd view, not for the bulk
#pragma unroll 1
        for (int i0 = 0; i0 < OPTIM_ITEMS && i0 * OPTIM_BLOCK < s.len; i0 += 4) {
            float p[4], g[4], m[4], v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = min((i0 + i) * OPTIM_BLOCK + tid, s.len - 1);
                g[i] = optim_ld1(G + e); m[i] = optim_ld1(M + e); v[i] = optim_ld1(V + e); p[i] = optim_ld1(P + e);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = (i0 + i) * OPTIM_BLOCK + tid;
                optim_adam1(p[i], g[i] * gs, m[i], v[i], a, nss, bc);
                if (e < s.len) { optim_st1(M + e, m[i]); optim_st1(V + e, v[i]); optim_st1(P + e, p[i]); }
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------------
static inline long long optim_chunks(long long numel) { return (numel + SMIRK_OPTIM_CHUNK - 1) / SMIRK_OPTIM_CHUNK; }
static inline bool optim_bad_f32_ptr(const void* p) { return !p || ((uintptr_t)p & 3u) != 0; }
static const int OPTIM_ALL_KINDS = SMIRK_OPTIM_KIND_NORM | SMIRK_OPTIM_KIND_SCALE | SMIRK_OPTIM_KIND_ADAM;

extern "C" int smirk_optim_abi_version(void) { return SMIRK_OPTIM_ABI_VERSION; }

extern "C" int smirk_optim_plan(SmirkOptimTensor* tensors, const SmirkOptimStep* steps, int n, int kinds, long long* total_chunks) {
    if (!tensors || !total_chunks || n <= 0 || kinds == 0 || (kinds & ~OPTIM_ALL_KINDS)) return SMIRK_ERR_BAD_ARG;
    const bool adam = (kinds & SMIRK_OPTIM_KIND_ADAM) != 0;
    for (int k = 0; k < n; ++k) {
        const SmirkOptimTensor& t = tensors[k];
        if (t.numel < 0) return SMIRK_ERR_BAD_ARG;
        if (t.numel > 0) {
            if (adam && (optim_bad_f32_ptr(t.param) || optim_bad_f32_ptr(t.exp_avg) || optim_bad_f32_ptr(t.exp_avg_sq))) return SMIRK_ERR_BAD_ARG;
            if (steps && optim_bad_f32_ptr(steps[k].grad)) return SMIRK_ERR_BAD_ARG;
        }
        if (steps && adam) {
            const float ss = steps[k].step_size, bc = steps[k].bias_correction2_sqrt;
            if (!(ss >= 0.0f) || !std::isfinite(ss) || !(bc > 0.0f) || !std::isfinite(bc)) return SMIRK_ERR_BAD_ARG;
        }
    }
    long long chunk = 0;
    for (int k = 0; k < n; ++k) {
        if (tensors[k].numel >= (1LL << 31)) return SMIRK_ERR_UNSUPPORTED;
        if (chunk + optim_chunks(tensors[k].numel) > (long long)INT32_MAX) return SMIRK_ERR_UNSUPPORTED;
        chunk += optim_chunks(tensors[k].numel);
    }
    chunk = 0;
    for (int k = 0; k < n; ++k) {                                                  // nothing is written before every refusal has had its say
        tensors[k].first_chunk = (int)chunk;
        chunk += optim_chunks(tensors[k].numel);
    }
    *total_chunks = chunk;
    return SMIRK_OK;
}

extern "C" int smirk_optim_chunk_map(const SmirkOptimTensor* tensors, int n, int* map, long long total_chunks) {
    if (!tensors || n <= 0 || total_chunks < 0 || total_chunks > (long long)INT32_MAX || (!map && total_chunks > 0)) return SMIRK_ERR_BAD_ARG;
    long long chunk = 0;
    for (int k = 0; k < n; ++k) {
        if (tensors[k].numel < 0 || tensors[k].numel >= (1LL << 31) || tensors[k].first_chunk != chunk) return SMIRK_ERR_BAD_ARG;
        chunk += optim_chunks(tensors[k].numel);
        if (chunk > total_chunks) return SMIRK_ERR_BAD_ARG;
    }
    if (chunk != total_chunks) return SMIRK_ERR_BAD_ARG;
    for (int k = 0; k < n; ++k) {
        const long long c1 = tensors[k].first_chunk + optim_chunks(tensors[k].numel);
        for (long long c = tensors[k].first_chunk; c < c1; ++c) map[c] = k;
    }
    return SMIRK_OK;
}

// what every launch entry can check of its tables: they live on the device
static int optim_check_tables(const void* tensors, const void* steps, const void* map, int n, long long total_chunks) {
    if (!tensors || !steps || n <= 0 || total_chunks < 0 || (!map && total_chunks > 0)) return SMIRK_ERR_BAD_ARG;
    if (((uintptr_t)tensors & 7u) || ((uintptr_t)steps & 7u) || ((uintptr_t)map & 3u)) return SMIRK_ERR_BAD_ARG;
    if (total_chunks > (long long)INT32_MAX) return SMIRK_ERR_UNSUPPORTED;
    return SMIRK_OK;
}

extern "C" size_t smirk_optim_grad_norm_workspace_bytes(long long total_chunks) {
    if (total_chunks < 0 || total_chunks > (long long)INT32_MAX) return 0;
    return smirk_align_up((size_t)(total_chunks > 0 ? total_chunks : 1) * sizeof(double), 256);
}

extern "C" int smirk_optim_grad_norm(const SmirkOptimTensor* tensors, const SmirkOptimStep* steps, const int* chunk_map, int n, long long total_chunks, float max_norm,
                                     void* partials_ws, size_t ws_bytes, float* norm_coef_out, void* stream) {
    const int bad = optim_check_tables(tensors, steps, chunk_map, n, total_chunks);
    if (bad != SMIRK_OK) return bad;
    if (!partials_ws || ((uintptr_t)partials_ws & 7u) || optim_bad_f32_ptr(norm_coef_out)) return SMIRK_ERR_BAD_ARG;
    if (!std::isfinite(max_norm) || max_norm < 0.0f) return SMIRK_ERR_BAD_ARG;
    if (ws_bytes < smirk_optim_grad_norm_workspace_bytes(total_chunks)) return SMIRK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double* partials = (double*)partials_ws;
    if (total_chunks > 0) {
        smirk_prof_next(nullptr, 0.0, (double)total_chunks * (SMIRK_OPTIM_CHUNK * sizeof(float) + sizeof(double)));     // an upper bound: last chunks are partial
        OPTIM_LAUNCH(optim_sumsq_partials, dim3((unsigned)total_chunks), dim3(OPTIM_BLOCK), st, tensors, steps, chunk_map, partials);
    }
    smirk_prof_next(nullptr, 0.0, (double)total_chunks * sizeof(double) + 2 * sizeof(float));
    OPTIM_LAUNCH(optim_norm_finalise, dim3(1), dim3(OPTIM_BLOCK), st, (const double*)partials, (int)total_chunks, max_norm, norm_coef_out);
    return smirk_launch_status();
}

extern "C" int smirk_optim_scale_grads(const SmirkOptimTensor* tensors, const SmirkOptimStep* steps, const int* chunk_map, int n, long long total_chunks,
                                       const float* coef, void* stream) {
    const int bad = optim_check_tables(tensors, steps, chunk_map, n, total_chunks);
    if (bad != SMIRK_OK) return bad;
    if (optim_bad_f32_ptr(coef)) return SMIRK_ERR_BAD_ARG;
    if (total_chunks == 0) return SMIRK_OK;
    smirk_prof_next(nullptr, 0.0, (double)total_chunks * SMIRK_OPTIM_CHUNK * 2 * sizeof(float));
    OPTIM_LAUNCH(optim_scale, dim3((unsigned)total_chunks), dim3(OPTIM_BLOCK), (hipStream_t)stream, tensors, steps, chunk_map, coef);
    return smirk_launch_status();
}

extern "C" int smirk_optim_adam_step(const SmirkOptimTensor* tensors, const SmirkOptimStep* steps, const int* chunk_map, int n, long long total_chunks, double beta1,
                                     double beta2, double eps, const float* grad_scale, void* stream) {
    const int bad = optim_check_tables(tensors, steps, chunk_map, n, total_chunks);
    if (bad != SMIRK_OK) return bad;
    if (!std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps)) return SMIRK_ERR_BAD_ARG;
    if (beta1 < 0.0 || beta1 >= 1.0 || beta2 < 0.0 || beta2 >= 1.0 || eps < 0.0) return SMIRK_ERR_BAD_ARG;
    if (grad_scale && ((uintptr_t)grad_scale & 3u)) return SMIRK_ERR_BAD_ARG;
    if (total_chunks == 0) return SMIRK_OK;
    OptimAdamArgs a;
    a.w1 = (float)(1.0 - beta1); a.one_minus_w1 = 1.0f - a.w1; a.beta2 = (float)beta2; a.w2 = (float)(1.0 - beta2); a.eps = (float)eps;
    smirk_prof_next(nullptr, 0.0, (double)total_chunks * SMIRK_OPTIM_CHUNK * 7 * sizeof(float));
    OPTIM_LAUNCH(optim_adam, dim3((unsigned)total_chunks), dim3(OPTIM_BLOCK), (hipStream_t)stream, tensors, steps, chunk_map, a, grad_scale);
    return smirk_launch_status();
}
