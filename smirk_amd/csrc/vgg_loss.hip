// Perceptual (VGG-16) term of the trainer's first path for MI355X (gfx950): everything AROUND the ten convolutions of src/losses/VGGPerceptualLoss.py:23-47
// (smirk_trainer.py:104).  The convolutions, their data gradients and the pools are the existing entries (conv.hip, wgrad.hip, train.hip); this unit holds
//   vgg_prepare_kernel            x, y NCHW fp32 -> ONE split16 NHWC tensor [2B][H][W][8]: the affine map of :24-27 in fp32, NCHW -> NHWC, channel padding and the
//                                 split in one pass; the range audit in its NaN-catching form (these values come from outside the library)
//   vgg_prepare_backward_kernel   d [B][H][W][8] split16 -> dx [B][3][H][W] fp32 = d_c / std_c * 0.5 (autograd's own order of the two operations)
//   vgg_l1_partial_kernel         one workgroup per chunk of SMIRK_VGG_L1_CHUNK 8-channel groups of a half of a tapped feature tensor: d = fx - fy in fp32 from the
//                                 decoded pairs (exact), |d| summed in float64 per thread in group order, across the wave by a fixed butterfly, across the four
//                                 waves in wave order.  The chunk -> partial mapping depends on the shapes only, never on the CU count; no atomics.
//   vgg_l1_finalise_kernel        one wave per tap: every lane adds a strided share of the tap's partials in index order, the wave combines them by the same
//                                 butterfly (a fixed tree over all lanes: one lane walking 6272 partials at B = 64 is the serial form DESIGN §14 measured), divides
//                                 by the element count and stores the fp32 term; thread 0 adds the unrounded terms in float64 and rounds once.
//   vgg_relu_tap_backward_kernel  dz = (d_in + g * coef * sign(fx - fy)) * [fx > 0] on a tapped layer, dz = d_in * [fx > 0] elsewhere: one kernel, the mode is
//                                 a kernel-uniform branch on fy.  16-byte loads of the hi and lo halves, eight values per thread in registers.
// Gradient scale: coef = 1 / numel(tap) is 3e-7 .. 1e-5 for ONE 224 x 224 image and 64 times smaller at B = 64, far inside fp16's subnormal range, where a
// split16 pair keeps an absolute resolution of 2^-35 only (1e-4 of such a value, 6e-3 at B = 64).  The backward is linear, so the caller multiplies the injected
// term by a power of two (`scale` of the tap kernel) and divides it out, exactly, in vgg_prepare_backward_kernel.
// All of them are bandwidth-class: no LDS beyond the 32-byte reduction scratch, no MFMA.
#include <limits.h>

#include "conv_common.h"

#define VGG_BLOCK 256
#define VGG_L1_ITEMS (SMIRK_VGG_L1_CHUNK / VGG_BLOCK)                              // groups per thread and chunk
static_assert(SMIRK_VGG_L1_CHUNK % VGG_BLOCK == 0, "a chunk is a whole number of groups per thread");

__global__ __launch_bounds__(VGG_BLOCK) void vgg_prepare_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ mean,
                                                                const float* __restrict__ sd, float* __restrict__ out, int B, int HW) {
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2], s0 = sd[0], s1 = sd[1], s2 = sd[2];
    const size_t total = (size_t)2 * B * HW;
    for (size_t i = (size_t)blockIdx.x * VGG_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * VGG_BLOCK) {
        const size_t b2 = i / HW, p = i - b2 * HW;
        const float* src = b2 < (size_t)B ? x + b2 * 3 * HW + p : y + (b2 - B) * 3 * HW + p;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        v[0] = (fmaf(src[0], 0.5f, 0.5f) - m0) / s0;                               // 0.5 v is exact, so the fused form rounds where `v * 0.5 + 0.5` does
        v[1] = (fmaf(src[HW], 0.5f, 0.5f) - m1) / s1;
        v[2] = (fmaf(src[2 * (size_t)HW], 0.5f, 0.5f) - m2) / s2;
        smirk_range_audit1(v[0]); smirk_range_audit1(v[1]); smirk_range_audit1(v[2]);
        half8 hi, lo;
        split8_noaudit(v, hi, lo);
        *(half8*)(out + i * 8) = hi;
        *(half8*)(out + i * 8 + 4) = lo;
    }
}

__global__ __launch_bounds__(VGG_BLOCK) void vgg_prepare_backward_kernel(const float* __restrict__ d, const float* __restrict__ sd, float* __restrict__ dx, int B,
                                                                         int HW, float half_scale) {
    const float s0 = sd[0], s1 = sd[1], s2 = sd[2];
    const size_t total = (size_t)B * HW;
    for (size_t i = (size_t)blockIdx.x * VGG_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * VGG_BLOCK) {
        const size_t b = i / HW, p = i - b * HW;
        const half8 hi = *(const half8*)(d + i * 8), lo = *(const half8*)(d + i * 8 + 4);
        float* o = dx + b * 3 * HW + p;
        o[0] = join1(hi[0], lo[0]) / s0 * half_scale;
        o[HW] = join1(hi[1], lo[1]) / s1 * half_scale;
        o[2 * (size_t)HW] = join1(hi[2], lo[2]) / s2 * half_scale;
    }
}

// sum over the workgroup in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double vgg_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(VGG_BLOCK) void vgg_l1_partial_kernel(const float* __restrict__ f, size_t half_groups, double* __restrict__ partials) {
    __shared__ double red[VGG_BLOCK / 64];
    const size_t g0 = (size_t)blockIdx.x * SMIRK_VGG_L1_CHUNK + threadIdx.x;
    const float* fy = f + half_groups * 8;
    double acc = 0.0;
#pragma unroll 2
    for (int i = 0; i < VGG_L1_ITEMS; ++i) {
        const size_t g = g0 + (size_t)i * VGG_BLOCK;
        if (g >= half_groups) break;
        const half8 xh = *(const half8*)(f + g * 8), xl = *(const half8*)(f + g * 8 + 4);
        const half8 yh = *(const half8*)(fy + g * 8), yl = *(const half8*)(fy + g * 8 + 4);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += (double)fabsf(join1(xh[q], xl[q]) - join1(yh[q], yl[q]));
    }
    acc = vgg_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

struct VggL1Args {
    long long half_elems[SMIRK_VGG_TAPS];
    int chunk0[SMIRK_VGG_TAPS + 1];                                                // first partial of each tap; chunk0[n] = their total number
    int n;
};

__global__ __launch_bounds__(64 * SMIRK_VGG_TAPS) void vgg_l1_finalise_kernel(VggL1Args a, const double* __restrict__ partials, float* __restrict__ out_terms,
                                                                              float* __restrict__ out_total) {
    __shared__ double term[SMIRK_VGG_TAPS];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (k < a.n) {                                                                 // wave-uniform
        double s = 0.0;
        for (int c = a.chunk0[k] + lane; c < a.chunk0[k + 1]; c += 64) s += partials[c];
        s = vgg_wave_sum(s);
        if (lane == 0) {
            const double v = s / (double)a.half_elems[k];
            term[k] = v;
            out_terms[k] = (float)v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int j = 0; j < a.n; ++j) tot += term[j];
        *out_total = (float)tot;
    }
}

__global__ __launch_bounds__(VGG_BLOCK) void vgg_relu_tap_backward_kernel(const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ d_in,
                                                                          const float* __restrict__ grad_total, float coef, float* __restrict__ dz, size_t ng) {
    const float gc = fy ? grad_total[0] * coef : 0.f;
    for (size_t i = (size_t)blockIdx.x * VGG_BLOCK + threadIdx.x; i < ng; i += (size_t)gridDim.x * VGG_BLOCK) {
        const half8 xh = *(const half8*)(fx + i * 8), xl = *(const half8*)(fx + i * 8 + 4);
        float v[8];
        if (d_in) {
            const half8 dh = *(const half8*)(d_in + i * 8), dl = *(const half8*)(d_in + i * 8 + 4);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = join1(dh[q], dl[q]);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = 0.f;
        }
        if (fy) {
            const half8 yh = *(const half8*)(fy + i * 8), yl = *(const half8*)(fy + i * 8 + 4);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float a = join1(xh[q], xl[q]), df = a - join1(yh[q], yl[q]);
                const float s = df > 0.f ? gc : df < 0.f ? -gc : 0.f;              // sign(0) = 0, like torch's l1_loss backward
                v[q] = a > 0.f ? v[q] + s : 0.f;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = join1(xh[q], xl[q]) > 0.f ? v[q] : 0.f;
        }
        half8 hi, lo;
        split8(v, hi, lo);
        *(half8*)(dz + i * 8) = hi;
        *(half8*)(dz + i * 8 + 4) = lo;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------------
static inline bool vgg_scale_ok(float s) { return s > 0.f && s <= 3.0e38f; }       // positive and finite (NaN fails both)
static inline bool vgg_bad_ptr(const void* p) { return !p || ((uintptr_t)p & 15u) != 0; }
static inline unsigned vgg_grid(size_t total) { const size_t g = (total + VGG_BLOCK - 1) / VGG_BLOCK; return (unsigned)(g > 16384 ? 16384 : (g ? g : 1)); }
static inline long long vgg_chunks(long long half_elems) { return (half_elems / 8 + SMIRK_VGG_L1_CHUNK - 1) / SMIRK_VGG_L1_CHUNK; }

static int vgg_prepare_validate(const void* a, const void* b, int B, int H, int W) {
    if (vgg_bad_ptr(a) || vgg_bad_ptr(b) || B < 1 || H < 1 || W < 1) return SMIRK_ERR_BAD_ARG;
    if (!conv_fits32((long long)2 * B * H * W * 8)) return SMIRK_ERR_UNSUPPORTED;
    return SMIRK_OK;
}

extern "C" int smirk_vgg_prepare_split16(const float* x, const float* y, const float* mean, const float* std, void* out, int B, int H, int W, void* stream) {
    if (!mean || !std || vgg_bad_ptr(out)) return SMIRK_ERR_BAD_ARG;
    const int bad = vgg_prepare_validate(x, y, B, H, W);
    if (bad != SMIRK_OK) return bad;
    const size_t px = (size_t)2 * B * H * W;
    smirk_prof_next(nullptr, 0.0, (double)px * (3 * 4 + 32));
    SMIRK_LAUNCH(vgg_prepare_kernel, dim3(vgg_grid(px)), dim3(VGG_BLOCK), 0, (hipStream_t)stream, x, y, mean, std, (float*)out, B, H * W);
    return smirk_launch_status();
}

extern "C" int smirk_vgg_prepare_backward_split16(const void* d, const float* std, float* dx, int B, int H, int W, float scale, void* stream) {
    if (!std || !vgg_scale_ok(scale)) return SMIRK_ERR_BAD_ARG;
    const int bad = vgg_prepare_validate(d, dx, B, H, W);
    if (bad != SMIRK_OK) return bad;
    const size_t px = (size_t)B * H * W;
    smirk_prof_next(nullptr, 0.0, (double)px * (3 * 4 + 32));
    SMIRK_LAUNCH(vgg_prepare_backward_kernel, dim3(vgg_grid(px)), dim3(VGG_BLOCK), 0, (hipStream_t)stream, (const float*)d, std, dx, B, H * W, 0.5f * scale);
    return smirk_launch_status();
}

// the taps of a call sequence -> partial layout; SMIRK_OK or the refusal
static int vgg_l1_fill(VggL1Args& a, const long long* half_elems, int n_taps) {
    if (!half_elems || n_taps < 1 || n_taps > SMIRK_VGG_TAPS) return SMIRK_ERR_BAD_ARG;
    for (int k = 0; k < n_taps; ++k)
        if (half_elems[k] < 8 || half_elems[k] % 8) return SMIRK_ERR_BAD_ARG;
    for (int k = 0; k < n_taps; ++k)
        if (half_elems[k] > LLONG_MAX / 8 || !conv_fits32(2 * half_elems[k])) return SMIRK_ERR_UNSUPPORTED;
    long long chunk = 0;
    a = VggL1Args{};
    a.n = n_taps;
    for (int k = 0; k < n_taps; ++k) {
        a.half_elems[k] = half_elems[k];
        a.chunk0[k] = (int)chunk;
        chunk += vgg_chunks(half_elems[k]);                                       // at most 2^28 / 2^15 chunks per tap
    }
    a.chunk0[n_taps] = (int)chunk;
    return SMIRK_OK;
}

extern "C" size_t smirk_vgg_l1_workspace_bytes(const long long* half_elems, int n_taps) {
    VggL1Args a;
    if (vgg_l1_fill(a, half_elems, n_taps) != SMIRK_OK) return 0;
    return smirk_align_up((size_t)a.chunk0[n_taps] * sizeof(double), 256);
}

extern "C" int smirk_vgg_l1_partials_split16(const void* f, int C, int tap, const long long* half_elems, int n_taps, void* ws, size_t ws_bytes, void* stream) {
    if (vgg_bad_ptr(f) || vgg_bad_ptr(ws) || C < 8 || C % 8) return SMIRK_ERR_BAD_ARG;
    VggL1Args a;
    const int bad = vgg_l1_fill(a, half_elems, n_taps);
    if (bad != SMIRK_OK) return bad;
    if (tap < 0 || tap >= n_taps) return SMIRK_ERR_BAD_ARG;
    if (ws_bytes < smirk_vgg_l1_workspace_bytes(half_elems, n_taps)) return SMIRK_ERR_WORKSPACE;
    const int chunks = a.chunk0[tap + 1] - a.chunk0[tap];
    smirk_prof_next(nullptr, 0.0, 8.0 * (double)half_elems[tap] + (double)chunks * sizeof(double));
    SMIRK_LAUNCH(vgg_l1_partial_kernel, dim3((unsigned)chunks), dim3(VGG_BLOCK), 0, (hipStream_t)stream, (const float*)f, (size_t)(half_elems[tap] / 8),
                 (double*)ws + a.chunk0[tap]);
    return smirk_launch_status();
}

extern "C" int smirk_vgg_l1_finalise(const long long* half_elems, int n_taps, const void* ws, size_t ws_bytes, float* out_terms, float* out_total, void* stream) {
    if (vgg_bad_ptr(ws) || !out_terms || !out_total) return SMIRK_ERR_BAD_ARG;
    VggL1Args a;
    const int bad = vgg_l1_fill(a, half_elems, n_taps);
    if (bad != SMIRK_OK) return bad;
    if (ws_bytes < smirk_vgg_l1_workspace_bytes(half_elems, n_taps)) return SMIRK_ERR_WORKSPACE;
    smirk_prof_next(nullptr, 0.0, (double)a.chunk0[n_taps] * sizeof(double) + (n_taps + 1) * sizeof(float));
    SMIRK_LAUNCH(vgg_l1_finalise_kernel, dim3(1), dim3(64 * SMIRK_VGG_TAPS), 0, (hipStream_t)stream, a, (const double*)ws, out_terms, out_total);
    return smirk_launch_status();
}

extern "C" int smirk_vgg_relu_tap_backward_split16(const void* fx, const void* fy, const void* d_in, const float* grad_total, void* dz, long long elems, int C,
                                                   float scale, void* stream) {
    if (vgg_bad_ptr(fx) || vgg_bad_ptr(dz) || (fy && vgg_bad_ptr(fy)) || (d_in && vgg_bad_ptr(d_in))) return SMIRK_ERR_BAD_ARG;
    if ((!fy && !d_in) || (fy && !grad_total)) return SMIRK_ERR_BAD_ARG;
    if (elems < 8 || elems % 8 || C < 8 || C % 8 || !vgg_scale_ok(scale)) return SMIRK_ERR_BAD_ARG;
    if (!conv_fits32(elems)) return SMIRK_ERR_UNSUPPORTED;
    const size_t ng = (size_t)(elems / 8);
    smirk_prof_next(nullptr, 0.0, 4.0 * (double)elems * (2 + (fy ? 1 : 0) + (d_in ? 1 : 0)));
    SMIRK_LAUNCH(vgg_relu_tap_backward_kernel, dim3(vgg_grid(ng)), dim3(VGG_BLOCK), 0, (hipStream_t)stream, (const float*)fx, (const float*)fy, (const float*)d_in,
                 grad_total, (float)((double)scale / (double)elems), (float*)dz, ng);
    return smirk_launch_status();
}
