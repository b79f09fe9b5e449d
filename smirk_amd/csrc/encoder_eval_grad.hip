// Image gradient through a FROZEN SmirkEncoder backbone in .eval() (smirk_amd/encoder_eval_grad.py): the even steps of the reference's training run
// (base_trainer.py:258-268; smirk_trainer.py:367-368 freeze_module, :300 / :375 the cycle loss back-propagated through the frozen encoder into the generator).
// BatchNorm(eval) is a per-channel affine map, so in the backward it is the factor s[c] = gamma / sqrt(running_var + eps); ReLU is the mask [y > 0] of the
// unit's stored output.  Pointwise data gradients run on the implicit-GEMM kernels (conv.hip) with that factor folded into the transposed weight where the
// unit has no ReLU.  This file adds the two streaming kernels of the schedule:
//   * dw_eval_bwd_kernel: mask + factor of the depthwise unit, depthwise 3x3 data gradient (+ skip gradient), mask + factor of the unit before it — one launch
//     that reads dy, y_out, y_in and writes dx, where the train-mode path runs BatchNorm backward, the data gradient and BatchNorm backward again;
//   * relu_scale_bwd_kernel: dz = dy * s[c] * [y > 0] (the "cn" block under the head).
// Both are HBM-bound: one lane = one pixel x one 8-channel split16 group (two 16-byte loads per operand), fp32 arithmetic, flat index like dw_dgrad_kernel
// (train_encoder.hip: consecutive lanes walk consecutive 32-byte pieces whatever G is).  32-bit index arithmetic: the entries refuse tensors of 2 GiB and more.
#include "conv_common.h"

namespace {

// dX[b,iy,ix,c] = (add + sum_{ky,kx} dY[b,oy,ox,c] * s_out[c] * [Y_out[b,oy,ox,c] > 0] * w[ky,kx,c]) * (s_in[c] * [Y_in[b,iy,ix,c] > 0])   with oy*s - pt + ky = iy
template <bool HAS_IN>
__global__ __launch_bounds__(256) void dw_eval_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y_out, const float* __restrict__ s_out,
                                                          const float* __restrict__ w /*[9][C]*/, const float* __restrict__ add, const float* __restrict__ y_in,
                                                          const float* __restrict__ s_in, float* __restrict__ dx, int B, int H, int W, int G, int stride) {
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const int pt = smirk_same_pad_lead(H, stride), pl = smirk_same_pad_lead(W, stride), C = G * 8;
    const unsigned total = (unsigned)B * H * W * G;                        // < 2^26 groups (entry)
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned g = i % (unsigned)G;
        unsigned t = i / (unsigned)G;
        const int ix = (int)(t % (unsigned)W); t /= (unsigned)W;
        const int iy = (int)(t % (unsigned)H);
        const unsigned b = t / (unsigned)H;
        float acc[8], so[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { acc[q] = 0.f; so[q] = s_out[g * 8 + q]; }
        if (add) load_group(add + (size_t)i * 8, acc);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ty = iy + pt - ky;
            if (ty < 0 || ty % stride) continue;
            const int oy = ty / stride;
            if (oy >= Ho) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int tx = ix + pl - kx;
                if (tx < 0 || tx % stride) continue;
                const int ox = tx / stride;
                if (ox >= Wo) continue;
                const size_t o = ((size_t)((b * Ho + oy) * Wo + ox) * G + g) * 8;
                float v[8], yo[8];
                load_group(dy + o, v);
                load_group(y_out + o, yo);
                const float* ww = w + (ky * 3 + kx) * C + g * 8;
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[q] = fmaf(yo[q] > 0.f ? v[q] * so[q] : 0.f, ww[q], acc[q]);
            }
        }
        if (HAS_IN) {
            float yi[8];
            load_group(y_in + (size_t)i * 8, yi);
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = yi[q] > 0.f ? acc[q] * s_in[g * 8 + q] : 0.f;
        }
        store_group(dx + (size_t)i * 8, acc);
    }
}

// dZ[m][c] = dY[m][c] * s[c] * [Y[m][c] > 0]
__global__ __launch_bounds__(256) void relu_scale_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ s,
                                                             float* __restrict__ dz, unsigned total /*groups*/, int G) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned g = i % (unsigned)G;
        float v[8], yy[8];
        load_group(dy + (size_t)i * 8, v);
        load_group(y + (size_t)i * 8, yy);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = yy[q] > 0.f ? v[q] * s[g * 8 + q] : 0.f;
        store_group(dz + (size_t)i * 8, v);
    }
}

inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15u) != 0; }

}  // namespace

extern "C" int smirk_dwconv3x3_eval_backward_split16(const void* dy, const void* y_out, const float* s_out, const float* w, const void* add, const void* y_in,
                                                     const float* s_in, void* dx, int B, int H, int W, int C, int stride, void* stream) {
    if (!dy || !y_out || !s_out || !w || !dx || (!y_in != !s_in) || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || (stride != 1 && stride != 2))
        return SMIRK_ERR_BAD_ARG;
    if (misaligned16(dy) || misaligned16(y_out) || misaligned16(add) || misaligned16(y_in) || misaligned16(dx)) return SMIRK_ERR_BAD_ARG;
    const long long px = (long long)B * H * W;
    if (px > 0x7fffffffll || !conv_fits32(px * C)) return SMIRK_ERR_UNSUPPORTED;          // dx (the largest of the tensors): 32-bit flat index
    const double in = (double)px * C, out = (double)B * ((H + stride - 1) / stride) * ((W + stride - 1) / stride) * C;
    smirk_prof_next(nullptr, 2.0 * 9.0 * out + 2.0 * out + (y_in ? in : 0.0), 4.0 * (in * (1.0 + (add ? 1.0 : 0.0) + (y_in ? 1.0 : 0.0)) + 2.0 * out));
    const dim3 grid(blocks_for((size_t)px * (C / 8), 16384));
    if (y_in)
        SMIRK_LAUNCH(dw_eval_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)dy, (const float*)y_out, s_out, w, (const float*)add,
                     (const float*)y_in, s_in, (float*)dx, B, H, W, C / 8, stride);
    else
        SMIRK_LAUNCH(dw_eval_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)dy, (const float*)y_out, s_out, w, (const float*)add,
                     (const float*)y_in, s_in, (float*)dx, B, H, W, C / 8, stride);
    return smirk_launch_status();
}

extern "C" int smirk_relu_scale_backward_split16(const void* dy, const void* y, const float* s, void* dz, long long M, int C, void* stream) {
    if (!dy || !y || !s || !dz || M <= 0 || C <= 0 || C % 8) return SMIRK_ERR_BAD_ARG;
    if (misaligned16(dy) || misaligned16(y) || misaligned16(dz)) return SMIRK_ERR_BAD_ARG;
    if (M > 0x7fffffffll || !conv_fits32(M * C)) return SMIRK_ERR_UNSUPPORTED;
    const size_t groups = (size_t)M * (C / 8);
    smirk_prof_next(nullptr, (double)M * C, 12.0 * (double)M * C);
    SMIRK_LAUNCH(relu_scale_bwd_kernel, dim3(blocks_for(groups, 16384)), dim3(256), 0, (hipStream_t)stream, (const float*)dy, (const float*)y, s, (float*)dz,
                 (unsigned)groups, C / 8);
    return smirk_launch_status();
}
