// The frozen MICA network of the pre-training stage for MI355X (gfx950): everything AROUND the convolutions of src/models/MICA/arcface.py:32-198 and
// mica.py:34-94 (smirk_trainer.py:128-131).  The convolutions are smirk_conv_igemm_f16x3 (conv.hip) with the BatchNorm that follows them as the epilogue's
// scale / shift; this unit holds the entries of include/smirk_mica.h:
//   mica_prepare_kernel       img NCHW fp32 -> split16 NHWC [B][H][W][8]: v = (img - 0.5) * 2 (the division by 0.5 of mica.py:70 is exact), channels
//                             [2, 1, 0], channels 3..7 zero; the range audit in its NaN-catching form (these values come from outside the library)
//   mica_affine_prelu_kernel  z = x * scale[c] + shift[c], y = z > 0 ? z : slope[c] * z: a block's leading BatchNorm (it cannot be folded into the weights of
//                             the zero-padded convolution behind it: the border taps would see the shift) and the PReLU between a block's convolutions.  One
//                             lane = one pixel x one 8-channel group over a flat index, as relu_scale_bwd_kernel (encoder_eval_grad.hip); HBM-bound.
//   mica_fc_kernel            the fully connected layer, out[b][n] = sum_k x[b][k] w[n][k] with B <= 64 rows: memory-bound on w (51 MB at 512 x 25088), so every
//                             weight element is read from memory once and used for all rows.  A workgroup owns 64 neurons x one K split; per 32-wide K step it
//                             stages w [64][32] and the decoded x [64][32] in LDS (rows padded to 36 floats: lanes 0..15 of a 16-byte read start on 16 different
//                             multiples of four banks), and each of the 256 threads keeps a 4 row x 4 neuron fp32 tile; the loads of the next step are issued before the
//                             current step is computed.  The K split depends on K alone
//                             (mica_fc_splits), the partials go to the workspace and mica_fc_reduce_kernel adds them in split order and then the bias.
//   mica_head_kernel          F.normalize (eps 1e-12) and the five Linear layers of the mapping network, one workgroup of 16 waves per face, activations in LDS.  A wave
//                             takes four output neurons at a time: its lanes walk the four weight rows in 256-byte pieces, a fixed butterfly adds the 64
//                             partial sums of each.
// 32-bit index arithmetic throughout: the entries refuse tensors of 2 GiB and more.  No float atomics; every sum has one order, fixed by the shapes.
#include "conv_common.h"

#include "../../include/smirk_mica.h"

namespace {

constexpr int MICA_BLOCK = 256;
constexpr int FC_NT = 64, FC_BT = SMIRK_MICA_FC_MAX_B, FC_KS = 32, FC_LD = FC_KS + 4;      // neurons / rows / K step of a workgroup; padded LDS row
constexpr int FC_MAX_SPLITS = 64;
constexpr int HEAD_BLOCK = 1024, HEAD_WAVES = HEAD_BLOCK / 64;
constexpr float HEAD_EPS = 1e-12f, HEAD_SLOPE = 0.2f;

__global__ __launch_bounds__(MICA_BLOCK) void mica_prepare_kernel(const float* __restrict__ img, float* __restrict__ out, unsigned total /*pixels*/, unsigned HW) {
    for (unsigned i = blockIdx.x * MICA_BLOCK + threadIdx.x; i < total; i += gridDim.x * MICA_BLOCK) {
        const unsigned b = i / HW, p = i - b * HW;
        const float* src = img + (size_t)b * 3 * HW + p;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        v[0] = (src[2 * (size_t)HW] - 0.5f) * 2.0f;
        v[1] = (src[HW] - 0.5f) * 2.0f;
        v[2] = (src[0] - 0.5f) * 2.0f;
        smirk_range_audit1(v[0]); smirk_range_audit1(v[1]); smirk_range_audit1(v[2]);
        half8 hi, lo;
        split8_noaudit(v, hi, lo);
        *(half8*)(out + (size_t)i * 8) = hi;
        *(half8*)(out + (size_t)i * 8 + 4) = lo;
    }
}

// in and out may be the same tensor: a lane reads its group before it writes it and no other lane touches that group
__global__ __launch_bounds__(MICA_BLOCK) void mica_affine_prelu_kernel(const float* in, const float* __restrict__ scale, const float* __restrict__ shift,
                                                                       const float* __restrict__ slope, float* out, unsigned total /*groups*/, int G) {
    for (unsigned i = blockIdx.x * MICA_BLOCK + threadIdx.x; i < total; i += gridDim.x * MICA_BLOCK) {
        const unsigned c0 = (i % (unsigned)G) * 8;
        float v[8];
        load_group(in + (size_t)i * 8, v);
        if (scale) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] *= scale[c0 + q];
        }
        if (shift) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] += shift[c0 + q];
        }
        if (slope) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = v[q] > 0.f ? v[q] : slope[c0 + q] * v[q];
        }
        store_group(out + (size_t)i * 8, v);
    }
}

// grid (ceil(N / 64), splits); partial[split][b][n], b < B
__global__ __launch_bounds__(MICA_BLOCK) void mica_fc_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ partial, int B, int K, int N,
                                                             int k_per_split) {
    __shared__ __attribute__((aligned(16))) float xs[FC_BT * FC_LD];
    __shared__ __attribute__((aligned(16))) float ws[FC_NT * FC_LD];
    const int tid = threadIdx.x, tn = tid & 15, tb = tid >> 4;
    const int n0 = blockIdx.x * FC_NT;
    const int k_begin = blockIdx.y * k_per_split, k_end = min(K, k_begin + k_per_split);
    // staging: thread -> row r = tid / 4 (0..63) and the 8-wide piece tid % 4 of the 32-wide K step
    const int sr = tid >> 2, sk = (tid & 3) * 8;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    // this thread's piece of a K step, still as stored (x: the hi and lo halves of one group); zeros where the row, the neuron or the piece does not exist
    f32x4 xh, xl, w0, w1;
    auto fetch = [&](int k0) {
        const int k = k0 + sk;                                                   // k_end and k are multiples of 8: a piece is whole or absent
        xh = xl = w0 = w1 = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k < k_end) {
            if (sr < B) {
                const float* xp = x + (size_t)sr * K + k;
                xh = *(const f32x4*)xp;
                xl = *(const f32x4*)(xp + 4);
            }
            if (n0 + sr < N) {
                const float* wp = w + (size_t)(n0 + sr) * K + k;
                w0 = *(const f32x4*)wp;
                w1 = *(const f32x4*)(wp + 4);
            }
        }
    };
    fetch(k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += FC_KS) {
        float xv[8];
        {
            const half8 hi = __builtin_bit_cast(half8, xh), lo = __builtin_bit_cast(half8, xl);
#pragma unroll
            for (int q = 0; q < 8; ++q) xv[q] = join1(hi[q], lo[q]);
        }
        __syncthreads();                                                         // the previous step's reads are done
        *(f32x4*)(xs + sr * FC_LD + sk) = f32x4{xv[0], xv[1], xv[2], xv[3]};
        *(f32x4*)(xs + sr * FC_LD + sk + 4) = f32x4{xv[4], xv[5], xv[6], xv[7]};
        *(f32x4*)(ws + sr * FC_LD + sk) = w0;
        *(f32x4*)(ws + sr * FC_LD + sk + 4) = w1;
        __syncthreads();
        fetch(k0 + FC_KS);                                                       // the next step's loads fly while this step computes
#pragma unroll
        for (int kk = 0; kk < FC_KS; kk += 4) {
            f32x4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *(const f32x4*)(xs + (tb * 4 + i) * FC_LD + kk);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *(const f32x4*)(ws + (tn + 16 * j) * FC_LD + kk);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i][q], b[j][q], acc[i][j]);
        }
    }
    float* p = partial + (size_t)blockIdx.y * B * N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = tb * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tn + 16 * j;
            if (b < B && n < N) p[(size_t)b * N + n] = acc[i][j];
        }
    }
}

__global__ __launch_bounds__(MICA_BLOCK) void mica_fc_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bias, float* __restrict__ out, int BN,
                                                                    int N, int splits) {
    const int i = blockIdx.x * MICA_BLOCK + threadIdx.x;
    if (i >= BN) return;
    float s = partial[i];
    for (int k = 1; k < splits; ++k) s += partial[(size_t)k * BN + i];
    out[i] = s + bias[i % N];
}

__device__ __forceinline__ float mica_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(HEAD_BLOCK) void mica_head_kernel(const float* __restrict__ feat, SmirkMicaHead head, float* __restrict__ out) {
    __shared__ float h[2][SMIRK_MICA_HEAD_MAX_DIM];
    __shared__ float red[HEAD_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = head.layer[0].n_in;
    const float* f = feat + (size_t)blockIdx.x * n0;
    float sq = 0.f;
    for (int i = tid; i < n0; i += HEAD_BLOCK) {
        const float v = f[i];
        h[0][i] = v;
        sq = fmaf(v, v, sq);
    }
    sq = mica_wave_sum(sq);
    if (lane == 0) red[wave] = sq;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int k = 0; k < HEAD_WAVES; ++k) total += red[k];                        // wave order
    const float norm = fmaxf(sqrtf(total), HEAD_EPS);
    for (int i = tid; i < n0; i += HEAD_BLOCK) h[0][i] /= norm;                  // each thread rescales what it wrote
    __syncthreads();
    int cur = 0;
#pragma unroll                                                                   // compile-time indices into the by-value struct: it stays in the argument segment
    for (int l = 0; l < SMIRK_MICA_HEAD_LAYERS; ++l) {
        const SmirkMicaLinear L = head.layer[l];
        const bool last = l == SMIRK_MICA_HEAD_LAYERS - 1;
        float* dst = last ? out + (size_t)blockIdx.x * L.n_out : h[cur ^ 1];
        // four neurons per wave and pass: four independent loads in flight per lane (one neuron per wave was bound by the latency of its chain of loads);
        // a neuron past the end repeats the last one and is not stored
        for (int j0 = wave * 4; j0 < L.n_out; j0 += HEAD_WAVES * 4) {
            const float* wr[4];
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) wr[r] = L.w + (size_t)min(j0 + r, L.n_out - 1) * L.n_in;
            for (int i = lane; i < L.n_in; i += 64) {
                const float hv = h[cur][i];
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] = fmaf(wr[r][i], hv, s[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = mica_wave_sum(s[r]) + L.b[min(j0 + r, L.n_out - 1)];
                if (lane == 0 && j0 + r < L.n_out) dst[j0 + r] = last ? v : (v > 0.f ? v : HEAD_SLOPE * v);
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

inline bool mica_bad_ptr(const void* p) { return !p || ((uintptr_t)p & 15u) != 0; }
inline bool mica_odd_ptr(const void* p) { return p && ((uintptr_t)p & 15u) != 0; }    // a nullable pointer that is given must be aligned

// K split of the fully connected layer: at most 64 pieces of at least 64 and a multiple of 8, from K alone (never from the device)
inline int mica_fc_k_per_split(int K) {
    const int splits = K / 64 < 1 ? 1 : (K / 64 > FC_MAX_SPLITS ? FC_MAX_SPLITS : K / 64);
    return ((K + splits - 1) / splits + 7) / 8 * 8;
}
inline int mica_fc_splits(int K) { const int per = mica_fc_k_per_split(K); return (K + per - 1) / per; }

int mica_fc_validate(int B, int K, int N) {
    if (B < 1 || B > SMIRK_MICA_FC_MAX_B || K < 8 || K % 8 || N < 1) return SMIRK_ERR_BAD_ARG;
    if (!conv_fits32((long long)N * K) || !conv_fits32((long long)B * K) || !conv_fits32((long long)FC_MAX_SPLITS * B * N)) return SMIRK_ERR_UNSUPPORTED;
    return SMIRK_OK;
}

}  // namespace

extern "C" int smirk_mica_abi_version(void) { return SMIRK_MICA_ABI_VERSION; }

extern "C" int smirk_mica_prepare_split16(const float* img, void* out, int B, int H, int W, void* stream) {
    if (mica_bad_ptr(img) || mica_bad_ptr(out) || B < 1 || H < 1 || W < 1) return SMIRK_ERR_BAD_ARG;
    if (!conv_fits32((long long)B * H * W * 8)) return SMIRK_ERR_UNSUPPORTED;
    const size_t px = (size_t)B * H * W;
    smirk_prof_next(nullptr, 0.0, (double)px * (3 * 4 + 32));
    SMIRK_LAUNCH(mica_prepare_kernel, dim3(blocks_for(px, 16384)), dim3(MICA_BLOCK), 0, (hipStream_t)stream, img, (float*)out, (unsigned)px, (unsigned)(H * W));
    return smirk_launch_status();
}

extern "C" int smirk_mica_affine_prelu_split16(const void* in, const float* scale, const float* shift, const float* slope, void* out, long long M, int C,
                                               void* stream) {
    if (mica_bad_ptr(in) || mica_bad_ptr(out) || mica_odd_ptr(scale) || mica_odd_ptr(shift) || mica_odd_ptr(slope) || M < 1 || C < 8 || C % 8) return SMIRK_ERR_BAD_ARG;
    if (M >= (1ll << 31) || !conv_fits32(M * C)) return SMIRK_ERR_UNSUPPORTED;
    const size_t groups = (size_t)M * (C / 8);
    smirk_prof_next(nullptr, 2.0 * (double)M * C, 8.0 * (double)M * C);
    SMIRK_LAUNCH(mica_affine_prelu_kernel, dim3(blocks_for(groups, 16384)), dim3(MICA_BLOCK), 0, (hipStream_t)stream, (const float*)in, scale, shift, slope, (float*)out,
                 (unsigned)groups, C / 8);
    return smirk_launch_status();
}

extern "C" size_t smirk_mica_fc_workspace_bytes(int B, int K, int N) {
    if (mica_fc_validate(B, K, N) != SMIRK_OK) return 0;
    return smirk_align_up((size_t)mica_fc_splits(K) * B * N * sizeof(float), 256);
}

extern "C" int smirk_mica_fc_split16(const void* x, const float* w, const float* bias, float* out, void* ws, size_t ws_bytes, int B, int K, int N, void* stream) {
    if (mica_bad_ptr(x) || mica_bad_ptr(w) || mica_bad_ptr(bias) || mica_bad_ptr(out) || mica_bad_ptr(ws)) return SMIRK_ERR_BAD_ARG;
    const int bad = mica_fc_validate(B, K, N);
    if (bad != SMIRK_OK) return bad;
    if (ws_bytes < smirk_mica_fc_workspace_bytes(B, K, N)) return SMIRK_ERR_WORKSPACE;
    const int per = mica_fc_k_per_split(K), splits = mica_fc_splits(K);
    smirk_prof_next(nullptr, 2.0 * B * (double)N * K, 4.0 * ((double)N * K + (double)B * K + (double)splits * B * N));
    SMIRK_LAUNCH(mica_fc_kernel, dim3((unsigned)((N + FC_NT - 1) / FC_NT), (unsigned)splits), dim3(MICA_BLOCK), 0, (hipStream_t)stream, (const float*)x, w, (float*)ws, B,
                 K, N, per);
    smirk_prof_next(nullptr, (double)splits * B * N, 4.0 * ((double)splits * B * N + (double)B * N + N));
    SMIRK_LAUNCH(mica_fc_reduce_kernel, dim3((unsigned)((B * N + MICA_BLOCK - 1) / MICA_BLOCK)), dim3(MICA_BLOCK), 0, (hipStream_t)stream, (const float*)ws, bias, out,
                 B * N, N, splits);
    return smirk_launch_status();
}

extern "C" int smirk_mica_head(const float* feat, const SmirkMicaHead* head, float* out, int B, void* stream) {
    if (mica_bad_ptr(feat) || !head || mica_bad_ptr(out) || B < 1) return SMIRK_ERR_BAD_ARG;
    double flop = 0.0, bytes = 0.0;
    for (int l = 0; l < SMIRK_MICA_HEAD_LAYERS; ++l) {
        const SmirkMicaLinear& L = head->layer[l];
        if (mica_bad_ptr(L.w) || mica_bad_ptr(L.b) || L.n_in < 1 || L.n_out < 1 || (l > 0 && L.n_in != head->layer[l - 1].n_out)) return SMIRK_ERR_BAD_ARG;
        flop += 2.0 * L.n_in * L.n_out;
        bytes += 4.0 * (L.n_in + 1.0) * L.n_out;
    }
    for (int l = 0; l < SMIRK_MICA_HEAD_LAYERS; ++l)
        if (head->layer[l].n_in > SMIRK_MICA_HEAD_MAX_DIM || head->layer[l].n_out > SMIRK_MICA_HEAD_MAX_DIM) return SMIRK_ERR_UNSUPPORTED;
    if (!conv_fits32((long long)B * SMIRK_MICA_HEAD_MAX_DIM)) return SMIRK_ERR_UNSUPPORTED;
    smirk_prof_next(nullptr, flop * B, bytes + 4.0 * B * (head->layer[0].n_in + head->layer[SMIRK_MICA_HEAD_LAYERS - 1].n_out));
    SMIRK_LAUNCH(mica_head_kernel, dim3((unsigned)B), dim3(HEAD_BLOCK), 0, (hipStream_t)stream, feat, *head, out);
    return smirk_launch_status();
}
