// The frozen emotion network of the first path for MI355X (gfx950): the parts of EMOCA's Bottleneck ResNet-50 (src/losses/resnet.py with emoca_specific,
// src/losses/ExpressionLoss.py; smirk_trainer.py:108-119) that no entry of smirk_hip.h serves.  The 1x1 and 3x3 convolutions, forward and data gradient, are
// smirk_conv_igemm_f16x3 (conv.hip); this unit holds the entries of include/smirk_emotion.h:
//   emotion_stem_kernel         Conv2d(3, 64, 7, stride 2, pad 3) + shift + ReLU as an implicit GEMM on the fp16 matrix pipe.  A workgroup of four waves owns a
//                               16 x 16 tile of output pixels of one image: it stages the 37 x 37 x 3 fp32 input patch in LDS once (zeros outside the image; the
//                               NaN-catching audit here: the pixels come from outside), every wave keeps the hi / lo B fragments of its 32 output channels for all
//                               of K in registers (80 VGPRs) and walks four 32-pixel row blocks, building the A fragments from the patch with compile-time tap
//                               offsets.  K = 147 ordered (ky, kx, c) and padded flat to 160 = ten 32x32x16 steps: 8.8 % of the MFMA work multiplies zeros (padding
//                               every kernel row of 21 to 24 gives 168, eleven steps: 20 %; a 7 x 8 x 4 box 52 %).  Three MFMAs per step (hi hi, hi lo, lo hi; fp32 accumulate): the
//                               accuracy class of f16x3.  The accumulators go through LDS so that every lane stores whole 8-channel split16 groups.
//   emotion_stem_dgrad_kernel   the data gradient in gather form: one lane per image pixel of one parity class (blockIdx.y), so that all lanes of a wave walk the
//                               same <= 4 x 4 taps and the weights are wave-uniform loads; three fp32 sums per lane in one fixed order.
//   emotion_maxpool_*           MaxPool2d(3, 2, 1) and its backward (a gather over the <= 4 windows of a pixel, first maximum in row-major order as ATen), one
//                               lane per pixel and 8-channel group.
//   emotion_dilate2_kernel      the adjoint of a stride-2 subsampling: the gradient goes to the even positions of a zero grid (optionally scaled, masked, added to)
//   emotion_pool_kernel, emotion_loss_kernel, emotion_head_bwd_kernel   AvgPool2d(7), the three metrics and the seed gradient
// 32-bit index arithmetic throughout: the entries refuse tensors of 2 GiB and more.  No scratch memory, no float atomics; every sum has one order.
#include "conv_common.h"

#include "../../include/smirk_emotion.h"

namespace {

constexpr int EMO_BLOCK = 256;
constexpr int ST_TILE = 16;                                                      // output pixels per side of a workgroup's tile
constexpr int ST_PATCH = 2 * (ST_TILE - 1) + 7;                                  // 37 input pixels per side
constexpr int ST_K = SMIRK_EMOTION_STEM_K, ST_KP = SMIRK_EMOTION_STEM_KPAD, ST_KSTEPS = ST_KP / 16;
constexpr int ST_N = SMIRK_EMOTION_STEM_COUT;
constexpr int ST_LD = 33;                                                        // pitch of the epilogue's staging rows
constexpr float COS_EPS = 1e-8f;

// offset of product k = (ky * 7 + kx) * 3 + c inside the patch [3][37][37], relative to the top left input pixel of an output pixel
__host__ __device__ constexpr int st_off(int k) { return k < ST_K ? ((k % 3) * ST_PATCH + (k / 3) / 7) * ST_PATCH + (k / 3) % 7 : 0; }

// grid: 2B * tiles_y * tiles_x
__global__ __launch_bounds__(EMO_BLOCK) void emotion_stem_kernel(const float* __restrict__ gen, const float* __restrict__ tar, const float* __restrict__ w,
                                                                 const float* __restrict__ shift, float* __restrict__ out, int B, int H, int W, int Ho, int Wo,
                                                                 int tiles_x, int tiles_y) {
    __shared__ float patch[3 * ST_PATCH * ST_PATCH];
    __shared__ float stage[4][32 * ST_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, n = t / tiles_y;
    const float* img = n < B ? gen + (size_t)n * 3 * H * W : tar + (size_t)(n - B) * 3 * H * W;
    const int oy0 = ty * ST_TILE, ox0 = tx * ST_TILE, iy0 = oy0 * 2 - 3, ix0 = ox0 * 2 - 3;
    for (int i = tid; i < 3 * ST_PATCH * ST_PATCH; i += EMO_BLOCK) {
        const int c = i / (ST_PATCH * ST_PATCH), rem = i - c * (ST_PATCH * ST_PATCH), py = rem / ST_PATCH, px = rem - py * ST_PATCH;
        const int iy = iy0 + py, ix = ix0 + px;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            v = img[((size_t)c * H + iy) * W + ix];
            smirk_range_audit1(v);
        }
        patch[i] = v;
    }
    // B fragments: lane (r, h) holds w[channel nb * 32 + r][k = 16 ks + 8 h + j]
    const int nb = wave & 1, ch = nb * 32 + r;
    half8 bh[ST_KSTEPS], bl[ST_KSTEPS];
    {
        const float* wr = w + (size_t)ch * ST_KP + 8 * h;
#pragma unroll
        for (int ks = 0; ks < ST_KSTEPS; ++ks) {
            const f32x4 w0 = *(const f32x4*)(wr + ks * 16), w1 = *(const f32x4*)(wr + ks * 16 + 4);
            const float v[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
#pragma unroll
            for (int q = 0; q < 8; ++q) smirk_range_audit1(v[q]);
            split8_noaudit(v, bh[ks], bl[ks]);
        }
    }
    const float sh = shift[ch];
    __syncthreads();
    SmirkRangeAcc ra;
    for (int i = 0; i < 4; ++i) {
        const int mb = (wave >> 1) * 4 + i;                                      // 32-pixel row block of the tile: two rows of sixteen
        const int ly = mb * 2 + (r >> 4), lx = r & 15;
        const float* pp = patch + (2 * ly) * ST_PATCH + 2 * lx;
        f32x16 acc0, acc1;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc0[q] = acc1[q] = 0.f;
#pragma unroll
        for (int ks = 0; ks < ST_KSTEPS; ++ks) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k0 = ks * 16 + j, k1 = k0 + 8;                         // compile-time: the lane's half picks one of two constants
                const float x = pp[h ? st_off(k1) : st_off(k0)];
                v[j] = (h ? k1 < ST_K : k0 < ST_K) ? x : 0.f;
            }
            half8 ah, al;
            split8_noaudit(v, ah, al);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[ks], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[ks], acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[ks], acc1, 0, 0, 0);
        }
        __syncthreads();                                                         // the previous block's staging rows have been read
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float z = acc0[q] + acc1[q] * (1.0f / 2048.0f) + sh;
            stage[wave][mfma32_row(q, lane) * ST_LD + r] = z > 0.f ? z : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int item = lane + 64 * u, p = item >> 2, grp = item & 3;
            const int oy = oy0 + mb * 2 + (p >> 4), ox = ox0 + (p & 15);
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = stage[wave][p * ST_LD + grp * 8 + q];
            if (oy < Ho && ox < Wo) {
                half8 hi, lo;
                split8(v, hi, lo, ra);
                float* o = out + ((size_t)(n * Ho + oy) * Wo + ox) * ST_N + (nb * 4 + grp) * 8;
                *(half8*)o = hi;
                *(half8*)(o + 4) = lo;
            }
        }
    }
    ra.commit();
}

// grid (blocks, 4 parity classes): class (py, px) holds the pixels iy = 2 jy + py, ix = 2 jx + px
__global__ __launch_bounds__(EMO_BLOCK) void emotion_stem_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ wd, const float* __restrict__ gup,
                                                                       float inv_lift, float* __restrict__ dimg, int B, int H, int W, int Ho, int Wo) {
    const int py = blockIdx.y >> 1, px = blockIdx.y & 1;
    const int Hc = (H - py + 1) / 2, Wc = (W - px + 1) / 2;
    const unsigned total = (unsigned)B * Hc * Wc;
    const int ky0 = (py + 1) & 1, kx0 = (px + 1) & 1;                            // iy + 3 - ky even
    for (unsigned i = blockIdx.x * EMO_BLOCK + threadIdx.x; i < total; i += gridDim.x * EMO_BLOCK) {
        const int jx = (int)(i % (unsigned)Wc);
        unsigned t = i / (unsigned)Wc;
        const int jy = (int)(t % (unsigned)Hc);
        const int b = (int)(t / (unsigned)Hc);
        const int iy = 2 * jy + py, ix = 2 * jx + px;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int ky = ky0; ky < 7; ky += 2) {
            const int ty = iy + 3 - ky;
            if (ty < 0 || (ty >> 1) >= Ho) continue;
            for (int kx = kx0; kx < 7; kx += 2) {
                const int tx = ix + 3 - kx;
                if (tx < 0 || (tx >> 1) >= Wo) continue;
                const float* p = dz + ((size_t)(b * Ho + (ty >> 1)) * Wo + (tx >> 1)) * ST_N;
                const float* ww = wd + (ky * 7 + kx) * 3 * ST_N;
#pragma unroll
                for (int g = 0; g < ST_N / 8; ++g) {
                    float v[8];
                    load_group(p + g * 8, v);
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        a0 = fmaf(v[q], ww[g * 8 + q], a0);
                        a1 = fmaf(v[q], ww[ST_N + g * 8 + q], a1);
                        a2 = fmaf(v[q], ww[2 * ST_N + g * 8 + q], a2);
                    }
                }
            }
        }
        const float f = gup[b] * inv_lift;
        float* o = dimg + ((size_t)b * 3 * H + iy) * W + ix;
        o[0] = a0 * f;
        o[(size_t)H * W] = a1 * f;
        o[2 * (size_t)H * W] = a2 * f;
    }
}

__global__ __launch_bounds__(EMO_BLOCK) void emotion_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned total /*output groups*/, int H,
                                                                    int W, int Ho, int Wo, int G) {
    for (unsigned i = blockIdx.x * EMO_BLOCK + threadIdx.x; i < total; i += gridDim.x * EMO_BLOCK) {
        const unsigned g = i % (unsigned)G;
        unsigned t = i / (unsigned)G;
        const int ox = (int)(t % (unsigned)Wo);
        t /= (unsigned)Wo;
        const int oy = (int)(t % (unsigned)Ho);
        const unsigned n = t / (unsigned)Ho;
        float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool first = true;
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = 2 * oy - 1 + dy;
            if (iy < 0 || iy >= H) continue;
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = 2 * ox - 1 + dx;
                if (ix < 0 || ix >= W) continue;
                float v[8];
                load_group(x + (((size_t)n * H + iy) * W + ix) * G * 8 + g * 8, v);
#pragma unroll
                for (int q = 0; q < 8; ++q) m[q] = first || v[q] > m[q] ? v[q] : m[q];
                first = false;
            }
        }
        half8 hi, lo;
        split8_noaudit(m, hi, lo);                                               // copies of audited values
        *(half8*)(y + (size_t)i * 8) = hi;
        *(half8*)(y + (size_t)i * 8 + 4) = lo;
    }
}

__global__ __launch_bounds__(EMO_BLOCK) void emotion_maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                                        unsigned total /*input groups*/, int H, int W, int Ho, int Wo, int G, int relu_mask) {
    for (unsigned i = blockIdx.x * EMO_BLOCK + threadIdx.x; i < total; i += gridDim.x * EMO_BLOCK) {
        const unsigned g = i % (unsigned)G;
        unsigned t = i / (unsigned)G;
        const int ix = (int)(t % (unsigned)W);
        t /= (unsigned)W;
        const int iy = (int)(t % (unsigned)H);
        const unsigned n = t / (unsigned)H;
        float xv[8], acc[8];
        load_group(x + (size_t)i * 8, xv);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = 0.f;
        // the windows whose rows 2 oy - 1 .. 2 oy + 1 contain iy: oy = iy / 2 and, for an odd iy, iy / 2 + 1
        for (int oy = iy >> 1; oy <= ((iy + 1) >> 1); ++oy) {
            if (oy >= Ho) continue;
            for (int ox = ix >> 1; ox <= ((ix + 1) >> 1); ++ox) {
                if (ox >= Wo) continue;
                bool win[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) win[q] = true;
                for (int a = 0; a < 3; ++a) {
                    const int jy = 2 * oy - 1 + a;
                    if (jy < 0 || jy >= H) continue;
                    for (int c = 0; c < 3; ++c) {
                        const int jx = 2 * ox - 1 + c;
                        if (jx < 0 || jx >= W || (jy == iy && jx == ix)) continue;
                        const bool before = jy < iy || (jy == iy && jx < ix);
                        float v[8];
                        load_group(x + (((size_t)n * H + jy) * W + jx) * G * 8 + g * 8, v);
#pragma unroll
                        for (int q = 0; q < 8; ++q) win[q] = win[q] && (before ? xv[q] > v[q] : xv[q] >= v[q]);
                    }
                }
                float d[8];
                load_group(dy + (((size_t)n * Ho + oy) * Wo + ox) * G * 8 + g * 8, d);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[q] += win[q] ? d[q] : 0.f;
            }
        }
        if (relu_mask) {
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = xv[q] > 0.f ? acc[q] : 0.f;
        }
        store_group(dx + (size_t)i * 8, acc);
    }
}

__global__ __launch_bounds__(EMO_BLOCK) void emotion_dilate2_kernel(const float* __restrict__ dz, const float* __restrict__ y, const float* __restrict__ s,
                                                                    const float* __restrict__ add, float* __restrict__ out, unsigned total /*output groups*/,
                                                                    int Hl, int Wl, int H, int W, int G) {
#pragma clang fp contract(off)                                                   // the product and the sum round on their own, as the header says
    for (unsigned i = blockIdx.x * EMO_BLOCK + threadIdx.x; i < total; i += gridDim.x * EMO_BLOCK) {
        const unsigned g = i % (unsigned)G;
        unsigned t = i / (unsigned)G;
        const int ix = (int)(t % (unsigned)W);
        t /= (unsigned)W;
        const int iy = (int)(t % (unsigned)H);
        const unsigned n = t / (unsigned)H;
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = 0.f;
        if (!(iy & 1) && !(ix & 1)) {
            const size_t o = ((((size_t)n * Hl + (iy >> 1)) * Wl + (ix >> 1)) * G + g) * 8;
            load_group(dz + o, v);
            if (s) {
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = __fmul_rn(v[q], s[g * 8 + q]);
            }
            if (y) {
                float yy[8];
                load_group(y + o, yy);
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = yy[q] > 0.f ? v[q] : 0.f;
            }
        }
        if (add) {
            float a[8];
            load_group(add + (size_t)i * 8, a);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = __fadd_rn(v[q], a[q]);
        }
        store_group(out + (size_t)i * 8, v);
    }
}

// pooled[n][c] = (sum_p feat[n][p][c]) / HW, p ascending
__global__ __launch_bounds__(EMO_BLOCK) void emotion_pool_kernel(const float* __restrict__ feat, float* __restrict__ pooled, unsigned total /*N * G*/, int HW, int G) {
    const unsigned i = blockIdx.x * EMO_BLOCK + threadIdx.x;
    if (i >= total) return;
    const unsigned g = i % (unsigned)G, n = i / (unsigned)G;
    float s[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = 0.f;
    const float* p = feat + ((size_t)n * HW * G + g) * 8;
    for (int k = 0; k < HW; ++k) {
        float v[8];
        load_group(p + (size_t)k * G * 8, v);
#pragma unroll
        for (int q = 0; q < 8; ++q) s[q] += v[q];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) pooled[(size_t)i * 8 + q] = s[q] / (float)HW;
}

// one workgroup: per sample three sums over the channels (lane-strided partials, then a fixed tree over the 256 partials), the loss, and the batch mean
__global__ __launch_bounds__(EMO_BLOCK) void emotion_loss_kernel(const float* __restrict__ pooled, float* __restrict__ aux, float* __restrict__ loss,
                                                                 float* __restrict__ mean, int B, int C, int metric) {
    __shared__ float red[3][EMO_BLOCK];
    const int tid = threadIdx.x;
    float total = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* g = pooled + (size_t)b * C;
        const float* t = pooled + (size_t)(B + b) * C;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int c = tid; c < C; c += EMO_BLOCK) {
            const float gv = g[c], tv = t[c], d = gv - tv;
            if (metric == SMIRK_EMOTION_L2) s0 = fmaf(d, d, s0);
            else if (metric == SMIRK_EMOTION_L1) s0 += fabsf(d);
            else { s0 = fmaf(gv, tv, s0); s1 = fmaf(gv, gv, s1); s2 = fmaf(tv, tv, s2); }
        }
        __syncthreads();                                                         // the previous sample's tree has been read
        red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s2;
        __syncthreads();
        for (int o = EMO_BLOCK / 2; o > 0; o >>= 1) {
            if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; red[2][tid] += red[2][tid + o]; }
            __syncthreads();
        }
        if (tid == 0) {
            float l;
            if (metric == SMIRK_EMOTION_COS) {
                const float ng = sqrtf(red[1][0]), nt = sqrtf(red[2][0]);
                l = 1.0f - red[0][0] / (fmaxf(ng, COS_EPS) * fmaxf(nt, COS_EPS));
                aux[b * 4 + 0] = red[0][0]; aux[b * 4 + 1] = ng; aux[b * 4 + 2] = nt; aux[b * 4 + 3] = 0.f;
            } else {
                l = red[0][0] / (float)C;
                aux[b * 4 + 0] = aux[b * 4 + 1] = aux[b * 4 + 2] = aux[b * 4 + 3] = 0.f;
            }
            loss[b] = l;
            total += l;
        }
    }
    if (tid == 0 && mean) *mean = total / (float)B;
}

__global__ __launch_bounds__(EMO_BLOCK) void emotion_head_bwd_kernel(const float* __restrict__ feat, const float* __restrict__ pooled, const float* __restrict__ aux,
                                                                     float* __restrict__ gout, unsigned total /*B * HW * G*/, int B, int HW, int G, int metric,
                                                                     float lift) {
    const int C = G * 8;
    const float f = lift / (float)HW;
    for (unsigned i = blockIdx.x * EMO_BLOCK + threadIdx.x; i < total; i += gridDim.x * EMO_BLOCK) {
        const unsigned g = i % (unsigned)G, b = i / ((unsigned)G * HW);
        const float* pg = pooled + (size_t)b * C + g * 8;
        const float* pt = pooled + (size_t)(B + b) * C + g * 8;
        float fv[8], v[8];
        load_group(feat + (size_t)i * 8, fv);
        float dot = 0.f, cg = 1.f, ct = 1.f;
        bool live = false;
        if (metric == SMIRK_EMOTION_COS) {
            dot = aux[b * 4];
            const float ng = aux[b * 4 + 1], nt = aux[b * 4 + 2];
            cg = fmaxf(ng, COS_EPS); ct = fmaxf(nt, COS_EPS);
            live = ng > COS_EPS;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float gv = pg[q], tv = pt[q], d = gv - tv;
            float sd;
            if (metric == SMIRK_EMOTION_L2) sd = 2.0f * d / (float)C;
            else if (metric == SMIRK_EMOTION_L1) sd = (d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.f)) / (float)C;
            else sd = -(tv / (cg * ct) - (live ? dot * gv / (cg * cg * cg * ct) : 0.f));
            v[q] = fv[q] > 0.f ? sd * f : 0.f;
        }
        store_group(gout + (size_t)i * 8, v);
    }
}

inline bool emo_bad_ptr(const void* p) { return !p || ((uintptr_t)p & 15u) != 0; }
inline bool emo_odd_ptr(const void* p) { return p && ((uintptr_t)p & 15u) != 0; }    // a nullable pointer that is given must be aligned
inline bool emo_bad_metric(int m) { return m != SMIRK_EMOTION_L2 && m != SMIRK_EMOTION_L1 && m != SMIRK_EMOTION_COS; }

// [N][H][W][C] split16 with N, H, W >= 1, C a positive multiple of 8: SMIRK_OK, or why not
int emo_tensor(long long N, int H, int W, int C) {
    if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8) return SMIRK_ERR_BAD_ARG;
    if (N >= (1ll << 31) || H > 32767 || W > 32767 || N * H >= (1ll << 31) || N * H * W >= (1ll << 31) || !conv_fits32(N * H * W * C)) return SMIRK_ERR_UNSUPPORTED;
    return SMIRK_OK;
}

}  // namespace

extern "C" int smirk_emotion_abi_version(void) { return SMIRK_EMOTION_ABI_VERSION; }

extern "C" int smirk_emotion_stem_split16(const float* gen, const float* tar, const float* w, const float* shift, void* out, int B, int H, int W, void* stream) {
    if (emo_bad_ptr(gen) || emo_bad_ptr(tar) || emo_bad_ptr(w) || emo_bad_ptr(shift) || emo_bad_ptr(out)) return SMIRK_ERR_BAD_ARG;
    if (B < 1 || H < 1 || W < 1) return SMIRK_ERR_BAD_ARG;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int bad = emo_tensor(2ll * B, H, W, 8);                                // the images (3 channels) are smaller than this
    if (bad != SMIRK_OK) return bad;
    const int bad_out = emo_tensor(2ll * B, Ho, Wo, ST_N);
    if (bad_out != SMIRK_OK) return bad_out;
    const int tiles_x = (Wo + ST_TILE - 1) / ST_TILE, tiles_y = (Ho + ST_TILE - 1) / ST_TILE;
    const long long blocks = 2ll * B * tiles_x * tiles_y;
    if (blocks >= (1ll << 31)) return SMIRK_ERR_UNSUPPORTED;
    const double px = 2.0 * B * Ho * Wo;
    smirk_prof_next(nullptr, 2.0 * px * ST_N * ST_K, 4.0 * (2.0 * B * 3 * H * W + px * ST_N + (double)ST_N * ST_KP));
    SMIRK_LAUNCH(emotion_stem_kernel, dim3((unsigned)blocks), dim3(EMO_BLOCK), 0, (hipStream_t)stream, gen, tar, w, shift, (float*)out, B, H, W, Ho, Wo, tiles_x,
                 tiles_y);
    return smirk_launch_status();
}

extern "C" int smirk_emotion_stem_dgrad_split16(const void* dz, const float* wd, const float* gup, float inv_lift, float* dimg, int B, int H, int W, void* stream) {
    if (emo_bad_ptr(dz) || emo_bad_ptr(wd) || emo_bad_ptr(gup) || emo_bad_ptr(dimg) || !(inv_lift > 0.f) || !(inv_lift < 3.0e38f)) return SMIRK_ERR_BAD_ARG;
    if (B < 1 || H < 1 || W < 1) return SMIRK_ERR_BAD_ARG;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int bad = emo_tensor(B, H, W, 8);
    if (bad != SMIRK_OK) return bad;
    const int bad_dz = emo_tensor(B, Ho, Wo, ST_N);
    if (bad_dz != SMIRK_OK) return bad_dz;
    const double px = (double)B * H * W;
    smirk_prof_next(nullptr, 2.0 * px * 3 * ST_N * 49 / 4, 4.0 * (px * 3 + px / 4 * ST_N + 49.0 * 3 * ST_N));
    SMIRK_LAUNCH(emotion_stem_dgrad_kernel, dim3(blocks_for((size_t)B * Ho * Wo, 8192), 4), dim3(EMO_BLOCK), 0, (hipStream_t)stream, (const float*)dz, wd, gup,
                 inv_lift, dimg, B, H, W, Ho, Wo);
    return smirk_launch_status();
}

extern "C" int smirk_emotion_maxpool_split16(const void* x, void* y, int N, int H, int W, int C, void* stream) {
    if (emo_bad_ptr(x) || emo_bad_ptr(y)) return SMIRK_ERR_BAD_ARG;
    const int bad = emo_tensor(N, H, W, C);
    if (bad != SMIRK_OK) return bad;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, G = C / 8;
    const size_t groups = (size_t)N * Ho * Wo * G;
    smirk_prof_next(nullptr, 9.0 * groups * 8, 4.0 * ((double)N * H * W * C + (double)groups * 8));
    SMIRK_LAUNCH(emotion_maxpool_kernel, dim3(blocks_for(groups, 16384)), dim3(EMO_BLOCK), 0, (hipStream_t)stream, (const float*)x, (float*)y, (unsigned)groups, H, W,
                 Ho, Wo, G);
    return smirk_launch_status();
}

extern "C" int smirk_emotion_maxpool_backward_split16(const void* x, const void* dy, void* dx, int N, int H, int W, int C, int relu_mask, void* stream) {
    if (emo_bad_ptr(x) || emo_bad_ptr(dy) || emo_bad_ptr(dx)) return SMIRK_ERR_BAD_ARG;
    const int bad = emo_tensor(N, H, W, C);
    if (bad != SMIRK_OK) return bad;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, G = C / 8;
    const size_t groups = (size_t)N * H * W * G;
    smirk_prof_next(nullptr, 36.0 * groups * 8, 4.0 * (2.0 * groups * 8 + (double)N * Ho * Wo * C));
    SMIRK_LAUNCH(emotion_maxpool_bwd_kernel, dim3(blocks_for(groups, 16384)), dim3(EMO_BLOCK), 0, (hipStream_t)stream, (const float*)x, (const float*)dy, (float*)dx,
                 (unsigned)groups, H, W, Ho, Wo, G, relu_mask);
    return smirk_launch_status();
}

extern "C" int smirk_emotion_dilate2_split16(const void* dz, const void* y, const float* s, const void* add, void* out, int N, int Hl, int Wl, int H, int W, int C,
                                             void* stream) {
    if (emo_bad_ptr(dz) || emo_odd_ptr(y) || emo_odd_ptr(s) || emo_odd_ptr(add) || emo_bad_ptr(out)) return SMIRK_ERR_BAD_ARG;
    const int bad = emo_tensor(N, H, W, C);
    if (bad != SMIRK_OK) return bad;
    if (Hl != (H + 1) / 2 || Wl != (W + 1) / 2) return SMIRK_ERR_BAD_ARG;
    const int G = C / 8;
    const size_t groups = (size_t)N * H * W * G;
    smirk_prof_next(nullptr, 2.0 * N * Hl * Wl * C, 4.0 * ((double)groups * 8 * (add ? 2.0 : 1.0) + (double)N * Hl * Wl * C * (y ? 2.0 : 1.0)));
    SMIRK_LAUNCH(emotion_dilate2_kernel, dim3(blocks_for(groups, 16384)), dim3(EMO_BLOCK), 0, (hipStream_t)stream, (const float*)dz, (const float*)y, s,
                 (const float*)add, (float*)out, (unsigned)groups, Hl, Wl, H, W, G);
    return smirk_launch_status();
}

extern "C" int smirk_emotion_head_forward_split16(const void* feat, float* pooled, float* aux, float* loss, float* mean, int B, int HW, int C, int metric,
                                                  void* stream) {
    if (emo_bad_ptr(feat) || emo_bad_ptr(pooled) || emo_bad_ptr(aux) || emo_bad_ptr(loss) || emo_odd_ptr(mean) || emo_bad_metric(metric)) return SMIRK_ERR_BAD_ARG;
    if (B < 1) return SMIRK_ERR_BAD_ARG;
    const int bad = emo_tensor(2ll * B, HW, 1, C);
    if (bad != SMIRK_OK) return bad;
    const size_t items = (size_t)2 * B * (C / 8);
    smirk_prof_next(nullptr, (double)items * 8 * HW, 4.0 * ((double)items * 8 * (HW + 1)));
    SMIRK_LAUNCH(emotion_pool_kernel, dim3((unsigned)((items + EMO_BLOCK - 1) / EMO_BLOCK)), dim3(EMO_BLOCK), 0, (hipStream_t)stream, (const float*)feat, pooled,
                 (unsigned)items, HW, C / 8);
    smirk_prof_next(nullptr, 6.0 * B * C, 4.0 * (2.0 * B * C + 6.0 * B));
    SMIRK_LAUNCH(emotion_loss_kernel, dim3(1), dim3(EMO_BLOCK), 0, (hipStream_t)stream, (const float*)pooled, aux, loss, mean, B, C, metric);
    return smirk_launch_status();
}

extern "C" int smirk_emotion_head_backward_split16(const void* feat, const float* pooled, const float* aux, void* g, int B, int HW, int C, int metric, float lift,
                                                   void* stream) {
    if (emo_bad_ptr(feat) || emo_bad_ptr(pooled) || emo_bad_ptr(aux) || emo_bad_ptr(g) || emo_bad_metric(metric) || !(lift > 0.f) || !(lift < 3.0e38f))
        return SMIRK_ERR_BAD_ARG;
    if (B < 1) return SMIRK_ERR_BAD_ARG;
    const int bad = emo_tensor(2ll * B, HW, 1, C);
    if (bad != SMIRK_OK) return bad;
    const size_t groups = (size_t)B * HW * (C / 8);
    smirk_prof_next(nullptr, 4.0 * groups * 8, 4.0 * (2.0 * groups * 8 + 2.0 * B * C));
    SMIRK_LAUNCH(emotion_head_bwd_kernel, dim3(blocks_for(groups, 16384)), dim3(EMO_BLOCK), 0, (hipStream_t)stream, (const float*)feat, pooled, aux, (float*)g,
                 (unsigned)groups, B, HW, C / 8, metric, lift);
    return smirk_launch_status();
}
