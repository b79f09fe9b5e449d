// Training-mode building blocks of the SmirkGenerator on MI355X (BASELINE config 5, first slice: the generator is 97 % of the step's FLOPs):
//   * BatchNorm2d in TRAIN mode — batch statistics, normalise + affine (+ residual) (+ ReLU), running-stat update    (nn.BatchNorm2d inside
//     smirk_generator.py:88-119 `_block` and :121-178 `ResnetBlock` after `self.train()`, base_trainer.py:108-111) — and its backward;
//   * the streaming backward companions of the forward kernels: 2x2 max-pool backward, reflection-pad fold, space-to-depth of the ConvTranspose2d output
//     gradient, final 1x1 conv + sigmoid backward;
//   * the per-step packing of the convolution weights into the forward and data-gradient operand images.
// The weight gradient of the convolutions, the one GEMM of the backward pass, is a unit of its own (wgrad.hip).  Data gradients need no kernel of their own:
// dX = conv(dZ, W rotated by 180 degrees with Cin <-> Cout swapped) runs on the forward implicit-GEMM / ping-pong / halo-patch kernels (the host repacks the
// weights once per step).
//
// Activations and their gradients are split16 NHWC tensors (conv_common.h): every kernel here decodes 8-channel groups to fp32, computes in
// fp32 (reductions in fp64, two-stage and in a fixed order => bit-reproducible) and re-splits.  All kernels are HBM-bound streaming kernels.
#include "conv_common.h"

namespace {

inline unsigned row_blocks(size_t M, int RPB) {                             // blocks of 256 / G rows, about 8 per CU at most
    const size_t b = (M + RPB - 1) / RPB;
    return (unsigned)(b > 2048 ? 2048 : (b ? b : 1));
}
#define RED_BLOCKS 512
// blocks of a two-stage column reduction over a [M][C] split16 tensor.  (Round 6 tried up to 1024 blocks chosen by tensor size, eight rows in flight per thread in the
// statistics pass and four in the apply kernels: bn_apply 3.96 -> 4.40 ms per training step, the backward sums 3.26 -> 3.69 ms, the statistics pass unchanged — the
// extra registers cost more occupancy than the loads in flight bought — and went back to this.)
inline unsigned red_blocks(size_t M, int C, int RPB) {
    (void)C;
    const size_t by_rows = (M + RPB - 1) / RPB;
    return (unsigned)(by_rows > RED_BLOCKS ? RED_BLOCKS : (by_rows ? by_rows : 1));
}
// (Round 6 swept rows in flight per thread {1, 2, 4} x stage-1 blocks {512 ... 4096} on the step's tensor shapes, profiles/r06_bn_sweep.txt: timed ALONE the three launches
// of a BatchNorm move their 3 (forward) / 5 (backward) passes at 4.9-5.9 TB/s on the U-Net's 100-400 MB tensors whatever U is, and 512 blocks is the best count at every size —
// more blocks only lengthen stage 2.  These kernels are at the HBM rate the part delivers; what is left to take out of BatchNorm is passes, not kernel tuning.)

// ---------------------------------------------------------------------------------------------------------------------------------
// per-channel sums over the rows of a [M][C] split16 tensor: S1 = sum f(x), S2 = sum g(x); two stages, fp64, fixed order
//   MODE 0 (statistics)      f = z,            g = z*z
//   MODE 1 (BN backward)     f = dyh,          g = dyh * xhat      with dyh = dy * [relu ? (xhat*gamma+beta > 0) : 1], xhat = (z-mean)*invstd
// ---------------------------------------------------------------------------------------------------------------------------------
// DEV = true: device-coherent accesses (relaxed agent-scope atomics) for values that workgroups of ONE launch hand to each other.  Unused by the shipped
// three-launch BatchNorm; the one-launch cooperative form that needed it was measured slower on this 8-XCD part (a grid barrier costs 15-20 us, a dependent
// launch less: DESIGN.md 8.9, profiles/r02ai_bn_one_launch_experiment.txt) and was removed from the library in round 3 (git history: train.hip @ 9afbeda).
template <bool DEV, typename T>
__device__ __forceinline__ void st_x(T* p, T v) {
    if (DEV) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
template <bool DEV, typename T>
__device__ __forceinline__ T ld_x(const T* p) {
    if (DEV) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <int MODE, bool DEV, int U = 4>
__device__ __forceinline__ void colsum_partial(const float* __restrict__ z, const float* __restrict__ dy, size_t M, int G,
                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                               const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                               double* __restrict__ part /*[blocks][C][2]*/, double* red /*[256 * 16] in LDS*/) {
    const int tid = threadIdx.x, g = tid % G, rl = tid / G, RPB = 256 / G;          // RPB rows in flight per block iteration; when G does not
    const bool active = rl < RPB;                                                   // divide 256 the last 256 - RPB*G threads only attend the barriers
    double s1[8], s2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { s1[q] = 0.0; s2[q] = 0.0; }
    float mu[8], is[8], ga[8], be[8];
    if (MODE == 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { mu[q] = mean[g * 8 + q]; is[q] = invstd[g * 8 + q]; ga[q] = gamma[g * 8 + q]; be[q] = beta[g * 8 + q]; }
    }
    // four rows per iteration: all their loads are issued before the first is consumed.  One row in flight per thread (8 waves per CU x 2 KB) is
    // 16 KB per CU against ~2 us of HBM latency = the 2.1-2.6 TB/s this kernel measured; the accumulation order per thread stays row-ascending.
    const size_t S = (size_t)gridDim.x * RPB;
    for (size_t r0 = (size_t)blockIdx.x * RPB + rl; active && r0 < M; r0 += U * S) {
        float v[U][8], d[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t r = r0 + u * S;
            if (r < M) {
                load_group(z + (r * G + g) * 8, v[u]);
                if (MODE == 1) load_group(dy + (r * G + g) * 8, d[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r0 + u * S >= M) break;
            if (MODE == 0) {
#pragma unroll
                for (int q = 0; q < 8; ++q) { s1[q] += (double)v[u][q]; s2[q] += (double)v[u][q] * (double)v[u][q]; }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float xh = (v[u][q] - mu[q]) * is[q];
                    const float dh = (relu && !(xh * ga[q] + be[q] > 0.f)) ? 0.f : d[u][q];
                    s1[q] += (double)dh; s2[q] += (double)dh * (double)xh;
                }
            }
        }
    }
    // reduce over the RPB row lanes of each channel group in a fixed order (row lane 0, 1, ...): all 16 sums of a thread go to LDS at once and
    // G * 16 threads each add up one (group, channel, which) column — one barrier, not sixteen, and no single thread walking 64 entries 8 times
    // (that serial tail, not the streaming loop, was most of this kernel: 2.1 TB/s)
    for (int q = 0; q < 8; ++q) { red[tid * 16 + q * 2] = s1[q]; red[tid * 16 + q * 2 + 1] = s2[q]; }
    __syncthreads();
    for (int o = tid; o < G * 16; o += 256) {
        const int gg = o >> 4, k = o & 15;
        double a = 0.0;
        for (int r = 0; r < RPB; ++r) a += red[(r * G + gg) * 16 + k];
        st_x<DEV>(&part[((size_t)blockIdx.x * G * 8 + gg * 8 + (k >> 1)) * 2 + (k & 1)], a);
    }
}
template <int MODE, int U = 4>
__global__ __launch_bounds__(256) void colsum_stage1(const float* __restrict__ z, const float* __restrict__ dy, size_t M, int G,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                                     double* __restrict__ part /*[blocks][C][2]*/) {
    __shared__ double red[256 * 16];
    colsum_partial<MODE, false, U>(z, dy, M, G, mean, invstd, gamma, beta, relu, part, red);
}

// stage 2: the <= 512 per-block partials of a channel are summed by 16 threads (strided, fixed order) and combined in LDS in a fixed order;
// one workgroup = 16 channels x 16 partial lanes.  (A single thread per channel walking 512 partials was 0.1 ms of pure load latency per launch.)
template <bool DEV = false>
__device__ __forceinline__ bool stage2_sum(const double* __restrict__ part, int nblocks, int C, int c, double& a, double& b, double (*red)[16][2]) {
    const int j = threadIdx.x >> 4, cl = threadIdx.x & 15;
    double sa = 0.0, sb = 0.0;
    if (c < C)
        // eight partials are loaded before the first is added (same addition order): the rolled loop waited for every load before issuing the next one —
        // 32 dependent L2 round trips, 13 us for a kernel with microseconds of work, 279 times per training step
        for (int k0 = j; k0 < nblocks; k0 += 16 * 8) {
            double va[8], vb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + 16 * u;
                const bool on = k < nblocks;
                va[u] = on ? ld_x<DEV>(&part[((size_t)k * C + c) * 2]) : 0.0;
                vb[u] = on ? ld_x<DEV>(&part[((size_t)k * C + c) * 2 + 1]) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { sa += va[u]; sb += vb[u]; }
        }
    red[j][cl][0] = sa; red[j][cl][1] = sb;
    __syncthreads();
    if (j != 0 || c >= C) return false;
    a = 0.0; b = 0.0;
    for (int k = 0; k < 16; ++k) { a += red[k][cl][0]; b += red[k][cl][1]; }
    return true;
}
// MODE 0: mean, biased variance, invstd, running-stat update (momentum; running_var takes the unbiased variance)
__global__ __launch_bounds__(256) void bn_finalize_kernel(const double* __restrict__ part, int nblocks, int C, double n, float eps, float momentum,
                                                          float* __restrict__ mean, float* __restrict__ var, float* __restrict__ invstd,
                                                          float* __restrict__ running_mean, float* __restrict__ running_var, long long* __restrict__ nbt) {
    __shared__ double red[16][16][2];
    if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;          // nn.BatchNorm2d.forward: num_batches_tracked.add_(1) (one launch less per layer)
    const int c = blockIdx.x * 16 + (threadIdx.x & 15);
    double a, b;
    if (!stage2_sum(part, nblocks, C, c, a, b, red)) return;
    const double m = a / n;
    double v = b / n - m * m;
    if (v < 0.0) v = 0.0;
    mean[c] = (float)m; var[c] = (float)v; invstd[c] = (float)(1.0 / sqrt(v + (double)eps));
    if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)m;
    if (running_var) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)(n > 1.0 ? v * n / (n - 1.0) : v);
}

// The same finalisation from the fp32 per-tile partial sums that the convolution kernels leave behind (ConvArgs::stats: [P][C][2] = (sum z, sum z^2) per partial row):
// one workgroup = 16 channels x 2 sums (one 128-byte segment of every partial row) x 32 row lanes; every thread adds its rows k*32 + rl in ascending order into
// eight interleaved fp64 chains (eight loads in flight), the chains and then the 32 row lanes are combined in a fixed order -> bit-reproducible run to run.
// P = M / 64 ... M / 128 partial rows: 98-196 for the 14 x 14 layers (one round trip), 12544 for a 112 x 112 layer at 64 frames (49 round trips of L2 hits).
__global__ __launch_bounds__(1024) void bn_finalize_partials_kernel(const float* __restrict__ part, int P, int C, double n, float eps, float momentum,
                                                                    float* __restrict__ mean, float* __restrict__ var, float* __restrict__ invstd,
                                                                    float* __restrict__ running_mean, float* __restrict__ running_var, long long* __restrict__ nbt) {
    __shared__ double red[32][33];
    if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
    const int t = threadIdx.x & 31, rl = threadIdx.x >> 5, c0 = blockIdx.x * 16;
    const bool on = c0 * 2 + t < C * 2;
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (on) {
        const float* p = part + (size_t)c0 * 2 + t;
        int k = rl;
        for (; k + 7 * 32 < P; k += 8 * 32) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(k + 32 * u) * C * 2];
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u] += (double)v[u];
        }
        for (int u = 0; k < P; k += 32, ++u) s[u] += (double)p[(size_t)k * C * 2];
    }
    red[rl][t] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (rl != 0 || !on) return;
    double a = 0.0;
    for (int k = 0; k < 32; ++k) a += red[k][t];
    const double b = __shfl_xor(a, 1, 64);                               // lanes (2c, 2c + 1) hold (sum z, sum z^2) of channel c0 + c
    if (t & 1) return;
    const int c = c0 + (t >> 1);
    const double m = a / n;
    double v = b / n - m * m;
    if (v < 0.0) v = 0.0;
    mean[c] = (float)m; var[c] = (float)v; invstd[c] = (float)(1.0 / sqrt(v + (double)eps));
    if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)m;
    if (running_var) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)(n > 1.0 ? v * n / (n - 1.0) : v);
}

// MODE 1 / plain column sums: out1[c] = S1, out2[c] = S2 (as fp32)
__global__ __launch_bounds__(256) void colsum_stage2(const double* __restrict__ part, int nblocks, int C, float* __restrict__ out1, float* __restrict__ out2) {
    __shared__ double red[16][16][2];
    const int c = blockIdx.x * 16 + (threadIdx.x & 15);
    double a, b;
    if (!stage2_sum(part, nblocks, C, c, a, b, red)) return;
    if (out1) out1[c] = (float)a;
    if (out2) out2[c] = (float)b;
}

// The two BatchNorm element-wise kernels give every thread a FIXED 8-channel group and let it walk rows (256 / G rows in flight per block), so
// the per-channel coefficients are loaded once into registers and no per-element index division is needed.
// y = [relu]( (z - mean) * invstd * gamma + beta [+ residual] )
template <bool DEV = false>
__device__ __forceinline__ void bn_apply_body(const float* __restrict__ z, size_t M, int G, const float* mean,
                                              const float* invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                              const float* __restrict__ residual, int relu, float* __restrict__ y) {
    const int tid = threadIdx.x, g = tid % G, rl = tid / G, RPB = 256 / G;
    if (rl >= RPB) return;
    float mu[8], is[8], ga[8], be[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { mu[q] = ld_x<DEV>(mean + g * 8 + q); is[q] = ld_x<DEV>(invstd + g * 8 + q); ga[q] = gamma[g * 8 + q]; be[q] = beta[g * 8 + q]; }
    for (size_t r = (size_t)blockIdx.x * RPB + rl; r < M; r += (size_t)gridDim.x * RPB) {
        const size_t i = r * G + g;
        float v[8];
        load_group(z + i * 8, v);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (v[q] - mu[q]) * is[q] * ga[q] + be[q];
        if (residual) {
            float rr[8];
            load_group(residual + i * 8, rr);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] += rr[q];
        }
        if (relu) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = fmaxf(v[q], 0.f);
        }
        store_group(y + i * 8, v);
    }
}
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, size_t M, int G, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ residual, int relu, float* __restrict__ y) {
    bn_apply_body(z, M, G, mean, invstd, gamma, beta, residual, relu, y);
}

// dz = gamma * invstd * (dyh - sum_dyh / n - xhat * sum_dyh_xhat / n)
template <bool DEV = false>
__device__ __forceinline__ void bn_backward_apply_body(const float* __restrict__ z, const float* __restrict__ dy, size_t M, int G, float inv_n,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* sum_dy, const float* sum_dy_xhat, int relu,
                                                       float* __restrict__ dz) {
    const int tid = threadIdx.x, g = tid % G, rl = tid / G, RPB = 256 / G;
    if (rl >= RPB) return;
    float mu[8], is[8], ga[8], be[8], s1[8], s2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = g * 8 + q;
        mu[q] = mean[c]; is[q] = invstd[c]; ga[q] = gamma[c]; be[q] = beta[c]; s1[q] = ld_x<DEV>(sum_dy + c) * inv_n; s2[q] = ld_x<DEV>(sum_dy_xhat + c) * inv_n;
    }
    for (size_t r = (size_t)blockIdx.x * RPB + rl; r < M; r += (size_t)gridDim.x * RPB) {
        const size_t i = r * G + g;
        float v[8], d[8];
        load_group(z + i * 8, v);
        load_group(dy + i * 8, d);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float xh = (v[q] - mu[q]) * is[q];
            const float dh = (relu && !(xh * ga[q] + be[q] > 0.f)) ? 0.f : d[q];
            v[q] = ga[q] * is[q] * (dh - s1[q] - xh * s2[q]);
        }
        store_group(dz + i * 8, v);
    }
}
__global__ __launch_bounds__(256) void bn_backward_apply_kernel(const float* __restrict__ z, const float* __restrict__ dy, size_t M, int G, float inv_n,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ sum_dy, const float* __restrict__ sum_dy_xhat, int relu,
                                                                float* __restrict__ dz) {
    bn_backward_apply_body(z, dy, M, G, inv_n, mean, invstd, gamma, beta, sum_dy, sum_dy_xhat, relu, dz);
}

// (Round 6 built a one-launch "finalise + apply" for tensors of <= 64 MB — element-wise workgroups owning a 32-channel column block and a row range, each reducing the
// partial rows of its own channels first — to drop the 279 tiny stage-2 launches of a training step.  Measured on the MI355X: the column-block mapping (four lanes per
// 128-byte row segment, rows C * 4 bytes apart) streams at 0.6-0.8 TB/s where the whole-row mapping below reaches 3-4.5 TB/s; the step went 41.2 -> 45.7 ms.  Removed
// again: on this part a dependent launch stays the cheap way to hand 2 KB of statistics to 2048 workgroups.  profiles/r06d_bench_train64_fin.txt)
// 2x2/2 max-pool backward: the gradient goes to the first maximum of the window in scan order (ATen's max_pool2d picks `val > max`), plus an
// optional second gradient of the same tensor (the U-Net skip connection) added in.  x, dx [B][H][W][G*8]; dy [B][H/2][W/2][G*8]
__global__ __launch_bounds__(256) void maxpool_backward_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ add,
                                                               float* __restrict__ dx, int B, int H, int W, int G) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)B * Ho * Wo * G;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int g = (int)(i % G);
        size_t t = i / G;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho);
        const int b = (int)(t / Ho);
        const size_t p00 = ((((size_t)b * H + 2 * oy) * W + 2 * ox) * G + g) * 8, sx = (size_t)G * 8, sy = (size_t)W * G * 8;
        float v[4][8], gy[8], o[4][8];
        load_group(x + p00, v[0]); load_group(x + p00 + sx, v[1]); load_group(x + p00 + sy, v[2]); load_group(x + p00 + sy + sx, v[3]);
        load_group(dy + i * 8, gy);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            int best = 0;
            float m = v[0][q];
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k][q] > m) { m = v[k][q]; best = k; }
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k][q] = (k == best) ? gy[q] : 0.f;
        }
        const size_t off[4] = {p00, p00 + sx, p00 + sy, p00 + sy + sx};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (add) {
                float a[8];
                load_group(add + off[k], a);
#pragma unroll
                for (int q = 0; q < 8; ++q) o[k][q] += a[q];
            }
            store_group(dx + off[k], o[k]);
        }
    }
}

// backward of ReflectionPad2d(1): dxp [B][H+2][W+2][G*8] -> dx [B][H][W][G*8] (+ optional add); padded index 0 mirrors row 1, H+1 mirrors row H-2
__global__ __launch_bounds__(256) void reflect_fold_kernel(const float* __restrict__ dxp, const float* __restrict__ add, float* __restrict__ dx, int B, int H,
                                                           int W, int G) {
    const size_t total = (size_t)B * H * W * G;
    const int Hp = H + 2, Wp = W + 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int g = (int)(i % G);
        size_t t = i / G;
        const int x = (int)(t % W); t /= W;
        const int y = (int)(t % H);
        const int b = (int)(t / H);
        int ys[2] = {y + 1, -1}, xs[2] = {x + 1, -1};
        if (y == 1) ys[1] = 0;
        if (y == H - 2) ys[1] = (ys[1] < 0) ? Hp - 1 : ys[1];            // H == 3: both borders mirror into row 1 (handled below)
        if (x == 1) xs[1] = 0;
        if (x == W - 2) xs[1] = (xs[1] < 0) ? Wp - 1 : xs[1];
        float acc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = 0.f;
        if (add) load_group(add + i * 8, acc);
        // general form (also right for H or W == 3, where a row collects both borders): walk all padded rows / cols that reflect onto (y, x)
        for (int yp = 0; yp < Hp; ++yp) {
            int ry = yp - 1; ry = ry < 0 ? -ry : ry; ry = ry >= H ? 2 * H - 2 - ry : ry;
            if (ry != y) continue;
            for (int xp = 0; xp < Wp; ++xp) {
                int rx = xp - 1; rx = rx < 0 ? -rx : rx; rx = rx >= W ? 2 * W - 2 - rx : rx;
                if (rx != x) continue;
                float v[8];
                load_group(dxp + ((((size_t)b * Hp + yp) * Wp + xp) * G + g) * 8, v);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[q] += v[q];
            }
        }
        (void)ys; (void)xs;
        store_group(dx + i * 8, acc);
    }
}

// ConvTranspose2d(k=2, s=2) output gradient [B][2H][2W][Co] -> [B][H][W][(dy,dx,co)] : the layout in which its input gradient is a 1x1 convolution
__global__ __launch_bounds__(256) void space_to_depth_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int H, int W, int G) {
    const size_t total = (size_t)B * H * W * 4 * G;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int g = (int)(i % G);
        size_t t = i / G;
        const int q = (int)(t % 4); t /= 4;
        const int x = (int)(t % W); t /= W;
        const int y = (int)(t % H);
        const int b = (int)(t / H);
        const float* src = in + ((((size_t)b * 2 * H + 2 * y + (q >> 1)) * 2 * W + 2 * x + (q & 1)) * G + g) * 8;
        *(f32x4*)(out + i * 8) = *(const f32x4*)src;
        *(f32x4*)(out + i * 8 + 4) = *(const f32x4*)(src + 4);
    }
}

// final 1x1 conv + sigmoid backward (smirk_generator.py:47-49,76): dl[o] = dy * y * (1 - y) -> dl8 (split16, [pixels][8], channels >= Cout zero: the
// "output gradient" operand from which the generic weight-gradient / column-sum kernels produce dW and db deterministically);
// dd[c] = sum_o dl[o] w[o][c] (split16 out)
__global__ __launch_bounds__(256) void final_backward_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ w,
                                                             float* __restrict__ dd, float* __restrict__ dl8, int B, int HW, int C, int Cout) {
    const size_t total = (size_t)B * HW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / HW, p = i % HW;
        float dl[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (o < Cout) {
                const float yy = y[(b * Cout + o) * HW + p];
                dl[o] = dy[(b * Cout + o) * HW + p] * yy * (1.0f - yy);
            }
        store_group(dl8 + i * 8, dl);
        for (int g = 0; g < C / 8; ++g) {
            float o8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float s = 0.f;
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (o < Cout) s = fmaf(dl[o], w[o * C + g * 8 + q], s);
                o8[q] = s;
            }
            store_group(dd + (i * (C / 8) + g) * 8, o8);
        }
    }
}

// One launch per convolution and training step: nn.Conv2d weight [Cout][Cin][KH][KH] fp32 -> the two split16 operand images the step needs,
//   fwd  [Cout][(ky,kx,c)]        c < cin_pad (zero beyond Cin)                      : the forward implicit-GEMM weight
//   dgr  [cin_pad][(ky',kx',co)]  = W[co][ci][KH-1-ky'][KH-1-kx'] (zero rows beyond Cin): the data-gradient convolution's weight (180-degree rotation,
//                                                                                        Cin <-> Cout); for KH = 1 simply the transpose.
__global__ __launch_bounds__(256) void pack_conv_weights_kernel(const float* __restrict__ w, int Cout, int cin_total, int cin_off, int Cin, int KH, int cin_pad,
                                                                float* __restrict__ fwd, float* __restrict__ dgr) {
    const int T = KH * KH;
    const size_t nf = (size_t)Cout * T * cin_pad / 8, nd = (size_t)cin_pad * T * Cout / 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nf + nd; i += (size_t)gridDim.x * blockDim.x) {
        float v[8];
        if (i < nf) {
            if (!fwd) continue;
            const size_t k0 = (i * 8) % ((size_t)T * cin_pad);
            const int co = (int)((i * 8) / ((size_t)T * cin_pad)), tap = (int)(k0 / cin_pad), c0 = (int)(k0 % cin_pad);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (c0 + q < Cin) ? w[((size_t)co * cin_total + cin_off + c0 + q) * T + tap] : 0.f;
            store_group(fwd + i * 8, v);
        } else {
            if (!dgr) continue;
            const size_t j = i - nf, k0 = (j * 8) % ((size_t)T * Cout);
            const int ci = (int)((j * 8) / ((size_t)T * Cout)), tap = (int)(k0 / Cout), co0 = (int)(k0 % Cout);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (ci < Cin) ? w[((size_t)(co0 + q) * cin_total + cin_off + ci) * T + (T - 1 - tap)] : 0.f;
            store_group(dgr + j * 8, v);
        }
    }
}

// every weight of a network in ONE launch: job j owns the vector range [start_j, start_{j+1}) of the flattened work list; a thread finds its job by
// binary search (<= 8 steps for 256 jobs).  A training step re-packed its 59 convolution weights with 118 launches of ~13 us each.
__global__ __launch_bounds__(256) void pack_conv_weights_batch_kernel(const SmirkPackJob* __restrict__ jobs, int njobs, unsigned long long total) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * blockDim.x) {
        int lo = 0, hi = njobs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].start <= i) lo = mid; else hi = mid - 1;
        }
        const SmirkPackJob J = jobs[lo];
        const size_t li = (size_t)(i - J.start);
        if (J.KH == SMIRK_PACK_DEPTHWISE) {                        // nn.Conv2d(C, C, 3, groups=C) weight [C][1][3][3] -> fp32 [9][C] (the depthwise kernels' tap-major image)
            const int k = (int)((li * 8) / (size_t)J.Cout), c0 = (int)((li * 8) % (size_t)J.Cout);
            float* o = (float*)J.fwd + li * 8;
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = J.w[(size_t)(c0 + q) * 9 + k];
            continue;
        }
        if (J.KH == SMIRK_PACK_STEM) {                             // Conv2d(3, Cout, 3) weight [Cout][3][3][3] -> fp32 [Cout][(ky,kx,c)]; one item = one float (27 per row)
            const int co = (int)(li / 27), k = (int)(li % 27), c = k % 3, t = k / 3;
            ((float*)J.fwd)[li] = J.w[((size_t)co * 3 + c) * 9 + t];
            continue;
        }
        if (J.KH == SMIRK_PACK_CONVT2X2) {                         // nn.ConvTranspose2d(Cin_t, Cout_t, 2, 2) weight [Cin_t][Cout_t][2][2]; Cout = Cin_t, Cin = Cout_t here
            const int Ci = J.Cout, Co = J.Cin;                     //   fwd   [(dydx, co)][ci]  split16: the forward 1x1 form (out_mode CONVT2X2)
            const size_t nfw = J.fwd ? (size_t)4 * Co * Ci / 8 : 0; //   dgrad [ci][(dydx, co)]  split16: its data gradient (a 1x1 convolution over the space-to-depth gradient)
            float v[8];
            if (li < nfw) {
                const int row = (int)((li * 8) / (size_t)Ci), ci0 = (int)((li * 8) % (size_t)Ci), t = row / Co, co = row % Co;
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = J.w[((size_t)(ci0 + q) * Co + co) * 4 + t];
                store_group((float*)J.fwd + li * 8, v);
            } else {
                const size_t j = li - nfw;
                const int ci = (int)((j * 8) / (size_t)(4 * Co)), col = (int)((j * 8) % (size_t)(4 * Co)), t = col / Co, co0 = col % Co;
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = J.w[((size_t)ci * Co + co0 + q) * 4 + t];
                store_group((float*)J.dgrad + j * 8, v);
            }
            continue;
        }
        const int T = J.KH * J.KH;
        const size_t nf = J.fwd ? (size_t)J.Cout * T * J.cin_pad / 8 : 0;
        float v[8];
        if (li < nf) {
            const size_t k0 = (li * 8) % ((size_t)T * J.cin_pad);
            const int co = (int)((li * 8) / ((size_t)T * J.cin_pad)), tap = (int)(k0 / J.cin_pad), c0 = (int)(k0 % J.cin_pad);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (c0 + q < J.Cin) ? J.w[((size_t)co * J.cin_total + J.cin_off + c0 + q) * T + tap] : 0.f;
            store_group((float*)J.fwd + li * 8, v);
        } else {
            const size_t j = li - nf, k0 = (j * 8) % ((size_t)T * J.Cout);
            const int ci = (int)((j * 8) / ((size_t)T * J.Cout)), tap = (int)(k0 / J.Cout), co0 = (int)(k0 % J.Cout);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (ci < J.Cin) ? J.w[((size_t)(co0 + q) * J.cin_total + J.cin_off + ci) * T + (T - 1 - tap)] : 0.f;
            store_group((float*)J.dgrad + j * 8, v);
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int smirk_pack_conv_weights_batch_split16(const SmirkPackJob* jobs_device, int njobs, unsigned long long total_vectors, void* stream) {
    if (!jobs_device || njobs <= 0 || njobs > 4096 || total_vectors == 0) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(pack_conv_weights_batch_kernel, dim3(blocks_for((size_t)total_vectors, 8192)), dim3(256), 0, (hipStream_t)stream, jobs_device, njobs, total_vectors);
    return smirk_launch_status();
}

extern "C" int smirk_pack_conv_weights_split16(const float* w, int Cout, int cin_total, int cin_off, int Cin, int KH, int cin_pad, void* fwd, void* dgrad,
                                               void* stream) {
    if (!w || (!fwd && !dgrad) || Cout <= 0 || Cin <= 0 || cin_off < 0 || cin_off + Cin > cin_total || Cout % 8 || cin_pad % 8 || cin_pad < Cin ||
        (KH != 1 && KH != 3))
        return SMIRK_ERR_BAD_ARG;
    const size_t n = ((size_t)Cout * KH * KH * cin_pad + (size_t)cin_pad * KH * KH * Cout) / 8;
    SMIRK_LAUNCH(pack_conv_weights_kernel, dim3(blocks_for(n, 4096)), dim3(256), 0, (hipStream_t)stream, w, Cout, cin_total, cin_off, Cin, KH, cin_pad, (float*)fwd, (float*)dgrad);
    return smirk_launch_status();
}

extern "C" size_t smirk_train_reduce_workspace_bytes(int C) { return (size_t)RED_BLOCKS * (size_t)C * 2 * sizeof(double); }

extern "C" int smirk_bn_train_forward_split16(const void* z, size_t M, int C, const float* gamma, const float* beta, const void* residual, int relu,
                                              float eps, float momentum, float* running_mean, float* running_var, long long* num_batches_tracked,
                                              float* save_mean, float* save_var, float* save_invstd, void* y, void* ws, size_t ws_bytes, void* stream) {
    if (!z || !gamma || !beta || !save_mean || !save_var || !save_invstd || !y || !ws || M == 0 || C <= 0 || C % 8 || C / 8 > 256) return SMIRK_ERR_BAD_ARG;
    if (ws_bytes < smirk_train_reduce_workspace_bytes(C)) return SMIRK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int G = C / 8, RPB = 256 / G;
    const unsigned nb = red_blocks(M, C, RPB);
    smirk_prof_next(nullptr, 0.0, (double)M * C * 4);
    SMIRK_LAUNCH(colsum_stage1<0>, dim3(nb), dim3(256), 0, st, (const float*)z, (const float*)nullptr, M, G, (const float*)nullptr, (const float*)nullptr,
                 (const float*)nullptr, (const float*)nullptr, 0, (double*)ws);
    SMIRK_LAUNCH(bn_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, st, (const double*)ws, (int)nb, C, (double)M, eps, momentum, save_mean, save_var,
                 save_invstd, running_mean, running_var, num_batches_tracked);
    smirk_prof_next(nullptr, 0.0, (double)M * C * 4 * (residual ? 3 : 2));
    SMIRK_LAUNCH(bn_apply_kernel, dim3(row_blocks(M, RPB)), dim3(256), 0, st, (const float*)z, M, G, (const float*)save_mean,
                 (const float*)save_invstd, gamma, beta, (const float*)residual, relu, (float*)y);
    return smirk_launch_status();
}

/* The same BatchNorm forward when the convolution that produced z already left the per-tile partial sums of z (smirk_conv_igemm_stats_split16, rows > 0):
 * finalise from the P partial rows (fixed-order fp64) + apply — the statistics pass over z and one launch are gone. */
extern "C" int smirk_bn_train_forward_partials_split16(const void* z, size_t M, int C, const float* gamma, const float* beta, const void* residual, int relu,
                                                       float eps, float momentum, float* running_mean, float* running_var, long long* num_batches_tracked,
                                                       float* save_mean, float* save_var, float* save_invstd, void* y, const void* partials_v, int P,
                                                       int partials_fp64, void* stream) {
    if (!z || !gamma || !beta || !save_mean || !save_var || !save_invstd || !y || !partials_v || P <= 0 || M == 0 || C <= 0 || C % 8 || C / 8 > 256)
        return SMIRK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int G = C / 8, RPB = 256 / G;
    if (partials_fp64) {                                             // stage-1 rows of a reduction kernel (smirk_dwconv3x3_stats_split16): [P][C][2] doubles
        SMIRK_LAUNCH(bn_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, st, (const double*)partials_v, P, C, (double)M, eps, momentum, save_mean, save_var,
                     save_invstd, running_mean, running_var, num_batches_tracked);
        smirk_prof_next(nullptr, 0.0, (double)M * C * 4 * (residual ? 3 : 2));
        SMIRK_LAUNCH(bn_apply_kernel, dim3(row_blocks(M, RPB)), dim3(256), 0, st, (const float*)z, M, G, (const float*)save_mean, (const float*)save_invstd, gamma,
                     beta, (const float*)residual, relu, (float*)y);
        return smirk_launch_status();
    }
    const float* partials = (const float*)partials_v;
    SMIRK_LAUNCH(bn_finalize_partials_kernel, dim3((C + 15) / 16), dim3(1024), 0, st, partials, P, C, (double)M, eps, momentum, save_mean, save_var, save_invstd,
                 running_mean, running_var, num_batches_tracked);
    smirk_prof_next(nullptr, 0.0, (double)M * C * 4 * (residual ? 3 : 2));
    SMIRK_LAUNCH(bn_apply_kernel, dim3(row_blocks(M, RPB)), dim3(256), 0, st, (const float*)z, M, G, (const float*)save_mean,
                 (const float*)save_invstd, gamma, beta, (const float*)residual, relu, (float*)y);
    return smirk_launch_status();
}

extern "C" int smirk_bn_train_backward_split16(const void* z, const void* dy, size_t M, int C, const float* gamma, const float* beta, const float* save_mean,
                                               const float* save_invstd, int relu, void* dz, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                                               void* stream) {
    if (!z || !dy || !gamma || !beta || !save_mean || !save_invstd || !dz || !dgamma || !dbeta || !ws || M == 0 || C <= 0 || C % 8 || C / 8 > 256)
        return SMIRK_ERR_BAD_ARG;
    if (ws_bytes < smirk_train_reduce_workspace_bytes(C)) return SMIRK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int G = C / 8, RPB = 256 / G;
    const unsigned nb = red_blocks(M, C, RPB);
    SMIRK_LAUNCH(colsum_stage1<1>, dim3(nb), dim3(256), 0, st, (const float*)z, (const float*)dy, M, G, save_mean, save_invstd, gamma, beta, relu, (double*)ws);
    SMIRK_LAUNCH(colsum_stage2, dim3((C + 15) / 16), dim3(256), 0, st, (const double*)ws, (int)nb, C, dbeta, dgamma);
    smirk_prof_next(nullptr, 0.0, (double)M * C * 4 * 3);
    SMIRK_LAUNCH(bn_backward_apply_kernel, dim3(row_blocks(M, RPB)), dim3(256), 0, st, (const float*)z, (const float*)dy, M, G,
                 (float)(1.0 / (double)M), save_mean, save_invstd, gamma, beta, (const float*)dbeta, (const float*)dgamma, relu, (float*)dz);
    return smirk_launch_status();
}

// ---- eval-mode BatchNorm of the differentiable generator (smirk_trainer.py:108-113: the frozen generator in .eval() inside a graph that is
//      back-propagated to its input): y = [relu]((z - running_mean) * rsqrt(running_var + eps) * gamma + beta [+ residual]); the backward is the same
//      element-wise kernel as in train mode with the two batch sums set to zero (dz = gamma * invstd * dy * relu mask).  No statistics, no reduction.
__global__ __launch_bounds__(256) void bn_invstd_kernel(const float* __restrict__ var, float eps, int C, float* __restrict__ invstd, float* __restrict__ zeros) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) { invstd[c] = 1.0f / sqrtf(var[c] + eps); zeros[c] = 0.f; }
}

extern "C" int smirk_bn_eval_forward_split16(const void* z, size_t M, int C, const float* gamma, const float* beta, const float* running_mean,
                                             const float* running_var, const void* residual, int relu, float eps, float* save_invstd, float* zeros,
                                             void* y, void* stream) {
    if (!z || !gamma || !beta || !running_mean || !running_var || !save_invstd || !zeros || !y || M == 0 || C <= 0 || C % 8 || C / 8 > 256)
        return SMIRK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int G = C / 8, RPB = 256 / G;
    SMIRK_LAUNCH(bn_invstd_kernel, dim3((C + 255) / 256), dim3(256), 0, st, running_var, eps, C, save_invstd, zeros);
    smirk_prof_next(nullptr, 0.0, (double)M * C * 4 * (residual ? 3 : 2));
    SMIRK_LAUNCH(bn_apply_kernel, dim3(row_blocks(M, RPB)), dim3(256), 0, st, (const float*)z, M, G, running_mean, (const float*)save_invstd, gamma, beta,
                 (const float*)residual, relu, (float*)y);
    return smirk_launch_status();
}

extern "C" int smirk_bn_eval_backward_split16(const void* z, const void* dy, size_t M, int C, const float* gamma, const float* beta,
                                              const float* running_mean, const float* invstd, const float* zeros, int relu, void* dz, void* stream) {
    if (!z || !dy || !gamma || !beta || !running_mean || !invstd || !zeros || !dz || M == 0 || C <= 0 || C % 8 || C / 8 > 256) return SMIRK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int G = C / 8, RPB = 256 / G;
    smirk_prof_next(nullptr, 0.0, (double)M * C * 4 * 3);
    SMIRK_LAUNCH(bn_backward_apply_kernel, dim3(row_blocks(M, RPB)), dim3(256), 0, st, (const float*)z, (const float*)dy, M, G, 0.0f, running_mean, invstd,
                 gamma, beta, zeros, zeros, relu, (float*)dz);
    return smirk_launch_status();
}

extern "C" int smirk_colsum_split16(const void* x, size_t M, int C, float* sums, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !sums || !ws || M == 0 || C <= 0 || C % 8 || C / 8 > 256) return SMIRK_ERR_BAD_ARG;
    if (ws_bytes < smirk_train_reduce_workspace_bytes(C)) return SMIRK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int G = C / 8, RPB = 256 / G;
    const unsigned nb = red_blocks(M, C, RPB);
    SMIRK_LAUNCH(colsum_stage1<0>, dim3(nb), dim3(256), 0, st, (const float*)x, (const float*)nullptr, M, G, (const float*)nullptr, (const float*)nullptr,
                 (const float*)nullptr, (const float*)nullptr, 0, (double*)ws);
    SMIRK_LAUNCH(colsum_stage2, dim3((C + 15) / 16), dim3(256), 0, st, (const double*)ws, (int)nb, C, sums, (float*)nullptr);
    return smirk_launch_status();
}

extern "C" int smirk_maxpool2x2_backward_split16(const void* x, const void* dy, const void* add, void* dx, int B, int H, int W, int C, void* stream) {
    if (!x || !dy || !dx || B <= 0 || H % 2 || W % 2 || C % 8 || C <= 0) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(maxpool_backward_kernel, dim3(blocks_for((size_t)B * (H / 2) * (W / 2) * (C / 8), 16384)), dim3(256), 0, (hipStream_t)stream,
                 (const float*)x, (const float*)dy, (const float*)add, (float*)dx, B, H, W, C / 8);
    return smirk_launch_status();
}

extern "C" int smirk_reflect_pad1_backward_split16(const void* dxp, const void* add, void* dx, int B, int H, int W, int C, void* stream) {
    if (!dxp || !dx || B <= 0 || H < 2 || W < 2 || C % 8 || C <= 0) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(reflect_fold_kernel, dim3(blocks_for((size_t)B * H * W * (C / 8), 16384)), dim3(256), 0, (hipStream_t)stream, (const float*)dxp,
                 (const float*)add, (float*)dx, B, H, W, C / 8);
    return smirk_launch_status();
}

extern "C" int smirk_space_to_depth2_split16(const void* in, void* out, int B, int H, int W, int C, void* stream) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || C % 8 || C <= 0) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(space_to_depth_kernel, dim3(blocks_for((size_t)B * H * W * 4 * (C / 8), 16384)), dim3(256), 0, (hipStream_t)stream, (const float*)in,
                 (float*)out, B, H, W, C / 8);
    return smirk_launch_status();
}

extern "C" int smirk_conv1x1_sigmoid_backward_split16(const float* dy, const float* y, const float* w, void* dd, void* dl8, int B, int H, int W, int C,
                                                      int Cout, void* stream) {
    if (!dy || !y || !w || !dd || !dl8 || B <= 0 || C % 8 || C <= 0 || Cout <= 0 || Cout > 4) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(final_backward_kernel, dim3(blocks_for((size_t)B * H * W, 16384)), dim3(256), 0, (hipStream_t)stream, dy, y, w, (float*)dd, (float*)dl8, B,
                 H * W, C, Cout);
    return smirk_launch_status();
}
