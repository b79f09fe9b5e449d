// Mesh-based masking utilities for MI355X (gfx950) — the step between Renderer and SmirkGenerator
// (src/utils/masking.py:39-181; callers demo.py:146-167, smirk_trainer.py:76-93,268-293).  All HBM/latency-bound integer + fp32 work:
//   mask_face_weights   per (image, FLAME triangle): mean z of its 3 vertex normals, visibility gate (< 0.05), xy shoelace area,
//                       region probability  -> sampling weight                                  (masking.py:144-160)
//   sample_faces        one workgroup per image: LDS prefix sum of the 9976 weights (the CDF), then every lane draws with a counter-
//                       based Philox4x32-10 generator and binary-searches the CDF (multinomial with replacement) and draws the
//                       folded-uniform barycentrics                                            (masking.py:51-68,163-166)
//   points_to_pixels    .5*(1+p)*S -> int64 (truncation) -> clamp x,y                          (masking.py:172-175)
//   maxpool_sq          (2r+1)^2 stride-1 max pool with -inf padding as two separable passes   (masking.py:78,96)
//   bernoulli_field / masking_compose / transfer_pixels                                        (masking.py:71-102,116-129)
//   masking_handoff / sample_transfer_points + train_masking_handoff     the chains above fused for the inference path (smirk_handoff.h) and
//                       for the trainer's two paths (smirk_train_handoff.h): same draws, same bits, the generator's packed input stored beside
// Random draws are reproducible from (seed, call offset) but are NOT torch's CPU/CUDA streams — the reference itself draws
// different numbers on CPU and GPU; deterministic entry points (coords= / explicit fields) are what the parity tests pin.
#include "conv_common.h"
#include "../../include/smirk_handoff.h"
#include "../../include/smirk_train_handoff.h"

// ---- Philox4x32-10 (Salmon et al. 2011), counter = (idx, stream, 0, 0), key = seed ------------------------------------------------
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                           uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }   // [0,1), 24 bits like torch.rand

__global__ __launch_bounds__(256) void mask_face_weights_kernel(const float* __restrict__ tv, const float* __restrict__ normals,
                                                                const int32_t* __restrict__ faces, const float* __restrict__ prob,
                                                                int B, int V, int F, float* __restrict__ w) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * F) return;
    const int b = (int)(i / F), f = (int)(i % F);
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    const float* nb = normals + (size_t)b * V * 3;
    const float* vb = tv + (size_t)b * V * 3;
    const float nz = ((nb[i0 * 3 + 2] + nb[i1 * 3 + 2]) + nb[i2 * 3 + 2]) / 3.0f;
    const float x1 = vb[i0 * 3], y1 = vb[i0 * 3 + 1], x2 = vb[i1 * 3], y2 = vb[i1 * 3 + 1], x3 = vb[i2 * 3], y3 = vb[i2 * 3 + 1];
    const float area = 0.5f * fabsf(x1 * y2 + x2 * y3 + x3 * y1 - x2 * y1 - x3 * y2 - x1 * y3);
    const float p = (nz < 0.05f) ? prob[f] : 0.0f;
    w[i] = p * area;
}

// The CDF of one frame's face weights into LDS: cdf [F] inclusive prefix sums, wtot [blockDim / 64] wave totals.  Returns the total.  Block scan in chunks of
// blockDim: the sequential carry keeps the summation order fixed (deterministic).  Shared by sample_faces_kernel and sample_transfer_points_kernel.
__device__ __forceinline__ float face_cdf_scan(const float* __restrict__ wb, int F, float* cdf, float* wtot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    float carry = 0.f;
    for (int base = 0; base < F; base += blockDim.x) {
        const int i = base + tid;
        float v = (i < F) ? wb[i] : 0.f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
        if (lane == 63) wtot[wave] = v;
        __syncthreads();
        float pre = carry;
        for (int k = 0; k < wave; ++k) pre += wtot[k];
        if (i < F) cdf[i] = v + pre;
        float all = carry;
        for (int k = 0; k < nw; ++k) all += wtot[k];
        __syncthreads();
        carry = all;
    }
    return carry;
}

// draw `ctr` of stream 0: the sampled face (multinomial with replacement over the CDF) and its folded-uniform barycentrics
__device__ __forceinline__ int face_draw(const float* cdf, int F, float total, uint64_t seed, uint64_t ctr, float bc[3]) {
    uint32_t r[4];
    philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float target = u01(r[0]) * total;
    int lo = 0, hi = F - 1;                      // first index whose cdf exceeds target (zero-weight faces are never chosen)
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdf[mid] > target) hi = mid; else lo = mid + 1; }
    float u = u01(r[1]), v = u01(r[2]);
    if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }                           // masking.py:58-60
    bc[0] = 1.0f - (u + v); bc[1] = u; bc[2] = v;                               // masking.py:63-68
    return lo;
}

__global__ __launch_bounds__(1024) void sample_faces_kernel(const float* __restrict__ w, int F, int num, uint64_t seed,
                                                            uint64_t offset, int32_t* __restrict__ idx, float* __restrict__ bary) {
    extern __shared__ float cdf[];               // [F] inclusive prefix sums, + 32 wave totals
    const int b = blockIdx.x;
    const float total = face_cdf_scan(w + (size_t)b * F, F, cdf, cdf + F);
    for (int t = threadIdx.x; t < num; t += blockDim.x) {
        float bc[3];
        idx[(size_t)b * num + t] = face_draw(cdf, F, total, seed, offset + (uint64_t)b * num + t, bc);
        float* o = bary + ((size_t)b * num + t) * 3;
        o[0] = bc[0]; o[1] = bc[1]; o[2] = bc[2];
    }
}

__global__ __launch_bounds__(256) void points_to_pixels_kernel(const float* __restrict__ p, size_t n, int S, long long* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = 0.5f * (1.0f + p[i * 3 + c]) * (float)S;               // masking.py:172
        long long q = (long long)v;                                             // .long(): truncation toward zero
        if (c < 2) q = q < 0 ? 0 : (q > S - 1 ? S - 1 : q);                     // masking.py:174-175
        out[i * 3 + c] = q;
    }
}

// one pass of a separable (2r+1) max filter with -inf padding; dir 0 = along x, 1 = along y.  in/out [B][H][W]
// Generic fallback (any radius / width); the shipped sizes take maxpool_sq_lds_kernel below.  vectorize(disable): the loop vectoriser turned
// the complement + max chain into v_pk_add_f32, an instruction class that must not appear in this library (build.py).
__global__ __launch_bounds__(256) void maxfilter1d_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int H, int W,
                                                          int r, int dir, int complement_in, int complement_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const size_t base = i - (size_t)y * W - x;
    float m = -INFINITY;
    if (dir == 0) {
        const int lo = max(x - r, 0), hi = min(x + r, W - 1);
#pragma clang loop vectorize(disable) interleave(disable)
        for (int k = lo; k <= hi; ++k) { float v = in[base + (size_t)y * W + k]; if (complement_in) v = 1.0f - v; m = fmaxf(m, v); }
    } else {
        const int lo = max(y - r, 0), hi = min(y + r, H - 1);
#pragma clang loop vectorize(disable) interleave(disable)
        for (int k = lo; k <= hi; ++k) { float v = in[base + (size_t)k * W + x]; if (complement_in) v = 1.0f - v; m = fmaxf(m, v); }
    }
    out[i] = complement_out ? 1.0f - m : m;
}

// (2R+1)^2 max pool, both passes in ONE launch: a workgroup owns MP_ROWS output rows of one image over the full width.  It stages the
// rows [y0-R, y0+MP_ROWS+R) once in LDS (complemented on the way in if asked; -inf outside the image and in an R-wide margin left and
// right), runs the x pass LDS -> LDS with every thread producing 4 neighbouring outputs from 4+2R staged values (6 LDS reads per output
// instead of 21 global ones), then the y pass the same way down a column (lanes are neighbouring x: conflict-free) and writes the result.
// max is exact and order-free, so the output equals the two-pass form bit for bit (tests/test_masking_gpu.py).
#define MP_ROWS 32
__host__ __device__ static inline int mp_row_stride(int W, int R) { return (W + 3) / 4 * 4 + (2 * R + 3) / 4 * 4 + 4; }
template <int R>
__global__ __launch_bounds__(512) void maxpool_sq_lds_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                            int complement_in, int complement_out) {
    extern __shared__ __attribute__((aligned(16))) float mp_lds[];
    // staged row stride: the W + 2R columns (margins included) rounded up so that every thread's 4 + 2R window, read as whole 16-byte vectors, stays inside its
    // row.  The x pass reads the window of a lane with ds_read_b128 (lane stride 16 bytes: conflict-free); as scalar reads at a lane stride of 4 floats every
    // access was a 4-way bank conflict - 58-64 % of this kernel's LDS cycles (profiles/r03v_pmc_census_full.txt).
    const int SW = mp_row_stride(W, R);
    const int NR = MP_ROWS + 2 * R;                     // staged rows
    float* A = mp_lds;                                  // [NR][SW]  input rows
    float* Hx = mp_lds + NR * SW;                       // [NR][W]   after the x pass
    const int tiles = (H + MP_ROWS - 1) / MP_ROWS;
    const int b = blockIdx.x / tiles, y0 = (blockIdx.x % tiles) * MP_ROWS;
    const float* src = in + (size_t)b * H * W;
    // eight requests in flight per lane and trip, clamped addresses + select: a rolled load -> store loop pays one dependent global round trip per iteration (25 of them)
    for (int base = 0; base < NR * SW; base += 512 * 8) {
        float sv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + 512 * u + (int)threadIdx.x, rr = i / SW, cx = i - rr * SW - R, y = y0 - R + rr;
            const bool in = i < NR * SW && y >= 0 && y < H && cx >= 0 && cx < W;
            const float t = src[(size_t)min(max(y, 0), H - 1) * W + min(max(cx, 0), W - 1)];
            sv[u] = in ? (complement_in ? 1.0f - t : t) : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + 512 * u + (int)threadIdx.x;
            if (i < NR * SW) A[i] = sv[u];
        }
    }
    __syncthreads();
    const int W4 = (W + 3) / 4;
    for (int i = threadIdx.x; i < NR * W4; i += 512) {
        const int rr = i / W4, x = (i - rr * W4) * 4;
        const f32x4* a4 = (const f32x4*)(A + rr * SW + x);   // a[k] = column x - R + k; 16-byte aligned: SW and x are multiples of 4
        constexpr int NV = (4 + 2 * R + 3) / 4;
        float v[4 * NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const f32x4 t = a4[j];
            v[4 * j] = t[0]; v[4 * j + 1] = t[1]; v[4 * j + 2] = t[2]; v[4 * j + 3] = t[3];
        }
        float c = v[3];
#pragma unroll
        for (int k = 4; k <= 2 * R; ++k) c = fmaxf(c, v[k]);
        const float o0 = fmaxf(fmaxf(c, v[2]), fmaxf(v[1], v[0]));
        const float o1 = fmaxf(fmaxf(c, v[2]), fmaxf(v[1], v[2 * R + 1]));
        const float o2 = fmaxf(fmaxf(c, v[2]), fmaxf(v[2 * R + 2], v[2 * R + 1]));
        const float o3 = fmaxf(fmaxf(c, v[2 * R + 3]), fmaxf(v[2 * R + 2], v[2 * R + 1]));
        float* h = Hx + rr * W + x;
        if ((W & 3) == 0) {                             // uniform: rows of Hx are 16-byte aligned
            const f32x4 o = {o0, o1, o2, o3};
            *(f32x4*)h = o;
        } else {
            h[0] = o0;
            if (x + 1 < W) h[1] = o1;
            if (x + 2 < W) h[2] = o2;
            if (x + 3 < W) h[3] = o3;
        }
    }
    __syncthreads();
    float* dst = out + (size_t)b * H * W;
    for (int i = threadIdx.x; i < (MP_ROWS / 4) * W; i += 512) {
        const int q = i / W, x = i - q * W;
        const float* h = Hx + (q * 4) * W + x;        // h[k * W] = staged row q*4 + k = image row y0 + q*4 - R + k
        float v[4 + 2 * R];
#pragma unroll
        for (int k = 0; k < 4 + 2 * R; ++k) v[k] = h[k * W];
        float c = v[3];
#pragma unroll
        for (int k = 4; k <= 2 * R; ++k) c = fmaxf(c, v[k]);
        float o[4];
        o[0] = fmaxf(fmaxf(c, v[2]), fmaxf(v[1], v[0]));
        o[1] = fmaxf(fmaxf(c, v[2]), fmaxf(v[1], v[2 * R + 1]));
        o[2] = fmaxf(fmaxf(c, v[2]), fmaxf(v[2 * R + 2], v[2 * R + 1]));
        o[3] = fmaxf(fmaxf(c, v[2 * R + 3]), fmaxf(v[2 * R + 2], v[2 * R + 1]));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = y0 + q * 4 + k;
            if (y < H) dst[(size_t)y * W + x] = complement_out ? 1.0f - o[k] : o[k];
        }
    }
}

__global__ __launch_bounds__(256) void bernoulli_field_kernel(float* __restrict__ out, size_t n, float p, uint64_t seed, uint64_t offset) {
    const size_t i4 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= n) return;
    uint32_t r[4];
    const uint64_t ctr = offset + i4 / 4;
    philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), 1u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i4 + k < n) out[i4 + k] = u01(r[k]) < p ? 1.0f : 0.0f;
}

// One element of masking(): masked = x * m; e = extra value (* noise) (* keep); out = e > 0 ? e : masked (masking.py:91-101).  The one place the expression is
// spelled: masking_compose_kernel and masking_handoff_kernel both call it, so the compiler contracts it the same way in both.  The generated noise is
// N(1, 0.05) by Box-Muller from Philox block `ctr` of stream 2.  Where e == 0 the draw is skipped: e * noise * keep is +-0 whatever the (finite) noise is, `e > 0`
// is false and the output is `masked` either way.  The comparison is false for a NaN, which takes the full path as before.
__device__ __forceinline__ float masking_compose1(float x, float m, float e, const float* noise_mult, int gen_noise, uint64_t seed, uint64_t ctr,
                                                  bool has_keep, float keep) {
    const float masked = x * m;
    if (noise_mult) e = e * *noise_mult;
    else if (gen_noise && !(e == 0.0f)) {
        uint32_t r[4];
        philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), 2u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        const float u1 = fmaxf(u01(r[0]), 5.96e-8f), u2 = u01(r[1]);
        const float z = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);      // Box-Muller
        e = e * (z * 0.05f + 1.0f);                                                          // masking.py:91-92
    }
    if (has_keep) e = e * keep;
    return (e > 0.0f) ? e : masked;                                                          // masking.py:101
}

// masked = img * mask * (1 - rendered_mask); extra = extra_points * (noise ? N(1, 0.05) : 1) * keep; out = extra > 0 ? extra : masked
// img / extra / out [B][C][H][W]; mask, rendered_mask, keep [B][1][H][W] (rendered_mask / keep nullable)
__global__ __launch_bounds__(256) void masking_compose_kernel(const float* __restrict__ img, const float* __restrict__ mask,
                                                              const float* __restrict__ rendered_mask,
                                                              const float* __restrict__ extra, const float* __restrict__ pmask,
                                                              const float* __restrict__ keep,
                                                              const float* __restrict__ noise_mult, int B, int C, int HW,
                                                              int gen_noise, uint64_t seed, uint64_t offset,
                                                              float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * C * HW) return;
    const size_t b = i / ((size_t)C * HW), p = i % HW;
    float m = mask[b * HW + p];
    if (rendered_mask) m = m * (1.0f - rendered_mask[b * HW + p]);
    const float e = extra ? extra[i] : img[i] * pmask[b * HW + p];                           // demo.py:163 extra_points = image * pmask
    out[i] = masking_compose1(img[i], m, e, noise_mult ? noise_mult + i : nullptr, gen_noise, seed, offset + i, keep != nullptr,
                              keep ? keep[b * HW + p] : 0.0f);
}

// ---- masking -> generator hand-off in ONE launch (include/smirk_handoff.h) ------------------------------------------------------------------
// What demo_masked_image -> SmirkGenerator.forward_pair ran as six launches (rendered_mask, maxpool_sq<10>, bernoulli_field, maxpool_sq<5>, masking_compose,
// pack_split): a workgroup owns HO_ROWS rows of one image over the full width and reads only img, rendered_img, the hull mask and pmask.
//   1  stage 1 - hull for rows [y0 - 10, y0 + HO_ROWS + 10) (A1) and draw the Bernoulli patch centres for rows [y0 - 5, y0 + HO_ROWS + 5) (A2): pixel i of the
//      [B][H][W] field is lane i % 4 of Philox block offset + i / 4 of stream 1, as bernoulli_field_kernel draws it, so a halo pixel is recomputed and never read;
//      -inf outside the image and in the margins, as the max pool pads
//   2  the x passes (21 and 11 taps) IN PLACE: a wave owns a whole staged row and walks it left to right, every lane reads its 4 + 2R window with ds_read_b128
//      (conflict-free, see maxpool_sq_lds_kernel) and writes its 4 maxima at the window's first 4 cells.  Reads precede the write in the wave's program order (LDS
//      operations of a wave retire in order) and a later 256-column step reads only cells at or right of its own outputs, so no second image of the rows is needed
//   3  per thread 4 rows of one column: the y passes from LDS (lanes are neighbouring x: conflict-free), the rendered mask from the three rendered_img values that
//      are loaded for the pack anyway, the composition (masking_compose1), masked_img and the split-fp16 NHWC group of pack_split_kernel
// LDS: (HO_ROWS + 20) * mp_row_stride(W, 10) + (HO_ROWS + 10) * mp_row_stride(W, 5) floats = 61,248 bytes at W = 224: two workgroups per CU.
#define HO_ROWS 16
#define HO_THREADS 512
#define HO_R1 10                                    // masking.py:78 through demo.py:161: the hull mask's erosion radius
#define HO_R2 5                                     // masking.py:96: 11 x 11 patches
static inline size_t ho_lds_bytes(int W) {
    return ((size_t)(HO_ROWS + 2 * HO_R1) * mp_row_stride(W, HO_R1) + (size_t)(HO_ROWS + 2 * HO_R2) * mp_row_stride(W, HO_R2)) * sizeof(float);
}

// A[rr][x] <- max(A[rr][x .. x + 2R]) for x < W, rr < NR; A[rr][c] holds column c - R on entry
template <int R>
__device__ __forceinline__ void ho_xpass_inplace(float* A, int NR, int SW, int W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W4 = (W + 3) / 4;
    for (int rr = wave; rr < NR; rr += HO_THREADS / 64) {
        for (int x4 = lane; x4 < W4; x4 += 64) {
            float* a = A + rr * SW + x4 * 4;                     // 16-byte aligned: SW is a multiple of 4
            const f32x4* a4 = (const f32x4*)a;
            constexpr int NV = (4 + 2 * R + 3) / 4;
            float v[4 * NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const f32x4 t = a4[j];
                v[4 * j] = t[0]; v[4 * j + 1] = t[1]; v[4 * j + 2] = t[2]; v[4 * j + 3] = t[3];
            }
            float c = v[3];
#pragma unroll
            for (int k = 4; k <= 2 * R; ++k) c = fmaxf(c, v[k]);
            const f32x4 o = {fmaxf(fmaxf(c, v[2]), fmaxf(v[1], v[0])), fmaxf(fmaxf(c, v[2]), fmaxf(v[1], v[2 * R + 1])),
                             fmaxf(fmaxf(c, v[2]), fmaxf(v[2 * R + 2], v[2 * R + 1])), fmaxf(fmaxf(c, v[2 * R + 3]), fmaxf(v[2 * R + 2], v[2 * R + 1]))};
            *(f32x4*)a = o;                                      // cells x4 * 4 + 3 >= W of a ragged row lie in the margin, which nobody reads again
        }
    }
}

// 4 consecutive outputs of a (2R+1)-tap column maximum: o[k] = max(h[(k .. k + 2R) * SW])
template <int R>
__device__ __forceinline__ void ho_ypass4(const float* h, int SW, float* o) {
    float v[4 + 2 * R];
#pragma unroll
    for (int k = 0; k < 4 + 2 * R; ++k) v[k] = h[k * SW];
    float c = v[3];
#pragma unroll
    for (int k = 4; k <= 2 * R; ++k) c = fmaxf(c, v[k]);
    o[0] = fmaxf(fmaxf(c, v[2]), fmaxf(v[1], v[0]));
    o[1] = fmaxf(fmaxf(c, v[2]), fmaxf(v[1], v[2 * R + 1]));
    o[2] = fmaxf(fmaxf(c, v[2]), fmaxf(v[2 * R + 2], v[2 * R + 1]));
    o[3] = fmaxf(fmaxf(c, v[2 * R + 3]), fmaxf(v[2 * R + 2], v[2 * R + 1]));
}

// stage 1a of the hand-off kernels: A1 [NR1][SW1] <- 1 - hull for rows [y0 - 10, y0 + HO_ROWS + 10), -inf outside the image and in the margins
__device__ __forceinline__ void ho_stage_hull(const float* __restrict__ hsrc, float* A1, int y0, int H, int W) {
    const int SW1 = mp_row_stride(W, HO_R1), tid = threadIdx.x;
    constexpr int NR1 = HO_ROWS + 2 * HO_R1;
    // ---- 1a: the hull rows (eight requests in flight per lane and trip, clamped addresses + select, as maxpool_sq_lds_kernel stages them) ----
    for (int base = 0; base < NR1 * SW1; base += HO_THREADS * 8) {
        float sv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + HO_THREADS * u + tid, rr = i / SW1, cx = i - rr * SW1 - HO_R1, y = y0 - HO_R1 + rr;
            const bool in = i < NR1 * SW1 && y >= 0 && y < H && cx >= 0 && cx < W;
            const float t = hsrc[(size_t)min(max(y, 0), H - 1) * W + min(max(cx, 0), W - 1)];
            sv[u] = in ? 1.0f - t : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + HO_THREADS * u + tid;
            if (i < NR1 * SW1) A1[i] = sv[u];
        }
    }
}

// stage 1b: A2 [NR2][SW2] <- the patch centres of rows [y0 - 5, y0 + HO_ROWS + 5) of image `b` of the flat [.][H][W] field, -inf outside the image
__device__ __forceinline__ void ho_stage_centres(float* A2, int b, int y0, int H, int W, float p_field, uint64_t seed, uint64_t field_offset) {
    const int SW2 = mp_row_stride(W, HO_R2), tid = threadIdx.x;
    constexpr int NR2 = HO_ROWS + 2 * HO_R2;
    const size_t HW = (size_t)H * W;
    // ---- 1b: the patch-centre rows.  Cells outside the image first, then one Philox block per 4 consecutive pixels of the flat field (disjoint cells: no barrier) ----
    for (int i = tid; i < NR2 * SW2; i += HO_THREADS) {
        const int rr = i / SW2, cx = i - rr * SW2 - HO_R2, y = y0 - HO_R2 + rr;
        if (!(y >= 0 && y < H && cx >= 0 && cx < W)) A2[i] = -INFINITY;
    }
    {
        const int ylo = max(y0 - HO_R2, 0), yhi = min(y0 + HO_ROWS + HO_R2, H);
        const size_t img0 = (size_t)b * HW, s = img0 + (size_t)ylo * W, e = img0 + (size_t)yhi * W;
        for (size_t g = s / 4 + tid; g * 4 < e; g += HO_THREADS) {
            uint32_t r[4];
            const uint64_t ctr = field_offset + g;
            philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), 1u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t i = g * 4 + k;
                if (i >= s && i < e) {
                    const int rel = (int)(i - img0), y = rel / W, x = rel - y * W;
                    A2[(y - (y0 - HO_R2)) * SW2 + x + HO_R2] = u01(r[k]) < p_field ? 1.0f : 0.0f;
                }
            }
        }
    }
}

// img / rendered / masked [B][3][H][W]; hull [B or 1][H][W] with batch stride hull_bs (0 or H * W); pmask [B][H][W]; packed [B][H][W][8] split-fp16 (32 bytes a pixel)
__global__ __launch_bounds__(HO_THREADS) void masking_handoff_kernel(const float* __restrict__ img, const float* __restrict__ rendered,
                                                                      const float* __restrict__ hull, size_t hull_bs, const float* __restrict__ pmask,
                                                                      int H, int W, float p_field, uint64_t seed, uint64_t field_offset,
                                                                      uint64_t noise_offset, float* __restrict__ masked, float* __restrict__ packed) {
    extern __shared__ __attribute__((aligned(16))) float ho_lds[];
    const int SW1 = mp_row_stride(W, HO_R1), SW2 = mp_row_stride(W, HO_R2);
    constexpr int NR1 = HO_ROWS + 2 * HO_R1, NR2 = HO_ROWS + 2 * HO_R2;
    float* A1 = ho_lds;                                 // [NR1][SW1]  1 - hull, then its x maxima
    float* A2 = ho_lds + NR1 * SW1;                     // [NR2][SW2]  patch centres, then their x maxima
    const int tiles = (H + HO_ROWS - 1) / HO_ROWS;
    const int b = blockIdx.x / tiles, y0 = (blockIdx.x % tiles) * HO_ROWS;
    const size_t HW = (size_t)H * W;
    const int tid = threadIdx.x;
    ho_stage_hull(hull + (size_t)b * hull_bs, A1, y0, H, W);
    ho_stage_centres(A2, b, y0, H, W, p_field, seed, field_offset);
    __syncthreads();
    // ---- 2: x passes in place ----
    ho_xpass_inplace<HO_R1>(A1, NR1, SW1, W);
    ho_xpass_inplace<HO_R2>(A2, NR2, SW2, W);
    __syncthreads();
    // ---- 3: y passes, composition, both stores ----
    const float* ib = img + (size_t)b * 3 * HW;
    const float* rb = rendered + (size_t)b * 3 * HW;
    const float* pb = pmask + (size_t)b * HW;
    float* mb = masked + (size_t)b * 3 * HW;
    float* kb = packed + (size_t)b * HW * 8;
    for (int i = tid; i < (HO_ROWS / 4) * W; i += HO_THREADS) {
        const int q = i / W, x = i - q * W;
        float er[4], dl[4];
        ho_ypass4<HO_R1>(A1 + (q * 4) * SW1 + x, SW1, er);        // staged row q*4 + k = image row y0 + q*4 - R + k
        ho_ypass4<HO_R2>(A2 + (q * 4) * SW2 + x, SW2, dl);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = y0 + q * 4 + k;
            if (y >= H) continue;
            const size_t pix = (size_t)y * W + x;
            float mask_d = 1.0f - er[k], keep = 1.0f - dl[k];     // what the two max pools stored: 1 - maxpool(1 - mask), 1 - maxpool(centres)
            asm("" : "+v"(mask_d));                               // rounded fp32 values, as when they came back from memory
            asm("" : "+v"(keep));
            const float pm = pb[pix];
            float v[8];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = rb[c * HW + pix];
            const bool all0 = v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f;
            float rm = all0 ? 0.0f : 1.0f;                        // rendered_mask_kernel
            asm("" : "+v"(rm));
            const float m = mask_d * (1.0f - rm);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float xin = ib[c * HW + pix];
                const float o = masking_compose1(xin, m, xin * pm, nullptr, 1, seed, noise_offset + ((size_t)b * 3 + c) * HW + pix, true, keep);
                mb[c * HW + pix] = o;
                v[3 + c] = o;
            }
            v[6] = 0.f; v[7] = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) smirk_range_audit1(v[c]);  // the network INPUT, as pack_split_kernel audits it
            half8 hi, lo;
            split8(v, hi, lo);
            *(half8*)(kb + pix * 8) = hi;
            *(half8*)(kb + pix * 8 + 4) = lo;
        }
    }
}

// retained[b,:,p2y,p2x] = img[b,:,p1y,p1x] for l < rbound[b]; duplicates in points2: the highest l wins (CPU index_put order)
__global__ __launch_bounds__(256) void transfer_winner_kernel(const long long* __restrict__ p2, const long long* __restrict__ rbound,
                                                              int B, int L, int H, int W, int* __restrict__ winner) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * L) return;
    const int b = (int)(i / L), l = (int)(i % L);
    if (rbound && l >= rbound[b]) return;
    const long long x = p2[i * 3 + 0], y = p2[i * 3 + 1];
    if (x < 0 || x >= W || y < 0 || y >= H) return;
    atomicMax(&winner[((size_t)b * H + y) * W + x], l);
}
__global__ __launch_bounds__(256) void transfer_gather_kernel(const float* __restrict__ img, const long long* __restrict__ p1,
                                                              const int* __restrict__ winner, int B, int C, int L, int H, int W,
                                                              float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * C * H * W) return;
    const size_t HW = (size_t)H * W, b = i / (C * HW), c = (i / HW) % C, p = i % HW;
    const int l = winner[b * HW + p];
    float v = 0.f;
    if (l >= 0) {
        long long x = p1[((size_t)b * L + l) * 3 + 0], y = p1[((size_t)b * L + l) * 3 + 1];
        x = x < 0 ? x + W : x; y = y < 0 ? y + H : y;                    // python negative indexing never occurs after the clamps; kept for safety
        v = img[(b * C + c) * HW + (size_t)y * W + x];
    }
    out[i] = v;
}

// pmask[b,0,y,x] = 1 at the first rbound[b] sampled points (demo.py:153-159, smirk_trainer.py:86-88); out must be zero-filled
__global__ __launch_bounds__(256) void scatter_points_kernel(const long long* __restrict__ pts, const long long* __restrict__ rbound,
                                                             int B, int L, int H, int W, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * L) return;
    const int b = (int)(i / L), l = (int)(i % L);
    if (rbound && l >= rbound[b]) return;
    const long long x = pts[i * 3], y = pts[i * 3 + 1];
    if (x >= 0 && x < W && y >= 0 && y < H) out[((size_t)b * H + y) * W + x] = 1.0f;
}
// rendered_mask = 1 - (rendered_img == 0).all(dim=1)   (demo.py:146, smirk_trainer.py:79)
__global__ __launch_bounds__(256) void rendered_mask_kernel(const float* __restrict__ img, int B, int C, int HW, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * HW) return;
    const size_t b = i / HW, p = i % HW;
    bool all0 = true;
    for (int c = 0; c < C; ++c) all0 = all0 && (img[(b * C + c) * HW + p] == 0.0f);
    out[i] = all0 ? 0.0f : 1.0f;
}

static unsigned nblk(size_t n) { return (unsigned)((n + 255) / 256); }

extern "C" int smirk_scatter_points_mask(const int64_t* points, const int64_t* rbound, int B, int L, int H, int W, float* out, void* stream) {
    if (!points || !out || B <= 0 || L <= 0) return SMIRK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, (size_t)B * H * W * 4, st) != hipSuccess) return SMIRK_ERR_LAUNCH;
    SMIRK_LAUNCH(scatter_points_kernel, dim3(nblk((size_t)B * L)), dim3(256), 0, st, (const long long*)points, (const long long*)rbound,
                       B, L, H, W, out);
    return smirk_launch_status();
}

extern "C" int smirk_rendered_mask(const float* rendered_img, int B, int C, int H, int W, float* out, void* stream) {
    if (!rendered_img || !out || B <= 0 || C <= 0) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(rendered_mask_kernel, dim3(nblk((size_t)B * H * W)), dim3(256), 0, (hipStream_t)stream, rendered_img, B, C, H * W, out);
    return smirk_launch_status();
}

extern "C" int smirk_mask_face_weights(const float* tverts, const float* normals, const int32_t* faces, const float* face_prob,
                                       int B, int V, int F, float* weights, void* stream) {
    if (!tverts || !normals || !faces || !face_prob || !weights || B <= 0 || F <= 0) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(mask_face_weights_kernel, dim3(nblk((size_t)B * F)), dim3(256), 0, (hipStream_t)stream, tverts, normals, faces,
                       face_prob, B, V, F, weights);
    return smirk_launch_status();
}

extern "C" int smirk_sample_faces(const float* weights, int B, int F, int num, uint64_t seed, uint64_t offset, int32_t* idx,
                                  float* bary, void* stream) {
    if (!weights || !idx || !bary || B <= 0 || F <= 0 || num <= 0 || F > 38000) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(sample_faces_kernel, dim3(B), dim3(1024), (size_t)(F + 32) * 4, (hipStream_t)stream, weights, F, num, seed,
                       offset, idx, bary);
    return smirk_launch_status();
}

extern "C" int smirk_points_to_pixels(const float* points, int B, int L, int image_size, int64_t* out, void* stream) {
    if (!points || !out || B <= 0 || L <= 0 || image_size <= 0) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(points_to_pixels_kernel, dim3(nblk((size_t)B * L)), dim3(256), 0, (hipStream_t)stream, points, (size_t)B * L,
                       image_size, (long long*)out);
    return smirk_launch_status();
}

// returns false when the > 64 KB dynamic-LDS opt-in failed on this device (the caller then takes the two-pass kernels instead of a launch that would fail)
template <int R>
static bool launch_maxpool_lds(const float* in, float* out, int B, int H, int W, int complement, hipStream_t st) {
    const size_t lds = (size_t)(MP_ROWS + 2 * R) * ((size_t)mp_row_stride(W, R) + W) * sizeof(float);
    if (smirk_raise_dynamic_lds((const void*)maxpool_sq_lds_kernel<R>, 160 * 1024) != SMIRK_OK) return false;   // retried on the next call
    const int tiles = (H + MP_ROWS - 1) / MP_ROWS;
    smirk_prof_next(nullptr, 0.0, 2.0 * B * H * W * sizeof(float));
    SMIRK_LAUNCH(maxpool_sq_lds_kernel<R>, dim3((unsigned)(B * tiles)), dim3(512), lds, st, in, out, H, W, complement & 1, (complement >> 1) & 1);
    return true;
}

extern "C" int smirk_maxpool_sq(const float* in, float* tmp, float* out, int B, int H, int W, int radius, int complement, void* stream) {
    if (!in || !tmp || !out || B <= 0 || H <= 0 || W <= 0 || radius < 0) return SMIRK_ERR_BAD_ARG;
    const size_t n = (size_t)B * H * W;
    // the fused LDS form covers the radii the reference uses (masking.py:78 -> 10, :96 -> 5) at widths whose staged rows fit 160 KB of LDS
    const size_t staged = (size_t)(MP_ROWS + 2 * radius) * ((size_t)W + mp_row_stride(W, radius)) * sizeof(float);
    // The fused form reads rows [y0 - R, y0 + 32 + R) of `in` while other workgroups write `out`: in == out (alias-safe in the two-pass form, which goes
    // through tmp) would race, so an aliased call keeps the two-pass kernels.  `tmp` must not alias either tensor in any form.
    if (tmp == in || tmp == out) return SMIRK_ERR_BAD_ARG;
    const bool lds_ok = staged <= 160 * 1024 && (size_t)B * ((H + MP_ROWS - 1) / MP_ROWS) < 0x7fffffffull && in != out;
    if (lds_ok && radius == 10 && launch_maxpool_lds<10>(in, out, B, H, W, complement, (hipStream_t)stream)) return smirk_launch_status();
    if (lds_ok && radius == 5 && launch_maxpool_lds<5>(in, out, B, H, W, complement, (hipStream_t)stream)) return smirk_launch_status();
    SMIRK_LAUNCH(maxfilter1d_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, in, tmp, B, H, W, radius, 0, complement & 1, 0);
    SMIRK_LAUNCH(maxfilter1d_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, (const float*)tmp, out, B, H, W, radius, 1, 0,
                       (complement >> 1) & 1);
    return smirk_launch_status();
}

extern "C" int smirk_bernoulli_field(float* out, size_t n, float p, uint64_t seed, uint64_t offset, void* stream) {
    if (!out || n == 0) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(bernoulli_field_kernel, dim3(nblk((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, n, p, seed, offset);
    return smirk_launch_status();
}

extern "C" int smirk_masking_compose(const float* img, const float* mask, const float* rendered_mask, const float* extra_points,
                                     const float* pmask, const float* keep, const float* noise_mult, int B, int C, int H, int W,
                                     int gen_noise, uint64_t seed, uint64_t offset, float* out, void* stream) {
    if (!img || !mask || (!extra_points && !pmask) || !out || B <= 0 || C <= 0) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(masking_compose_kernel, dim3(nblk((size_t)B * C * H * W)), dim3(256), 0, (hipStream_t)stream, img, mask,
                       rendered_mask, extra_points, pmask, keep, noise_mult, B, C, H * W, gen_noise, seed, offset, out);
    return smirk_launch_status();
}

extern "C" int smirk_transfer_pixels(const float* img, const int64_t* points1, const int64_t* points2, const int64_t* rbound, int B,
                                     int C, int L, int H, int W, int32_t* winner_ws, float* out, void* stream) {
    if (!img || !points1 || !points2 || !winner_ws || !out || B <= 0 || L <= 0) return SMIRK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(winner_ws, 0xFF, (size_t)B * H * W * 4, st) != hipSuccess) return SMIRK_ERR_LAUNCH;   // -1
    SMIRK_LAUNCH(transfer_winner_kernel, dim3(nblk((size_t)B * L)), dim3(256), 0, st, (const long long*)points2,
                       (const long long*)rbound, B, L, H, W, winner_ws);
    SMIRK_LAUNCH(transfer_gather_kernel, dim3(nblk((size_t)B * C * H * W)), dim3(256), 0, st, img, (const long long*)points1,
                       (const int*)winner_ws, B, C, L, H, W, out);
    return smirk_launch_status();
}

// demo.py:154-156: rsing = randint(0, 2) * 2 - 1, rscale = rand() * (mul - 1) + 1, rbound = (n * (1 / mul) * rscale ** rsing).long() — per image,
// drawn on the device so the step has no host round trip (the reference draws them on the host and copies them over)
__global__ __launch_bounds__(256) void point_budget_kernel(long long* __restrict__ rbound, int B, int n_points, float mul, uint64_t seed,
                                                           uint64_t offset) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t r[4];
    const uint64_t ctr = offset + (uint64_t)b;
    philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), 3u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float rscale = u01(r[0]) * (mul - 1.0f) + 1.0f;
    const float f = (r[1] & 1u) ? rscale : 1.0f / rscale;
    rbound[b] = (long long)((float)n_points * (1.0f / mul) * f);
}

extern "C" int smirk_random_point_budget(int64_t* rbound, int B, int n_points, float mul, uint64_t seed, uint64_t offset, void* stream) {
    if (!rbound || B <= 0 || n_points <= 0 || !(mul >= 1.0f)) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(point_budget_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, (long long*)rbound, B, n_points, mul, seed, offset);
    return smirk_launch_status();
}

// ---- include/smirk_handoff.h -------------------------------------------------------------------------------------------------------------------------------
extern "C" int smirk_handoff_abi_version(void) { return SMIRK_HANDOFF_ABI_VERSION; }

extern "C" int smirk_masking_handoff(const float* img, const float* rendered_img, const float* hull_mask, long long hull_batch_stride, const float* pmask,
                                     int B, int H, int W, float random_mask, uint64_t seed, uint64_t field_offset, uint64_t noise_offset, float* masked_img,
                                     void* packed, void* stream) {
    if (!img || !rendered_img || !hull_mask || !pmask || !masked_img || !packed || B <= 0 || H <= 0 || W <= 0) return SMIRK_ERR_BAD_ARG;
    if (hull_batch_stride != 0 && hull_batch_stride != (long long)H * W) return SMIRK_ERR_BAD_ARG;
    if (!(random_mask > 0.0f)) return SMIRK_ERR_BAD_ARG;                                            // masking() draws no field then: that path keeps its launches
    const size_t lds = ho_lds_bytes(W);
    const long long tiles = (H + HO_ROWS - 1) / HO_ROWS;
    // two workgroups per CU need at most 80 KB each; the flat field index of a pixel is taken relative to its image in 32 bits
    if (lds > 80 * 1024 || (long long)B * tiles >= 0x7fffffffll || (long long)H * W >= 0x7fffffffll) return SMIRK_ERR_UNSUPPORTED;
    if (smirk_raise_dynamic_lds((const void*)masking_handoff_kernel, 80 * 1024) != SMIRK_OK) return SMIRK_ERR_UNSUPPORTED;
    smirk_prof_next(nullptr, 0.0, (double)B * H * W * (4.0 * (3 + 3 + 1 + 1 + 3) + 32.0));
    SMIRK_LAUNCH(masking_handoff_kernel, dim3((unsigned)(B * tiles)), dim3(HO_THREADS), lds, (hipStream_t)stream, img, rendered_img, hull_mask,
                 (size_t)hull_batch_stride, pmask, H, W, random_mask, seed, field_offset, noise_offset, masked_img, (float*)packed);
    return smirk_launch_status();
}

// ---- training paths: sampled points -> generator input (include/smirk_train_handoff.h) -------------------------------------------------------
// One sampled point on one frame: the landmark gather of v2l_kernel (flame.hip) and the quantisation of points_to_pixels_kernel, operation for operation.  The
// gather is spelled with the roundings that unit's contraction chose, (p1 * b1, then + p0 * b0 and + p2 * b2 each as one fused multiply-add), because a pixel
// flips if they move (tests/test_train_handoff_gpu.py compares the bits); the quantisation has no product that feeds a sum, so it contracts nowhere.
__device__ __forceinline__ void stp_point(const float* __restrict__ vb, int i0, int i1, int i2, const float bc[3], int S, int32_t* __restrict__ xy,
                                          long long* __restrict__ np) {
    long long q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float p = __fmaf_rn(vb[i2 * 3 + c], bc[2], __fmaf_rn(vb[i0 * 3 + c], bc[0], __fmul_rn(vb[i1 * 3 + c], bc[1])));
        asm("" : "+v"(p));                                                      // a rounded fp32 value, as when it came back from memory
        const float v = 0.5f * (1.0f + p) * (float)S;                           // masking.py:172
        q[c] = (long long)v;                                                    // .long(): truncation toward zero
        if (c < 2) q[c] = q[c] < 0 ? 0 : (q[c] > S - 1 ? S - 1 : q[c]);         // masking.py:174-175
    }
    xy[0] = (int32_t)q[0]; xy[1] = (int32_t)q[1];
    if (np) { np[0] = q[0]; np[1] = q[1]; np[2] = q[2]; }
}

// One workgroup per source frame b: the CDF of its face weights, then per thread the draws of sample_faces_kernel (same counters), the point on the source frame
// and on each of its Ke target frames k * B + b.  tv_dst == nullptr: no target frames (the first path transfers every point onto itself).
__global__ __launch_bounds__(1024) void sample_transfer_points_kernel(const float* __restrict__ w, const float* __restrict__ tv_src,
                                                                      const float* __restrict__ tv_dst, const int32_t* __restrict__ faces, int B, int Ke,
                                                                      int V, int F, int num, int S, uint64_t seed, uint64_t offset,
                                                                      int32_t* __restrict__ psrc, int32_t* __restrict__ pdst, long long* __restrict__ fidx,
                                                                      float* __restrict__ bary, long long* __restrict__ np_src,
                                                                      long long* __restrict__ np_dst) {
    extern __shared__ float cdf[];               // [F] inclusive prefix sums, + 32 wave totals
    const int b = blockIdx.x;
    const float total = face_cdf_scan(w + (size_t)b * F, F, cdf, cdf + F);
    for (int t = threadIdx.x; t < num; t += blockDim.x) {
        float bc[3];
        const int f = face_draw(cdf, F, total, seed, offset + (uint64_t)b * num + t, bc);
        const size_t i = (size_t)b * num + t;
        if (fidx) fidx[i] = f;
        if (bary) { bary[i * 3] = bc[0]; bary[i * 3 + 1] = bc[1]; bary[i * 3 + 2] = bc[2]; }
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        stp_point(tv_src + (size_t)b * V * 3, i0, i1, i2, bc, S, psrc + i * 2, np_src ? np_src + i * 3 : nullptr);
        if (tv_dst)
            for (int k = 0; k < Ke; ++k) {
                const size_t j = ((size_t)k * B + b) * num + t;
                stp_point(tv_dst + ((size_t)k * B + b) * V * 3, i0, i1, i2, bc, S, pdst + j * 2, np_dst ? np_dst + j * 3 : nullptr);
            }
    }
}

// masking_handoff_kernel's band scheme over the Ke * B output frames of a training path.  Output frame kb reads img and hull of source frame kb % B, its own
// rendering and its own targets; the pixel transfer happens in LDS:
//   1  stage 1 - hull and the patch centres as there (the field is drawn per OUTPUT frame), and a [HO_ROWS][W] winner band set to -1
//   2  the x passes in place; meanwhile the frame's N targets are scanned and every one that lands in the band raises its pixel's cell to its point index with an
//      LDS atomicMax: the highest index wins, as transfer_winner_kernel decides over the whole image.  Both touch disjoint LDS, so they share one barrier interval
//   3  the y passes; the extra value of a pixel is the source pixel of its winner (else 0); the rendered mask under `rule`; composition, masked and packed
// LDS: ho_lds_bytes(W) + HO_ROWS * W * 4 = 75,584 bytes at W = 224: two workgroups per CU.
static inline size_t tho_lds_bytes(int W) { return ho_lds_bytes(W) + (size_t)HO_ROWS * W * sizeof(int); }

__global__ __launch_bounds__(HO_THREADS) void train_masking_handoff_kernel(const float* __restrict__ img, const float* __restrict__ rendered,
                                                                            const float* __restrict__ hull, size_t hull_bs, const int2* __restrict__ psrc,
                                                                            const int2* __restrict__ pdst, int B, int N, int H, int W, int rule, float p_field,
                                                                            uint64_t seed, uint64_t field_offset, uint64_t noise_offset,
                                                                            float* __restrict__ masked, float* __restrict__ packed) {
    extern __shared__ __attribute__((aligned(16))) float ho_lds[];
    const int SW1 = mp_row_stride(W, HO_R1), SW2 = mp_row_stride(W, HO_R2);
    constexpr int NR1 = HO_ROWS + 2 * HO_R1, NR2 = HO_ROWS + 2 * HO_R2;
    float* A1 = ho_lds;                                 // [NR1][SW1]  1 - hull, then its x maxima
    float* A2 = ho_lds + NR1 * SW1;                     // [NR2][SW2]  patch centres, then their x maxima
    int* win = (int*)(A2 + NR2 * SW2);                  // [HO_ROWS][W] highest point index that lands on the pixel, -1: none
    const int tiles = (H + HO_ROWS - 1) / HO_ROWS;
    const int kb = blockIdx.x / tiles, y0 = (blockIdx.x % tiles) * HO_ROWS, bs = kb % B;
    const size_t HW = (size_t)H * W;
    const int tid = threadIdx.x;
    ho_stage_hull(hull + (size_t)bs * hull_bs, A1, y0, H, W);
    ho_stage_centres(A2, kb, y0, H, W, p_field, seed, field_offset);
    for (int i = tid; i < HO_ROWS * W; i += HO_THREADS) win[i] = -1;
    __syncthreads();
    // ---- 2: the transfer's winners, and the x passes in place ----
    const int2* pd = pdst + (size_t)kb * N;
    for (int l = tid; l < N; l += HO_THREADS) {
        const int2 t = pd[l];
        const int ry = t.y - y0;
        if (t.x >= 0 && t.x < W && t.y >= 0 && t.y < H && ry >= 0 && ry < HO_ROWS) atomicMax(&win[ry * W + t.x], l);
    }
    ho_xpass_inplace<HO_R1>(A1, NR1, SW1, W);
    ho_xpass_inplace<HO_R2>(A2, NR2, SW2, W);
    __syncthreads();
    // ---- 3: y passes, transfer, composition, both stores ----
    const float* ib = img + (size_t)bs * 3 * HW;
    const float* rb = rendered + (size_t)kb * 3 * HW;
    const int2* ps = psrc + (size_t)bs * N;
    float* mb = masked + (size_t)kb * 3 * HW;
    float* pk = packed + (size_t)kb * HW * 8;
    for (int i = tid; i < (HO_ROWS / 4) * W; i += HO_THREADS) {
        const int q = i / W, x = i - q * W;
        float er[4], dl[4];
        ho_ypass4<HO_R1>(A1 + (q * 4) * SW1 + x, SW1, er);        // staged row q*4 + k = image row y0 + q*4 - R + k
        ho_ypass4<HO_R2>(A2 + (q * 4) * SW2 + x, SW2, dl);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = y0 + q * 4 + k;
            if (y >= H) continue;
            const size_t pix = (size_t)y * W + x;
            float mask_d = 1.0f - er[k], keep = 1.0f - dl[k];     // what the two max pools stored: 1 - maxpool(1 - mask), 1 - maxpool(centres)
            asm("" : "+v"(mask_d));                               // rounded fp32 values, as when they came back from memory
            asm("" : "+v"(keep));
            const int l = win[(q * 4 + k) * W + x];
            size_t spix = 0;
            bool has = false;
            if (l >= 0) {
                const int2 s = ps[l];
                has = s.x >= 0 && s.x < W && s.y >= 0 && s.y < H;
                if (has) spix = (size_t)s.y * W + s.x;
            }
            float v[8];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = rb[c * HW + pix];
            const bool covered = rule == SMIRK_RENDERED_RULE_POSITIVE ? (v[0] > 0.0f && v[1] > 0.0f && v[2] > 0.0f)      // (r > 0).all(1)
                                                                      : !(v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f); // 1 - (r == 0).all(1)
            float rm = covered ? 1.0f : 0.0f;
            asm("" : "+v"(rm));
            const float m = mask_d * (1.0f - rm);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float e = has ? ib[c * HW + spix] : 0.0f;   // transfer_gather_kernel
                const float o = masking_compose1(ib[c * HW + pix], m, e, nullptr, 1, seed, noise_offset + ((size_t)kb * 3 + c) * HW + pix, true, keep);
                mb[c * HW + pix] = o;
                v[3 + c] = o;
            }
            v[6] = 0.f; v[7] = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) smirk_range_audit1(v[c]);  // the network INPUT, as pack_split_kernel audits it
            half8 hi, lo;
            split8(v, hi, lo);
            *(half8*)(pk + pix * 8) = hi;
            *(half8*)(pk + pix * 8 + 4) = lo;
        }
    }
}

extern "C" int smirk_train_handoff_abi_version(void) { return SMIRK_TRAIN_HANDOFF_ABI_VERSION; }

extern "C" int smirk_sample_transfer_points(const float* weights, const float* tv_src, const float* tv_dst, const int32_t* faces, int B, int Ke, int V, int F,
                                            int num, int image_size, uint64_t seed, uint64_t offset, int32_t* points_src, int32_t* points_dst,
                                            int64_t* faces_idx, float* bary, int64_t* npoints_src, int64_t* npoints_dst, void* stream) {
    if (!weights || !tv_src || !faces || !points_src) return SMIRK_ERR_BAD_ARG;
    if (B <= 0 || Ke <= 0 || V <= 0 || F <= 0 || num <= 0 || image_size <= 0 || F > 38000 || image_size > 32768) return SMIRK_ERR_BAD_ARG;
    if (tv_dst ? !points_dst : (Ke != 1 || points_dst || npoints_dst)) return SMIRK_ERR_BAD_ARG;
    SMIRK_LAUNCH(sample_transfer_points_kernel, dim3(B), dim3(1024), (size_t)(F + 32) * 4, (hipStream_t)stream, weights, tv_src, tv_dst, faces, B, Ke, V, F, num,
                 image_size, seed, offset, points_src, points_dst, (long long*)faces_idx, bary, (long long*)npoints_src, (long long*)npoints_dst);
    return smirk_launch_status();
}

extern "C" int smirk_train_masking_handoff(const float* img, const float* rendered_img, const float* hull_mask, long long hull_batch_stride,
                                           const int32_t* points_src, const int32_t* points_dst, int B, int Ke, int N, int H, int W, int rendered_rule,
                                           float random_mask, uint64_t seed, uint64_t field_offset, uint64_t noise_offset, float* masked_img, void* packed,
                                           void* stream) {
    if (!img || !rendered_img || !hull_mask || !points_src || !points_dst || !masked_img || !packed) return SMIRK_ERR_BAD_ARG;
    if (B <= 0 || Ke <= 0 || N <= 0 || H <= 0 || W <= 0) return SMIRK_ERR_BAD_ARG;
    if (hull_batch_stride != 0 && hull_batch_stride != (long long)H * W) return SMIRK_ERR_BAD_ARG;
    if (!(random_mask > 0.0f)) return SMIRK_ERR_BAD_ARG;                                            // masking() draws no field then: that path keeps its launches
    if (rendered_rule != SMIRK_RENDERED_RULE_NONZERO && rendered_rule != SMIRK_RENDERED_RULE_POSITIVE) return SMIRK_ERR_BAD_ARG;
    const size_t lds = tho_lds_bytes(W);
    const long long tiles = (H + HO_ROWS - 1) / HO_ROWS, frames = (long long)B * Ke;
    // two workgroups per CU need at most 80 KB each; the flat field index of a pixel is taken relative to its frame in 32 bits
    if (lds > 80 * 1024 || frames * tiles >= 0x7fffffffll || (long long)H * W >= 0x7fffffffll) return SMIRK_ERR_UNSUPPORTED;
    if (smirk_raise_dynamic_lds((const void*)train_masking_handoff_kernel, 80 * 1024) != SMIRK_OK) return SMIRK_ERR_UNSUPPORTED;
    smirk_prof_next(nullptr, 0.0, (double)frames * H * W * (4.0 * (3 + 3 + 1 + 3) + 32.0));
    SMIRK_LAUNCH(train_masking_handoff_kernel, dim3((unsigned)(frames * tiles)), dim3(HO_THREADS), lds, (hipStream_t)stream, img, rendered_img, hull_mask,
                 (size_t)hull_batch_stride, (const int2*)points_src, (const int2*)points_dst, B, N, H, W, rendered_rule, random_mask, seed, field_offset,
                 noise_offset, masked_img, (float*)packed);
    return smirk_launch_status();
}
