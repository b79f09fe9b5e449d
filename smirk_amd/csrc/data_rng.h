// Random draws of the batch preparation (data.hip; included by that unit only).
//
// Generator: Philox4x32-10 with the counter layout of augment_rng.h / masking.hip: counter = (idx lo, idx hi, stream id, 0), key = seed, where
// idx = offset + a local counter index.  masking.hip owns stream ids 0-3, augment.hip 4 and 5; this unit owns 6 and 7.  One counter yields x0..x3.
//
//   stream DATA_STREAM_FRAME (6), DATA_FRAME_COUNTERS = 8 counters per frame f  (u = a 24-bit uniform, "coin t" = u < p[t], "U" = lo + (hi - lo) u):
//     idx = offset + 8 f + 0   x0 crop scale U(scale_lo, scale_hi)   x1 coin BrightnessContrast   x2 alpha = 1 + U(+-contrast)   x3 beta = U(+-brightness)
//     idx = offset + 8 f + 1   x0 coin Gamma          x1 gamma = U(lo, hi) / 100     x2 coin ColorJitter     x3 jitter brightness = 1 + U(+-limit)
//     idx = offset + 8 f + 2   x0 jitter contrast     x1 jitter saturation           x2 jitter hue U(+-limit) x3 coin CLAHE
//     idx = offset + 8 f + 3   x0 clip = U(lo, hi)    x1 coin RGBShift               x2 shift R U(+-limit)   x3 shift G
//     idx = offset + 8 f + 4   x0 shift B             x1 coin Blur                   x2 k = 3 + 2 ((uint64(x2) * n_k) >> 32), n_k = (blur_max - 1) / 2     x3 coin GaussNoise
//     idx = offset + 8 f + 5   x0 variance U(lo, hi)  x1 coin ShiftScaleRotate       x2 angle U(+-rotate)    x3 scale = 1 + U(+-limit)
//     idx = offset + 8 f + 6   x0 dx U(+-shift)       x1 dy U(+-shift)               x2, x3 unused
//     idx = offset + 8 f + 7   unused
//   stream DATA_STREAM_PIXEL (7), one counter per crop pixel (f, row, col) — the pixel of the image BEFORE ShiftScaleRotate:
//     idx = offset + (f S + row) S + col    (x0, x1) -> Box-Muller pair: cos branch = z of R, sin branch = z of G;   (x2, x3) -> cos branch = z of B
//
// Every draw is made whether or not its coin falls, so a frame's draws depend on (seed, offset, f) only.  A call consumes  N * max(S * S, 8)  counters
// (the two stream ids share the index range): that is what a PhiloxStream advances by (smirk_amd/data.py n_counters).
//
// Uniforms are 24-bit: u = (x >> 8) / 2^24 in [0, 1), as a double.  Box-Muller in float64: radius from ((x0 >> 8) + 1) / 2^24 in (0, 1], angle
// 2 pi (x1 >> 8) / 2^24 evaluated with log, sqrt and sincospi (the angle in half turns is exact).
#pragma once
#include <stdint.h>

#define DATA_STREAM_FRAME 6u
#define DATA_STREAM_PIXEL 7u
#define DATA_FRAME_COUNTERS 8

struct DataDraw { uint32_t x0, x1, x2, x3; };

__device__ __forceinline__ DataDraw data_philox(uint64_t idx, uint32_t stream, uint64_t seed) {
    uint32_t c0 = (uint32_t)idx, c1 = (uint32_t)(idx >> 32), c2 = stream, c3 = 0u, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    DataDraw d = {c0, c1, c2, c3};
    return d;
}

__device__ __forceinline__ double data_u01(uint32_t x) { return (double)(x >> 8) * (1.0 / 16777216.0); }   // [0, 1)

// (cos branch, sin branch) of one Box-Muller pair, float64
__device__ __forceinline__ void data_normal2(uint32_t xa, uint32_t xb, double& zc, double& zs) {
    const double u1 = (double)((xa >> 8) + 1u) * (1.0 / 16777216.0);                                        // (0, 1], exact
    const double rad = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * data_u01(xb), &s, &c);
    zc = rad * c; zs = rad * s;
}
