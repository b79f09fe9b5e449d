// Random draws of the cycle path's parameter augmentation (augment.hip; included by that unit only).
//
// Generator: Philox4x32-10 (Salmon et al. 2011) with the counter layout of masking.hip: counter = (idx lo, idx hi, stream id, 0), key = seed, where
// idx = offset + a local counter index.  masking.hip owns stream ids 0-3; this unit owns 4 and 5.  One counter yields four 32-bit words x0..x3.
//
//   stream AUG_STREAM_ROW (4), four counters per output row r (N = Ke * B rows):
//     idx = offset + 4 r + 0   x0  key of the group permutation (rows ranked by key, ties by row index; rank cut at N/4, 2N/4, 3N/4)
//                              x1  key of the permutation inside group 1 (same ranking, over the rows of group 1 only)
//                              x2  template class  = (uint64(x2) * n_classes) >> 32
//                              x3  row in the class = (uint64(x3) * rows_in_class) >> 32
//     idx = offset + 4 r + 1   x0  u   (1 + 2u in group 0, 0.25 + 1.25u in groups 1 and 2)
//                              x1  u'  (0.2 u' scales the additive noise of the row, every group)
//                              x2  bit 0: the jaw Bernoulli b                          x3 unused
//     idx = offset + 4 r + 2   (x0, x1) -> Box-Muller pair: jaw[0] = cos branch, jaw[1] = sin branch;  (x2, x3) -> jaw[2] = cos branch
//     idx = offset + 4 r + 3   x0, x1  the two eyelid jitters of step 6;  x2, x3  the two eyelid values of group 3
//   stream AUG_STREAM_ELEM (5), one counter per expression element (r, c):
//     idx = offset + r E + c   (x0, x1) -> Box-Muller pair (za = cos branch, zb = sin branch): za is n1 of group 0, zb is the additive noise n of every group
//                              x2  bit 0: the element mask m of group 0                 x3 unused
//
// A call therefore consumes  N * max(E, 4)  counters: that is what a PhiloxStream advances by (smirk_amd/augment.py n_counters).
//
// Uniforms are 24-bit: u = (x >> 8) / 2^24 in [0, 1).  Box-Muller takes the radius from (x0 >> 8) + 1 (so the logarithm's argument is in (0, 1]) and the
// angle as 2 pi (x1 >> 8) / 2^24, evaluated with logf and sincospif (the angle in half turns is exact, no range reduction error); no fast intrinsics.
#pragma once
#include <stdint.h>

#define AUG_STREAM_ROW 4u
#define AUG_STREAM_ELEM 5u

struct AugDraw { uint32_t x0, x1, x2, x3; };

__device__ __forceinline__ AugDraw aug_philox(uint64_t idx, uint32_t stream, uint64_t seed) {
    uint32_t c0 = (uint32_t)idx, c1 = (uint32_t)(idx >> 32), c2 = stream, c3 = 0u, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    AugDraw d = {c0, c1, c2, c3};
    return d;
}

__device__ __forceinline__ float aug_u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }   // [0, 1)

// (cos branch, sin branch) of one Box-Muller pair
__device__ __forceinline__ void aug_normal2(uint32_t xa, uint32_t xb, float& zc, float& zs) {
    const float u1 = (float)((xa >> 8) + 1u) * (1.0f / 16777216.0f);                                      // (0, 1], exact
    const float rad = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * aug_u01(xb), &s, &c);
    zc = rad * c; zs = rad * s;
}
