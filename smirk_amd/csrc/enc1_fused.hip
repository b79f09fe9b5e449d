// enc1_fused.hip — the U-Net's first encoder block at full resolution in ONE launch (split-fp16 arithmetic, see conv.hip for the number format):
//
//     conv3x3(8 -> 32) + BN + ReLU  ->  conv3x3(32 -> 32) + BN + ReLU  ->  e1 (skip tensor)  +  2x2 max-pool(e1)
//     src/smirk_generator.py:52-53 (encoder1 = _block(in_channels, features); pool1), _block :88-119
//
// Why.  Unfused, the 32-channel 224 x 224 tensor between the two convolutions is written and read back (6.6 GB each way per 1024 frames) and e1 is read a
// third time by the pool: 29.7 GB for a block whose unique traffic is 9.9 GB (input 1.6, e1 6.6, pooled 1.65) — three HBM-bound launches, 8.4 ms
// (profiles/r04b_conv_sweep_B128_B1024.txt: enc1a 3.27 + enc1b 3.38, pool 1.6).  Here a 16 x 16 output patch is produced from its 20 x 20 x 8-channel
// input halo (12.8 KB) entirely inside the CU:
//   conv1 on the 18 x 18 halo of the patch (halo RECOMPUTE, 1.27x of the cheap convolution) -> BN + ReLU -> split16 -> LDS (zero outside the image: it is
//   conv2's zero padding) -> conv2 on the 16 x 16 patch from LDS -> BN + ReLU -> e1 and the pooled patch, both staged through LDS and stored as whole
//   1 KiB runs of consecutive pixels (every lane storing its own 8-byte pieces straight to global memory was measured: 5.8 -> 6.4 ms per 1024 frames, the
//   partner group's conv2 phase doubles while the store instructions drain; git history of this file).
//   * conv1's K = 9 taps x 8 channels is packed TWO TAPS per 16-k MFMA step (a lane half = a tap): 5 steps instead of the 18 the generic patch kernel
//     spends on a 32-channel chunk that is 3/4 zeros.
//   * operands are swapped (weights first): the 32 x 32 accumulator then holds, per lane, 4 CONSECUTIVE CHANNELS x 4 groups of ONE pixel, so BN / ReLU /
//     the fp16 split happen in registers and a lane's results go to LDS as 8-byte pieces of the final [pixel][8 hi | 8 lo] layout — no fp32 transpose
//     buffer, no scalar ds_write_b32 (the generic epilogue's 5.3 k of 15 k cycles per patch, tools/patch_timeline.py).
//   * fp32 -> (hi, lo) uses v_cvt_pk_f16_f32 (gfx950): 4 VALU per value instead of 6 (same roundings, same results).
//   * One 512-thread workgroup per CU = TWO 4-wave groups, each walking its own patches through conv1 | epilogue 1 | conv2 | epilogue 2, ONE PHASE APART
//     and separated by the workgroup barrier: while one group's waves issue MFMAs the other group's waves on the same SIMDs run an epilogue (VALU / LDS /
//     stores).  The groups share the weights (W2 36 KB + W1 10 KB) — two independent workgroups per CU would not fit (2 x 90 KB).
// LDS: W2 36,864 + W1 10,240 + coefficients 512 + 2 x (input halo 14,336 + intermediate 41,472) = 159,232 B.
//
// Bound: per patch 597 MFMAs (conv1 165 on 11 row tiles, conv2 432) = 4.8 k matrix-pipe cycles per CU against 9.9 GB / 1024 frames of HBM traffic
// (~2 ms at 5 TB/s): MFMA / VALU co-bound, HBM close behind.  Algorithmic flop = 2 * B*H*W * 32 * (72 + 288).

#include "conv_common.h"

typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef unsigned uint2v __attribute__((ext_vector_type(2)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));

#ifndef E1_PHASE_OFFSET
#define E1_PHASE_OFFSET 1                           // 1: group 1 runs one phase behind group 0; 0: both groups in the same phase
#endif
#define E1_PT 16                                  // output patch edge
#define E1_IH (E1_PT + 2)                         // intermediate (conv1 output) halo edge: 18
#define E1_XH (E1_PT + 4)                         // input halo edge: 20
#define E1_IPIX (E1_IH * E1_IH)                   // 324
#define E1_XPIX (E1_XH * E1_XH)                   // 400
#define E1_XSLOTS 448                             // 7 DMA instructions of 64 pixels per half plane
#define E1_W2_BYTES (9 * 32 * 128)                // [tap][n][32 dwords], XOR piece swizzle
#define E1_W1_BYTES (5 * 2 * 2 * 32 * 16)         // [k-step][hi|lo][lane half][n] 16-byte pieces
#define E1_COEF_BYTES 512                         // scale1, shift1, scale2, shift2 (32 floats each)
#define E1_XIN_BYTES (2 * E1_XSLOTS * 16)         // planar: hi pieces of the 400 (+48) halo pixels, then their lo pieces
#define E1_INT_BYTES (E1_IPIX * 128)              // [pixel][4 groups x (8 hi | 8 lo)], piece swizzle by halo column
#define E1_GROUP_BYTES (E1_XIN_BYTES + E1_INT_BYTES)
#define E1_LDS_BYTES (E1_W2_BYTES + E1_W1_BYTES + E1_COEF_BYTES + 2 * E1_GROUP_BYTES)
#define E1_STAGE_BYTES (32 * 128 + 8 * 128)       // per wave, inside the (dead) intermediate: one 32-pixel e1 tile + its 8 pooled pixels

struct Enc1Args {
    const float *x, *w1, *w2, *sc1, *sh1, *sc2, *sh2;
    float *e1, *pool;
    int B, H, W;
    int npatch;            // B * (H/16) * (W/16)
};

typedef __attribute__((address_space(3))) void* e1_lptr_t;
typedef const __attribute__((address_space(1))) void* e1_gptr_t;

// fp32 pair -> split-fp16 pairs packed as dwords (value = hi + lo * 2^-11; smirk_split1's roundings, two values per conversion instruction)
__device__ __forceinline__ void e1_split2(float a, float b, unsigned& hi, unsigned& lo) {
    asm("" : "+v"(a));
    asm("" : "+v"(b));                                             // rounded fp32 register values (see smirk_split1)
    const float2v v = {a, b};
    const half2v h = __builtin_convertvector(v, half2v);
    const float da = (a - (float)h.x) * 2048.0f, db = (b - (float)h.y) * 2048.0f;
    const float2v d = {da, db};
    const half2v l = __builtin_convertvector(d, half2v);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}

// 8 fp32 values -> 4 packed hi dwords + 4 packed lo dwords, written STAGE BY STAGE (8 independent instructions per stage, a scheduling fence between
// stages).  Left to itself hipcc's scheduler, minimising register pressure next to the 255-VGPR matrix phases, emitted each value's nine dependent
// operations back to back through ONE temporary register: ~9 cycles per VALU instruction, 4-6 k cycles per epilogue (tools/enc1_timeline.py).
#define E1_FENCE() __builtin_amdgcn_sched_barrier(0)
template <bool AUDIT>
__device__ __forceinline__ void e1_split8(float (&y)[8], unsigned (&hi)[4], unsigned (&lo)[4], SmirkRangeAccS& rng) {
    // split-fp16 range audit (common.h) at ONE of the three split sites, the stored output: an overflow of the conv1 intermediate turns into inf / NaN in every
    // output channel of conv2 and is caught there; the pooled values are maxima of audited values
    if constexpr (AUDIT) rng.see8(y);
    half2v h[4];
    float d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) asm("" : "+v"(y[k]));                // rounded fp32 register values (see smirk_split1)
#pragma unroll
    for (int k = 0; k < 4; ++k) { const float2v v = {y[2 * k], y[2 * k + 1]}; h[k] = __builtin_convertvector(v, half2v); }
    E1_FENCE();
#pragma unroll
    for (int k = 0; k < 4; ++k) { d[2 * k] = (float)h[k].x; d[2 * k + 1] = (float)h[k].y; }
    E1_FENCE();
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = y[k] - d[k];
    E1_FENCE();
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] *= 2048.0f;
    E1_FENCE();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float2v v = {d[2 * k], d[2 * k + 1]};
        const half2v l = __builtin_convertvector(v, half2v);
        hi[k] = __builtin_bit_cast(unsigned, h[k]);
        lo[k] = __builtin_bit_cast(unsigned, l);
    }
    E1_FENCE();
}

// max without the canonicalising v_max(x, x) hipcc puts in front of fmaxf on values it cannot prove quiet (everything here is a finite ReLU output)
__device__ __forceinline__ float e1_max(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// 2 x 2 max over the lanes (fr ^ 1, fr ^ 16) = the pixel's horizontal / vertical neighbour in the 2 x 16 row tile, VALID IN THE ODD 16-LANE ROWS (ry == 1):
// DPP quad permute, then gfx950's v_permlane16_swap, whose first result is [A.row0, B.row0, A.row2, B.row2] (measured, tools/micro/pool_probe.hip; with
// hipcc 7.0 the builtin's SECOND result comes back equal to the first, so only the first is used): an odd row receives its even partner's value — no LDS traffic
__device__ __forceinline__ float e1_pool4(float y) {
    const float h = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y), 0xB1, 0xF, 0xF, true));     // quad_perm [1,0,3,2]
    const float z = e1_max(y, h);
    const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, z), __builtin_bit_cast(unsigned, z), false, false);
    return e1_max(z, __builtin_bit_cast(float, r[0]));
}

__device__ __forceinline__ int e1_w2_piece(int row, int piece) { return row * 128 + ((piece ^ ((row >> 1) & 7)) << 4); }          // bytes
__device__ __forceinline__ int e1_int_piece(int pix, int x, int piece) { return pix * 128 + ((piece ^ ((x >> 1) & 7)) << 4); }    // bytes; x = halo column
__device__ __forceinline__ int e1_stage_piece(int row, int piece) { return row * 128 + ((piece ^ ((row >> 1) & 7)) << 4); }       // bytes

__device__ __forceinline__ void e1_frag_ready(const half8& a, const half8& b, const half8& c, const half8& d) {
    asm volatile("" ::"v"(a), "v"(b), "v"(c), "v"(d));
}

__global__ __launch_bounds__(512, 2) void enc1_fused_kernel(Enc1Args a) {
    extern __shared__ __attribute__((aligned(16))) char e1_lds[];
    SmirkRangeAccS rng;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int group = wave_all >> 2, wave = wave_all & 3;
    const int fr = lane & 31, hb = lane >> 5;
    char* const W2l = e1_lds;
    char* const W1l = e1_lds + E1_W2_BYTES;
    const float* const coef = (const float*)(e1_lds + E1_W2_BYTES + E1_W1_BYTES);
    char* const XIN = e1_lds + E1_W2_BYTES + E1_W1_BYTES + E1_COEF_BYTES + group * E1_GROUP_BYTES;
    const int H = a.H, W = a.W;
    const int tiles_x = W / E1_PT, tiles_per_img = (H / E1_PT) * tiles_x;

    // ---- weights and coefficients -> LDS, once per (persistent) workgroup ---------------------------------------------------------------------------
    {   // W2: row (tap, n) = 128 bytes = channels 0..31 of w2[n][tap*32 ...] as 8 pieces; 8 rows per wave-wide LDS-DMA instruction
        for (int r0 = wave_all * 8; r0 < 9 * 32; r0 += 64) {
            const int row = r0 + (lane >> 3), pos = lane & 7;
            const int piece = pos ^ ((row >> 1) & 7);
            const int tap = row >> 5, n = row & 31;
            __builtin_amdgcn_global_load_lds((e1_gptr_t)(a.w2 + (size_t)n * 288 + tap * 32 + piece * 4), (e1_lptr_t)(W2l + r0 * 128), 16, 0, 0);
        }
        // W1: piece ((s*2 + hl)*2 + h)*32 + n  <-  w1[n][tap = 2s + h] (8 channels: 4 dwords hi, 4 dwords lo); tap 9 does not exist -> zeros
        for (int i = tid; i < 5 * 2 * 2 * 32; i += 512) {
            const int n = i & 31, h = (i >> 5) & 1, hl = (i >> 6) & 1, s = i >> 7;
            const int tap = 2 * s + h;
            uint4v v = {0u, 0u, 0u, 0u};
            if (tap < 9) v = *(const uint4v*)(a.w1 + (size_t)n * 72 + tap * 8 + hl * 4);
            *(uint4v*)(W1l + i * 16) = v;
        }
        if (tid < 128) {
            const float* src = tid < 32 ? a.sc1 : tid < 64 ? a.sh1 : tid < 96 ? a.sc2 : a.sh2;
            ((float*)(e1_lds + E1_W2_BYTES + E1_W1_BYTES))[tid] = src[tid & 31];
        }
    }
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, (int)((long long)a.B * H * W * 32), 0x00020000);

    // patch n of this group -> (image, origin)
    const int logical = xcd_logical(blockIdx.x, gridDim.x);
    const int gidx = logical * 2 + group, gstride = gridDim.x * 2;
    auto patch_origin = [&](int p, int& b, int& oy0, int& ox0) {
        b = p / tiles_per_img;
        const int t = p - b * tiles_per_img;
        const int ty = t / tiles_x;
        oy0 = ty * E1_PT;
        ox0 = (t - ty * tiles_x) * E1_PT;
    };
    // input halo of patch p -> XIN (planar hi / lo pieces of the 20 x 20 pixels); pixels outside the image carry an out-of-range offset -> zeros
    auto issue_xin = [&](int p) {
        int b, oy0, ox0;
        patch_origin(p, b, oy0, ox0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = wave + 4 * k;                               // instruction 0..13: half plane q / 7, 64-pixel run q % 7
            if (q < 14) {
                const int hl = q >= 7 ? 1 : 0, run = q - 7 * hl;
                int pl = lane;
                asm volatile("" : "+v"(pl));                         // nothing derived from the slot is hoisted out of the patch loop (registers)
                const int pidx = run * 64 + pl;
                const int iy = (pidx * 3277) >> 16, ix = pidx - iy * E1_XH;                   // pidx / 20 for pidx < 448
                const int gy = oy0 - 2 + iy, gx = ox0 - 2 + ix;
                const bool ok = pidx < E1_XPIX && gy >= 0 && gy < H && gx >= 0 && gx < W;
                const unsigned vo = ok ? (unsigned)((b * H + gy) * W + gx) * 32u + (unsigned)hl * 16u : 0x80000000u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (e1_lptr_t)(XIN + hl * (E1_XSLOTS * 16) + run * 1024), 16, vo, 0, 0, 0);
            }
        }
    };

    // ---- per-lane address bases (byte offsets from e1_lds).  Every region starts on a 128-byte boundary, every per-lane base below keeps its variable part
    //      in bits 4-6 (+ bit 3), so "the other pieces of the same row" are XORs with compile-time constants and the (tap / tile) displacements are multiples of
    //      128 that go into the instruction's immediate offset: a handful of base registers instead of one hoisted address per (tap, k-step, half) ---------
    const unsigned lds_x = (unsigned)(E1_W2_BYTES + E1_W1_BYTES + E1_COEF_BYTES + group * E1_GROUP_BYTES), lds_i = lds_x + E1_XIN_BYTES;
    auto L = [&](unsigned off) -> char* { return e1_lds + off; };
    // conv1: row tile T = 3 wave + t covers intermediate pixels m = 32 T + fr (clamped to 323; tile 11 is all padding)
    unsigned c1_q[3];                                                // the lane's pixel (tap (0,0)) in the hi plane of XIN
    int c1_m[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int m = (3 * wave + t) * 32 + fr;
        c1_m[t] = m;
        const int mc = m < E1_IPIX ? m : E1_IPIX - 1;
        const int hy = (mc * 3641) >> 16, hx = mc - hy * E1_IH;      // mc / 18 for mc < 400
        c1_q[t] = lds_x + (unsigned)(hy * E1_XH + hx) * 16u;
    }
    unsigned c1_tap[5];                                              // this lane half's tap in k-step s: tap = 2 s + hb (tap 9: any address, its weights are zero)
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int tap = 2 * s + hb < 9 ? 2 * s + hb : 8;
        c1_tap[s] = (unsigned)((tap / 3) * E1_XH + tap % 3) * 16u;
    }
    const unsigned w1_base = (unsigned)E1_W2_BYTES + (unsigned)(hb * 32 + fr) * 16u;     // + ((s*2 + hl)*2) * 512
    const int ry = fr >> 4, rx = fr & 15;                            // conv2 / epilogue 2: the lane's pixel inside a 2 x 16 row tile
    // conv2 A operand: pixel (4 wave + 2 i + ry + ky, rx + kx) of INT, piece P = 2 (2 sstep + hb) + hl  ->  (base[kx] ^ ((sstep << 6) | (hl << 4))) + (2 i + ky) * 18 * 128
    unsigned c2_a[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
        c2_a[kx] = lds_i + (unsigned)((4 * wave + ry) * E1_IH + rx + kx) * 128u + (unsigned)(((((rx + kx) >> 1) & 7) << 4) ^ (hb << 5));
    // conv2 B operand: row tap * 32 + fr of W2: (row >> 1) & 7 == (fr >> 1) & 7
    const unsigned c2_b = (unsigned)fr * 128u + (unsigned)((((fr >> 1) & 7) << 4) ^ (hb << 5));          // + tap * 4096, ^ ((sstep << 6) | (hl << 4))
    // epilogue 2 staging (inside INT): row fr of the wave's tile, 8-byte half hb of piece 2 j + hl  ->  (base ^ ((2 j + hl) << 4))
    const unsigned stg0 = lds_i + (unsigned)wave * E1_STAGE_BYTES;
    const unsigned e2_w = stg0 + (unsigned)fr * 128u + (unsigned)(((fr >> 1) & 7) << 4) + (unsigned)hb * 8u;
    const bool pool_lane = ry == 1 && (rx & 1) == 0;                  // e1_pool4's result is valid in the odd 16-lane rows
    const unsigned e2_pw = stg0 + 32u * 128u + (unsigned)(rx >> 1) * 128u + (unsigned)(((rx >> 2) & 7) << 4) + (unsigned)hb * 8u;
    const unsigned e2_r = stg0 + (unsigned)(lane >> 3) * 128u + (unsigned)(((lane & 7) ^ ((lane >> 4) & 7)) << 4);        // read-back: row q*8 + lane/8, piece lane%8

    // ---- prologue: first halo of each group in flight, weights landed -----------------------------------------------------------------------------
    const int np_group = (a.npatch - gidx + gstride - 1) / gstride;  // patches this group owns (may be 0)
    const int np_max = (a.npatch + gstride - 1) / gstride;           // trip count of every group of every workgroup's loop (barrier parity)
    if (np_group > 0) issue_xin(gidx);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#if E1_PHASE_OFFSET
    if (group == 1) __builtin_amdgcn_s_barrier();                    // group 1 runs one phase behind group 0
#endif

    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < np_max; ++it) {
        const bool act = it < np_group;
        const int p = gidx + it * gstride;
        int b = 0, oy0 = 0, ox0 = 0;
        if (act) patch_origin(p, b, oy0, ox0);

        // ================= phase 0: conv1 (8 -> 32) on the 18 x 18 halo, two taps per k-step ============================================================
        f32x16 acc0[3], acc1[3];
        if (act) {
            // address bases are made opaque at the start of the phase that uses them: whatever is derived from them (per-step sums, XOR variants) is then
            // computed inside that phase and does not occupy registers during the other three (hoisted, they cost ~60 VGPRs and spilled)
            unsigned q1[3] = {c1_q[0], c1_q[1], c1_q[2]};
            asm volatile("" : "+v"(q1[0]), "+v"(q1[1]), "+v"(q1[2]));
            half8 wh[2], wl[2], xh[2][3], xl[2][3];
            auto fetch1 = [&](int s, int set) {
                wh[set] = *(const half8*)L(w1_base + (unsigned)((s * 2 + 0) * 2) * 512u);
                wl[set] = *(const half8*)L(w1_base + (unsigned)((s * 2 + 1) * 2) * 512u);
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const unsigned q = q1[t] + c1_tap[s];
                    xh[set][t] = *(const half8*)L(q);
                    xl[set][t] = *(const half8*)L(q + E1_XSLOTS * 16);
                }
            };
            fetch1(0, 0);
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const int cur = s & 1;
                e1_frag_ready(wh[cur], wl[cur], xh[cur][2], xl[cur][2]);
                if (s + 1 < 5) fetch1(s + 1, cur ^ 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < 3; ++t) acc0[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[cur], xh[cur][t], s == 0 ? zero16 : acc0[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 3; ++t) acc1[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[cur], xh[cur][t], s == 0 ? zero16 : acc1[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 3; ++t) acc1[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[cur], xl[cur][t], acc1[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                // every wave of the group has read XIN: it may be refilled

        // ================= phase 1: conv1 epilogue: BN + ReLU, zero outside the image, split16 -> INT =================================
        if (act) {
            f32x4 sc[4], sh[4];                                       // this lane's 16 channels (4 per group j): one LDS round trip per phase
#pragma unroll
            for (int j = 0; j < 4; ++j) { sc[j] = *(const f32x4*)(coef + 0 + j * 8 + hb * 4); sh[j] = *(const f32x4*)(coef + 32 + j * 8 + hb * 4); }
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                if (3 * wave + t < 11) {                              // wave-uniform: row tile 11 is all padding
                    int m = c1_m[t];
                    asm volatile("" : "+v"(m));                       // the pixel decomposition is redone per patch (cheap) instead of living in registers
                    const int mc = m < E1_IPIX ? m : E1_IPIX - 1;
                    const int hy = (mc * 3641) >> 16, hx = mc - hy * E1_IH;
                    const int gy = oy0 - 1 + hy, gx = ox0 - 1 + hx;
                    const bool inimg = gy >= 0 && gy < H && gx >= 0 && gx < W;
                    const unsigned dst = lds_i + (unsigned)mc * 128u + (unsigned)hb * 8u + (unsigned)(((hx >> 1) & 7) << 4);
                    const bool own = m < E1_IPIX;                     // rows past the halo (tile 10 holds 4 pixels) store nothing
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {                  // 8 values (channel groups 2 hf, 2 hf + 1) at a time: enough independent work, half the temporaries
                        float y[8];
                        E1_FENCE();
#pragma unroll
                        for (int r = 0; r < 8; ++r) y[r] = acc0[t][hf * 8 + r] + acc1[t][hf * 8 + r] * (1.0f / 2048.0f);
                        E1_FENCE();
#pragma unroll
                        for (int r = 0; r < 8; ++r) y[r] = y[r] * sc[hf * 2 + (r >> 2)][r & 3] + sh[hf * 2 + (r >> 2)][r & 3];
                        E1_FENCE();
#pragma unroll
                        for (int r = 0; r < 8; ++r) y[r] = inimg ? fmaxf(y[r], 0.f) : 0.f;
                        E1_FENCE();
                        unsigned hi[4], lo[4];
                        e1_split8<false>(y, hi, lo, rng);
                        if (own) {                                    // (a dump row for the other lanes serialises: same-address LDS writes are bank conflicts)
#pragma unroll
                            for (int jj = 0; jj < 2; ++jj) {
                                const int j = hf * 2 + jj;
                                const uint2v vh = {hi[2 * jj], hi[2 * jj + 1]}, vl = {lo[2 * jj], lo[2 * jj + 1]};
                                *(uint2v*)L(dst ^ (unsigned)((2 * j) << 4)) = vh;
                                *(uint2v*)L(dst ^ (unsigned)((2 * j + 1) << 4)) = vl;
                            }
                        }
                        E1_FENCE();
                    }
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                // INT is complete

        // ================= phase 2: conv2 (32 -> 32) on the 16 x 16 patch from INT; wave w owns output rows 4 w .. 4 w + 3 =================================
        f32x16 d0[2], d1[2];
        if (act) {
            // the next patch's input halo is requested here, under the MFMAs (XIN is free since the barrier that ended phase 0); issued from the epilogue
            // phase it cost that phase ~1.1 k cycles (address arithmetic + the LDS-DMA instructions' own issue time) and the epilogues set the period
            if (it + 1 < np_group) issue_xin(p + gstride);
            unsigned a2[3] = {c2_a[0], c2_a[1], c2_a[2]}, b2 = c2_b;
            asm volatile("" : "+v"(a2[0]), "+v"(a2[1]), "+v"(a2[2]), "+v"(b2));
            half8 bh[2], bl[2], ah[2][2], al[2][2];
            auto fetch2 = [&](int t, int set) {
                const int tap = t >> 1, sstep = t & 1, ky = tap / 3, kx = tap % 3;
                const unsigned ch = (unsigned)(sstep << 6), cl = ch | 16u;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const unsigned disp = (unsigned)((2 * i + ky) * E1_IH * 128);
                    ah[set][i] = *(const half8*)L((a2[kx] ^ ch) + disp);
                    al[set][i] = *(const half8*)L((a2[kx] ^ cl) + disp);
                }
                bh[set] = *(const half8*)L((b2 ^ ch) + (unsigned)tap * 4096u);
                bl[set] = *(const half8*)L((b2 ^ cl) + (unsigned)tap * 4096u);
            };
            fetch2(0, 0);
#pragma unroll
            for (int t = 0; t < 18; ++t) {
                const int cur = t & 1;
                e1_frag_ready(bh[cur], bl[cur], ah[cur][1], al[cur][1]);
                if (t + 1 < 18) fetch2(t + 1, cur ^ 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 2; ++i) d0[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[cur], ah[cur][i], t == 0 ? zero16 : d0[i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i) d1[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[cur], ah[cur][i], t == 0 ? zero16 : d1[i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i) d1[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[cur], al[cur][i], d1[i], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the next patch's halo (requested at the start of this phase) has landed before anyone passes this barrier; no store of this wave is outstanding here
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                // INT is dead: it becomes the per-wave output staging area

        // ================= phase 3: conv2 epilogue: BN + ReLU -> e1 tile + pooled tile, staged through LDS, 1 KiB stores ====================================
        if (act) {
            unsigned w3 = e2_w, pw3 = e2_pw, r3 = e2_r;
            asm volatile("" : "+v"(w3), "+v"(pw3), "+v"(r3));
            f32x4 sc[4], sh[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { sc[j] = *(const f32x4*)(coef + 64 + j * 8 + hb * 4); sh[j] = *(const f32x4*)(coef + 96 + j * 8 + hb * 4); }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    float y[8], pz[8], pw[8];
                    E1_FENCE();
#pragma unroll
                    for (int r = 0; r < 8; ++r) y[r] = d0[i][hf * 8 + r] + d1[i][hf * 8 + r] * (1.0f / 2048.0f);
                    E1_FENCE();
#pragma unroll
                    for (int r = 0; r < 8; ++r) y[r] = y[r] * sc[hf * 2 + (r >> 2)][r & 3] + sh[hf * 2 + (r >> 2)][r & 3];
                    E1_FENCE();
#pragma unroll
                    for (int r = 0; r < 8; ++r) y[r] = fmaxf(y[r], 0.f);
                    E1_FENCE();
                    // 2 x 2 max (valid in the odd 16-lane rows, see e1_pool4), stage by stage
#pragma unroll
                    for (int r = 0; r < 8; ++r) pz[r] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y[r]), 0xB1, 0xF, 0xF, true));
                    E1_FENCE();
#pragma unroll
                    for (int r = 0; r < 8; ++r) pz[r] = e1_max(y[r], pz[r]);
                    E1_FENCE();
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, pz[r]), __builtin_bit_cast(unsigned, pz[r]), false, false);
                        pw[r] = __builtin_bit_cast(float, sw[0]);
                    }
                    E1_FENCE();
#pragma unroll
                    for (int r = 0; r < 8; ++r) pz[r] = e1_max(pz[r], pw[r]);
                    E1_FENCE();
                    unsigned hi[4], lo[4], phi[4], plo[4];
                    e1_split8<true>(y, hi, lo, rng);
                    e1_split8<false>(pz, phi, plo, rng);
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const int j = hf * 2 + jj;
                        const uint2v vh = {hi[2 * jj], hi[2 * jj + 1]}, vl = {lo[2 * jj], lo[2 * jj + 1]};
                        *(uint2v*)L(w3 ^ (unsigned)((2 * j) << 4)) = vh;
                        *(uint2v*)L(w3 ^ (unsigned)((2 * j + 1) << 4)) = vl;
                    }
                    if (pool_lane) {                                  // 16 of the 64 lanes own a pooled pixel (exec mask; a shared dump address would serialise)
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj) {
                            const int j = hf * 2 + jj;
                            const uint2v ph = {phi[2 * jj], phi[2 * jj + 1]}, pl = {plo[2 * jj], plo[2 * jj + 1]};
                            *(uint2v*)L(pw3 ^ (unsigned)((2 * j) << 4)) = ph;
                            *(uint2v*)L(pw3 ^ (unsigned)((2 * j + 1) << 4)) = pl;
                        }
                    }
                    E1_FENCE();
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // per-wave staging: LDS operations of one wave execute in order
                const int oy = oy0 + 4 * wave + 2 * i;
                // 64 lanes x 16 B = 8 consecutive pixels = 1 KiB per instruction: rows q*8 .. q*8+7 of the tile are pixels (q >> 1, (q & 1) * 8 ..) of the 2 x 16 tile;
                // their swizzle term (row >> 1) & 7 = ((q & 1) << 2) | (lane >> 4): bit 6 of the address flips for odd q
                float* const orow = a.e1 + (((size_t)b * H + oy) * W + ox0) * 32 + lane * 4;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint4v val = *(const uint4v*)L((r3 ^ (unsigned)((q & 1) << 6)) + (unsigned)q * 1024u);
                    *(uint4v*)(orow + ((size_t)(q >> 1) * W + (q & 1) * 8) * 32) = val;
                }
                {                                                     // the 8 pooled pixels of this tile: one 1 KiB run of the pooled row
                    const uint4v val = *(const uint4v*)L(r3 + 4096u);
                    float* o = a.pool + (((size_t)b * (H >> 1) + (oy >> 1)) * (W >> 1) + (ox0 >> 1)) * 32 + lane * 4;
                    *(uint4v*)o = val;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the staging area is rewritten by the next tile
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                // staging reads done: INT may be written by the next patch's phase 1
    }
#if E1_PHASE_OFFSET
    if (group == 0) __builtin_amdgcn_s_barrier();                    // both groups have executed the same number of barriers
#endif
    rng.commit();
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
// Reference: src/smirk_generator.py:52-53 (enc1 = self.encoder1(x); self.pool1(enc1)), _block :88-119 (Conv2d 3x3 pad 1 bias=False, BatchNorm2d, ReLU, twice).
extern "C" int smirk_enc1_fused_supported(int cin_pad, int features, int H, int W) {
    return cin_pad == 8 && features == 32 && H >= E1_PT && W >= E1_PT && H % E1_PT == 0 && W % E1_PT == 0 && !smirk_switch(SMIRK_SW_DISABLE_ENC1_FUSED);
}

extern "C" int smirk_enc1_fused_split16(const void* x, const void* w1, const float* scale1, const float* shift1, const void* w2, const float* scale2,
                                        const float* shift2, void* e1, void* pooled, int B, int H, int W, void* stream) {
    if (!x || !w1 || !w2 || !scale1 || !shift1 || !scale2 || !shift2 || !e1 || !pooled || B <= 0) return SMIRK_ERR_BAD_ARG;
    if (H < E1_PT || W < E1_PT || H % E1_PT || W % E1_PT) return SMIRK_ERR_UNSUPPORTED;
    if (const int rc = smirk_raise_dynamic_lds((const void*)enc1_fused_kernel, E1_LDS_BYTES)) return rc;
    const int n_cu = smirk_device_cus();
    // the input halo goes through a buffer resource with 32-bit byte offsets: frames are independent, so larger batches run as chunks below 2 GiB of x
    const long long per_frame = (long long)H * W * 32;
    const int max_b = (int)(((1ll << 31) - 1) / per_frame);
    if (max_b <= 0) return SMIRK_ERR_UNSUPPORTED;
    for (int b0 = 0; b0 < B; b0 += max_b) {
        const int nb = B - b0 < max_b ? B - b0 : max_b;
        Enc1Args a;
        a.x = (const float*)x + (size_t)b0 * H * W * 8;
        a.w1 = (const float*)w1; a.w2 = (const float*)w2;
        a.sc1 = scale1; a.sh1 = shift1; a.sc2 = scale2; a.sh2 = shift2;
        a.e1 = (float*)e1 + (size_t)b0 * H * W * 32;
        a.pool = (float*)pooled + (size_t)b0 * (H / 2) * (W / 2) * 32;
        a.B = nb; a.H = H; a.W = W;
        a.npatch = nb * (H / E1_PT) * (W / E1_PT);
        const int want = (a.npatch + 1) / 2;
        const int grid = want < n_cu ? want : n_cu;
        if (g_smirk_prof_on) {
            const double px = (double)nb * H * W;
            smirk_prof_next("enc1_fused_kernel[conv8-32+conv32-32+pool]", 2.0 * px * 32.0 * (72.0 + 288.0), px * (32.0 + 128.0 + 32.0) + 4.0 * 32.0 * (72 + 288));
        }
        SMIRK_LAUNCH(enc1_fused_kernel, dim3(grid), dim3(512), E1_LDS_BYTES, (hipStream_t)stream, a);
        const int rc = smirk_launch_status();
        if (rc != SMIRK_OK) return rc;
    }
    return SMIRK_OK;
}
