// conv_halo.hip — halo-staged ping-pong implicit GEMM for the generator's deep 3x3 layers (split-fp16 arithmetic; 56^2 x 128, 28^2 x 256,
// 14^2 x 512 channels): conv_pp.hip's 8-wave schedule with the A (im2col) operand staged ONCE per 32-channel chunk instead of once per tap.
//
// Why.  conv_pp_kernel streams nine shifted copies of every input pixel through LDS (one 256-row x 128-byte A image per (tap, channel chunk)):
// 36 of a wave's 54 LDS-DMA instructions per channel chunk, the lever its own ablation identified (no A DMA: -19 % time) and
// the 2x over-fetch the PMC counters show.  Here GEMM rows are image pixels in RASTER order, so the tile's rows m0 .. m0+255 are consecutive
// NHWC pixels and tap (ky, kx) of row r is the pixel (ky-1) W + (kx-1) further on: ONE halo of 256 + 2 (W + 1) consecutive pixels x 32 channels
// serves all nine taps.  A lane reads its A fragment of tap t from halo row  r + (W+1) + dy_t W + dx_t; at image borders dy / dx are folded back
// (reflect padding) or the lane is pointed at a row of zeros (zero padding) — a per-lane table of 9 x 2 LDS offsets computed once per tile.
//   * A traffic L2 -> LDS per channel chunk: 1.12-1.45 x the tile (W = 14 .. 56) instead of 9 x; DMA instructions per wave and channel
//     chunk 5-6 + 18 (A + B) instead of 54; no per-chunk address VALU (the halo's per-lane source offset is one shift-add of a constant).
//   * B (weights) keeps conv_pp's 3-stage ring (one 128 x 32-k chunk per (tap, channel chunk)); the halo is double-buffered across channel
//     chunks: the pieces of chunk cc+1 are issued one per tap during the first taps of chunk cc.
//   * Same K order (channel-chunk-major, taps back to back) and the same per-accumulator MFMA sequence as conv_igemm_kernel's channel-major
//     walk and conv_pp_kernel: BIT-IDENTICAL results (tests/test_conv_gpu.py).
// LDS: B ring 48 KB + 2 halo buffers of 8 NPA KB (+ a 128-byte zero row each) = 128 KB (NPA 5: W <= 31) or 144 KB (NPA 6: W <= 63); one
// 512-thread workgroup per CU, the two waves of a SIMD one phase apart (conv_pp.hip header has the ordering rules; they apply unchanged:
// the halo buffer of chunk cc+1 was last read in chunk cc-1, whose last load phase every wave left through a barrier with lgkmcnt(0)).
//
// Bound: MFMA (dense fp16 2.5 PF, 3 MFMAs per product).  Algorithmic flop = 2*M*N*K per launch.
#include <stdio.h>
#include <type_traits>

#include "conv_common.h"

#define HS_BN 128                               /* HS_BM (256) and the 4 wave rows HS_WGM: conv_common.h, the dispatcher sizes the statistics rows from them */
#define HS_NSTAGE 3
#define HS_BRING_BYTES (HS_NSTAGE * HS_BN * 128) /* 49,152 B */
#define HS_EPI_LD (2 * 32 + 4)
#define HS_DEFAULT_EB 0

typedef __attribute__((address_space(3))) void* hs_lptr_t;

template <int K>
using hs_ic = std::integral_constant<int, K>;

// byte offset inside the B ring of (row, stage, 16-byte piece): blocks of 8 rows, the three stages of a block adjacent (conv_pp.hip)
template <int NST = HS_NSTAGE>
__device__ __forceinline__ int hs_b_off(int row, int stage, int piece) {
    return ((((row >> 3) * NST + stage) << 8) + ((row & 7) << 5) + ((piece ^ ((row >> 1) & 7)) << 2)) * 4;
}

// NPA: halo pieces (1 KiB = 8 pixel rows of 128 B) per wave and channel chunk; the halo buffer holds 64 NPA rows >= 256 + 2 (W + 1)
// EB:  "early barrier" — how many of a matrix phase's 24 MFMAs are issued AFTER the barrier that ends it (0, 4 or 8).  The phase timeline
//      (tools/halo_timeline.py) shows the matrix pipe idle for ~130 cycles at every hand-over: the finishing wave reaches the barrier, the barrier
//      releases, the partner wakes up and issues its first MFMA.  With the barrier placed EB MFMAs before the end, the finishing wave's tail keeps the
//      pipe busy while the partner wakes up.  Nothing the barrier orders depends on the position of a wave's MFMAs (they only touch registers).
// X1:  one fp16 MFMA per product block on the hi halves only (the training path's "f16x1" arithmetic, generator_train.TRAIN_ARITH): the lo fragments are neither
//      read from LDS nor multiplied — 8 of the 24 MFMAs and 8 of the 16 fragment reads of a chunk remain.  Same K order as conv_igemm_kernel's X1 instantiation.
// UP:  the coarse half of a decoder level whose ConvTranspose2d(k2 s2) is composed into the 3x3 convolution that reads it: GEMM rows are COARSE
//      raster pixels of ONE output parity class (dy, dx) (the class comes from the grid), K walks channel chunks x the class's 2 x 2 coarse taps
//      {dy-1, dy} x {dx-1, dx}, the weights are Weff[class] (ordinary conv rows [N][4 Cin]), the halo is the 256 + W + 1 consecutive pixels from the class's first
//      tap on (5 pieces for every W <= 63).  Four taps per chunk: the B ring has FOUR stages so that a tap's stage stays a compile-time constant.  Epilogue:
//      scale, the shift row of (class, row edge, column edge), no activation, stored at the FINE pixel (2y + dy, 2x + dx).
//      LDS: 64 KB ring + 2 x (40 KB + 128 B) halo = 147,712 B; 234 VGPRs, no scratch (-Rpass-analysis=kernel-resource-usage).
template <int NPA, int EB, bool X1, bool STATS = false, bool UP = false>
__device__ __forceinline__ void conv_halo_body(const ConvArgs& a) {
    constexpr int NTAP = UP ? 4 : 9, NST = UP ? 4 : HS_NSTAGE;
    constexpr int NL = UP ? 4 : 3;   // DMA instructions issued in the load phase: 1-3 measured equal, 0 (all among the MFMAs) 2-3 % slower (profiles/r03b_halo_nl_sweep.txt)
    extern __shared__ __attribute__((aligned(16))) float hs_smem[];
    char* lds = (char*)hs_smem;
    constexpr int ABUF = NPA * 8 * 1024;                            // one halo buffer
    constexpr int ASTRIDE = ABUF + 128;                             // + its row of zeros (byte offset ABUF inside the buffer)
    constexpr int A0 = NST * HS_BN * 128;                               // halo buffer u starts at A0 + u * ASTRIDE
    const SmirkConvDesc& d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int swave = __builtin_amdgcn_readfirstlane(wave);
    const int wm = wave >> 1, wn = wave & 1;                       // 4 (M) x 2 (N) waves of 64 x 64
    const int group = swave >> 2;                                    // 0: leads, 1: one phase behind (shares each SIMD with a wave of group 0)
    const int ntn = a.N / HS_BN;
    int logical = xcd_logical(blockIdx.x, gridDim.x);
    int cls = 0;                                                     // UP: the grid is 4 classes x tiles, a class's tiles adjacent (they share Weff[class] in L2)
    if constexpr (UP) { const int ntile = (int)gridDim.x >> 2; cls = logical / ntile; logical -= cls * ntile; }
    const int dyc = cls >> 1, dxc = cls & 1;
    const int m0 = (logical / ntn) * HS_BM, n0 = (logical % ntn) * HS_BN;
    const int W = d.W, HW = d.H * d.W;
    const float* const wcls = UP ? a.w + (size_t)cls * a.N * a.K : a.w;
    const int fr = lane & 31, hb = lane >> 5;

    // ---- zero rows (read by every tap that falls into the zero padding) ------------------------------------------------------------------------
    if (tid < 64) *(float*)(lds + A0 + (tid >> 5) * ASTRIDE + ABUF + (tid & 31) * 4) = 0.f;

    unsigned tabA[NTAP];                                              // per-lane tap table, filled in the prologue while the first DMAs fly
    // B fragment bases: (k-step 0, hi) piece of rows (wn*2 + j)*32 + fr in stage 0
    unsigned bB[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bB[j] = (unsigned)hs_b_off<NST>((wn * 2 + j) * 32 + fr, 0, 2 * hb);

    // ---- DMA coordinates ------------------------------------------------------------------------------------------------------------------------
    const int pos = lane & 7, lrow = lane >> 3;                    // a wave-wide LDS-DMA writes 8 rows x 8 pieces lane-linearly
    // halo piece k of this wave = block swave + 8k = halo rows 8 (swave + 8k) + lrow; (row >> 1) & 7 does not depend on k
    const unsigned colA16 = (unsigned)(pos ^ ((4 * (swave & 1) + (lrow >> 1)) & 7)) * 16u;
    const int qv0 = m0 + (UP ? (dyc - 1) * W + (dxc - 1) : -(W + 1)) + 8 * swave + lrow;                // linear pixel of piece 0's row (may be negative / beyond the tensor)
    const int npix = d.B * HW;
    unsigned voffB[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int brow = 8 * (swave + 8 * p) + lrow;
        voffB[p] = ((unsigned)min(n0 + brow, a.N - 1) * (unsigned)a.K + (unsigned)(pos ^ ((brow >> 1) & 7)) * 4u) * 4u;
    }
    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)a.in0, (short)0, (int)((long long)npix * d.C0 * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)(d.C1 > 0 ? a.in1 : a.in0), (short)0,
                                                                         (int)((long long)npix * (d.C1 > 0 ? d.C1 : d.C0) * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)wcls, (short)0, (int)((long long)a.N * a.K * 4), 0x00020000);
    const int sh0 = 31 - __builtin_clz((unsigned)d.C0) + 2, sh1 = d.C1 > 0 ? 31 - __builtin_clz((unsigned)d.C1) + 2 : sh0;
    const int ncc = (d.C0 + d.C1) / CV_BK;

    // halo piece KP of channel chunk cc -> halo buffer at byte offset abase
    auto dmaA = [&](int cc, int abase, auto kc) {
        constexpr int KP = decltype(kc)::value;
        const int c0 = cc * CV_BK;
        const bool s1 = c0 >= d.C0;
        const int q = qv0 + 64 * KP;
        unsigned vo = ((unsigned)q << (s1 ? sh1 : sh0)) + colA16;
        vo = ((unsigned)q < (unsigned)npix) ? vo : 0x80000000u;  // outside the tensor: beyond num_records => the DMA writes zeros
        const int so = (s1 ? c0 - d.C0 : c0) * 4;
        char* dst = lds + abase + (swave + 8 * KP) * 1024;
        if (s1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (hs_lptr_t)dst, 16, vo, so, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (hs_lptr_t)dst, 16, vo, so, 0, 0);
    };
    // weight chunk (cc, TAP) -> ring stage ST: piece P (of 2) of this wave
    auto dmaB1 = [&](int cc, auto tapc, auto stc, auto pc) {
        constexpr int TAP = decltype(tapc)::value, ST = decltype(stc)::value, P = decltype(pc)::value;
        const int so = (TAP * a.Cin + cc * CV_BK) * 4;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (hs_lptr_t)(lds + (((swave + 8 * P) * NST + ST) << 10)), 16, voffB[P], so, 0, 0);
    };
    auto dmaB = [&](int cc, auto tapc, auto stc) {
        dmaB1(cc, tapc, stc, hs_ic<0>{});
        dmaB1(cc, tapc, stc, hs_ic<1>{});
    };

    f32x16 acc0[2][2], acc1[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[i][j][r] = 0.f; acc1[i][j][r] = 0.f; }
    half8 ah[2][2], al[2][2], bh[2][2], bl[2][2];                   // [k-step][block]

    // one (load phase, matrix phase) pair for chunk (cc, TAP): A from the halo buffer at `acur`, B from ring stage TAP % 3
    auto body = [&](int cc, int acur, int anext, auto tapc) {
        constexpr int TAP = decltype(tapc)::value, ST = TAP % NST;
        // ---- load phase ------------------------------------------------------------------------------------------------------------------------
        {
            const unsigned t = tabA[TAP];
            const unsigned a0 = (t & 0xffffu) + (unsigned)acur, a1 = (t >> 16) + (unsigned)acur;
            ah[0][0] = *(const half8*)(lds + a0);
            ah[1][0] = *(const half8*)(lds + (a0 ^ 64u));
            ah[0][1] = *(const half8*)(lds + a1);
            ah[1][1] = *(const half8*)(lds + (a1 ^ 64u));
            if constexpr (!X1) {
                al[0][0] = *(const half8*)(lds + (a0 ^ 16u)); al[1][0] = *(const half8*)(lds + (a0 ^ 80u));
                al[0][1] = *(const half8*)(lds + (a1 ^ 16u)); al[1][1] = *(const half8*)(lds + (a1 ^ 80u));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const unsigned b0 = bB[j];
                bh[0][j] = *(const half8*)(lds + b0 + ST * 1024);
                bh[1][j] = *(const half8*)(lds + (b0 ^ 64u) + ST * 1024);
                if constexpr (!X1) {
                    bl[0][j] = *(const half8*)(lds + (b0 ^ 16u) + ST * 1024);
                    bl[1][j] = *(const half8*)(lds + (b0 ^ 80u) + ST * 1024);
                }
            }
        }
        // this phase pair's DMA list: [halo piece TAP of the NEXT channel chunk (taps 0 .. NPA-1),] the two weight pieces of the chunk two ahead.  Past
        // the end of K the clamped last chunk is fetched again into a buffer / stage nobody reads: no branch in the loop bodies.
        // (UP: a piece issued in phase q by a wave of the trailing group is only known to have landed when the leading group enters phase q + 2, so the next
        // chunk's halo must be out by tap 2 of 4: tap t < 3 issues pieces t and t + 3, NPA <= 6)
        constexpr int T2 = (TAP + 2) % NTAP;
        constexpr int HASA = UP ? (TAP < 3 ? 1 + (TAP + 3 < NPA ? 1 : 0) : 0) : (TAP < NPA ? 1 : 0), NDMA = 2 + HASA, NLD = NL < NDMA ? NL : NDMA;
        const int ccA = min(cc + 1, ncc - 1), ccB = min(cc + (TAP + 2 >= NTAP ? 1 : 0), ncc - 1);
        auto dma = [&](auto kc) {                                    // DMA instruction K of the list
            constexpr int K = decltype(kc)::value;
            if constexpr (K < HASA) dmaA(ccA, anext, hs_ic<(TAP + 3 * K < NPA ? TAP + 3 * K : 0)>{});
            else dmaB1(ccB, hs_ic<T2>{}, hs_ic<T2 % NST>{}, hs_ic<(K - HASA) & 1>{});
        };
        if constexpr (NLD > 0) dma(hs_ic<0>{});
        if constexpr (NLD > 1) dma(hs_ic<1>{});
        if constexpr (NLD > 2) dma(hs_ic<2>{});
        if constexpr (NLD > 3) dma(hs_ic<3>{});
        // everything older than this load phase's DMA instructions has landed (this wave's share of chunk q+1's weights, and every halo piece issued
        // in an earlier phase); fragment reads done
        if constexpr (NLD == 4) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else if constexpr (NLD == 3) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
        else if constexpr (NLD == 2) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        else if constexpr (NLD == 1) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- matrix phase: 24 MFMAs, operands in registers; dependent accumulations four instructions apart; the DMA instructions left over from
        //      the load phase go out one after every fourth MFMA (an LDS-DMA costs ~60 issue cycles among bare MFMAs, MI355X_MICROARCH.md) ---------
        __builtin_amdgcn_s_setprio(1);
        auto mm_dma = [&](auto gc) {
            constexpr int G = decltype(gc)::value;
            if constexpr (NLD + G < NDMA) {
                __builtin_amdgcn_sched_barrier(0);
                dma(hs_ic<(NLD + G < NDMA ? NLD + G : 0)>{});
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        auto mblock = [&](auto bc) {                                 // MFMA block B (0-5) of the chunk: 4 independent accumulators
            constexpr int BK = decltype(bc)::value;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if constexpr (BK == 0) acc0[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[0][i], bh[0][j], acc0[i][j], 0, 0, 0);
                    if constexpr (BK == 1 && !X1) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[0][i], bl[0][j], acc1[i][j], 0, 0, 0);
                    if constexpr (BK == 2 && !X1) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[0][i], bh[0][j], acc1[i][j], 0, 0, 0);
                    if constexpr (BK == 3) acc0[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[1][i], bh[1][j], acc0[i][j], 0, 0, 0);
                    if constexpr (BK == 4 && !X1) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[1][i], bl[1][j], acc1[i][j], 0, 0, 0);
                    if constexpr (BK == 5 && !X1) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[1][i], bh[1][j], acc1[i][j], 0, 0, 0);
                }
        };
        auto hand_over = [&]() {                                     // the barrier that ends the matrix phase
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        };
        mblock(hs_ic<0>{});
        mm_dma(hs_ic<0>{});
        mblock(hs_ic<1>{});
        mm_dma(hs_ic<1>{});
        mblock(hs_ic<2>{});
        mm_dma(hs_ic<2>{});
        mblock(hs_ic<3>{});
        if constexpr (EB == 8) hand_over();
        mblock(hs_ic<4>{});
        if constexpr (EB == 4) hand_over();
        mblock(hs_ic<5>{});
        __builtin_amdgcn_s_setprio(0);
        if constexpr (EB == 0) hand_over();
        else __builtin_amdgcn_sched_barrier(0);
    };

    // ---- prologue: the halo of chunk 0 and weight chunks 0 and 1 in flight, everything but weight chunk 1 landed; group 1 drops one phase behind ----
    dmaA(0, A0, hs_ic<0>{}); dmaA(0, A0, hs_ic<1>{}); dmaA(0, A0, hs_ic<2>{}); dmaA(0, A0, hs_ic<3>{}); dmaA(0, A0, hs_ic<4>{});
    if constexpr (NPA > 5) dmaA(0, A0, hs_ic<5>{});
    dmaB(0, hs_ic<0>{}, hs_ic<0>{});
    dmaB(0, hs_ic<1>{}, hs_ic<1>{});
    __builtin_amdgcn_sched_barrier(0);                             // the first operands are in flight while the tap table (4 integer divisions) is computed
    // ---- per-lane tap table: LDS byte offset (inside a halo buffer) of the (k-step 0, hi) piece of this lane's A row for each tap; rows i = 0 / 1
    //      of the wave tile in the low / high 16 bits.  The other three pieces of a row are offset ^ 16 (lo), ^ 64 (k-step 1), ^ 80. --------------
    {
        unsigned ent[2][NTAP];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rl = (wm * 2 + i) * 32 + fr;
            const int m = m0 + rl;
            const int b = m / HW, rem = m - b * HW, y = rem / W, x = rem - y * W;
#pragma unroll
            for (int t = 0; t < NTAP; ++t) {
                if constexpr (UP) {                               // tap (ta, tb) reads coarse pixel (y + dy - 1 + ta, x + dx - 1 + tb) = halo row rl + ta W + tb
                    const int ta = t >> 1, tb = t & 1, ay = y + dyc - 1 + ta, ax = x + dxc - 1 + tb;
                    const bool zero = m >= a.M || ay < 0 || ay >= d.H || ax < 0 || ax >= W;
                    const int p = rl + ta * W + tb;
                    ent[i][t] = zero ? (unsigned)ABUF : (unsigned)p * 128u + (unsigned)(((2 * hb) ^ ((p >> 1) & 7)) << 4);
                    continue;
                }
                int dy = t / 3 - 1, dx = t % 3 - 1;
                bool zero = m >= a.M;
                if (d.pad_mode == SMIRK_PAD_REFLECT) {
                    if (y + dy < 0 || y + dy >= d.H) dy = -dy;
                    if (x + dx < 0 || x + dx >= W) dx = -dx;
                } else {
                    zero = zero || y + dy < 0 || y + dy >= d.H || x + dx < 0 || x + dx >= W;
                }
                const int p = rl + (W + 1) + dy * W + dx;         // halo row
                const unsigned off = (unsigned)p * 128u + (unsigned)(((2 * hb) ^ ((p >> 1) & 7)) << 4);
                ent[i][t] = zero ? (unsigned)ABUF : off;
            }
        }
#pragma unroll
        for (int t = 0; t < NTAP; ++t) tabA[t] = ent[0][t] | (ent[1][t] << 16);
    }
    asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (group == 1) __builtin_amdgcn_s_barrier();
    for (int cc = 0; cc < ncc; ++cc) {
        const int acur = A0 + (cc & 1) * ASTRIDE, anext = A0 + ((cc + 1) & 1) * ASTRIDE;
        body(cc, acur, anext, hs_ic<0>{}); body(cc, acur, anext, hs_ic<1>{}); body(cc, acur, anext, hs_ic<2>{});
        body(cc, acur, anext, hs_ic<3>{});
        if constexpr (!UP) {
            body(cc, acur, anext, hs_ic<4>{}); body(cc, acur, anext, hs_ic<5>{});
            body(cc, acur, anext, hs_ic<6>{}); body(cc, acur, anext, hs_ic<7>{}); body(cc, acur, anext, hs_ic<8>{});
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the over-fetched pieces must have landed before LDS is reused
    // ---- epilogue operands, requested BEFORE the closing barriers so that the loads fly while the workgroup drains ------------------------------
    // Every lane serves ONE 8-channel group (g = lane % 8) of 4 pixel rows per 32-row block: scale / shift are loaded once, and all eight residual
    // groups (2 blocks x 4 rows) are requested up front: the epilogue pays one memory round trip, not one per block (the fragment registers are free now).
    float* ebuf = hs_smem + wave * 32 * HS_EPI_LD;
    constexpr int GPR = 8, ITEMS = 32 * GPR / 64;
    const int eg = lane & 7, erow = lane >> 3;                       // item = it * 64 + lane: row = it * 8 + erow, group = eg
    const int en = n0 + wn * 64 + eg * 8;
    f32x4 sc0 = {1.f, 1.f, 1.f, 1.f}, sc1 = sc0, sf0 = {0.f, 0.f, 0.f, 0.f}, sf1 = sf0;
    if (a.scale) { sc0 = *(const f32x4*)(a.scale + en); sc1 = *(const f32x4*)(a.scale + en + 4); }
    if (!UP && a.shift) { sf0 = *(const f32x4*)(a.shift + en); sf1 = *(const f32x4*)(a.shift + en + 4); }
    half8 resh[2][ITEMS], resl[2][ITEMS];
    // UP: every item's fine pixel (2y + dy, 2x + dx) and its shift row [class][row edge][column edge][N] — a class-dy row touches the border only at y = 0
    // (dy = 0) or y = H - 1 (dy = 1), columns likewise — requested up front like the residual groups
    size_t uo[2][ITEMS];
    f32x4 us0[2][ITEMS], us1[2][ITEMS];
    if constexpr (UP) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                const int m = min(m0 + (wm * 2 + i) * 32 + it * 8 + erow, a.M - 1);
                const int b = m / HW, rem = m - b * HW, y = rem / W, x = rem - y * W;
                const int re = y == (dyc ? d.H - 1 : 0), ce = x == (dxc ? W - 1 : 0);
                uo[i][it] = (((size_t)b * (2 * d.H) + (2 * y + dyc)) * (size_t)(2 * W) + (2 * x + dxc)) * d.Cout + en;
                const float* const srow = a.shift + (size_t)((cls * 2 + re) * 2 + ce) * a.N + en;
                us0[i][it] = *(const f32x4*)srow;
                us1[i][it] = *(const f32x4*)(srow + 4);
            }
    }
    if (!UP && a.residual) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                const int m = min(m0 + (wm * 2 + i) * 32 + it * 8 + erow, a.M - 1);
                const size_t o = (size_t)m * d.Cout + en;
                resh[i][it] = *(const half8*)(a.residual + o);
                resl[i][it] = *(const half8*)(a.residual + o + 4);
            }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (group == 0) __builtin_amdgcn_s_barrier();                   // both groups have executed the same number of barriers ...
    __builtin_amdgcn_s_barrier();                                   // ... and every wave's DMA has retired

    // ---- epilogue: per-wave transpose through LDS, whole 8-channel groups, BN scale/shift + residual + ReLU, re-split ---------------------------
    SmirkRangeAcc rng;                                              // split-fp16 range audit (common.h): one running max per lane, tested once after the stores
    float st1[2] = {0.f, 0.f}, st2[2] = {0.f, 0.f};                 // STATS (train mode): this lane's column sums over the wave's 64 rows (conv_common.h stats_block)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float x16[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                x16[r] = X1 ? acc0[i][j][r] : acc0[i][j][r] + acc1[i][j][r] * (1.0f / 2048.0f);
                ebuf[mfma32_row(r, lane) * HS_EPI_LD + j * 32 + fr] = x16[r];
            }
            if constexpr (STATS) stats_block(x16, lane, a.M - (m0 + (wm * 2 + i) * 32), st1[j], st2[j]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int row = it * 8 + erow;
            const int m = m0 + (wm * 2 + i) * 32 + row;
            if (m < a.M) {
                float v[8];
                *(f32x4*)v = *(const f32x4*)(ebuf + row * HS_EPI_LD + eg * 8);
                *(f32x4*)(v + 4) = *(const f32x4*)(ebuf + row * HS_EPI_LD + eg * 8 + 4);
                const size_t o = UP ? uo[i][it] : (size_t)m * d.Cout + en;   // raster order: GEMM row m IS the NHWC pixel index (UP: of the coarse tensor)
                if (a.scale) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { v[q] *= sc0[q]; v[4 + q] *= sc1[q]; }
                }
                if constexpr (UP) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { v[q] += us0[i][it][q]; v[4 + q] += us1[i][it][q]; }
                } else if (a.shift) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { v[q] += sf0[q]; v[4 + q] += sf1[q]; }
                }
                if (!UP && a.residual) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] += join1(resh[i][it][q], resl[i][it][q]);
                }
                if (!UP && d.act == SMIRK_ACT_RELU) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] = fmaxf(v[q], 0.f);
                }
                half8 hi, lo;
                split8(v, hi, lo, rng);
                *(half8*)(a.out + o) = hi;
                *(half8*)(a.out + o + 4) = lo;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    rng.commit();
    if constexpr (STATS) {                                           // partial row (M tile, wave row 0..3): [N][2] floats, each (row, channel) written by one lane
        float* prow = a.stats + (size_t)((m0 / HS_BM) * 4 + wm) * a.N * 2;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float t1 = stats_pair(st1[j]), t2 = stats_pair(st2[j]);
            const int n = n0 + wn * 64 + j * 32 + fr;
            if ((lane >> 5) == 0) { prow[n * 2] = t1; prow[n * 2 + 1] = t2; }
        }
    }
}

template <int NPA, int EB>
__global__ __launch_bounds__(512, 2) void conv_halo_kernel(ConvArgs a) { conv_halo_body<NPA, EB, false>(a); }
template <int NPA>
__global__ __launch_bounds__(512, 2) void conv_halo_x1_kernel(ConvArgs a) { conv_halo_body<NPA, 0, true>(a); }
// train mode: the same kernels leaving the BatchNorm partial sums of their raw output (ConvArgs::stats; one row per M tile and wave row)
template <int NPA, int EB>
__global__ __launch_bounds__(512, 2) void conv_halo_stats_kernel(ConvArgs a) { conv_halo_body<NPA, EB, false, true>(a); }
template <int NPA>
__global__ __launch_bounds__(512, 2) void conv_halo_x1_stats_kernel(ConvArgs a) { conv_halo_body<NPA, 0, true, true>(a); }
// the coarse half of a composed decoder level (UP above): grid = 4 classes x tiles, a.d describes the COARSE tensor, a.w = Weff, a.shift = the 16 shift rows
template <int NPA>
__global__ __launch_bounds__(512, 2) void conv_halo_up_kernel(ConvArgs a) { conv_halo_body<NPA, 0, false, false, true>(a); }
// ... in the generator's f16x1 inference arithmetic: the same walk over the same composed pairs, one MFMA per product block on their hi halves (X1 above)
template <int NPA>
__global__ __launch_bounds__(512, 2) void conv_halo_up_x1_kernel(ConvArgs a) { conv_halo_body<NPA, 0, true, false, true>(a); }

// Serves: split-fp16, 3x3, stride 1, pad 1, NHWC out, both sources power-of-two multiples of 32 channels, N a multiple of 128, W <= 63, operands < 2 GiB.
bool smirk_conv_halo_eligible(const ConvArgs& a) {
    const SmirkConvDesc& d = a.d;
    if (!smirk_switch(SMIRK_SW_IGEMM_HALO)) return false;
    if (d.KH != 3 || d.KW != 3 || d.stride != 1 || d.out_mode != SMIRK_OUT_NHWC || d.pad_t != 1 || d.pad_l != 1) return false;
    if (d.Ho != d.H || d.Wo != d.W || d.W > 63 || d.W < 2 || d.H < 2) return false;
    if (d.C0 % CV_BK || d.C1 % CV_BK || (d.C0 & (d.C0 - 1)) || (d.C1 & (d.C1 - 1))) return false;
    if (a.N % HS_BN || a.N < HS_BN) return false;
    if (!conv_operands_fit32(a)) return false;
    if (a.M < 4 * HS_BM) return false;                               // tiny problems stay on the 128-row tiles
    // Measured per layer against the kernels it replaces (tools/conv_sweep.py, profiles/r03c_halo_sweep.txt): at 1024 frames per pass every deep
    // layer gains 12-18 % (14x14: 421 -> 502-513 TFLOP/s, 28x28: 405-420 -> 487-523, 56x56: 361-398 -> 431-483); at 128 frames the layers with
    // K >= 2304 gain 3-13 % and the short-K layers (18-36 chunks per tile: the lone workgroup's prologue / epilogue are exposed) lose up to 8 % when timed
    // ALONE.  Rounds 3-4 therefore kept short-K layers with < 2048 tiles on the 128 x 128 tiles; inside the pipeline (other streams fill what a lone
    // workgroup per CU leaves idle) every eligible layer on this kernel measures +1.1 % at 128 frames per pass and +-0.1 % at 1024
    // (profiles/r04x_kernel_selection.txt; round 4 had seen the same +1 % on 4 hardware queues), so the threshold is gone.
    return true;
}

template <int NPA, int EB, bool X1>
static int hs_launch(const ConvArgs& a, hipStream_t st, size_t lds) {
    const void* fn = X1 ? (const void*)conv_halo_x1_kernel<NPA> : (const void*)conv_halo_kernel<NPA, EB>;
    const void* fns = X1 ? (const void*)conv_halo_x1_stats_kernel<NPA> : (const void*)conv_halo_stats_kernel<NPA, EB>;
    if (const int rc = smirk_raise_dynamic_lds(a.stats ? fns : fn, 160 * 1024)) return rc;
    const int ntm = (a.M + HS_BM - 1) / HS_BM, ntn = a.N / HS_BN;
    if (g_smirk_prof_on) {
        char nm[64];
        if (X1) snprintf(nm, sizeof(nm), "conv_halo_x1_kernel<%d>[256x128,8w,halo,f16x1]", NPA);
        else snprintf(nm, sizeof(nm), "conv_halo_kernel<%d,%d>[256x128,8w,halo]", NPA, EB);
        conv_prof_next(nm, a);
    }
    if (a.stats) {
        if constexpr (X1) SMIRK_LAUNCH((conv_halo_x1_stats_kernel<NPA>), dim3(ntm * ntn), dim3(512), lds, st, a);
        else SMIRK_LAUNCH((conv_halo_stats_kernel<NPA, EB>), dim3(ntm * ntn), dim3(512), lds, st, a);
        return smirk_launch_status();
    }
    if constexpr (X1) SMIRK_LAUNCH((conv_halo_x1_kernel<NPA>), dim3(ntm * ntn), dim3(512), lds, st, a);
    else SMIRK_LAUNCH((conv_halo_kernel<NPA, EB>), dim3(ntm * ntn), dim3(512), lds, st, a);
    return smirk_launch_status();
}

int smirk_conv_halo_launch(const ConvArgs& a, hipStream_t st, bool x1) {
    const int npa = (HS_BM + 2 * (a.d.W + 1) + 63) / 64;             // 64 halo rows per piece index (8 waves x 8 rows)
    const size_t lds = HS_BRING_BYTES + 2 * ((size_t)(npa <= 5 ? 5 : 6) * 8 * 1024 + 128);
    // (EB = MFMAs issued after the hand-over barrier: 4 / 8 measured 3-7 % slower without the time stamps in, profiles/r03b_halo_nl_sweep.txt, r04x_kernel_selection.txt;
    // the $SMIRK_HALO_EB switch and its instantiations left the library in round 5)
    if (x1) return npa <= 5 ? hs_launch<5, HS_DEFAULT_EB, true>(a, st, lds) : hs_launch<6, HS_DEFAULT_EB, true>(a, st, lds);
    return npa <= 5 ? hs_launch<5, HS_DEFAULT_EB, false>(a, st, lds) : hs_launch<6, HS_DEFAULT_EB, false>(a, st, lds);
}

// ---- decoder levels 3 / 4: ConvTranspose2d(2c -> c, k2 s2) composed into the first 3x3 convolution of the level ----------------------------------
//   out = ReLU(scale * conv3x3(skip; W3[:, c:]) + shift + partial'),   partial'(2y + dy, 2x + dx) = scale * (sum over the class's 2 x 2 coarse taps of Weff . d + Beff)
// as TWO launches: conv_halo_up_kernel writes partial' where `up` used to go, the unchanged conv_halo_kernel runs the skip half with partial' as its residual.
// updeep_compose_kernel rebuilds, on every forward (the weight struct has no field for a cached image; in-place weight updates stay correct), per level:
//   weff   [4 classes][c][4 taps * 2c]   ordinary split-fp16 conv rows, tap (ta, tb) = coarse offset (dy - 1 + ta, dx - 1 + tb)
//   shift16[4 classes][row edge][column edge][c] fp32 = scale * (sum of W3 . bias over the fine taps inside the image)
//   wskip  [c][9 * c]                    the skip half of the conv rows
// from hi + lo / 2048 in fp64, re-split.  Block roles per level: 64 x 64 tiles of the (class, tap) GEMMs Weff = sum over the fine taps of the pair W3tap [c x c] .
// Wup_sub [c x 2c] (16 fp64 k-steps per LDS stage, 4 x 4 outputs per thread), then one block per output channel for the shift rows, then the copy blocks.
struct UpdeepLevelArgs {
    const float *wup, *bup, *w3, *scale;
    float *weff, *shift16, *wskip;
    int c, blk0, ngemm, nshift;
};
struct UpdeepComposeArgs {
    UpdeepLevelArgs lv[2];
};

__device__ __forceinline__ double hs_dec64(const _Float16* row, int k) {
    return (double)(float)row[(k >> 3) * 16 + (k & 7)] + (double)(float)row[(k >> 3) * 16 + 8 + (k & 7)] * (1.0 / 2048.0);
}

__global__ __launch_bounds__(256) void updeep_compose_kernel(UpdeepComposeArgs args) {
    __shared__ __attribute__((aligned(16))) double As[16][64];
    __shared__ __attribute__((aligned(16))) double Bs[16][64];
    __shared__ double S[9];
    const int li = (int)blockIdx.x >= args.lv[1].blk0 ? 1 : 0;
    const UpdeepLevelArgs& L = args.lv[li];
    const int C = L.c, CIN = 2 * C, tid = threadIdx.x;
    int r = (int)blockIdx.x - L.blk0;
    const _Float16* const w3h = (const _Float16*)L.w3;
    const _Float16* const wuh = (const _Float16*)L.wup;
    if (r < L.ngemm) {
        const int nci = CIN / 64, nco = C / 64;
        const int ci0 = (r % nci) * 64, co0 = ((r / nci) % nco) * 64, ct = r / (nci * nco);
        const int cls = ct >> 2, tap = ct & 3, dy = cls >> 1, dx = cls & 1, ca = dy - 1 + (tap >> 1), cb = dx - 1 + (tap & 1);
        const int tx = tid & 15, ty = tid >> 4;
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int fy = -1; fy <= 1; ++fy) {
            if (((dy + fy) >> 1) != ca) continue;
            for (int fx = -1; fx <= 1; ++fx) {
                if (((dx + fx) >> 1) != cb) continue;
                const int sub = ((dy + fy) & 1) * 2 + ((dx + fx) & 1), t3 = (fy + 1) * 3 + (fx + 1);
                for (int cu0 = 0; cu0 < C; cu0 += 16) {
                    if (tid < 128) {                                  // A stage: W3[co0 + row][t3][cu0 + 8 g ..]: one 8-channel group per thread, stored k-major
                        const int row = tid >> 1, g = tid & 1;
                        const _Float16* const src = w3h + ((size_t)((co0 + row) * 9 + t3) * CIN + cu0 + g * 8) * 2;
                        const half8 hi = *(const half8*)src, lo = *(const half8*)(src + 8);
#pragma unroll
                        for (int q = 0; q < 8; ++q) As[g * 8 + q][row] = (double)(float)hi[q] + (double)(float)lo[q] * (1.0 / 2048.0);
                    } else {                                          // B stage: Wup[sub][cu0 + krow][ci0 + 8 g ..]
                        const int t2 = tid - 128, krow = t2 >> 3, g = t2 & 7;
                        const _Float16* const src = wuh + ((size_t)(sub * C + cu0 + krow) * CIN + ci0 + g * 8) * 2;
                        const half8 hi = *(const half8*)src, lo = *(const half8*)(src + 8);
#pragma unroll
                        for (int q = 0; q < 8; ++q) Bs[krow][g * 8 + q] = (double)(float)hi[q] + (double)(float)lo[q] * (1.0 / 2048.0);
                    }
                    __syncthreads();
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        double av[4], bv[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) { av[i] = As[k][ty * 4 + i]; bv[i] = Bs[k][tx * 4 + i]; }
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
                    }
                    __syncthreads();
                }
            }
        }
        _Float16* const weh = (_Float16*)L.weff;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = co0 + ty * 4 + i, k = tap * CIN + ci0 + tx * 4;      // 4 channels = half of an 8-channel group: 4 hi halves, 4 lo halves
            _Float16* const dst = weh + ((size_t)(cls * C + co) * 4 * CIN) * 2 + (k >> 3) * 16 + (k & 7);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = (float)acc[i][j];
                const _Float16 hi = (_Float16)v;
                dst[j] = hi;
                dst[8 + j] = (_Float16)((v - (float)hi) * 2048.0f);
            }
        }
        return;
    }
    r -= L.ngemm;
    if (r < L.nshift) {                                                  // S[t] = W3[co][t][:c] . bias (wave w: taps w, w + 4, w + 8; fixed reduction order), then 16 rows
        const int co = r, lane = tid & 63, wave = tid >> 6;
        for (int t = wave; t < 9; t += 4) {
            const _Float16* const w3row = w3h + ((size_t)(co * 9 + t) * CIN) * 2;
            double s = 0.0;
            for (int cu = lane; cu < C; cu += 64) s += hs_dec64(w3row, cu) * (double)L.bup[cu];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) S[t] = s;
        }
        __syncthreads();
        if (tid < 16) {
            const int ce = tid & 1, re = (tid >> 1) & 1, cls = tid >> 2, dy = cls >> 1, dx = cls & 1;
            double acc = 0.0;
            for (int fy = -1; fy <= 1; ++fy) {
                if (re && fy == (dy ? 1 : -1)) continue;                  // this tap's fine row lies in the zero padding
                for (int fx = -1; fx <= 1; ++fx) {
                    if (ce && fx == (dx ? 1 : -1)) continue;
                    acc += S[(fy + 1) * 3 + (fx + 1)];
                }
            }
            L.shift16[tid * C + co] = (float)((double)L.scale[co] * acc);
        }
        return;
    }
    r -= L.nshift;
    {                                                                    // skip half of the conv rows: 16-byte pieces
        const int ppr = C / 4, idx = r * 256 + tid;
        if (idx < 9 * C * ppr) {
            const int row = idx / ppr, pc = idx - row * ppr;
            *(f32x4*)(L.wskip + (size_t)row * C + pc * 4) = *(const f32x4*)(L.w3 + (size_t)row * CIN + C + pc * 4);
        }
    }
}

size_t smirk_updeep_weff_bytes(int c) { return (size_t)4 * c * 8 * c * 4; }      // 4 classes x c rows x (4 taps x 2c) split-fp16 pairs
size_t smirk_updeep_shift_bytes(int c) { return (size_t)16 * c * 4; }
size_t smirk_updeep_wskip_bytes(int c) { return (size_t)9 * c * c * 4; }

static ConvArgs updeep_args(int B, int H, int W, int c0, int cout, int taps) {
    ConvArgs a = {};
    SmirkConvDesc& d = a.d;
    d.B = B; d.H = H; d.W = W; d.C0 = c0; d.C1 = 0; d.Cout = cout; d.KH = d.KW = 3; d.stride = 1; d.pad_t = d.pad_l = 1; d.Ho = H; d.Wo = W;
    d.pad_mode = SMIRK_PAD_ZERO; d.act = SMIRK_ACT_NONE; d.out_mode = SMIRK_OUT_NHWC;
    a.Cin = c0; a.K = taps * c0; a.N = cout; a.M = B * H * W;
    return a;
}

// A level with c output channels on a fine image of H x W takes the composed pair when conv_halo accepts BOTH launches with their own M: the coarse one
// (B H/2 W/2 rows, 2c channels; its four Weff[class] are < 2 GiB each whenever the level's 9 * 2c rows are) and the skip half (B H W rows, c channels).
// $SMIRK_IGEMM_HALO=0 therefore restores the two-launch level.
bool smirk_updeep_eligible(int B, int H, int W, int c) {
    if (B <= 0 || H < 4 || W < 4 || (H & 1) || (W & 1) || (long long)B * H * W > (1ll << 30)) return false;
    if (!conv_fits32((long long)B * H * W * c)) return false;          // partial' / the output
    return smirk_conv_halo_eligible(updeep_args(B, H / 2, W / 2, 2 * c, c, 4)) && smirk_conv_halo_eligible(updeep_args(B, H, W, c, c, 9));
}

int smirk_updeep_compose(const SmirkUpdeepLevel* lv, int nlv, hipStream_t st) {
    if (nlv < 1 || nlv > 2) return SMIRK_ERR_BAD_ARG;
    UpdeepComposeArgs args = {};
    int blk = 0;
    double mac = 0.0, bytes = 0.0;
    for (int i = 0; i < 2; ++i) {
        UpdeepLevelArgs& L = args.lv[i];
        L.blk0 = blk;
        if (i >= nlv) continue;                                           // (an absent level owns no block: blk0 = the grid size)
        const SmirkUpdeepLevel& s = lv[i];
        const int c = s.c;
        if (c < 64 || c % 64 || !s.up || !s.conv || !s.up->w || !s.up->shift || s.up->scale || !s.conv->w || !s.conv->scale || !s.weff || !s.shift16 || !s.wskip)
            return SMIRK_ERR_BAD_ARG;
        L.wup = (const float*)s.up->w; L.bup = s.up->shift; L.w3 = (const float*)s.conv->w; L.scale = s.conv->scale;
        L.weff = (float*)s.weff; L.shift16 = (float*)s.shift16; L.wskip = (float*)s.wskip;
        L.c = c; L.ngemm = 16 * (c / 64) * (2 * c / 64); L.nshift = c;
        blk += L.ngemm + L.nshift + (9 * c * (c / 4) + 255) / 256;
        mac += 4.0 * 9 * c * c * 2 * c;
        bytes += 4.0 * (4.0 * c * 2 * c + 18.0 * c * c + 32.0 * c * c + 9.0 * c * c);
    }
    if (g_smirk_prof_on) smirk_prof_next("updeep_compose_kernel", 2.0 * mac, bytes);
    SMIRK_LAUNCH(updeep_compose_kernel, dim3(blk), dim3(256), 0, st, args);
    return smirk_launch_status();
}

// launch 1: partial'[B][H][W][c] from the coarse tensor d[B][H/2][W/2][2c]
int smirk_updeep_coarse_launch(const SmirkUpdeepLevel* lv, const void* d, void* partial, int B, int H, int W, bool x1, hipStream_t st) {
    if (!lv || !d || !partial || !smirk_updeep_eligible(B, H, W, lv->c)) return SMIRK_ERR_UNSUPPORTED;
    ConvArgs a = updeep_args(B, H / 2, W / 2, 2 * lv->c, lv->c, 4);
    a.in0 = (const float*)d; a.w = (const float*)lv->weff; a.scale = lv->conv->scale; a.shift = (const float*)lv->shift16; a.out = (float*)partial;
    constexpr size_t lds = 4 * HS_BN * 128 + 2 * (5 * 8 * 1024 + 128);        // four ring stages + two 5-piece halo buffers (256 + W + 1 <= 320 rows for W <= 63)
    if (const int rc = smirk_raise_dynamic_lds(x1 ? (const void*)conv_halo_up_x1_kernel<5> : (const void*)conv_halo_up_kernel<5>, 160 * 1024)) return rc;
    const int ntm = (a.M + HS_BM - 1) / HS_BM, ntn = a.N / HS_BN;
    if (g_smirk_prof_on) {
        const double px = (double)a.M;
        smirk_prof_next(x1 ? "conv_halo_up_x1_kernel<5>[256x128,8w,halo,composed upconv,f16x1]" : "conv_halo_up_kernel<5>[256x128,8w,halo,composed upconv]",
                        2.0 * (4.0 * a.M) * a.N * a.K, 4.0 * (px * a.Cin + 4.0 * px * a.N + 4.0 * a.N * a.K));
    }
    if (x1) SMIRK_LAUNCH((conv_halo_up_x1_kernel<5>), dim3(4 * ntm * ntn), dim3(512), lds, st, a);
    else SMIRK_LAUNCH((conv_halo_up_kernel<5>), dim3(4 * ntm * ntn), dim3(512), lds, st, a);
    return smirk_launch_status();
}
