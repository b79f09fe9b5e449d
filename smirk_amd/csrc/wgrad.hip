// Weight gradient of the 3x3 / 1x1 / transposed convolutions on MI355X: the one GEMM of the training step's backward pass that is not a forward kernel run
// on other operands.  Its reduction index is K = B*H*W pixels, so both operands (split16 NHWC activations and their gradients, conv_common.h) are "k-major"
// in memory.  That is exactly the operand layout of v_mfma_f32_32x32x2_f32 (one fp32 per lane: lanes 0-31 / 32-63 hold k, k+1) — the exact-fp32 kernels need no
// transposition but run at the fp32 matrix rate (157 TFLOP/s); the default kernels consume the split16 operands as stored on the 16x faster fp16 pipe and let
// ds_read_b64_tr_b16 produce the k-contiguous fragments that pipe wants (wgrad_f16_kernel, wgrad3x3_halo_f16_kernel).
// Two kernel families (tiled: any layer; halo: the few-channel 3x3 layers, all nine taps from one staged pixel halo), each in exact fp32, split-fp16 x3 and
// one-MFMA f16x1 arithmetic, split-K partials summed in a fixed order (bit-reproducible).  Which instantiation serves a layer, with what grid and how much
// workspace, is decided in ONE place: wgrad_plan, below the kernels.
#include <stdio.h>

#include <algorithm>
#include <atomic>

#include "conv_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// Weight gradient:  dW[co][n] = sum over pixels p of dZ[p][co] * X[p shifted by tap(n)][ci(n)],  n = tap * Cin + ci     (exact fp32, v_mfma_f32_32x32x2_f32)
//   GEMM with M = Cout, N = KH*KH*Cin (the taps are flattened INTO N, so a 32-channel layer still fills a 128-wide tile with four taps) and
//   K = B*H*W pixels split over gridDim.z.  Workgroup tile TM x 128 with TM in {32, 64, 128} chosen from Cout; 4 waves as 2 x 2 (TM = 128: 64 x 64 per
//   wave) or 1 x 4 (TM <= 64: TM x 32 per wave).  16 pixels per chunk, decoded from split16 into fp32 [k][TM + 4] / [k][128 + 4] in a DOUBLE-BUFFERED LDS
//   image: the next chunk's global loads are issued before the current chunk's MFMAs and land in registers underneath them; one barrier per chunk.
// part[split][Cout][N] fp32 partials are summed in split order by wgrad_reduce_kernel  (bit-reproducible).
// ---------------------------------------------------------------------------------------------------------------------------------
#define WG_KC 16
#define WG_LD 132
#define WG_MAX_SPLIT 512
struct WgradArgs {
    const float *dz, *x;         // split16 [B][H][W][Cout], [B][H][W][Cin]
    float* part;
    int B, H, W, Cout, Cin, KH, pad, reflect;
    int chunks_per_split;        // 16-pixel chunks per K split
};

template <int TM>
__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs a) {
    constexpr int WAVES_M = TM == 128 ? 2 : 1, WAVES_N = 4 / WAVES_M;
    constexpr int BM = TM / 32 / WAVES_M, BN = 4 / WAVES_N;                 // 32 x 32 MFMA blocks per wave
    constexpr int LDA = TM + 4;
    __shared__ __attribute__((aligned(16))) float As[2][WG_KC * LDA], Bs[2][WG_KC * WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int N = a.KH * a.KH * a.Cin;
    const int co0 = blockIdx.x * TM, n0 = blockIdx.y * 128, split = blockIdx.z;
    const long long npix = (long long)a.B * a.H * a.W;
    f32x16 acc[BM][BN];
#pragma unroll
    for (int i = 0; i < BM; ++i)
#pragma unroll
        for (int j = 0; j < BN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // staging: thread -> (pixel k = tid / 16, 8-wide group = tid % 16) of the 16 x 128 B tile and (for tid % 16 < TM / 8) of the 16 x TM A tile
    const int sk = tid >> 4, sg = tid & 15;
    const int Gout = a.Cout / 8, Gin = a.Cin / 8;
    const int gco = co0 / 8 + sg;
    const bool a_on = sg < TM / 8 && gco < Gout;
    const int nb = n0 + sg * 8;                                               // this thread's 8 B columns: one tap, 8 consecutive input channels
    const bool b_on = nb < N;
    const int tap = b_on ? nb / a.Cin : 0, gci = b_on ? (nb % a.Cin) / 8 : 0;
    const int ky = tap / a.KH, kx = tap % a.KH;
    float va[8], vb[8];
    auto fetch = [&](int c) {
        const long long p = ((long long)split * a.chunks_per_split + c) * WG_KC + sk;
#pragma unroll
        for (int q = 0; q < 8; ++q) { va[q] = 0.f; vb[q] = 0.f; }
        if (p < npix) {
            if (a_on) load_group(a.dz + ((size_t)p * Gout + gco) * 8, va);
            if (b_on) {
                const int x0 = (int)(p % a.W), y0 = (int)((p / a.W) % a.H);
                const long long b = p / ((long long)a.W * a.H);
                int iy = y0 + ky - a.pad, ix = x0 + kx - a.pad;
                bool ok = true;
                if (a.reflect) { iy = reflect_idx(iy, a.H); ix = reflect_idx(ix, a.W); }
                else ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                if (ok) load_group(a.x + ((((size_t)b * a.H + iy) * a.W + ix) * Gin + gci) * 8, vb);
            }
        }
    };
    fetch(0);
    for (int c = 0; c < a.chunks_per_split; ++c) {
        float* as = As[c & 1];
        float* bs = Bs[c & 1];
        if (sg < TM / 8) { *(f32x4*)(as + sk * LDA + sg * 8) = *(f32x4*)va; *(f32x4*)(as + sk * LDA + sg * 8 + 4) = *(f32x4*)(va + 4); }
        *(f32x4*)(bs + sk * WG_LD + sg * 8) = *(f32x4*)vb; *(f32x4*)(bs + sk * WG_LD + sg * 8 + 4) = *(f32x4*)(vb + 4);
        __syncthreads();                       // chunk c visible; the buffer written next iteration was last read two iterations ago, behind this barrier
        if (c + 1 < a.chunks_per_split) fetch(c + 1);
        const int kk = lane >> 5, mm = lane & 31;
#pragma unroll
        for (int k2 = 0; k2 < WG_KC; k2 += 2) {
            float fa[BM], fb[BN];
#pragma unroll
            for (int i = 0; i < BM; ++i) fa[i] = as[(k2 + kk) * LDA + (wm * BM + i) * 32 + mm];
#pragma unroll
            for (int j = 0; j < BN; ++j) fb[j] = bs[(k2 + kk) * WG_LD + (wn * BN + j) * 32 + mm];
#pragma unroll
            for (int i = 0; i < BM; ++i)
#pragma unroll
                for (int j = 0; j < BN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    }
    float* out = a.part + (size_t)split * a.Cout * N;
#pragma unroll
    for (int i = 0; i < BM; ++i)
#pragma unroll
        for (int j = 0; j < BN; ++j) {
            const int n = n0 + (wn * BN + j) * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (wm * BM + i) * 32 + mfma32_row(r, lane);
                if (co < a.Cout && n < N) out[(size_t)co * N + n] = acc[i][j][r];
            }
        }
}
// ---------------------------------------------------------------------------------------------------------------------------------
// The same GEMM on the fp16 matrix pipe: split-fp16 x3 (acc0 += dz_hi.x_hi ; acc1 += dz_hi.x_lo + dz_lo.x_hi ; dW = acc0 + acc1 * 2^-11 — fp16 x fp16 products
// are exact in fp32, only the 2^-22 lo.lo term is dropped: the arithmetic of the forward convolutions), 3 x v_mfma_f32_32x32x16_f16 per 32 x 32 x 16 block
// = 96 matrix-pipe cycles where the exact-fp32 instruction needs 512.  Both operands are ALREADY split16 in HBM, so nothing is converted; what the fp16
// instruction needs and memory does not offer is k (= pixel) contiguity per lane — 8 consecutive pixels of one channel — while memory is channel-contiguous
// per pixel.  gfx950's LDS transpose read does that re-arrangement for free: `ds_read_b64_tr_b16` lets the 16 lanes of a group fetch a [4 pixels][16 channels]
// block (lane 4r+q supplies the 8-byte address of pixel r, channels 4q..4q+3) and returns to lane c the four pixels of channel c.  Two such reads make one
// MFMA operand (pixels 8*(lane>>5) + 0..7 of channel lane&31); the pixel <-> (lane half, element) assignment is the same for both operands, which is all a
// reduction index has to satisfy.
// LDS image of a 16-pixel chunk of an operand with NG 8-channel groups, in 16-byte slots (one slot = the hi OR the lo halves of one group of one pixel):
//     slot(h, g, k) = ((h * NG/4 + g/4) * 4 + k/4) * 16  +  ((k%4 + g/4) % 4) * 4  +  g%4
// i.e. every aligned 256-byte bank row holds 4 pixels x 4 groups of one half.  A half-wave's transpose read (4 pixels x 32 channels = 4 groups) covers exactly
// one bank row -> conflict-free; the staging writes (`ds_write_b128`, 8 lanes = 8 consecutive groups of one pixel per LDS cycle) land on 8 distinct 16-byte
// bank slots because the row rotation by g/4 flips the slot's bit 2 between groups 0-3 and 4-7.
// Staging is register-based (global 16-byte loads of the raw hi / lo pieces, issued a chunk ahead, under the MFMAs), double-buffered, one barrier per SUB chunks.
// ---------------------------------------------------------------------------------------------------------------------------------
typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) fp16x4_t* lds_fp16x4_ptr;

__device__ __forceinline__ int wgf_slot(int ngq, int kq_per, int h, int g, int k) {      // 16-byte slot of (half h, group g, pixel k); kq_per = pixel quads per image
    return ((h * ngq + (g >> 2)) * kq_per + (k >> 2)) * 16 + ((((k & 3) + (g >> 2)) & 3) << 2) + (g & 3);
}
__device__ __forceinline__ half8 wgf_frag(const char* base, int off) {                    // two transpose reads -> one 32x32x16 MFMA operand (8 pixels of this lane's channel)
    union { fp16x4_t v[2]; half8 h; } u;
    u.v[0] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(base + off));
    u.v[1] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(base + off + 256));
    return u.h;
}

template <int TM, int SUB, bool X1 = false>   // X1: hi x hi only, one MFMA per block (BASELINE config 5's 16-bit class); its own instantiations
__global__ __launch_bounds__(256, 2) void wgrad_f16_kernel(WgradArgs a, int trmap) {
    constexpr int WAVES_M = TM == 128 ? 2 : 1, WAVES_N = 4 / WAVES_M;
    constexpr int BM = TM / 32 / WAVES_M, BN = 4 / WAVES_N;                 // 32 x 32 MFMA blocks per wave: 2x2 (TM 128), 2x1 (TM 64), 1x1 (TM 32)
    constexpr int GA = TM / 8, AQ = GA / 4, BQ = 4;                         // 8-channel groups / group quads of the A (dz) and B (x, 128 columns) tiles
    constexpr int A_BYTES = GA * 2 * 16 * 16, B_BYTES = 16 * 2 * 16 * 16;   // one 16-pixel chunk image
    __shared__ __attribute__((aligned(256))) char As[2][SUB][A_BYTES];
    __shared__ __attribute__((aligned(256))) char Bs[2][SUB][B_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int N = a.KH * a.KH * a.Cin;
    const int co0 = blockIdx.x * TM, n0 = blockIdx.y * 128, split = blockIdx.z;
    const long long npix = (long long)a.B * a.H * a.W;
    f32x16 acc0[BM][BN], acc1[BM][BN];
#pragma unroll
    for (int i = 0; i < BM; ++i)
#pragma unroll
        for (int j = 0; j < BN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[i][j][r] = 0.f; acc1[i][j][r] = 0.f; }
    // staging: thread -> (pixel sk, 8-wide group sg) of every 16-pixel chunk: the group's raw 32 bytes (hi piece, lo piece)
    const int sk = tid >> 4, sg = tid & 15;
    const int Gout = a.Cout / 8, Gin = a.Cin / 8;
    const int gco = co0 / 8 + sg;
    const bool a_on = sg < GA && gco < Gout;
    const int nb = n0 + sg * 8;
    const bool b_on = nb < N;
    const int tap = b_on ? nb / a.Cin : 0, gci = b_on ? (nb % a.Cin) / 8 : 0;
    const int ky = tap / a.KH, kx = tap % a.KH;
    const int wa_hi = wgf_slot(AQ, 4, 0, sg, sk) * 16, wa_lo = wgf_slot(AQ, 4, 1, sg, sk) * 16;
    const int wb_hi = wgf_slot(BQ, 4, 0, sg, sk) * 16, wb_lo = wgf_slot(BQ, 4, 1, sg, sk) * 16;
    const int iters = (a.chunks_per_split + SUB - 1) / SUB;
    // the pixel this thread stages in the NEXT chunk, kept decomposed (image, row, column) and advanced by 16 per chunk: no divisions in the loop
    const long long p0 = (long long)split * a.chunks_per_split * WG_KC + sk;
    int fb = (int)(p0 / ((long long)a.W * a.H));
    int fy, fx;
    { const int rem = (int)(p0 - (long long)fb * a.W * a.H); fy = rem / a.W; fx = rem - fy * a.W; }
    int fc = 0;
    // Operand fetch through buffer resources with running 32-bit offsets (both tensors are < 2 GiB here, the dispatcher checks): NHWC pixels are linear in
    // memory, so chunk c's dz piece sits 16 pixels after chunk c-1's, and (zero padding) the x pixel under this thread's tap is the linear pixel
    // p + (ky - pad) * W + (kx - pad) whenever it lies inside the image — one add per chunk instead of a 64-bit multiply chain; a lane with nothing to fetch
    // (past the split / the tensor, tap outside the image, column beyond N) carries an out-of-range offset and the load returns zeros: no branches, no zero
    // fill.  (PMC of the pointer-based first version: 8.8 VALU + 3.2 SALU instructions per MFMA, the VALU pipe as busy as the matrix pipe.)  Reflection
    // padding (three 14x14 layers) computes its source pixel explicitly.
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)a.dz, (short)0, (int)(npix * a.Cout * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, (int)(npix * a.Cin * 4), 0x00020000);
    const unsigned OOB = 0x80000000u;
    unsigned oa = (unsigned)(((unsigned long long)p0 * Gout + gco) * 32ull);
    unsigned ob = (unsigned)(((long long)p0 + (long long)(ky - a.pad) * a.W + (kx - a.pad)) * Gin + gci) * 32u;
    const unsigned a_step = (unsigned)(WG_KC * Gout * 32), b_step = (unsigned)(WG_KC * Gin * 32);
    u32x4_t ra[SUB][2], rb[SUB][2];
    auto fetch = [&]() {
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            const bool live = fc < a.chunks_per_split && fb < a.B;
            const unsigned va = (live && a_on) ? oa : OOB;
            ra[s][0] = __builtin_amdgcn_raw_buffer_load_b128(rsa, va, 0, 0);
            ra[s][1] = __builtin_amdgcn_raw_buffer_load_b128(rsa, va, 16, 0);
            const int iy = fy + ky - a.pad, ix = fx + kx - a.pad;
            unsigned vb;
            if (a.reflect) vb = (live && b_on) ? (unsigned)((((fb * a.H + reflect_idx(iy, a.H)) * a.W + reflect_idx(ix, a.W)) * Gin + gci) * 32) : OOB;
            else vb = (live && b_on && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) ? ob : OOB;
            rb[s][0] = __builtin_amdgcn_raw_buffer_load_b128(rsb, vb, 0, 0);
            rb[s][1] = __builtin_amdgcn_raw_buffer_load_b128(rsb, vb, 16, 0);
            ++fc;
            oa += a_step; ob += b_step;
            fx += WG_KC;
            while (fx >= a.W) { fx -= a.W; if (++fy == a.H) { fy = 0; ++fb; } }
        }
    };
    // transpose-read lane geometry: 16-lane group -> [4 pixels][16 channels]; lane i of the group supplies pixel r, channel quarter q
    const int li = lane & 15, r4 = trmap ? (li & 3) : (li >> 2), q4 = trmap ? (li >> 2) : (li & 3);
    const int gl = ((lane >> 4) & 1) * 2 + (q4 >> 1), khalf = lane >> 5;    // group within the block's quad; pixels 8*khalf.. of the chunk
    int offA[BM], offB[BN];                                                  // byte offset of (half hi, first read) inside a chunk image
#pragma unroll
    for (int i = 0; i < BM; ++i) {
        const int gq = wm * BM + i;
        offA[i] = (((gq * 4 + khalf * 2) * 16) + (((r4 + gq) & 3) << 2) + gl) * 16 + (q4 & 1) * 8;
    }
#pragma unroll
    for (int j = 0; j < BN; ++j) {
        const int gq = wn * BN + j;
        offB[j] = (((gq * 4 + khalf * 2) * 16) + (((r4 + gq) & 3) << 2) + gl) * 16 + (q4 & 1) * 8;
    }
    // (Round 6 kept a SECOND iteration's fetches in flight in a second register set — 207 -> 236 VGPRs, 64 KB outstanding per workgroup instead of 32 — on the theory that
    // the kernel is bound by bytes in flight: 4.903 -> 4.907 ms per training step, i.e. nothing.  It is not latency-bound; what limits it stays open.  Removed again.)
    fetch();
    for (int it = 0; it < iters; ++it) {
        const int buf = it & 1;
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            if (sg < GA) { *(u32x4_t*)(As[buf][s] + wa_hi) = ra[s][0]; *(u32x4_t*)(As[buf][s] + wa_lo) = ra[s][1]; }
            *(u32x4_t*)(Bs[buf][s] + wb_hi) = rb[s][0]; *(u32x4_t*)(Bs[buf][s] + wb_lo) = rb[s][1];
        }
        __syncthreads();                       // this stage visible; the stage written next iteration was last read two iterations ago, behind this barrier
        if (it + 1 < iters) fetch();
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            half8 ah[BM], al[BM], bh[BN], bl[BN];
#pragma unroll
            for (int i = 0; i < BM; ++i) { ah[i] = wgf_frag(As[buf][s], offA[i]); if constexpr (!X1) al[i] = wgf_frag(As[buf][s], offA[i] + AQ * 1024); }
#pragma unroll
            for (int j = 0; j < BN; ++j) { bh[j] = wgf_frag(Bs[buf][s], offB[j]); if constexpr (!X1) bl[j] = wgf_frag(Bs[buf][s], offB[j] + BQ * 1024); }
#pragma unroll
            for (int i = 0; i < BM; ++i)
#pragma unroll
                for (int j = 0; j < BN; ++j) {
                    acc0[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc0[i][j], 0, 0, 0);
                    if constexpr (!X1) {
                        acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc1[i][j], 0, 0, 0);
                        acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc1[i][j], 0, 0, 0);
                    }
                }
        }
    }
    float* out = a.part + (size_t)split * a.Cout * N;
#pragma unroll
    for (int i = 0; i < BM; ++i)
#pragma unroll
        for (int j = 0; j < BN; ++j) {
            const int n = n0 + (wn * BN + j) * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (wm * BM + i) * 32 + mfma32_row(r, lane);
                if (co < a.Cout && n < N) out[(size_t)co * N + n] = acc0[i][j][r] + acc1[i][j][r] * (1.0f / 2048.0f);
            }
        }
}

// Weight gradient of a 3x3 zero-padded convolution with FEW channels (the U-Net's 224^2 / 112^2 layers: Cout, Cin in {32, 64}).  There the generic kernel is
// bound by the L2 -> CU path, not by MFMA: a 32 x 128 tile re-loads 10 KB of operands for 131 kflop (13 flop/B, 36 TFLOP/s measured).  Here one workgroup owns ALL
// nine taps of its pixel chunk: the chunk is 16 consecutive pixels of one image row, x is staged ONCE as a [3 rows][18 pixels][Cin] halo and every tap reads its
// B fragment from that halo at a pixel offset — 9 KB per chunk for 295 kflop at Cin = Cout = 32 (33 flop/B).  The (Cout/32) x 9 x (Cin/32) MFMA blocks are dealt
// round-robin to the 4 waves; LDS double-buffered, next chunk's loads in flight under the MFMAs, K split over chunks like the generic kernel (same partial layout).
template <int TM, int CIN>
__global__ __launch_bounds__(256) void wgrad3x3_halo_kernel(WgradArgs a) {
    constexpr int LDA = TM + 4, LDB = CIN + 4, HPX = 3 * 18;
    constexpr int NB = (TM / 32) * 9 * (CIN / 32), MAXB = (NB + 3) / 4;
    constexpr int GA = TM / 8, GB = CIN / 8;                                   // 8-channel groups per pixel
    constexpr int NLB = (HPX * GB + 255) / 256;                               // B groups per thread and chunk
    __shared__ __attribute__((aligned(16))) float As[2][WG_KC * LDA], Bs[2][HPX * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.x;
    const int cpr = a.W / 16;                                                  // chunks per image row
    const long long nchunk = (long long)a.B * a.H * cpr;
    f32x16 acc[MAXB];
#pragma unroll
    for (int i = 0; i < MAXB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float va[8], vb[NLB][8];
    auto fetch = [&](int c) {
        const long long ch = (long long)split * a.chunks_per_split + c;
#pragma unroll
        for (int q = 0; q < 8; ++q) va[q] = 0.f;
#pragma unroll
        for (int u = 0; u < NLB; ++u)
#pragma unroll
            for (int q = 0; q < 8; ++q) vb[u][q] = 0.f;
        if (ch >= nchunk) return;
        const int xc = (int)(ch % cpr), y = (int)((ch / cpr) % a.H);
        const long long b = ch / ((long long)cpr * a.H);
        const int x0 = xc * 16;
        if (tid < WG_KC * GA) {                                                // dz: 16 pixels x GA groups
            const int k = tid / GA, g = tid % GA;
            load_group(a.dz + ((((size_t)b * a.H + y) * a.W + x0 + k) * GA + g) * 8, va);
        }
#pragma unroll
        for (int u = 0; u < NLB; ++u) {
            const int e = tid + u * 256;
            if (e < HPX * GB) {
                const int hp = e / GB, g = e % GB, hy = hp / 18, hx = hp % 18;
                const int iy = y - 1 + hy, ix = x0 - 1 + hx;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) load_group(a.x + ((((size_t)b * a.H + iy) * a.W + ix) * GB + g) * 8, vb[u]);
            }
        }
    };
    // this wave's MFMA blocks: blk = wave + 4 i  ->  (m block, tap, n block)
    int boffA[MAXB], boffB[MAXB];
#pragma unroll
    for (int i = 0; i < MAXB; ++i) {
        const int blk = wave + 4 * i, mb = blk / (9 * (CIN / 32)), rem = blk % (9 * (CIN / 32)), tap = rem / (CIN / 32), nb = rem % (CIN / 32);
        boffA[i] = mb * 32;
        boffB[i] = ((tap / 3) * 18 + (tap % 3)) * LDB + nb * 32;               // halo pixel offset of the tap: row ky, column kx (pixel k sits at column k + 1 - 1 + kx)
    }
    fetch(0);
    for (int c = 0; c < a.chunks_per_split; ++c) {
        float* as = As[c & 1];
        float* bs = Bs[c & 1];
        if (tid < WG_KC * GA) {
            const int k = tid / GA, g = tid % GA;
            *(f32x4*)(as + k * LDA + g * 8) = *(f32x4*)va; *(f32x4*)(as + k * LDA + g * 8 + 4) = *(f32x4*)(va + 4);
        }
#pragma unroll
        for (int u = 0; u < NLB; ++u) {
            const int e = tid + u * 256;
            if (e < HPX * GB) {
                const int hp = e / GB, g = e % GB;
                *(f32x4*)(bs + hp * LDB + g * 8) = *(f32x4*)vb[u]; *(f32x4*)(bs + hp * LDB + g * 8 + 4) = *(f32x4*)(vb[u] + 4);
            }
        }
        __syncthreads();
        if (c + 1 < a.chunks_per_split) fetch(c + 1);
        const int kk = lane >> 5, mm = lane & 31;
#pragma unroll
        for (int k2 = 0; k2 < WG_KC; k2 += 2) {
#pragma unroll
            for (int i = 0; i < MAXB; ++i) {
                if (wave + 4 * i < NB) {
                    const float fa = as[(k2 + kk) * LDA + boffA[i] + mm];
                    const float fb = bs[(k2 + kk) * LDB + boffB[i] + mm];      // pixel k of the chunk under tap (ky, kx) = halo (ky, k + kx)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[i], 0, 0, 0);
                }
            }
        }
    }
    const int N = 9 * CIN;
    float* out = a.part + (size_t)split * a.Cout * N;
#pragma unroll
    for (int i = 0; i < MAXB; ++i) {
        const int blk = wave + 4 * i;
        if (blk < NB) {
            const int mb = blk / (9 * (CIN / 32)), rem = blk % (9 * (CIN / 32)), tap = rem / (CIN / 32), nb = rem % (CIN / 32);
            const int n = tap * CIN + nb * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = mb * 32 + mfma32_row(r, lane);
                out[(size_t)co * N + n] = acc[i][r];
            }
        }
    }
}

// The all-taps halo kernel on the fp16 matrix pipe (split-fp16 x3, LDS transpose reads; see wgrad_f16_kernel for the arithmetic and the slot layout).
// Chunk = 16 consecutive pixels of one image row.  A image: dz [16 pixels][TM channels]; B image: the x halo [3 rows x 18 pixels -> 54 halo pixels, padded to 14
// pixel quads][CIN channels].  The B fragment of tap (ky, kx) for chunk pixel k is halo pixel ky*18 + kx + k: a per-lane constant added to the pixel index, so
// the shifted fragments of all nine taps are read from the ONE staged halo (adding 4 to a pixel index moves exactly one pixel quad, hence the second transpose
// read of an operand is again +256 bytes).  The (TM/32) x 9 x (CIN/32) MFMA blocks are dealt round-robin to NW waves; a wave's A fragments are read once per chunk.
template <int TM, int CIN, int NW, int SUB, bool BUF, bool X1 = false>
__global__ __launch_bounds__(NW * 64) void wgrad3x3_halo_f16_kernel(WgradArgs a, int trmap) {
    constexpr int NT = NW * 64, HPX = 54, HQ = 14;
    constexpr int MB = TM / 32, NBQ = CIN / 32;                               // 32-channel quads of A and B
    constexpr int NB = MB * 9 * NBQ, MAXB = (NB + NW - 1) / NW;
    constexpr int GA = TM / 8, GB = CIN / 8;
    constexpr int A_BYTES = GA * 2 * 16 * 16, B_BYTES = GB * 2 * HQ * 4 * 16;
    constexpr int NLA = (16 * GA + NT - 1) / NT, NLB = (HPX * GB + NT - 1) / NT;
    __shared__ __attribute__((aligned(256))) char As[2][SUB][A_BYTES];
    __shared__ __attribute__((aligned(256))) char Bs[2][SUB][B_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.x;
    const int cpr = a.W / 16;
    f32x16 acc0[MAXB], acc1[MAXB];
#pragma unroll
    for (int i = 0; i < MAXB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[i][r] = 0.f; acc1[i][r] = 0.f; }
    // chunk cursor (image, row, chunk of the row) of the NEXT chunk to fetch, advanced by one per chunk
    const long long ch0 = (long long)split * a.chunks_per_split;
    int fb = (int)(ch0 / ((long long)cpr * a.H));
    int fy, fxc;
    { const int rem = (int)(ch0 - (long long)fb * cpr * a.H); fy = rem / cpr; fxc = rem - fy * cpr; }
    int fc = 0;
    // Operand fetch through buffer resources with running 32-bit offsets (see wgrad_f16_kernel): W % 16 == 0, so consecutive chunks are consecutive runs of 16
    // pixels in memory — across row ends and image ends too — and a chunk's operands sit at (first pixel of the chunk) + a per-thread constant; halo pixels
    // outside the image and idle lanes carry an out-of-range offset (zeros).
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    const long long npix = (long long)a.B * a.H * a.W;
    const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)a.dz, (short)0, (int)(npix * TM * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, (int)(npix * CIN * 4), 0x00020000);
    const unsigned OOB = 0x80000000u;
    unsigned ca[NLA];                                   // per-thread constant part of the dz offset: (pixel k of the chunk, group g)
    int cbo[NLB], chy[NLB], chx[NLB];                   // x halo: offset relative to the chunk's first pixel, halo row / column
#pragma unroll
    for (int u = 0; u < NLA; ++u) {
        const int e = tid + u * NT;
        ca[u] = e < 16 * GA ? (unsigned)(e * 32) : OOB;                        // (k * GA + g) * 32 with e = k * GA + g
    }
#pragma unroll
    for (int u = 0; u < NLB; ++u) {
        const int e = tid + u * NT, hp = e / GB, g = e % GB;
        chy[u] = e < HPX * GB ? hp / 18 : -100000;                             // idle lane: a row no image has
        chx[u] = hp % 18;
        cbo[u] = (((chy[u] - 1) * a.W + chx[u] - 1) * GB + g) * 32;
    }
    unsigned pa = (unsigned)(ch0 * 16 * GA * 32), pb = (unsigned)(ch0 * 16 * GB * 32);     // byte offset of the next chunk's first pixel in dz / x
    u32x4_t ra[SUB][NLA][2], rb[SUB][NLB][2];
    auto fetch_buf = [&]() {
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            const bool live = fc < a.chunks_per_split && fb < a.B;
            const int x0 = fxc * 16;
            // waves whose 64 items all lie past the end of the list skip the instruction (wave-uniform test): with 6-12 waves and 64-432 items most waves
            // have nothing to fetch, and an all-out-of-range load still costs its issue slot in the memory pipeline
#pragma unroll
            for (int u = 0; u < NLA; ++u) {
                if (__builtin_amdgcn_readfirstlane(wave * 64 + u * NT) < 16 * GA) {
                    const unsigned va = (live && ca[u] != OOB) ? pa + ca[u] : OOB;
                    ra[s][u][0] = __builtin_amdgcn_raw_buffer_load_b128(rsa, va, 0, 0);
                    ra[s][u][1] = __builtin_amdgcn_raw_buffer_load_b128(rsa, va, 16, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < NLB; ++u) {
                if (__builtin_amdgcn_readfirstlane(wave * 64 + u * NT) < HPX * GB) {
                    const bool ok = live && (unsigned)(fy - 1 + chy[u]) < (unsigned)a.H && (unsigned)(x0 - 1 + chx[u]) < (unsigned)a.W;
                    const unsigned vb = ok ? pb + (unsigned)cbo[u] : OOB;
                    rb[s][u][0] = __builtin_amdgcn_raw_buffer_load_b128(rsb, vb, 0, 0);
                    rb[s][u][1] = __builtin_amdgcn_raw_buffer_load_b128(rsb, vb, 16, 0);
                }
            }
            ++fc;
            pa += 16 * GA * 32; pb += 16 * GB * 32;
            if (++fxc == cpr) { fxc = 0; if (++fy == a.H) { fy = 0; ++fb; } }
        }
    };
    // pointer-based variant (64-bit addresses, exec-masked loads): measured FASTER than the buffer form for the 6- and 12-wave instantiations (64x32: 120 vs 95-103
    // TFLOP/s, 32x64: 134 vs 102-119, 64x64: 204 vs 193-202) and slower for the 3-wave 32x32 one (121 vs 145-154), same box — BUF selects per instantiation
    auto fetch_ptr = [&]() {
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
#pragma unroll
            for (int u = 0; u < NLA; ++u) ra[s][u][0] = ra[s][u][1] = u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
            for (int u = 0; u < NLB; ++u) rb[s][u][0] = rb[s][u][1] = u32x4_t{0u, 0u, 0u, 0u};
            if (fc < a.chunks_per_split && fb < a.B) {
                const int x0 = fxc * 16;
#pragma unroll
                for (int u = 0; u < NLA; ++u) {
                    const int e = tid + u * NT;
                    if (e < 16 * GA) {
                        const int k = e / GA, g = e % GA;
                        const u32x4_t* q = (const u32x4_t*)(a.dz + ((((size_t)fb * a.H + fy) * a.W + x0 + k) * GA + g) * 8);
                        ra[s][u][0] = q[0]; ra[s][u][1] = q[1];
                    }
                }
#pragma unroll
                for (int u = 0; u < NLB; ++u) {
                    const int e = tid + u * NT;
                    if (e < HPX * GB) {
                        const int hp = e / GB, g = e % GB, hy = hp / 18, hx = hp % 18;
                        const int iy = fy - 1 + hy, ix = x0 - 1 + hx;
                        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                            const u32x4_t* q = (const u32x4_t*)(a.x + ((((size_t)fb * a.H + iy) * a.W + ix) * GB + g) * 8);
                            rb[s][u][0] = q[0]; rb[s][u][1] = q[1];
                        }
                    }
                }
            }
            ++fc;
            if (++fxc == cpr) { fxc = 0; if (++fy == a.H) { fy = 0; ++fb; } }
        }
    };
    auto fetch = [&]() { if constexpr (BUF) fetch_buf(); else fetch_ptr(); };
    // transpose-read lane geometry (see wgrad_f16_kernel)
    const int li = lane & 15, r4 = trmap ? (li & 3) : (li >> 2), q4 = trmap ? (li >> 2) : (li & 3);
    const int gl = ((lane >> 4) & 1) * 2 + (q4 >> 1), khalf = lane >> 5;
    int offA[MB], offB[MAXB];
#pragma unroll
    for (int m = 0; m < MB; ++m) offA[m] = (((m * 4 + khalf * 2) * 16) + (((r4 + m) & 3) << 2) + gl) * 16 + (q4 & 1) * 8;
#pragma unroll
    for (int i = 0; i < MAXB; ++i) {
        const int blk = wave + NW * i, rem = blk % (9 * NBQ), tap = rem / NBQ, nbq = rem % NBQ;
        const int hp0 = (tap / 3) * 18 + (tap % 3) + khalf * 8 + r4;            // halo pixel of chunk pixel 8*khalf + r4 under this tap
        offB[i] = (((nbq * HQ + (hp0 >> 2)) * 16) + ((((hp0 & 3) + nbq) & 3) << 2) + gl) * 16 + (q4 & 1) * 8;
    }
    const int iters = (a.chunks_per_split + SUB - 1) / SUB;
    fetch();
    for (int it = 0; it < iters; ++it) {
        const int buf = it & 1;
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
#pragma unroll
            for (int u = 0; u < NLA; ++u) {
                const int e = tid + u * NT;
                if (e < 16 * GA) {
                    const int k = e / GA, g = e % GA;
                    *(u32x4_t*)(As[buf][s] + wgf_slot(GA / 4, 4, 0, g, k) * 16) = ra[s][u][0];
                    *(u32x4_t*)(As[buf][s] + wgf_slot(GA / 4, 4, 1, g, k) * 16) = ra[s][u][1];
                }
            }
#pragma unroll
            for (int u = 0; u < NLB; ++u) {
                const int e = tid + u * NT;
                if (e < HPX * GB) {
                    const int hp = e / GB, g = e % GB;
                    *(u32x4_t*)(Bs[buf][s] + wgf_slot(GB / 4, HQ, 0, g, hp) * 16) = rb[s][u][0];
                    *(u32x4_t*)(Bs[buf][s] + wgf_slot(GB / 4, HQ, 1, g, hp) * 16) = rb[s][u][1];
                }
            }
        }
        __syncthreads();
        if (it + 1 < iters) fetch();
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            half8 ah[MB], al[MB];
#pragma unroll
            for (int m = 0; m < MB; ++m) { ah[m] = wgf_frag(As[buf][s], offA[m]); if constexpr (!X1) al[m] = wgf_frag(As[buf][s], offA[m] + (GA / 4) * 1024); }
#pragma unroll
            for (int i = 0; i < MAXB; ++i) {
                const int blk = wave + NW * i;
                if (blk < NB) {
                    const half8 bh = wgf_frag(Bs[buf][s], offB[i]);
                    half8 fah = ah[0];
                    if (MB == 2 && blk >= 9 * NBQ) fah = ah[MB - 1];
                    acc0[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah, bh, acc0[i], 0, 0, 0);
                    if constexpr (!X1) {
                        const half8 bl = wgf_frag(Bs[buf][s], offB[i] + (GB / 4) * HQ * 256);
                        half8 fal = al[0];
                        if (MB == 2 && blk >= 9 * NBQ) fal = al[MB - 1];
                        acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah, bl, acc1[i], 0, 0, 0);
                        acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fal, bh, acc1[i], 0, 0, 0);
                    }
                }
            }
        }
    }
    const int N = 9 * CIN;
    float* out = a.part + (size_t)split * a.Cout * N;
#pragma unroll
    for (int i = 0; i < MAXB; ++i) {
        const int blk = wave + NW * i;
        if (blk < NB) {
            const int mb = blk / (9 * NBQ), rem = blk % (9 * NBQ), tap = rem / NBQ, nbq = rem % NBQ;
            const int n = tap * CIN + nbq * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = mb * 32 + mfma32_row(r, lane);
                out[(size_t)co * N + n] = acc0[i][r] + acc1[i][r] * (1.0f / 2048.0f);
            }
        }
    }
}

// Sum of the split-K partials, written in the layout the CALLER keeps the gradient in (no permute-copy / torch.cat afterwards):
//   layout 0  packed  dw[co][(t, ci)]                                   (the forward operand layout; what the kernels above accumulate)
//   layout 1  nn.Conv2d parameter  dw[co][cin_off + ci][t]  of a [Cout][cin_total][KH][KH] tensor, ci < cin_real (padded input channels are dropped; the two
//             sources of a decoder convolution write the two channel ranges of ONE gradient tensor)
//   layout 2  nn.ConvTranspose2d(2, 2) parameter  dw[row][co][dydx]  of a [Cin_t][Cout_t][2][2] tensor, from the packed [row][(dydx, co)] (row = input channel)
struct WgradLayout { int mode, T, Cin, cin_total, cin_off, cin_real; };
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int nsplit, size_t n, float* __restrict__ dw, WgradLayout L) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};          // 8 independent chains keep 8 loads in flight; combined in a fixed order
        int k = 0;
        for (; k + 8 <= nsplit; k += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += part[(size_t)(k + j) * n + i];
        for (; k < nsplit; ++k) s[0] += part[(size_t)k * n + i];
        const float v = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
        if (L.mode == 0) {
            dw[i] = v;
        } else if (L.mode == 1) {
            const int N = L.T * L.Cin;
            const size_t co = i / (size_t)N;
            const int rem = (int)(i - co * N), t = rem / L.Cin, ci = rem - t * L.Cin;
            if (ci < L.cin_real) dw[((size_t)co * L.cin_total + L.cin_off + ci) * L.T + t] = v;
        } else {
            const int N = L.Cin;                                          // = 4 * Cout_t columns (dydx, co)
            const size_t row = i / (size_t)N;
            const int rem = (int)(i - row * N), ct = N / 4, dydx = rem / ct, co = rem - dydx * ct;
            dw[((size_t)row * ct + co) * 4 + dydx] = v;
        }
    }
}

}  // namespace

// ---- host side: which instantiation serves a layer ---------------------------------------------------------------------------------
// wgrad_plan is the ONE place that decides family, arithmetic, instantiation, split count, grid and workspace; the workspace query and the launch both read it.
enum { WG_REFUSED = -1, WG_EXACT = 0, WG_F16X3 = 1, WG_F16X1 = 2 };    // WG_REFUSED: one MFMA per product was asked for and no f16 kernel can serve the layer
// the halo family's shapes (TM = Cout), each with the waves, chunks per barrier and buffer-addressed staging of its f16 kernels
struct WgradHaloShape { int TM, CIN, NW, SUB; bool BUF; };
constexpr WgradHaloShape WG_HALO[4] = {{32, 32, 3, 2, true}, {64, 32, 6, 2, false}, {32, 64, 6, 1, false}, {64, 64, 12, 1, false}};
struct WgradPlan {
    int halo, arith, TM, SUB, trmap;      // index into WG_HALO or -1 = the tiled family; WG_*; tile height; f16 chunks per barrier; transpose-read lane geometry (mode "+16")
    int nsplit, chunks_per_split;
    dim3 grid;
    unsigned block;
    size_t ws_bytes;                      // part[nsplit][Cout][N] fp32
};
// K splits of a layer: a function of the SHAPE ONLY.  smirk_conv_wgrad_workspace_bytes sizes part[] from it and is told neither `reflect` nor the mode, so the
// count cannot depend on the family wgrad_plan chooses.  The first rule is sized for the halo kernels (one workgroup per split) and matches on their shapes alone:
// N = 9 * 32 or 9 * 64 columns, Cout 32 or 64.  A layer of that shape that the halo kernel refuses (W % 16 != 0, reflect padding, a 1x1 layer with Cin = 288 / 576)
// runs the TILED kernel with that count, 1536 or 1024, beyond WG_MAX_SPLIT.  Kept as it is: another count is another summation order.
static int wgrad_nsplit(long long npix, int Cout, int N, int TM) {
    const long long chunks = (npix + WG_KC - 1) / WG_KC;
    if ((Cout == 32 || Cout == 64) && (N == 288 || N == 576))                  // 64 x 576: 38 KB LDS -> 4 workgroups per CU, else 20-29 KB -> 6 per CU
        return (int)std::min<long long>((Cout == 64 && N == 576) ? 1024 : 1536, chunks);
    const long long tiles = (long long)((Cout + TM - 1) / TM) * ((N + 127) / 128);
    // 4 (TM = 128: 34 KB LDS each) / 6 workgroups per CU in ONE round (rounding up put 1152 on 1024 slots for the 512-channel layers: a second, 12 % full round)
    const long long want = std::min<long long>({(TM == 128 ? 1024 : 1536) / tiles, WG_MAX_SPLIT, chunks});
    return (int)(want < 1 ? 1 : want);
}
// mode: $SMIRK_WGRAD_F16 as wgrad_f16_mode() returns it; x1: one MFMA per product block.  nsplit and ws_bytes depend on neither, nor on reflect (the query passes 0).
static WgradPlan wgrad_plan(int B, int H, int W, int Cout, int Cin, int KH, int reflect, int mode, int x1) {
    WgradPlan p{};
    p.halo = -1;
    const long long npix = (long long)B * H * W, chunks = (npix + WG_KC - 1) / WG_KC;
    const int N = KH * KH * Cin;
    p.TM = Cout <= 32 ? 32 : Cout <= 64 ? 64 : 128;
    p.nsplit = wgrad_nsplit(npix, Cout, N, p.TM);
    p.chunks_per_split = p.nsplit > 0 ? (int)((chunks + p.nsplit - 1) / p.nsplit) : 0;
    p.ws_bytes = (size_t)p.nsplit * Cout * KH * KH * Cin * 4;
    // the f16 kernels fetch through buffer resources with 32-bit offsets: operands of 2 GiB and more take the exact-fp32 kernels (64-bit pointers)
    const int m = conv_fits32(npix * Cout) && conv_fits32(npix * Cin) ? mode : 0;
    p.arith = m ? (x1 ? WG_F16X1 : WG_F16X3) : (x1 ? WG_REFUSED : WG_EXACT);
    p.trmap = (m >> 4) & 1;
    p.SUB = x1 || (m & 15) != 1 ? 2 : 1;                                       // (tiled f16x1: always two chunks per barrier, the measured default)
    p.grid = dim3((Cout + p.TM - 1) / p.TM, (N + 127) / 128, p.nsplit);
    p.block = 256;
    for (int i = 0; i < 4; ++i)                                                // few-channel 3x3 layers: all nine taps from one staged halo
        if (KH == 3 && !reflect && W % 16 == 0 && Cout == WG_HALO[i].TM && Cin == WG_HALO[i].CIN) {       // (W % 16 == 0: a 16-pixel chunk never crosses a row)
            p.halo = i; p.SUB = WG_HALO[i].SUB;
            p.grid = dim3(p.nsplit); p.block = p.arith == WG_EXACT ? 256 : WG_HALO[i].NW * 64;
        }
    return p;
}
// the launch profiler's label: the instantiation as SMIRK_LAUNCH stringifies it where it is spelled out (profiles/, tools/ and bench.py's roofline key on these)
static const char* wgrad_label(const WgradPlan& p, char* nm, size_t n) {
    const char* x1 = p.arith == WG_F16X1 ? ",true" : "";
    const WgradHaloShape& s = WG_HALO[p.halo < 0 ? 0 : p.halo];
    if (p.halo < 0 && p.arith == WG_EXACT) snprintf(nm, n, "wgrad_kernel<%d>", p.TM);
    else if (p.halo < 0) snprintf(nm, n, "wgrad_f16_kernel<%d,%d%s>", p.TM, p.SUB, x1);
    else if (p.arith == WG_EXACT) snprintf(nm, n, "wgrad3x3_halo_kernel<%d,%d>", s.TM, s.CIN);
    else snprintf(nm, n, "wgrad3x3_halo_f16_kernel<%d,%d,%d,%d,%s%s>", s.TM, s.CIN, s.NW, s.SUB, s.BUF ? "true" : "false", x1);
    return nm;
}
template <int I>
static void launch_wgrad_halo(const WgradPlan& p, const WgradArgs& a, hipStream_t st) {
    constexpr WgradHaloShape S = WG_HALO[I];
    if (p.arith == WG_F16X1) SMIRK_LAUNCH((wgrad3x3_halo_f16_kernel<S.TM, S.CIN, S.NW, S.SUB, S.BUF, true>), p.grid, dim3(p.block), 0, st, a, p.trmap);
    else if (p.arith == WG_F16X3) SMIRK_LAUNCH((wgrad3x3_halo_f16_kernel<S.TM, S.CIN, S.NW, S.SUB, S.BUF>), p.grid, dim3(p.block), 0, st, a, p.trmap);
    else SMIRK_LAUNCH((wgrad3x3_halo_kernel<S.TM, S.CIN>), p.grid, dim3(p.block), 0, st, a);
}
template <int TM>
static void launch_wgrad_tile(const WgradPlan& p, const WgradArgs& a, hipStream_t st) {
    if (p.arith == WG_F16X1) SMIRK_LAUNCH((wgrad_f16_kernel<TM, 2, true>), p.grid, dim3(p.block), 0, st, a, p.trmap);
    else if (p.arith == WG_EXACT) SMIRK_LAUNCH(wgrad_kernel<TM>, p.grid, dim3(p.block), 0, st, a);
    else if (p.SUB == 1) SMIRK_LAUNCH((wgrad_f16_kernel<TM, 1>), p.grid, dim3(p.block), 0, st, a, p.trmap);
    else SMIRK_LAUNCH((wgrad_f16_kernel<TM, 2>), p.grid, dim3(p.block), 0, st, a, p.trmap);
}
// $SMIRK_WGRAD_F16 (switches.h): "0" = exact-fp32 MFMA kernel (wgrad_kernel), "1" / "2" = split-fp16 x3 kernel with 1 / 2 chunks per barrier (default 2);
// "+16" (17 / 18) selects the alternative lane geometry of the LDS transpose read (diagnostic)
static int g_wgrad_mode_override = -1;
static std::atomic<unsigned long long> g_wgrad_x1_fallbacks{0};
static int wgrad_f16_mode() { return g_wgrad_mode_override >= 0 ? g_wgrad_mode_override : smirk_switch(SMIRK_SW_WGRAD_F16); }
extern "C" int smirk_conv_wgrad_set_mode(int mode) { const int prev = wgrad_f16_mode(); g_wgrad_mode_override = mode; return prev; }
extern "C" size_t smirk_conv_wgrad_workspace_bytes(int B, int H, int W, int Cout, int Cin, int KH) { return wgrad_plan(B, H, W, Cout, Cin, KH, 0, 0, 0).ws_bytes; }
/* dW[Cout][(ky,kx,ci)] (fp32, the packed forward layout) = sum over pixels of dz[p][co] * x[p + tap][ci];  KH in {1, 3}, pad = (KH-1)/2 */
static int conv_wgrad_impl(const void* dz, const void* x, float* dw, int B, int H, int W, int Cout, int Cin, int KH, int reflect, void* ws, size_t ws_bytes,
                           void* stream, int x1, WgradLayout L = WgradLayout{0, 0, 0, 0, 0, 0}) {
    if (!dz || !x || !dw || !ws || B <= 0 || H <= 0 || W <= 0 || Cout % 8 || Cin % 8 || Cout <= 0 || Cin <= 0 || (KH != 1 && KH != 3)) return SMIRK_ERR_BAD_ARG;
    const WgradPlan p = wgrad_plan(B, H, W, Cout, Cin, KH, reflect, wgrad_f16_mode(), x1);
    if (ws_bytes < p.ws_bytes) return SMIRK_ERR_WORKSPACE;
    if (p.arith == WG_REFUSED) return SMIRK_ERR_UNSUPPORTED;                 // (before smirk_prof_next: a refused call leaves no pending profile label)
    const size_t n = (size_t)Cout * KH * KH * Cin;
    char nm[64];
    smirk_prof_next(g_smirk_prof_on ? wgrad_label(p, nm, sizeof(nm)) : nullptr, 2.0 * (double)B * H * W * n, 0.0);
    const WgradArgs a{(const float*)dz, (const float*)x, (float*)ws, B, H, W, Cout, Cin, KH, (KH - 1) / 2, reflect, p.chunks_per_split};
    hipStream_t st = (hipStream_t)stream;
    switch (p.halo >= 0 ? p.halo : -p.TM) {                                    // each halo shape and tile height once
        case 0: launch_wgrad_halo<0>(p, a, st); break;
        case 1: launch_wgrad_halo<1>(p, a, st); break;
        case 2: launch_wgrad_halo<2>(p, a, st); break;
        case 3: launch_wgrad_halo<3>(p, a, st); break;
        case -32: launch_wgrad_tile<32>(p, a, st); break;
        case -64: launch_wgrad_tile<64>(p, a, st); break;
        default: launch_wgrad_tile<128>(p, a, st); break;
    }
    SMIRK_LAUNCH(wgrad_reduce_kernel, dim3(blocks_for(n, 4096)), dim3(256), 0, st, (const float*)ws, p.nsplit, n, dw, L);
    return smirk_launch_status();
}
extern "C" int smirk_conv_wgrad_f32(const void* dz, const void* x, float* dw, int B, int H, int W, int Cout, int Cin, int KH, int reflect, void* ws, size_t ws_bytes,
                                    void* stream) {
    return conv_wgrad_impl(dz, x, dw, B, H, W, Cout, Cin, KH, reflect, ws, ws_bytes, stream, 0);
}
/* the same weight gradient with ONE MFMA per product block (hi halves of dz and x only, fp32 accumulation): BASELINE config 5's 16-bit class.  Needs the
 * f16 kernels (operands below 2 GiB, $SMIRK_WGRAD_F16 != 0): SMIRK_ERR_UNSUPPORTED otherwise — the caller falls back to smirk_conv_wgrad_f32 knowingly. */
extern "C" int smirk_conv_wgrad_f16x1(const void* dz, const void* x, float* dw, int B, int H, int W, int Cout, int Cin, int KH, int reflect, void* ws, size_t ws_bytes,
                                      void* stream) {
    return conv_wgrad_impl(dz, x, dw, B, H, W, Cout, Cin, KH, reflect, ws, ws_bytes, stream, 1);
}
/* The weight gradient summed straight into the PARAMETER's layout (WgradLayout above): layout 1 = nn.Conv2d weight [Cout][cin_total][KH][KH], channels
 * [cin_off, cin_off + cin_real) (Cin - cin_real padded operand channels are dropped); layout 2 = nn.ConvTranspose2d(2, 2) weight [Cout][Cin / 4][2][2] from the
 * 1x1 form the ConvTranspose backward uses (dz = the layer's INPUT, x = space-to-depth of the output gradient).  x1 != 0: one MFMA per product block. */
extern "C" int smirk_conv_wgrad_param(const void* dz, const void* x, float* dw_param, int B, int H, int W, int Cout, int Cin, int KH, int reflect, int layout,
                                      int cin_total, int cin_off, int cin_real, int x1, void* ws, size_t ws_bytes, void* stream) {
    if (layout == 1) {
        if (cin_real <= 0 || cin_real > Cin || cin_off < 0 || cin_off + cin_real > cin_total) return SMIRK_ERR_BAD_ARG;
    } else if (layout == 2) {
        if (KH != 1 || Cin % 4) return SMIRK_ERR_BAD_ARG;
    } else if (layout != 0) {
        return SMIRK_ERR_BAD_ARG;
    }
    const WgradLayout L{layout, KH * KH, Cin, cin_total, cin_off, cin_real};
    int rc = x1 ? conv_wgrad_impl(dz, x, dw_param, B, H, W, Cout, Cin, KH, reflect, ws, ws_bytes, stream, 1, L) : SMIRK_ERR_UNSUPPORTED;
    if (rc == SMIRK_ERR_UNSUPPORTED) {
        if (x1) g_wgrad_x1_fallbacks.fetch_add(1, std::memory_order_relaxed);     // a step that declared f16x1 ran this layer in the f32-class arithmetic: countable
        rc = conv_wgrad_impl(dz, x, dw_param, B, H, W, Cout, Cin, KH, reflect, ws, ws_bytes, stream, 0, L);
    }
    return rc;
}
/* how many smirk_conv_wgrad_param calls asked for the one-MFMA arithmetic (x1) and were served by the f32-class kernels instead (operands >= 2 GiB, or
 * $SMIRK_WGRAD_F16=0) since the library was loaded: the Python wrapper warns once when this moves, so a step never mixes arithmetics silently */
extern "C" unsigned long long smirk_conv_wgrad_x1_fallbacks(void) { return g_wgrad_x1_fallbacks.load(std::memory_order_relaxed); }
