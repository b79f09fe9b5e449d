// conv_upcat.hip — decoder levels 1 / 2 of the U-Net without their 2x-upsampled tensor: ConvTranspose2d(2c -> c, k2 s2) composed into the 3x3 convolution
// over cat(up, skip) that reads it (src/smirk_generator.py:70-75), split-fp16 (f16x3) arithmetic.  DESIGN.md 22 has the arithmetic and the measurements.
//
// out(Y, X) = conv3x3(skip; W3[:, c:]) + sum over the 2 x 2 coarse neighbours (a, b) of Weff[dy, dx][a, b] . d[y + a][x + b] + shift'[dy, dx][edge], (Y, X) = (2y + dy, 2x + dx):
// the 3x3 taps over `up` collapse to 2 x 2 taps over the coarse tensor d with one weight set per output sub-position (dy, dx) ("class"); the ConvTranspose bias goes
// into the BatchNorm shift, where it depends on the class and on whether the pixel touches an image border (taps that fall into the zero padding carry no bias).
// K per output pixel: 4 * 2c + 9 * c instead of 9 * 2c; the ConvTranspose launch, its B x 2h x 2w x c tensor and the re-read of it are gone.
//
//   upcat_compose_kernel<TN>    Weff (split-fp16, in MFMA B-fragment order) and the 16 shift' rows from the packed ConvTranspose / conv weights; run per forward
//                               (the weight struct has no field for a cached image, and in-place weight updates stay correct)
//   conv3x3_upcat_kernel<TN>    conv3x3_ring_kernel's frame (16 x 16 output patch per workgroup, skip-half weights through the 3-stage LDS ring, halo staged once per
//                               32-channel chunk by buffer-addressed LDS-DMA, fp32 transpose epilogue) with
//     * the row mapping by class: wave w owns class (w >> 1, w & 1) = the patch's 8 x 8 coarse pixels at that sub-position, MFMA row fr of tile i = coarse
//       pixel (4 i + (fr >> 3), fr & 7) — an MFMA row tile holds one class because the classes use different weights;
//     * the fine (skip) halo stored de-interleaved as four 9 x 9 parity planes, so a (class, tap) A fragment is 8 consecutive plane pixels on 4 plane rows;
//     * composed phases: two 32-channel chunks of the 10 x 10 coarse halo (row pitch 11 slots) staged at once in the halo area, four taps each, no barrier
//       between them; each wave's own B fragments come from global / L2 into registers (they differ per wave: an LDS stage for four classes would cost a
//       resident workgroup), the fragments of k-step s of the next phase requested as soon as this phase's k-step s has issued its MFMAs;
//     * LDS piece swizzle ((row & 3) << 1) | ((column >> 1) & 1) on both halo kinds (tests/test_upcat_cpu.py enumerates the banks: conflict-free);
//     * the epilogue's shift row chosen per pixel (class, row edge, column edge), and its ReLU saturating at 65504 with NaN counted as overflow (see there).
// K order: skip chunks -> taps, then coarse chunks -> taps.  Deterministic and batch-invariant (a patch's arithmetic does not depend on which workgroup runs it).
//
// Bound: MFMA; algorithmic flop 2 * B*H*W * c * (4 * 2c + 9 * c), bytes = coarse + skip + out + weights.
#include <stdlib.h>
#include <type_traits>

#include "conv_common.h"

#define UC_PT 16
#define UC_PLANE 81                                // 9 x 9 pixels of one parity plane of the 18 x 18 fine halo
#define UC_HALO_SLOTS 328                          // 4 planes = 324 slots of 128 B + 4 slots of zeros: 41 DMA instructions
#define UC_HALO_BYTES (UC_HALO_SLOTS * 128)
#define UC_CP 11                                   // coarse halo: 10 x 10 pixels at a row pitch of 11 slots (odd: consecutive rows start on different bank halves)
#define UC_CSLOTS 112                              // slots per staged coarse chunk: 14 DMA instructions (110 used)
#define UC_LDS_BYTES(COUT) (3 * (COUT) * 128 + UC_HALO_BYTES)

struct UpcatArgs {
    const float *d, *e, *w3, *weff, *scale, *shift4;
    float* out;
    int B, H, W, npatch;
};

typedef __attribute__((address_space(3))) void* uc_lptr_t;

// physical 16-byte piece of a halo slot = logical piece ^ uc_swz(row, column of the slot in its plane / coarse halo)
__host__ __device__ __forceinline__ int uc_swz(int row, int col) { return ((row & 3) << 1) | ((col >> 1) & 1); }

__device__ __forceinline__ void uc_frag_ready(const half8& a, const half8& b, const half8& c, const half8& d) {
    asm volatile("" ::"v"(a), "v"(b), "v"(c), "v"(d));
}

__device__ __forceinline__ float uc_dec(const _Float16* row, int k) { return (float)row[(k >> 3) * 16 + (k & 7)] + (float)row[(k >> 3) * 16 + 8 + (k & 7)] * (1.0f / 2048.0f); }

// Weff[class][coarse chunk][tap a, b][N tile][k-step][hi | lo][lane][8 halves] (1 KB per fragment: one coalesced 16-byte load per lane) and
// shift4[class][row edge][column edge][Cout] = shift + scale * (sum of W3 . bias over the taps inside the image)
template <int TN>
__global__ __launch_bounds__(256) void upcat_compose_kernel(const float* wup, const float* bup, const float* w3, const float* scale, const float* shift,
                                                            float* weff, float* shift4) {
    constexpr int C = 32 * TN, CIN = 2 * C, NCC = 2 * TN, NW = 4 * NCC * 4 * TN * 2 * 64;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const _Float16* const w3h = (const _Float16*)w3;
    const _Float16* const wuh = (const _Float16*)wup;
    if (idx < NW) {
        const int lane = idx & 63, s = (idx >> 6) & 1, j = (idx >> 7) % TN;
        int rest = (idx >> 7) / TN;
        const int tap = rest & 3;
        rest >>= 2;
        const int cc = rest % NCC, cls = rest / NCC;
        const int dy = cls >> 1, dx = cls & 1, ca = dy - 1 + (tap >> 1), cb = dx - 1 + (tap & 1);
        const int co = j * 32 + (lane & 31), ci0 = cc * 32 + s * 16 + (lane >> 5) * 8;
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int ty = -1; ty <= 1; ++ty) {
            if (((dy + ty) >> 1) != ca) continue;
            for (int tx = -1; tx <= 1; ++tx) {
                if (((dx + tx) >> 1) != cb) continue;
                const int sub = ((dy + ty) & 1) * 2 + ((dx + tx) & 1);
                const _Float16* const w3row = w3h + ((size_t)co * 9 * CIN + ((ty + 1) * 3 + (tx + 1)) * CIN) * 2;
#pragma unroll 8
                for (int cu = 0; cu < C; ++cu) {                     // (unrolled: eight rows' loads in flight — the kernel is a few thousand threads waiting on L2)
                    const double wv = (double)uc_dec(w3row, cu);
                    const _Float16* const g = wuh + ((size_t)(sub * C + cu) * CIN + ci0) * 2;      // one 8-channel group: hi halves, lo halves
#pragma unroll
                    for (int q = 0; q < 8; ++q) acc[q] += wv * ((double)(float)g[q] + (double)(float)g[8 + q] * (1.0 / 2048.0));
                }
            }
        }
        half8 hi, lo;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float v = (float)acc[q];
            hi[q] = (_Float16)v;
            lo[q] = (_Float16)((v - (float)hi[q]) * 2048.0f);
        }
        const int frag = ((((cls * NCC + cc) * 4 + tap) * TN + j) * 2 + s) * 2;
        ((half8*)weff)[(size_t)frag * 64 + lane] = hi;
        ((half8*)weff)[(size_t)(frag + 1) * 64 + lane] = lo;
    } else if (idx < NW + 16 * C) {
        const int i2 = idx - NW, co = i2 % C, var = i2 / C;
        const int ce = var & 1, re = (var >> 1) & 1, cls = var >> 2, dy = cls >> 1, dx = cls & 1;
        double acc = 0.0;
        for (int ty = -1; ty <= 1; ++ty) {
            if (re && ty == (dy ? 1 : -1)) continue;                  // this tap's fine row lies in the zero padding
            for (int tx = -1; tx <= 1; ++tx) {
                if (ce && tx == (dx ? 1 : -1)) continue;
                const _Float16* const w3row = w3h + ((size_t)co * 9 * CIN + ((ty + 1) * 3 + (tx + 1)) * CIN) * 2;
                for (int cu = 0; cu < C; ++cu) acc += (double)uc_dec(w3row, cu) * (double)bup[cu];
            }
        }
        shift4[i2] = (float)((double)shift[co] + (double)scale[co] * acc);
    }
}

// TN = output channels / 32 (1: decoder level 1, 64 @ 112^2 + 32 @ 224^2 -> 32; 2: level 2, 128 @ 56^2 + 64 @ 112^2 -> 64)
// X1: one fp16 MFMA per product block on the hi halves (the generator's "f16x1" inference arithmetic, as in conv_ring.hip): no lo fragment is read from LDS or — the
//     composed half — from global, one MFMA group of the three remains, the epilogue takes acc0 alone; the DMA schedule and its counted waits are the x3 ones.
template <int TN, bool X1 = false>
__global__ __launch_bounds__(256, TN == 1 ? 3 : 2) void conv3x3_upcat_kernel(UpcatArgs a) {
    constexpr int COUT = 32 * TN, C = COUT, CIN = 2 * C, K = 9 * CIN, STAGE = COUT * 128, EPI_LD = COUT + 4, GPR = COUT / 8, ITEMS = 32 * GPR / 64;
    constexpr int NSK = TN, NCC = 2 * TN, RING = 3 * STAGE;
    extern __shared__ __attribute__((aligned(16))) char uc_lds[];
    char* const ring = uc_lds;
    char* const halo = uc_lds + RING;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int dy = wave >> 1, dx = wave & 1;                          // this wave's class
    const int fr = lane & 31, hb = lane >> 5;
    const int H = a.H, W = a.W, h = H >> 1, w = W >> 1;
    const int tiles_x = W / UC_PT, tiles_per_img = (H / UC_PT) * tiles_x;

    const long long px_all = (long long)a.B * H * W;
    const __amdgpu_buffer_rsrc_t rsE = __builtin_amdgcn_make_buffer_rsrc((void*)a.e, (short)0, (int)(px_all * C * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc((void*)a.d, (short)0, (int)((px_all >> 2) * CIN * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w3, (short)0, COUT * K * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsF = __builtin_amdgcn_make_buffer_rsrc((void*)a.weff, (short)0, 4 * NCC * 4 * TN * 4 * 1024, 0x00020000);

    // skip-half weight chunk (cc, tap) -> ring stage st: conv3x3_ring_kernel's DMA over the channels C + 32 cc .. of the [Cout][9][2C] tensor
    unsigned voffB[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < TN; ++k) {
        const int row = 8 * (wave + 4 * k) + (lane >> 3);
        voffB[k] = ((unsigned)row * (unsigned)K + (unsigned)((lane & 7) ^ ((row >> 1) & 7)) * 4u) * 4u;
    }
    auto dmaB = [&](int cc, int tap, int st) {
        const int so = (tap * CIN + C + cc * 32) * 4;
#pragma unroll
        for (int k = 0; k < TN; ++k)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (uc_lptr_t)(ring + st * STAGE + (wave + 4 * k) * 1024), 16, voffB[k], so, 0, 0);
    };
    // fine halo of skip chunk cc: slot s = plane * 81 + py * 9 + px holds halo pixel (2 py + (plane >> 1), 2 px + (plane & 1)); outside the image -> zeros
    auto dmaE = [&](int b, int oy0, int ox0, int cc) {
        const int basepix = (b * H + oy0 - 1) * W + ox0 - 1;
#pragma unroll
        for (int q = 0; q < 11; ++q) {
            if ((q * 4 + wave) * 8 >= UC_HALO_SLOTS) continue;        // wave-uniform
            int l8 = lane >> 3;
            asm volatile("" : "+v"(l8));                              // slot arithmetic is redone per issue instead of living in registers
            const unsigned s = (unsigned)((q * 4 + wave) * 8 + l8);
            const unsigned pl = s / UC_PLANE, rem = s - pl * UC_PLANE, py = rem / 9u, px = rem - py * 9u;
            const int hy = 2 * (int)py + (int)(pl >> 1), hx = 2 * (int)px + (int)(pl & 1);
            const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;
            const bool ok = pl < 4u && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const int piece = (lane & 7) ^ uc_swz((int)py, (int)px);
            const unsigned vo = ok ? (unsigned)(basepix + hy * W + hx) * (unsigned)(C * 4) + (unsigned)piece * 16u : 0x80000000u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsE, (uc_lptr_t)(halo + (q * 4 + wave) * 8 * 128), 16, vo, cc * 128, 0, 0);
        }
    };
    // coarse halo, chunks cc0 and cc0 + 1: slot k * 112 + hy * 11 + hx holds coarse pixel (oy0 / 2 - 1 + hy, ox0 / 2 - 1 + hx), hy, hx < 10
    auto dmaC = [&](int b, int oy0, int ox0, int cc0) {
        const int y0 = (oy0 >> 1) - 1, x0 = (ox0 >> 1) - 1;
        const int basepix = (b * h + y0) * w + x0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q * 4 + wave >= UC_CSLOTS / 8) continue;          // wave-uniform: 14 instructions per chunk
                int l8 = lane >> 3;
                asm volatile("" : "+v"(l8));
                const unsigned t = (unsigned)((q * 4 + wave) * 8 + l8);
                const unsigned uy = t / (unsigned)UC_CP;
                const int hy = (int)uy, hx = (int)(t - uy * UC_CP);
                const int iy = y0 + hy, ix = x0 + hx;
                const bool ok = hy < 10 && hx < 10 && iy >= 0 && iy < h && ix >= 0 && ix < w;
                const int piece = (lane & 7) ^ uc_swz(hy, hx);
                const unsigned vo = ok ? (unsigned)(basepix + hy * w + hx) * (unsigned)(CIN * 4) + (unsigned)piece * 16u : 0x80000000u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsD, (uc_lptr_t)(halo + (k * UC_CSLOTS + (q * 4 + wave) * 8) * 128), 16, vo, (cc0 + k) * 128, 0, 0);
            }
        }
    };
    // A-fragment base (bytes) of tile 0: this lane's row (r, cx) = (fr >> 3, fr & 7) of a halo whose slot (r0 + r) * pitch + c0 + cx + sbase holds the pixel
    // under the tap; the swizzle depends on (row & 3, column) only, so tile 1 (4 rows further) is a constant displacement.  Formed per phase, not kept.
    auto a_base = [&](int sbase, int r0, int c0, int pitch) -> unsigned {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int r = (ln >> 3) & 3, cx = ln & 7;
        return (unsigned)RING + (unsigned)(sbase + (r0 + r) * pitch + c0 + cx) * 128u + (unsigned)((uc_swz(r0 + r, c0 + cx) << 4) ^ ((ln >> 5) << 5));
    };
    const unsigned bB = (unsigned)fr * 128u + (unsigned)((((fr >> 1) & 7) << 4) ^ (hb << 5));
    const unsigned fL = (unsigned)lane * 16u;                         // this lane's 16 bytes of a 1 KB Weff fragment

    float ep_sc[8];                                                  // scale of this lane's channel group (g = lane % GPR)
#pragma unroll
    for (int q = 0; q < 8; ++q) ep_sc[q] = a.scale[(lane % GPR) * 8 + q];

    int p = blockIdx.x;
    if (p >= a.npatch) return;
    dmaB(0, 0, 0);
    dmaB(0, 1, 1);
    f32x16 acc0[2][TN], acc1[2][TN];
    const f32x16 z16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    SmirkRangeAccS rng;
    for (; p < a.npatch; p += gridDim.x) {
        const int b = p / tiles_per_img, t = p - b * tiles_per_img, ty = t / tiles_x;
        const int oy0 = ty * UC_PT, ox0 = (t - ty * tiles_x) * UC_PT;

        // one k-chunk of 32 channels under one tap: 2 k-steps x (2 row tiles x TN column tiles) x 3 MFMAs
        auto mfma_step = [&](const half8 (&ah)[2], const half8 (&al)[2], const half8 (&bh)[TN], const half8 (&bl)[TN], bool zero) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc0[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], zero ? z16 : acc0[i][j], 0, 0, 0);
            if constexpr (!X1) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], zero ? z16 : acc1[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc1[i][j], 0, 0, 0);
            }
        };
        auto frag_ready = [&](const half8 (&ah)[2], const half8 (&al)[2], const half8 (&bh)[TN], const half8 (&bl)[TN]) {
            if constexpr (X1) uc_frag_ready(ah[0], ah[1], bh[0], bh[TN - 1]);
            else uc_frag_ready(ah[1], al[1], bh[TN - 1], bl[TN - 1]);
        };
        auto load_a = [&](unsigned av, unsigned tile_disp, half8 (&ah)[2][2], half8 (&al)[2][2]) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const unsigned ch = (unsigned)(s << 6), cl = ch | 16u;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    ah[s][i] = *(const half8*)(uc_lds + ((av ^ ch) + i * tile_disp));
                    if constexpr (!X1) al[s][i] = *(const half8*)(uc_lds + ((av ^ cl) + i * tile_disp));
                }
            }
        };

        // ---- skip half: conv3x3_ring_kernel's chunk / phase schedule over the de-interleaved fine halo ---------------------------------------------------
        for (int cc = 0; cc < NSK; ++cc) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            dmaE(b, oy0, ox0, cc);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int ccn = cc + 1 < NSK ? cc + 1 : 0;
            auto phase = [&](auto tapc, auto firstc) {
                constexpr int TAP = decltype(tapc)::value, ST = TAP % 3, KY = TAP / 3, KX = TAP % 3;
                constexpr bool FIRST = decltype(firstc)::value;
                if constexpr (TAP > 0) {
                    if constexpr (TN == 2) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                }
                constexpr int T2 = (TAP + 2) % 9;
                dmaB(TAP + 2 < 9 ? cc : ccn, T2, T2 % 3);            // (after the last skip phase of a patch: the next patch's taps 0 and 1; they wait in the ring)
                const int sy = dy + KY, sx = dx + KX;                 // halo pixel (2 cy + sy, 2 cx + sx): plane (sy & 1, sx & 1), plane pixel (cy + (sy >> 1), cx + (sx >> 1))
                unsigned av = a_base(((sy & 1) * 2 + (sx & 1)) * UC_PLANE, sy >> 1, sx >> 1, 9), bv = bB;
                asm volatile("" : "+v"(av), "+v"(bv));
                half8 ah[2][2], al[2][2], bh[2][TN], bl[2][TN];
                load_a(av, 4 * 9 * 128, ah, al);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const unsigned ch = (unsigned)(s << 6), cl = ch | 16u;
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        bh[s][j] = *(const half8*)(uc_lds + ((bv ^ ch) + (unsigned)(ST * STAGE + j * 4096)));
                        if constexpr (!X1) bl[s][j] = *(const half8*)(uc_lds + ((bv ^ cl) + (unsigned)(ST * STAGE + j * 4096)));
                    }
                }
                if constexpr (TN == 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    frag_ready(ah[s], al[s], bh[s], bl[s]);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_step(ah[s], al[s], bh[s], bl[s], FIRST && s == 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (TN == 2) __builtin_amdgcn_s_setprio(0);
            };
            if (cc == 0) phase(std::integral_constant<int, 0>{}, std::true_type{});
            else phase(std::integral_constant<int, 0>{}, std::false_type{});
            phase(std::integral_constant<int, 1>{}, std::false_type{}); phase(std::integral_constant<int, 2>{}, std::false_type{});
            phase(std::integral_constant<int, 3>{}, std::false_type{}); phase(std::integral_constant<int, 4>{}, std::false_type{});
            phase(std::integral_constant<int, 5>{}, std::false_type{}); phase(std::integral_constant<int, 6>{}, std::false_type{});
            phase(std::integral_constant<int, 7>{}, std::false_type{}); phase(std::integral_constant<int, 8>{}, std::false_type{});
        }

        // ---- composed half: pairs of coarse chunks; B fragments of this wave's class from global into registers --------------------------------------------
        half8 bh[2][TN], bl[2][TN];
        auto loadB = [&](int s, int phase_idx) {                      // phase_idx = chunk * 4 + tap
            const int so = ((wave * NCC * 4 + phase_idx) * TN * 4 + s * 2) * 1024;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bh[s][j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rsF, fL, so + j * 4096, 0));
                if constexpr (!X1) bl[s][j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rsF, fL, so + j * 4096 + 1024, 0));
            }
        };
        for (int pr = 0; pr < NCC / 2; ++pr) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                             // every wave has left the previous halo
            dmaC(b, oy0, ox0, 2 * pr);
            if (pr == 0) { loadB(0, 0); loadB(1, 0); }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            auto cphase = [&](auto kc, auto tapc) {
                constexpr int KC = decltype(kc)::value, TAP = decltype(tapc)::value, AI = TAP >> 1, BI = TAP & 1;
                const int idx = (2 * pr + KC) * 4 + TAP;
                const bool more = idx + 1 < NCC * 4;
                unsigned av = a_base(KC * UC_CSLOTS, dy + AI, dx + BI, UC_CP);
                asm volatile("" : "+v"(av));
                half8 ah[2][2], al[2][2];
                load_a(av, 4 * UC_CP * 128, ah, al);
                if constexpr (TN == 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    frag_ready(ah[s], al[s], bh[s], bl[s]);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_step(ah[s], al[s], bh[s], bl[s], false);
                    __builtin_amdgcn_sched_barrier(0);
                    if (more) loadB(s, idx + 1);                      // the next phase's fragments of this k-step fly during the other k-step
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (TN == 2) __builtin_amdgcn_s_setprio(0);
            };
            cphase(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}); cphase(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
            cphase(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{}); cphase(std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
            cphase(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}); cphase(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
            cphase(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{}); cphase(std::integral_constant<int, 1>{}, std::integral_constant<int, 3>{});
        }

        // ---- epilogue: conv3x3_ring_kernel's, with the class mapping of the rows and the shift row chosen per pixel ------------------------------------------
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        float* const ebuf = (float*)halo + wave * 32 * EPI_LD;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ebuf[mfma32_row(r, lane) * EPI_LD + j * 32 + fr] = X1 ? acc0[i][j][r] : acc0[i][j][r] + acc1[i][j][r] * (1.0f / 2048.0f);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // per-wave transpose buffer: LDS operations of one wave execute in order
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {                     // item e = it * 64 + lane: tile row e / GPR = coarse pixel (4 i + (row >> 3), row & 7), channel group e % GPR
                const int e = it * 64 + lane, row = e / GPR, g = e % GPR;
                const int Y = oy0 + 2 * (4 * i + (row >> 3)) + dy, X = ox0 + 2 * (row & 7) + dx;
                const int re = Y == (dy ? H - 1 : 0), ce = X == (dx ? W - 1 : 0);
                const float* const shp = a.shift4 + ((wave * 2 + re) * 2 + ce) * COUT + g * 8;
                const f32x4 s0 = *(const f32x4*)shp, s1 = *(const f32x4*)(shp + 4);
                const float* src = ebuf + row * EPI_LD + g * 8;
                float v[8];
                *(f32x4*)v = *(const f32x4*)src;
                *(f32x4*)(v + 4) = *(const f32x4*)(src + 4);
                // ReLU, then saturation at the format's largest value.  The NaN-propagating maximum (v_maximum3_f32) keeps a NaN accumulator, the minimum turns it
                // into 65504: an overflowed input (+inf under weights of both signs makes every accumulator of this level NaN) must stay visible in the pixels, and
                // the ReLUs downstream would flush NaN / inf - inf to clean zeros (tests/test_generator_gpu.py, the 1e4-scaled checkpoint).  The range audit sees the
                // values before the saturation.
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = __builtin_elementwise_maximum(v[q] * ep_sc[q] + s0[q], 0.f);
                    v[q + 4] = __builtin_elementwise_maximum(v[q + 4] * ep_sc[q + 4] + s1[q], 0.f);
                }
                rng.see8(v);
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = fminf(v[q], 65504.f);
                half8 hi, lo;
                split8_noaudit(v, hi, lo);
                float* o = a.out + (((size_t)b * H + Y) * W + X) * COUT + g * 8;
                *(half8*)o = hi;
                *(half8*)(o + 4) = lo;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // the buffer is rewritten by the next tile
        }
    }
    rng.commit();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the over-fetched weight pieces must have landed before the workgroup's LDS is released
}

// Serves: split-fp16 decoder levels with c = 32 or 64 output channels on a fine image whose sides are multiples of 16 and at least 64, unless
// $SMIRK_CONV_RING=0 (the ring family's A/B switch also restores the two-launch levels).
bool smirk_conv3x3_upcat_eligible(int c, int H, int W) {
    if (!smirk_switch(SMIRK_SW_CONV_RING)) return false;
    return (c == 32 || c == 64) && H % UC_PT == 0 && W % UC_PT == 0 && H >= 64 && W >= 64;
}

size_t smirk_conv3x3_upcat_weff_bytes(int c) { return (size_t)32 * c * c * 4; }       // 4 classes x 4 taps x 2c x c split-fp16 pairs
size_t smirk_conv3x3_upcat_shift_bytes(int c) { return (size_t)16 * c * 4; }

template <int TN, bool X1 = false>
static int uc_run(const UpcatArgs& proto, const float* wup, const float* bup, const float* shift, float* weff, float* shift4, int B, hipStream_t st) {
    constexpr int C = 32 * TN, PER_CU = TN == 1 ? 3 : 2;
    constexpr int NTHREADS = 4 * (2 * TN) * 4 * TN * 2 * 64 + 16 * C;
    if (g_smirk_prof_on) smirk_prof_next(TN == 1 ? "upcat_compose_kernel<1>" : "upcat_compose_kernel<2>", 2.0 * 4 * 9 * C * C * 2 * C, 4.0 * (4 * C * 2 * C + 18 * C * C + 32 * C * C));
    SMIRK_LAUNCH((upcat_compose_kernel<TN>), dim3((NTHREADS + 255) / 256), dim3(256), 0, st, wup, bup, proto.w3, proto.scale, shift, weff, shift4);
    if (const int rc = smirk_launch_status()) return rc;
    if (const int rc = smirk_raise_dynamic_lds((const void*)conv3x3_upcat_kernel<TN, X1>, UC_LDS_BYTES(C))) return rc;
    // batch chunks whose skip / output tensors stay below 2 GiB (32-bit buffer offsets; the coarse tensor is half their size)
    const long long per_img = (long long)proto.H * proto.W * C * 4;
    int bc = (int)((CONV_BUF_LIMIT - 1) / per_img);
    if (bc < 1) return SMIRK_ERR_UNSUPPORTED;
    const int n_cu = smirk_device_cus();
    for (int b0 = 0; b0 < B; b0 += bc) {
        const int nb = B - b0 < bc ? B - b0 : bc;
        UpcatArgs a = proto;
        a.d = proto.d + (size_t)b0 * (per_img / 8);                   // coarse: (H/2)(W/2) pixels x 2C dwords = per_img / 2 bytes
        a.e = proto.e + (size_t)b0 * (per_img / 4);
        a.out = proto.out + (size_t)b0 * (per_img / 4);
        a.B = nb;
        a.npatch = nb * (proto.H / UC_PT) * (proto.W / UC_PT);
        const int grid = a.npatch < PER_CU * n_cu ? a.npatch : PER_CU * n_cu;
        if (g_smirk_prof_on) {
            const double px = (double)nb * proto.H * proto.W;
            smirk_prof_next(X1 ? "conv3x3_upcat_kernel<2>[16x16 patch,composed upconv,f16x1]"
                            : TN == 1 ? "conv3x3_upcat_kernel<1>[16x16 patch,composed upconv]" : "conv3x3_upcat_kernel<2>[16x16 patch,composed upconv]",
                            2.0 * px * C * (4.0 * 2 * C + 9.0 * C), px * 0.25 * 2 * C * 4.0 + 2.0 * px * C * 4.0 + (9.0 * C * C + 32.0 * C * C) * 4.0);
        }
        SMIRK_LAUNCH((conv3x3_upcat_kernel<TN, X1>), dim3(grid), dim3(256), UC_LDS_BYTES(C), st, a);
        if (const int rc = smirk_launch_status()) return rc;
    }
    return SMIRK_OK;
}

// d: coarse tensor [B][H/2][W/2][2c]; e: skip tensor [B][H][W][c]; up: the ConvTranspose2d layer (w = [(dy,dx,co)][ci], shift = bias); conv: the level's first
// 3x3 layer over cat(up, e) with its folded BatchNorm; out [B][H][W][c] = ReLU(BN(conv)); weff / shift4: workspace of smirk_conv3x3_upcat_{weff,shift}_bytes(c)
int smirk_conv3x3_upcat_launch(int c, const void* d, const void* e, const SmirkConvLayer* up, const SmirkConvLayer* conv, void* out, int B, int H, int W,
                               void* weff, void* shift4, hipStream_t st, bool x1) {
    if (!smirk_conv3x3_upcat_eligible(c, H, W) || (x1 && c != 64)) return SMIRK_ERR_UNSUPPORTED;   // (the one-MFMA form: the 64-channel level only)
    if (!d || !e || !out || !weff || !shift4 || !up->w || !up->shift || up->scale || !conv->w || !conv->scale || !conv->shift || B <= 0) return SMIRK_ERR_BAD_ARG;
    UpcatArgs a;
    a.d = (const float*)d; a.e = (const float*)e; a.w3 = (const float*)conv->w; a.weff = (const float*)weff; a.scale = conv->scale; a.shift4 = (const float*)shift4;
    a.out = (float*)out; a.B = B; a.H = H; a.W = W; a.npatch = 0;
    if (x1) return uc_run<2, true>(a, (const float*)up->w, up->shift, conv->shift, (float*)weff, (float*)shift4, B, st);
    return c == 32 ? uc_run<1>(a, (const float*)up->w, up->shift, conv->shift, (float*)weff, (float*)shift4, B, st)
                   : uc_run<2>(a, (const float*)up->w, up->shift, conv->shift, (float*)weff, (float*)shift4, B, st);
}
