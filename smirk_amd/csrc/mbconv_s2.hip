// mbconv_s2.hip — the stride-2 InvertedResidual blocks of the timm "minimal" backbones (112^2 -> 56^2 ... 28^2 -> 14^2) with ONE WAVE per output tile (gfx950):
//
//      x --1x1 expand + BN + ReLU--> E --3x3 depthwise (stride 2, TF-SAME) + BN + ReLU--> D --1x1 project + BN--> out
//
// (reference call site smirk_encoder.py:11-21 `self.encoder(img)[-1]`.)  mbconv_fused_kernel<2,true,KS> (mbconv.hip) gives a 4 x 8 output tile to a
// 256-thread workgroup that crosses two workgroup barriers per 32-channel chunk; a tile is ~42 MFMAs, so the workgroup spends its time parked.  A 4 x 8
// stride-2 tile is exactly one 32-row MFMA block of outputs, so here a single wave owns a tile from its first load to its last store:
//   * x never goes through LDS: the expand A fragment of lane (fr, hb) is 32 contiguous bytes of one halo pixel, loaded from global memory (KS = 1: all five
//     32-row blocks of the 9 x 17 halo stay in registers across the chunks; KS = 2: re-fetched through L1 one row block ahead);
//   * E_c (153 halo pixels x 32 channels, fp32, zero outside the image) lives in a wave-private LDS region laid out for conflict-free stride-2 reads (s2w_idx);
//   * the depthwise result goes straight into the project GEMM's A fragments (lane = output pixel, 8 channels per 16-k step): D never exists in memory;
//   * project accumulators stay in registers across the chunks; bn3, a per-wave 32 x 32 transpose through the wave's own E region, split16 stores.
// One workgroup barrier in the kernel (after the depthwise taps are staged to LDS, shared by the four waves); after it a wave orders its own LDS traffic with
// s_waitcnt lgkmcnt(0) only.  A workgroup is four waves on four consecutive tiles; 2 workgroups = 8 independent waves per CU: 2 x (4 x 19,584 B + 9 mid floats) <= 160 KiB.
// Bound: LDS issue (~144 ds_read_b128 + ~160 ds_write_b32 per tile) and latency, hidden by the eight waves.  Arithmetic: the operations of mbconv_fused_kernel<2,true,KS>
// in the same order (results are bit-identical, tests/test_mbconv_s2_gpu.py).
#include <stdio.h>

#include "common.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

#define S2W_NH 153                       // 9 x 17 halo pixels
#define S2W_EB (S2W_NH * 128)            // bytes of a wave's E region
#define S2W_MAX_MID 96                   // 9 x mid depthwise taps beside the four E regions: 2 workgroups per CU

struct MBS2Args {
    const char* x;          // split16 NHWC, Cin*4 bytes per pixel
    const char* wexp;       // [mid][Cin] split16 rows
    const float *s1, *b1;   // [mid]
    const float* wdw;       // [9][mid]
    const float *s2, *b2;   // [mid]
    const char* wproj;      // [Cout][mid] split16 rows
    const float *s3, *b3;   // [Cout]
    char* out;              // split16 NHWC [B][Ho][Wo][Cout]
    int B, H, W, Cin, mid, Cout, Ho, Wo, pt, pl, tiles_x, tiles_y, ntiles;
};

// E-region cell of halo pixel (hy, hx), 0 <= hy < 9, 0 <= hx < 17.  A cell is 128 bytes (32 floats) whose eight 16-byte slots are XOR-swizzled with (cell >> 1) & 7, so the
// 16 lanes of a ds_read_b128 group read 16 distinct slots iff their 16 cells are distinct mod 16.  A group is two output rows x eight output columns (s2w_out_px) and a
// depthwise tap reads, for all of them, pixels of ONE row parity and ONE column parity: rows R0, R0 + 1 and eight consecutive columns J of that parity class.  Inside a class
// the cell is (R >> 1) * pitch + 2 J + (R & 1) with an even pitch: the two rows take the eight even and the eight odd residues (or 16 consecutive ones).  The classes are
// packed without a hole: even columns (9 per row) pitch 18, odd columns (8) pitch 16, and the single last row (hy = 8) of the odd-column class fills the odd cells that
// the last row of the even-column class leaves free: 153 cells for 153 pixels.
__device__ __forceinline__ int s2w_idx(int hy, int hx) {
    const int R = hy >> 1, J = hx >> 1;
    if (!(hx & 1)) return ((hy & 1) ? 85 : 0) + (R >> 1) * 18 + 2 * J + (R & 1);
    if (hy & 1) return 121 + (R >> 1) * 16 + 2 * J + (R & 1);
    return R < 4 ? 53 + (R >> 1) * 16 + 2 * J + (R & 1) : 37 + 2 * J;
}
// the inverse: halo pixel of cell p (row p of the expand GEMM is cell p, so an accumulator row's LDS address is linear in the row); false for p >= 153
__device__ __forceinline__ bool s2w_pix(int p, int& hy, int& hx) {
    int R, J, rp, cp;
    if (p < 53) {
        if (p < 36 || !(p & 1)) { const int pr = p / 18, rem = p - pr * 18; rp = 0; cp = 0; R = 2 * pr + (rem & 1); J = rem >> 1; }
        else { rp = 0; cp = 1; R = 4; J = (p - 37) >> 1; }
    } else if (p < 85) { const int u = p - 53; rp = 0; cp = 1; R = 2 * (u >> 4) + (u & 1); J = (u & 15) >> 1; }
    else if (p < 121) { const int u = p - 85, pr = u / 18, rem = u - pr * 18; rp = 1; cp = 0; R = 2 * pr + (rem & 1); J = rem >> 1; }
    else { const int u = p - 121; rp = 1; cp = 1; R = 2 * (u >> 4) + (u & 1); J = (u & 15) >> 1; }
    hy = 2 * R + rp; hx = 2 * J + cp;
    return p < S2W_NH;
}
// output pixel (oy, ox) of MFMA row m (= lane & 31 in the depthwise phase): the hardware serves a ds_read_b128 in the lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}
// (MI355X_MICROARCH.md); the 4-lane blocks are dealt so that the first group holds output rows 0-1 and the second rows 2-3, all eight columns each
__device__ __forceinline__ void s2w_out_px(int m, int& oy, int& ox) {
    const int k = m >> 2;
    oy = (0xD728 >> (2 * k)) & 3;
    ox = ((k >> 1) & 1) * 4 + (m & 3);
}

__device__ __forceinline__ void s2w_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }   // a wave's own LDS writes before its own reads (and back)

// KS = ceil(Cin / 16) 16-k steps of the expand GEMM, NT = ceil(Cout / 32) 32-column tiles of the project GEMM
template <int KS, int NT>
__global__ __launch_bounds__(256, 2) void mbconv_s2_wave_kernel(MBS2Args a) {
    constexpr bool HOLD = KS == 1;                        // x fragments of all five row blocks stay in registers (40 VGPRs); otherwise two blocks in flight
    constexpr int NB = 5;                                 // 32-row blocks of the expand GEMM (160 rows, 153 cells)
    extern __shared__ __attribute__((aligned(16))) char s2w_smem[];
    SmirkRangeAccS rng;                                   // split-fp16 range audit (common.h): one site, on the output
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 31, hb = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* Wt = (float*)(s2w_smem + 4 * S2W_EB);          // [9][mid] depthwise taps
    const int tile = (int)blockIdx.x * 4 + wave;
    const bool has = tile < a.ntiles;                     // waves beyond the last tile run the prologue on the last tile's (valid) addresses and leave after the barrier
    int bid = min(tile, a.ntiles - 1);
    const int tx = bid % a.tiles_x; bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int b = bid / a.tiles_y;
    const int oy0 = ty * 4, ox0 = tx * 8, iy0 = oy0 * 2 - a.pt, ix0 = ox0 * 2 - a.pl;
    const unsigned xrow = (unsigned)a.Cin * 4;
    const int gmax = a.Cin / 8;
    const int nchunks = (a.mid + 31) / 32;
    const half8 hz = {0, 0, 0, 0, 0, 0, 0, 0};
    const char* xb = a.x + (size_t)b * a.H * a.W * xrow;

    // ---- prologue: depthwise taps -> LDS (all requests before the first store); this lane's halo pixels; first fragments ---------------------------------
    {
        const int n = 9 * a.mid;                          // <= 864
        float cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) cv[u] = a.wdw[min(tid + 256 * u, n - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (tid + 256 * u < n) Wt[tid + 256 * u] = cv[u];
    }
    unsigned xo[NB], om[NB];                              // byte offset of halo pixel 32 t + fr (clamped into the image); validity of the accumulator rows of block t
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        int hy, hx;
        const bool cell = s2w_pix(32 * t + fr, hy, hx);
        const int iy = iy0 + hy, ix = ix0 + hx;
        const bool ok = cell && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const int yc = min(max(iy, 0), a.H - 1), xc = min(max(ix, 0), a.W - 1);
        xo[t] = (unsigned)(yc * a.W + xc) * xrow;
        // accumulator register r of this lane is row (r & 3) + 8 (r >> 2) + 4 hb of the block: bit (r & 3) + 8 (r >> 2) of om[t]
        om[t] = (unsigned)__builtin_amdgcn_ballot_w64(ok) >> (4 * hb);
    }
    // x fragments of row block t: clamped address, no branches; the pixels outside the image need no zeros (their E rows are forced to 0 below: the depthwise
    // conv pads E, not x), the channels beyond Cin do (Cin = 8 / 24: the upper half of the last k-step)
    auto load_x = [&](int t, half8 (*dst)[2]) {
        const char* px = xb + xo[t];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int g = 2 * s + hb, gc = min(g, gmax - 1);
            const half8 t0 = *(const half8*)(px + gc * 32), t1 = *(const half8*)(px + gc * 32 + 16);
            if (s == KS - 1) { dst[s][0] = g < gmax ? t0 : hz; dst[s][1] = g < gmax ? t1 : hz; }
            else { dst[s][0] = t0; dst[s][1] = t1; }
        }
    };
    half8 xa[HOLD ? NB : 2][KS][2];
    if constexpr (HOLD) {
#pragma unroll
        for (int t = 0; t < NB; ++t) load_x(t, xa[t]);
    } else {
        load_x(0, xa[0]);
    }
    half8 we[KS][2];                                      // expand-weight fragments of the current chunk (column = 32 c + fr) and its BN constants (zero beyond mid)
    float s1v, b1v;
    auto load_we = [&](int c) {
        const int ch = 32 * c + fr, chc = min(ch, a.mid - 1);
        const char* wrow = a.wexp + (size_t)chc * xrow;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int g = 2 * s + hb, gc = min(g, gmax - 1);
            const bool v = ch < a.mid && g < gmax;
            const half8 t0 = *(const half8*)(wrow + gc * 32), t1 = *(const half8*)(wrow + gc * 32 + 16);
            we[s][0] = v ? t0 : hz;
            we[s][1] = v ? t1 : hz;
        }
        const float t1 = a.s1[chc], t2 = a.b1[chc];
        s1v = ch < a.mid ? t1 : 0.f;
        b1v = ch < a.mid ? t2 : 0.f;
    };
    load_we(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the only workgroup barrier: the taps are staged (LDS only: the global fetches above stay in flight)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (!has) return;

    const unsigned ebase = (unsigned)wave * S2W_EB;
    // expand stores: accumulator register r of block t is cell 32 t + (r & 3) + 8 (r >> 2) + 4 hb, column fr.  (cell >> 1) & 7 = ((r >> 1) & 1) | hb << 1 | ((r >> 2) & 1) << 2:
    // the swizzle splits into a per-lane part (folded into est) and a compile-time part (one XOR for each of its four values); the cell itself is an immediate offset
    const unsigned est = ebase + hb * 512 + ((((unsigned)fr >> 2) ^ (hb << 1)) << 4) + (fr & 3) * 4;
    // depthwise reads: cell of each tap of this lane's output pixel, swizzle of channel group 2 hb folded in; channel quad 4 s + h is one more XOR
    unsigned ta[9];
    int my_oy, my_ox;
    s2w_out_px(fr, my_oy, my_ox);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int idx = s2w_idx(2 * my_oy + ky, 2 * my_ox + kx);
            ta[ky * 3 + kx] = ebase + idx * 128 + ((((idx >> 1) ^ (2 * hb)) & 7) << 4);
        }

    f32x16 pacc[NT][2];
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) pacc[q][h][r] = 0.f;

    for (int c = 0; c < nchunks; ++c) {
        // ---- expand chunk c: five 32-row blocks -> E (fp32, zero outside the image) ---------------------------------------------------------------------------
        if constexpr (!HOLD) {
            if (c > 0) {
#pragma unroll
                for (int s = 0; s < KS; ++s) { xa[0][s][0] = xa[1][s][0]; xa[0][s][1] = xa[1][s][1]; }
            }
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            if constexpr (!HOLD) {                        // one row block ahead (block 0 of the next chunk behind block 4)
                if (t + 1 < NB) load_x(t + 1, xa[(t + 1) & 1]);
                else if (c + 1 < nchunks) load_x(0, xa[1]);
            }
            half8 (*cur)[2] = xa[HOLD ? t : (t & 1)];
            unsigned et = est;
            if (NT > 1) asm volatile("" : "+v"(et));      // <2, 2>: the four swizzled store bases are re-derived per row block instead of living across the chunk loop
            f32x16 e0, e1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { e0[r] = 0.f; e1[r] = 0.f; }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                e0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[s][0], we[s][0], e0, 0, 0, 0);
                e1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[s][0], we[s][1], e1, 0, 0, 0);
                e1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[s][1], we[s][0], e1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = (r & 3) + 8 * (r >> 2);
                const unsigned cr = ((r >> 1) & 1) | (((r >> 2) & 1) << 2);
                if (t < NB - 1 || ro + 4 * hb < S2W_NH - 32 * (NB - 1)) {     // cells 153 .. 159 do not exist
                    const float v = fmaxf((e0[r] + e1[r] * (1.0f / 2048.0f)) * s1v + b1v, 0.f);
                    *(float*)(s2w_smem + (et ^ (cr << 4)) + (32 * t + ro) * 128) = ((om[t] >> ro) & 1u) ? v : 0.f;
                }
            }
        }
        if (c + 1 < nchunks) load_we(c + 1);              // same registers: the fetch runs under the depthwise phase
        // project-weight fragments of chunk c: issued before the depthwise arithmetic
        half8 wp[NT][2][2];
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int co = q * 32 + fr;
            const char* wrow = a.wproj + (size_t)(co < a.Cout ? co : 0) * a.mid * 4;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int kg = min(4 * c + 2 * s + hb, a.mid / 8 - 1);
                const bool v = co < a.Cout && (4 * c + 2 * s + hb) * 8 < a.mid;
                const half8 t0 = *(const half8*)(wrow + kg * 32), t1 = *(const half8*)(wrow + kg * 32 + 16);
                wp[q][s][0] = v ? t0 : hz;
                wp[q][s][1] = v ? t1 : hz;
            }
        }
        s2w_fence();
        // ---- depthwise 3x3 s2 + BN + ReLU of this lane's output pixel, 8 channels per 16-k step -> MFMA A fragments ------------------------------------------------
        half8 dh[2], dl[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int cg = 32 * c + 8 * (2 * s + hb), cb = min(cg, a.mid - 8);    // channel groups beyond mid (ragged last chunk): clamped reads, zero fragments
            const f32x4 sa = *(const f32x4*)(a.s2 + cb), sb = *(const f32x4*)(a.s2 + cb + 4);
            const f32x4 ba = *(const f32x4*)(a.b2 + cb), bb = *(const f32x4*)(a.b2 + cb + 4);
            const float* wt = Wt + cb;
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int k = ky * 3 + kx;
                    unsigned tk = ta[k];
                    if (NT > 1) asm volatile("" : "+v"(tk));      // <2, 2>: the 36 swizzled tap addresses are re-derived per use (hoisted out of the chunk loop they went to scratch)
                    const f32x4 v0 = *(const f32x4*)(s2w_smem + (tk ^ ((4 * s) << 4))), v1 = *(const f32x4*)(s2w_smem + (tk ^ ((4 * s + 1) << 4)));
                    const f32x4 w0 = *(const f32x4*)(wt + k * a.mid), w1 = *(const f32x4*)(wt + k * a.mid + 4);
#pragma unroll
                    for (int q = 0; q < 4; ++q) { acc[q] = fmaf(v0[q], w0[q], acc[q]); acc[4 + q] = fmaf(v1[q], w1[q], acc[4 + q]); }
                    if (NT > 1 && kx == 2) __builtin_amdgcn_sched_barrier(0);    // <2, 2>: at most one tap row (12 ds_read_b128 = 48 registers) in flight beside the 64 accumulators
                }
            half8 h8, l8;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float v = fmaxf(acc[q] * (q < 4 ? sa[q & 3] : sb[q & 3]) + (q < 4 ? ba[q & 3] : bb[q & 3]), 0.f);
                _Float16 h, l;
                smirk_split1(v, h, l);
                h8[q] = h; l8[q] = l;
            }
            dh[s] = cg < a.mid ? h8 : hz;
            dl[s] = cg < a.mid ? l8 : hz;
        }
        s2w_fence();                                      // E is read: the next chunk's expand (or the epilogue) may overwrite it
        // ---- project, accumulate over chunks ---------------------------------------------------------------------------------------------------------------
#pragma unroll
        for (int q = 0; q < NT; ++q)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                pacc[q][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh[s], wp[q][s][0], pacc[q][0], 0, 0, 0);
                pacc[q][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh[s], wp[q][s][1], pacc[q][1], 0, 0, 0);
                pacc[q][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dl[s], wp[q][s][0], pacc[q][1], 0, 0, 0);
            }
    }

    // ---- epilogue: bn3, per-wave 32 x 32 transposes through the wave's own E region, whole 8-channel split16 groups to HBM -----------------------------------
    {
        float* tb = (float*)(s2w_smem + ebase);           // 32 rows x 36 floats
        char* ob = a.out + (size_t)b * a.Ho * a.Wo * a.Cout * 4;
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int co = q * 32 + fr;
            const float s3 = co < a.Cout ? a.s3[co] : 0.f, b3 = co < a.Cout ? a.b3[co] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) tb[mfma32_row(r, lane) * 36 + fr] = (pacc[q][0][r] + pacc[q][1][r] * (1.0f / 2048.0f)) * s3 + b3;
            s2w_fence();
#pragma unroll
            for (int it = 0; it < 2; ++it) {              // 32 rows x 4 groups = 128 items over 64 lanes
                const int item = it * 64 + lane, row = item >> 2, g8 = q * 4 + (item & 3);
                int py, px;
                s2w_out_px(row, py, px);
                const int oy = oy0 + py, ox = ox0 + px;
                if (oy < a.Ho && ox < a.Wo && g8 * 8 < a.Cout) {
                    float v[8];
                    *(f32x4*)v = *(const f32x4*)(tb + row * 36 + (item & 3) * 8);
                    *(f32x4*)(v + 4) = *(const f32x4*)(tb + row * 36 + (item & 3) * 8 + 4);
                    half8 hi, lo;
                    rng.see8(v);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        _Float16 h, l;
                        smirk_split1(v[k], h, l);
                        hi[k] = h; lo[k] = l;
                    }
                    char* o = ob + ((size_t)oy * a.Wo + ox) * a.Cout * 4 + g8 * 32;
                    *(half8*)o = hi;
                    *(half8*)(o + 16) = lo;
                }
            }
            s2w_fence();
        }
    }
    rng.commit();
}

/* 1 if smirk_mbconv_s2_split16 serves this stride-2 InvertedResidual block: (ceil(Cin / 16), ceil(Cout / 32)) = (1, 1) | (2, 2), mid <= 96 */
extern "C" int smirk_mbconv_s2_supported(int Cin, int mid, int Cout) {
    if (Cin <= 0 || mid <= 0 || Cout <= 0 || Cin % 8 || mid % 8 || Cout % 8 || mid > S2W_MAX_MID) return 0;
    const int ks = (Cin + 15) / 16, nt = (Cout + 31) / 32;
    return (ks == 1 && nt == 1) || (ks == 2 && nt == 2);
}

template <int KS, int NT>
static int s2w_launch(const MBS2Args& a, unsigned grid, size_t lds, hipStream_t st) {
    if (const int rc = smirk_raise_dynamic_lds((const void*)mbconv_s2_wave_kernel<KS, NT>, 80 * 1024)) return rc;
    if (g_smirk_prof_on) {
        char nm[64];
        snprintf(nm, sizeof(nm), "mbconv_s2_wave_kernel<%d,%d>", KS, NT);
        smirk_prof_next_mbconv(nm, (double)a.B * a.H * a.W, (double)a.B * a.Ho * a.Wo, a.Cin, a.mid, a.Cout, true, false);
    }
    SMIRK_LAUNCH((mbconv_s2_wave_kernel<KS, NT>), dim3(grid), dim3(256), lds, st, a);
    return smirk_launch_status();
}

extern "C" int smirk_mbconv_s2_split16(const void* x, const void* wexp, const float* s1, const float* b1, const float* wdw, const float* s2,
                                       const float* b2, const void* wproj, const float* s3, const float* b3, void* out, int B, int H, int W,
                                       int Cin, int mid, int Cout, void* stream) {
    if (!x || !wexp || !s1 || !b1 || !wdw || !s2 || !b2 || !wproj || !s3 || !b3 || !out || B <= 0 || H <= 0 || W <= 0) return SMIRK_ERR_BAD_ARG;
    if ((((uintptr_t)s2) | ((uintptr_t)b2)) & 15) return SMIRK_ERR_BAD_ARG;          // read as 16-byte vectors
    if (!smirk_mbconv_s2_supported(Cin, mid, Cout)) return SMIRK_ERR_UNSUPPORTED;
    MBS2Args a;
    a.x = (const char*)x; a.wexp = (const char*)wexp; a.s1 = s1; a.b1 = b1; a.wdw = wdw; a.s2 = s2; a.b2 = b2;
    a.wproj = (const char*)wproj; a.s3 = s3; a.b3 = b3; a.out = (char*)out;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.mid = mid; a.Cout = Cout;
    a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2;
    a.pt = smirk_same_pad_lead(H, 2); a.pl = smirk_same_pad_lead(W, 2);
    a.tiles_x = (a.Wo + 7) / 8; a.tiles_y = (a.Ho + 3) / 4;
    const size_t ntiles = (size_t)B * a.tiles_x * a.tiles_y;
    if (ntiles > 0x7fffffffu / 4 || (size_t)H * W * Cin * 4 > 0x7fffffffu) return SMIRK_ERR_UNSUPPORTED;   // 32-bit tile ids and in-image byte offsets
    a.ntiles = (int)ntiles;
    const size_t lds = (size_t)4 * S2W_EB + smirk_align_up((size_t)9 * mid * 4, 16);
    const unsigned grid = (unsigned)((ntiles + 3) / 4);
    const int ks = (Cin + 15) / 16;
    if (ks == 1) return s2w_launch<1, 1>(a, grid, lds, (hipStream_t)stream);
    return s2w_launch<2, 2>(a, grid, lds, (hipStream_t)stream);
}
