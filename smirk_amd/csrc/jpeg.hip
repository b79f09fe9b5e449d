// Baseline JPEG encoding of finished uint8 pictures (reference: base_trainer.py:162 cv2.imwrite of the sheet, demo_video.py:211-214 cv2.VideoWriter of every grid;
// include/smirk_jpeg.h): uint8 [B][H][W][3] -> B complete JFIF files back to back.  Every step is integer arithmetic restated in tests/jpeg_law.py;
// the output equals the law's byte for byte.
//
//   jpeg_dct_kernel            one wave per 16 x 16 MCU: 64 aligned 16-byte loads (edge clamp) to LDS, colour conversion and chroma mean (one 2 x 2 quad per lane), the
//                              six 8 x 8 DCTs as two passes through LDS (one output per lane and block), quantisation, int16 zigzag coefficients stored as 48 vectors
//   jpeg_entropy_kernel<false> one lane per restart interval: the interval's bits are built in a 64-bit accumulator and only counted (stuffing included)
//   jpeg_scan_kernel           one block: interval sizes -> byte offsets, every file's header length added in front of its first interval
//   jpeg_entropy_kernel<true>  the same walk again, this time storing the bytes, then RSTm or EOI; B more blocks write the headers and the span table
// The Huffman tables are built at compile time from Annex K's BITS / HUFFVAL lists (the same lists go into the DHT segments) and are read from LDS; no kernel
// indexes a private array dynamically (the library has no scratch instruction: tests/test_isa_cpu.py).  Nothing here writes split-fp16.
#include "common.h"
#include "../../include/smirk_jpeg.h"

#define JPEG_PASS1_SHIFT 9

// ---- the constants of the law -------------------------------------------------------------------------------------------------------------------------------
static constexpr uint8_t JPEG_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static constexpr uint8_t JPEG_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
struct JpegHuffSpec { uint8_t bits[16]; uint8_t vals[162]; int n; };
static constexpr JpegHuffSpec JPEG_DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
static constexpr JpegHuffSpec JPEG_DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
static constexpr JpegHuffSpec JPEG_AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177, 193, 21,  82,  209, 240, 36,
     51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,
     84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147,
     148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201,
     202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    162};
static constexpr JpegHuffSpec JPEG_AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193, 9,   35,  51,  82,  240, 21,
     98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,
     83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138,
     146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199,
     200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    162};

// what the kernels read: T[u][x] of the DCT, natural index -> zigzag position, and per Huffman symbol  code | length << 16  (Annex C; 0 where the table has no code)
struct JpegDeviceTables {
    int32_t dct[64];
    uint32_t unzig[64];
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
static constexpr void jpeg_fill_codes(uint32_t* tab, const JpegHuffSpec& s) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) tab[s.vals[k++]] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
}
static constexpr JpegDeviceTables jpeg_build_tables() {
    constexpr int K[8] = {8192, 8035, 7568, 6811, 5793, 4551, 3135, 1598};             // round(2^13 cos(k pi / 16)): tests/jpeg_law.py DCT_K
    JpegDeviceTables t{};
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x) {
            int a = (2 * x + 1) * u % 32;
            if (a > 16) a = 32 - a;
            t.dct[u * 8 + x] = u == 0 ? K[4] : (a < 8 ? K[a] : -K[16 - a]);
        }
    for (int z = 0; z < 64; ++z) t.unzig[JPEG_ZIGZAG[z]] = (uint32_t)z;
    jpeg_fill_codes(t.dc[0], JPEG_DC_LUMA); jpeg_fill_codes(t.dc[1], JPEG_DC_CHROMA);
    jpeg_fill_codes(t.ac[0], JPEG_AC_LUMA); jpeg_fill_codes(t.ac[1], JPEG_AC_CHROMA);
    return t;
}
__constant__ JpegDeviceTables jpeg_tables = jpeg_build_tables();

// ---- geometry shared by the queries and the entry ----------------------------------------------------------------------------------------------------------
struct JpegGeometry {
    uint32_t mx, my, nmcu;       // MCUs of a picture
    uint32_t Re, nint;           // effective restart interval, intervals of a picture
    uint64_t total_mcu, total_int, img_bytes, max_bytes;
    size_t coef_bytes, sizes_bytes, ws_bytes;
};

static bool jpeg_geometry(int B, int H, int W, int R, JpegGeometry& g) {
    if (B <= 0 || H < 1 || H > SMIRK_JPEG_MAX_DIM || W < 1 || W > SMIRK_JPEG_MAX_DIM || R < 1) return false;
    g.mx = ((uint32_t)W + 15u) / 16u; g.my = ((uint32_t)H + 15u) / 16u; g.nmcu = g.mx * g.my;               // at most 4096^2
    g.Re = (uint32_t)R < g.nmcu ? (uint32_t)R : g.nmcu;
    if (g.Re > 65535u) g.Re = 65535u;
    g.nint = (g.nmcu + g.Re - 1u) / g.Re;
    g.total_mcu = (uint64_t)B * g.nmcu; g.total_int = (uint64_t)B * g.nint;
    g.img_bytes = (uint64_t)B * (uint64_t)H * (uint64_t)W * 3u;
    g.max_bytes = (uint64_t)B * (SMIRK_JPEG_HEADER_BYTES + (uint64_t)g.nint * (2ull * g.Re * SMIRK_JPEG_MCU_MAX_BYTES + 2ull));
    g.coef_bytes = smirk_align_up((size_t)g.total_mcu * 768, 256);
    g.sizes_bytes = smirk_align_up((size_t)g.total_int * 4, 256);
    g.ws_bytes = g.coef_bytes + 2 * g.sizes_bytes;
    return true;
}

extern "C" int smirk_jpeg_abi_version(void) { return SMIRK_JPEG_ABI_VERSION; }

extern "C" size_t smirk_jpeg_workspace_bytes(int B, int H, int W, int R) {
    JpegGeometry g;
    if (!jpeg_geometry(B, H, W, R, g) || g.img_bytes >= (1ull << 31) || g.max_bytes >= (1ull << 31)) return 0;
    return g.ws_bytes;
}

extern "C" size_t smirk_jpeg_max_bytes(int B, int H, int W, int R) {
    JpegGeometry g;
    return jpeg_geometry(B, H, W, R, g) ? (size_t)g.max_bytes : 0;
}

extern "C" int smirk_jpeg_quant_tables(int quality, uint8_t qt[2][64]) {
    if (!qt || quality < 1 || quality > 100) return SMIRK_ERR_BAD_ARG;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = (JPEG_BASE[t][i] * s + 50) / 100;
            qt[t][i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    return SMIRK_OK;
}

// ---- coefficients --------------------------------------------------------------------------------------------------------------------------------------------
struct JpegDctArgs {
    uint8_t q[2][64];            // natural order
    int32_t H, W, bgr;
    uint32_t mx, nmcu, total_mcu, img_bytes;
};

__device__ __forceinline__ int jpeg_quantise(int c, uint32_t q, uint32_t magic) {          // sign(c) * (((|c| >> 18) + q) / (2 q)); magic = ceil(2^32 / (2 q)), exact below 2^23
    const uint32_t n = __umulhi(((uint32_t)abs(c) >> 18) + q, magic);
    return c < 0 ? -(int)n : (int)n;
}

__global__ __launch_bounds__(256) void jpeg_dct_kernel(JpegDctArgs a, const uint8_t* __restrict__ img, uint4* __restrict__ coef) {
    __shared__ __align__(16) uint8_t s_pix[4][16 * 64];          // per wave: 16 rows of four aligned 16-byte chunks
    __shared__ __align__(16) int32_t s_x[4][6 * 64];             // level-shifted samples of the six blocks
    __shared__ __align__(16) int32_t s_p[4][6 * 64];             // pass 1
    __shared__ __align__(16) int16_t s_z[4][6 * 64];             // quantised, zigzag
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, u = lane & 7u, v = lane >> 3;
    int tu[8], tv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { tu[k] = jpeg_tables.dct[u * 8 + k]; tv[k] = jpeg_tables.dct[v * 8 + k]; }
    const uint32_t zpos = jpeg_tables.unzig[lane];
    const uint32_t q0 = a.q[0][lane], q1 = a.q[1][lane];
    const uint32_t m0 = (uint32_t)(((1ull << 32) + 2u * q0 - 1u) / (2u * q0)), m1 = (uint32_t)(((1ull << 32) + 2u * q1 - 1u) / (2u * q1));
    const uint32_t H = (uint32_t)a.H, W = (uint32_t)a.W;

    for (uint32_t base = blockIdx.x * 4u; base < a.total_mcu; base += gridDim.x * 4u) {         // uniform over the block: every wave reaches every barrier
        const uint32_t mcu = base + wave;
        const bool live = mcu < a.total_mcu;
        const uint32_t b = mcu / a.nmcu, r = mcu - b * a.nmcu, j = r / a.mx, i = r - j * a.mx, y0 = j * 16u, x0 = i * 16u;
        if (live) {                                                                             // lane = (row, chunk): the aligned chunks that cover the row's 48 bytes
            const uint32_t row = lane >> 2, chunk = lane & 3u, yc = min(y0 + row, H - 1u);
            const uint32_t start = ((b * H + yc) * W + x0) * 3u, at = (start & ~15u) + chunk * 16u;      // img_bytes < 2^31
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (at + 16u <= a.img_bytes) {
                w = *(const uint4*)(img + at);
            } else if (at < a.img_bytes) {                                                      // the chunk that holds the batch's last bytes
                uint32_t p[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (uint32_t k = 0; k < 16u; ++k)
                    if (at + k < a.img_bytes) p[k >> 2] |= (uint32_t)img[at + k] << (8u * (k & 3u));
                w = make_uint4(p[0], p[1], p[2], p[3]);
            }
            *(uint4*)(s_pix[wave] + row * 64u + chunk * 16u) = w;
        }
        __syncthreads();
        if (live) {                                                                             // lane = one 2 x 2 quad
            const uint32_t cy = lane >> 3, cx = lane & 7u;
            int cbs = 2, crs = 2;
#pragma unroll
            for (uint32_t dy = 0; dy < 2u; ++dy) {
                const uint32_t py = 2u * cy + dy, yc = min(y0 + py, H - 1u);
                const uint32_t off = (((b * H + yc) * W + x0) * 3u) & 15u;
#pragma unroll
                for (uint32_t dx = 0; dx < 2u; ++dx) {
                    const uint32_t px = 2u * cx + dx, xg = min(x0 + px, W - 1u) - x0;
                    const uint8_t* p = s_pix[wave] + py * 64u + off + 3u * xg;
                    const int c0 = p[0], g = p[1], c2 = p[2];
                    const int R = a.bgr ? c2 : c0, B = a.bgr ? c0 : c2;
                    const int Y = (19595 * R + 38470 * g + 7471 * B + 32768) >> 16;
                    const int Cb = ((-11059 * R - 21709 * g + 32768 * B + 32768) >> 16) + 128;
                    const int Cr = ((32768 * R - 27439 * g - 5329 * B + 32768) >> 16) + 128;
                    cbs += min(max(Cb, 0), 255); crs += min(max(Cr, 0), 255);
                    s_x[wave][((py >> 3) * 2u + (px >> 3)) * 64u + (py & 7u) * 8u + (px & 7u)] = Y - 128;
                }
            }
            s_x[wave][4 * 64 + lane] = (cbs >> 2) - 128;
            s_x[wave][5 * 64 + lane] = (crs >> 2) - 128;
        }
        __syncthreads();
        if (live) {                                                                             // pass 1, lane = (y, u)
#pragma unroll
            for (int blk = 0; blk < 6; ++blk) {
                const int4 lo = *(const int4*)(s_x[wave] + blk * 64 + v * 8u), hi = *(const int4*)(s_x[wave] + blk * 64 + v * 8u + 4u);
                const int s = tu[0] * lo.x + tu[1] * lo.y + tu[2] * lo.z + tu[3] * lo.w + tu[4] * hi.x + tu[5] * hi.y + tu[6] * hi.z + tu[7] * hi.w;
                s_p[wave][blk * 64 + lane] = (s + (1 << (JPEG_PASS1_SHIFT - 1))) >> JPEG_PASS1_SHIFT;
            }
        }
        __syncthreads();
        if (live) {                                                                             // pass 2 and quantisation, lane = (v, u)
#pragma unroll
            for (int blk = 0; blk < 6; ++blk) {
                int s = 0;
#pragma unroll
                for (int y = 0; y < 8; ++y) s += tv[y] * s_p[wave][blk * 64 + y * 8 + (int)u];
                int n = jpeg_quantise(s, blk < 4 ? q0 : q1, blk < 4 ? m0 : m1);
                if (lane) n = min(max(n, -1023), 1023);
                s_z[wave][blk * 64 + (int)zpos] = (int16_t)n;
            }
        }
        __syncthreads();
        if (live && lane < 48u) coef[(size_t)mcu * 48u + lane] = *(const uint4*)(s_z[wave] + lane * 8u);
    }
}

// ---- entropy coding ------------------------------------------------------------------------------------------------------------------------------------------
struct JpegScanArgs {
    uint32_t nmcu, Re, nint, total_int, B;
    uint32_t entropy_blocks;     // blocks of the emit launch that code intervals; the B after them write the headers
};
struct JpegHeader { uint8_t b[640]; };

// MSB-first bit sink: at most 27 bits per put on top of fewer than 8 pending ones.  EMIT = false only counts.
template <bool EMIT>
struct JpegSink {
    uint64_t acc;
    uint32_t nbits, pos;
    uint8_t* out;
    __device__ __forceinline__ void byte(uint32_t v) {
        if (EMIT) out[pos] = (uint8_t)v;
        ++pos;
    }
    __device__ __forceinline__ void put(uint32_t code, uint32_t len) {
        acc = (acc << len) | code;
        nbits += len;
        while (nbits >= 8u) {
            nbits -= 8u;
            const uint32_t v = (uint32_t)(acc >> nbits) & 0xffu;
            byte(v);
            if (v == 0xffu) byte(0u);
        }
    }
};

// code and magnitude bits of value v under the table entry `e` (code | length << 16) of its symbol
template <bool EMIT>
__device__ __forceinline__ void jpeg_put_value(JpegSink<EMIT>& sink, uint32_t e, int v, uint32_t size) {
    const uint32_t mag = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
    sink.put(((e & 0xffffu) << size) | mag, (e >> 16) + size);
}

template <bool EMIT>
__device__ __forceinline__ void jpeg_block(JpegSink<EMIT>& sink, const uint4* __restrict__ c, const uint32_t* dc, const uint32_t* ac, int& pred) {
    uint32_t run = 0;
#pragma unroll 1
    for (int vec = 0; vec < 8; ++vec) {
        const uint4 w = c[vec];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t word = e < 2 ? w.x : e < 4 ? w.y : e < 6 ? w.z : w.w;
            const int v = (int)(int16_t)(word >> (16 * (e & 1)));
            if (e == 0 && vec == 0) {
                const int d = v - pred;
                pred = v;
                const uint32_t size = 32u - (uint32_t)__clz(abs(d));
                jpeg_put_value(sink, dc[size], d, size);
            } else if (v == 0) {
                ++run;
            } else {
                while (run > 15u) { const uint32_t z = ac[0xf0]; sink.put(z & 0xffffu, z >> 16); run -= 16u; }
                const uint32_t size = 32u - (uint32_t)__clz(abs(v));
                jpeg_put_value(sink, ac[(run << 4) | size], v, size);
                run = 0;
            }
        }
    }
    if (run) { const uint32_t z = ac[0]; sink.put(z & 0xffffu, z >> 16); }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void jpeg_entropy_kernel(JpegScanArgs a, JpegHeader hdr, const uint4* __restrict__ coef, uint32_t* __restrict__ sizes,
                                                           const uint32_t* __restrict__ offsets, uint8_t* __restrict__ out, uint32_t* __restrict__ spans) {
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    if (EMIT && blockIdx.x >= a.entropy_blocks) {                                               // one block per file: header and span
        const uint32_t b = blockIdx.x - a.entropy_blocks, first = b * a.nint;
        const uint32_t start = offsets[first] - SMIRK_JPEG_HEADER_BYTES;
        for (uint32_t i = threadIdx.x; i < SMIRK_JPEG_HEADER_BYTES; i += 256u) out[start + i] = hdr.b[i];
        if (threadIdx.x == 0) {
            const uint32_t end = b + 1u < a.B ? offsets[first + a.nint] - SMIRK_JPEG_HEADER_BYTES : offsets[a.total_int - 1u] + sizes[a.total_int - 1u];
            spans[2u * b] = start; spans[2u * b + 1u] = end - start;
        }
        return;
    }
    for (uint32_t i = threadIdx.x; i < 32u; i += 256u) s_dc[i >> 4][i & 15u] = jpeg_tables.dc[i >> 4][i & 15u];
    for (uint32_t i = threadIdx.x; i < 512u; i += 256u) s_ac[i >> 8][i & 255u] = jpeg_tables.ac[i >> 8][i & 255u];
    __syncthreads();
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= a.total_int) return;
    const uint32_t b = idx / a.nint, k = idx - b * a.nint, first = k * a.Re, last = min(first + a.Re, a.nmcu);
    const uint4* c = coef + ((size_t)b * a.nmcu + first) * 48u;
    JpegSink<EMIT> sink;
    sink.acc = 0ull; sink.nbits = 0u; sink.out = out;
    sink.pos = EMIT ? offsets[idx] : 0u;
    int py = 0, pcb = 0, pcr = 0;
    for (uint32_t m = first; m < last; ++m) {
#pragma unroll 1
        for (int blk = 0; blk < 4; ++blk, c += 8) jpeg_block(sink, c, s_dc[0], s_ac[0], py);
        jpeg_block(sink, c, s_dc[1], s_ac[1], pcb); c += 8;
        jpeg_block(sink, c, s_dc[1], s_ac[1], pcr); c += 8;
    }
    if (sink.nbits) sink.put((1u << (8u - sink.nbits)) - 1u, 8u - sink.nbits);                 // 1-bits up to the byte boundary
    if (EMIT) {
        out[sink.pos] = 0xffu;
        out[sink.pos + 1u] = k + 1u < a.nint ? (uint8_t)(0xd0u + (k & 7u)) : (uint8_t)0xd9u;   // RSTm, or EOI after the file's last interval
    } else {
        sizes[idx] = sink.pos + 2u;
    }
}

// offsets[i] = where interval i's first byte goes: the sizes before it, and SMIRK_JPEG_HEADER_BYTES for its own file and every file before.  One block; thread t
// owns a contiguous run of intervals, the 1024 run totals are scanned in LDS.
__global__ __launch_bounds__(1024) void jpeg_scan_kernel(const uint32_t* __restrict__ sizes, uint32_t* __restrict__ offsets, uint32_t total, uint32_t nint) {
    __shared__ uint32_t s[1024];
    const uint32_t t = threadIdx.x, per = (total + 1023u) / 1024u, lo = min(t * per, total), hi = min(lo + per, total);
    uint32_t sum = 0, phase = lo % nint;                        // phase == 0: the first interval of a file
    for (uint32_t i = lo, p = phase; i < hi; ++i) {
        sum += sizes[i] + (p == 0u ? (uint32_t)SMIRK_JPEG_HEADER_BYTES : 0u);
        if (++p == nint) p = 0u;
    }
    s[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t add = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    uint32_t at = s[t] - sum;
    for (uint32_t i = lo, p = phase; i < hi; ++i) {
        if (p == 0u) at += SMIRK_JPEG_HEADER_BYTES;
        offsets[i] = at;
        at += sizes[i];
        if (++p == nint) p = 0u;
    }
}

// ---- the entry -----------------------------------------------------------------------------------------------------------------------------------------------
static size_t jpeg_segment(uint8_t* h, size_t at, uint8_t marker, const uint8_t* payload, size_t n) {
    h[at++] = 0xff; h[at++] = marker; h[at++] = (uint8_t)((n + 2) >> 8); h[at++] = (uint8_t)((n + 2) & 0xff);
    for (size_t i = 0; i < n; ++i) h[at++] = payload[i];
    return at;
}

static size_t jpeg_header(JpegHeader& hd, int H, int W, const uint8_t qt[2][64], uint32_t Re) {
    uint8_t* h = hd.b;
    uint8_t p[256];
    size_t at = 0;
    h[at++] = 0xff; h[at++] = 0xd8;
    const uint8_t app0[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    at = jpeg_segment(h, at, 0xe0, app0, 14);
    for (int t = 0; t < 2; ++t) {
        p[0] = (uint8_t)t;
        for (int z = 0; z < 64; ++z) p[1 + z] = qt[t][JPEG_ZIGZAG[z]];
        at = jpeg_segment(h, at, 0xdb, p, 65);
    }
    const uint8_t sof[15] = {8, (uint8_t)(H >> 8), (uint8_t)(H & 255), (uint8_t)(W >> 8), (uint8_t)(W & 255), 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
    at = jpeg_segment(h, at, 0xc0, sof, 15);
    const JpegHuffSpec* specs[4] = {&JPEG_DC_LUMA, &JPEG_AC_LUMA, &JPEG_DC_CHROMA, &JPEG_AC_CHROMA};
    const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        p[0] = ids[t];
        for (int i = 0; i < 16; ++i) p[1 + i] = specs[t]->bits[i];
        for (int i = 0; i < specs[t]->n; ++i) p[17 + i] = specs[t]->vals[i];
        at = jpeg_segment(h, at, 0xc4, p, 17 + (size_t)specs[t]->n);
    }
    const uint8_t dri[2] = {(uint8_t)(Re >> 8), (uint8_t)(Re & 255u)};
    at = jpeg_segment(h, at, 0xdd, dri, 2);
    const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    at = jpeg_segment(h, at, 0xda, sos, 10);
    return at;
}

extern "C" int smirk_jpeg_encode_u8(const uint8_t* img, int B, int H, int W, int bgr, const uint8_t qt[2][64], int R, void* ws, size_t ws_bytes, uint8_t* out,
                                    size_t out_bytes, uint32_t* spans, void* stream) {
    JpegGeometry g;
    if (!img || !qt || !ws || !out || !spans || !jpeg_geometry(B, H, W, R, g)) return SMIRK_ERR_BAD_ARG;
    if (((uintptr_t)img & 15u) || ((uintptr_t)out & 15u) || ((uintptr_t)ws & 255u) || ((uintptr_t)spans & 7u)) return SMIRK_ERR_BAD_ARG;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i)
            if (qt[t][i] == 0) return SMIRK_ERR_BAD_ARG;
    if (g.img_bytes >= (1ull << 31) || g.max_bytes >= (1ull << 31)) return SMIRK_ERR_UNSUPPORTED;
    if (ws_bytes < g.ws_bytes || out_bytes < g.max_bytes) return SMIRK_ERR_WORKSPACE;

    JpegDctArgs d = {};
    JpegHeader hd = {};
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) d.q[t][i] = qt[t][i];
    d.H = H; d.W = W; d.bgr = bgr != 0; d.mx = g.mx; d.nmcu = g.nmcu; d.total_mcu = (uint32_t)g.total_mcu; d.img_bytes = (uint32_t)g.img_bytes;
    if (jpeg_header(hd, H, W, qt, g.Re) != SMIRK_JPEG_HEADER_BYTES) return SMIRK_ERR_BAD_ARG;      // cannot happen: the segments above add up to the constant
    JpegScanArgs a = {};
    a.nmcu = g.nmcu; a.Re = g.Re; a.nint = g.nint; a.total_int = (uint32_t)g.total_int; a.B = (uint32_t)B;
    a.entropy_blocks = (a.total_int + 255u) / 256u;

    uint4* coef = (uint4*)ws;
    uint32_t* sizes = (uint32_t*)((uint8_t*)ws + g.coef_bytes);
    uint32_t* offsets = (uint32_t*)((uint8_t*)ws + g.coef_bytes + g.sizes_bytes);
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t groups = (d.total_mcu + 3u) / 4u, cap = (uint32_t)smirk_device_cus() * 8u;
    const double coef_io = (double)g.total_mcu * 768.0;
    smirk_prof_next(nullptr, 0.0, (double)g.img_bytes + coef_io);
    SMIRK_LAUNCH(jpeg_dct_kernel, dim3(groups < cap ? groups : cap), dim3(256), 0, st, d, img, coef);
    smirk_prof_next(nullptr, 0.0, coef_io + 4.0 * (double)g.total_int);
    SMIRK_LAUNCH(jpeg_entropy_kernel<false>, dim3(a.entropy_blocks), dim3(256), 0, st, a, hd, (const uint4*)coef, sizes, (const uint32_t*)offsets, out, spans);
    smirk_prof_next(nullptr, 0.0, 12.0 * (double)g.total_int);
    SMIRK_LAUNCH(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)sizes, offsets, a.total_int, a.nint);
    smirk_prof_next(nullptr, 0.0, coef_io + 8.0 * (double)g.total_int);
    SMIRK_LAUNCH(jpeg_entropy_kernel<true>, dim3(a.entropy_blocks + (uint32_t)B), dim3(256), 0, st, a, hd, (const uint4*)coef, sizes, (const uint32_t*)offsets, out, spans);
    return smirk_launch_status();
}
