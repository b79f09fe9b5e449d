// The trainer's visualisation sheet (reference: base_trainer.py:130-162 save_visualizations, utils.py:65-90; include/smirk_visual.h): fp32 NCHW
// panels -> one uint8 [H][W][3] sheet, every column torchvision's make_grid of its panel.  The law of every function below is restated in numpy float32 in
// tests/visual_law.py; this unit is compiled with -ffp-contract=off so that every product and sum rounds as written there.
//
//   visual_clear_kernel   zeroes the overlay map [B][S][S], 16 bytes per lane
//   visual_dots_kernel    one lane per (layer, frame, point): atomic OR of the layer's bit into the five pixels of a radius-1 disc
//   visual_sheet_kernel   one lane per 16 consecutive sheet bytes: column lookup, grid geometry, nearest resample, blend, overlay, quantisation, one vector store
// All streaming.  The column descriptors are kernel arguments; the sheet kernel walks them with a wave-uniform index, so a descriptor field is a scalar load and no
// private array is indexed dynamically (the library has no scratch instruction: tests/test_isa_cpu.py).
#include "common.h"
#include "../../include/smirk_visual.h"

#define VISUAL_SLOTS 6                     // 16 bytes starting at any channel touch exactly six pixels

struct VisualSheetArgs {
    SmirkVisualColumn col[SMIRK_VISUAL_MAX_COLUMNS];
    int32_t start[SMIRK_VISUAL_MAX_COLUMNS + 1];      // first sheet x of every column; start[ncols] = W
    int32_t count[SMIRK_VISUAL_MAX_COLUMNS];          // images of the column
    int32_t xmaps[SMIRK_VISUAL_MAX_COLUMNS];
    float fy[SMIRK_VISUAL_MAX_COLUMNS], fx[SMIRK_VISUAL_MAX_COLUMNS];     // float32(Hs / S), float32(Ws / S)
    int32_t ncols, B, S, H, W, bgr;
    uint32_t magic;                                   // ceil(2^32 / (S + 2)): n / (S + 2) = umulhi(n, magic) for n (S + 2) < 2^32
    uint32_t npixels, nchunks;
};

struct VisualGeometry { int32_t H, W; size_t bytes; int32_t start[SMIRK_VISUAL_MAX_COLUMNS + 1], count[SMIRK_VISUAL_MAX_COLUMNS], xmaps[SMIRK_VISUAL_MAX_COLUMNS]; };

static bool visual_size_ok(int S) { return S >= SMIRK_VISUAL_MIN_SIZE && S <= SMIRK_VISUAL_MAX_SIZE; }

// SMIRK_OK and the geometry, or the refusal the size and the sheet entry share
static int visual_geometry(const SmirkVisualColumn* cols, int ncols, int B, int S, VisualGeometry& G) {
    if (!cols || ncols < 1 || ncols > SMIRK_VISUAL_MAX_COLUMNS || B <= 0) return SMIRK_ERR_BAD_ARG;
    int marked = 0;
    for (int c = 0; c < ncols; ++c) {
        const SmirkVisualColumn& d = cols[c];
        if ((d.channels != 1 && d.channels != 3) || (d.nsrc != 1 && d.nsrc != 4) || d.Hs <= 0 || d.Ws <= 0 || d.nrow <= 0) return SMIRK_ERR_BAD_ARG;
        if (d.nsrc == 4 && d.nrow % 4 != 0) return SMIRK_ERR_BAD_ARG;
        if (d.landmarks && (d.nsrc != 1 || ++marked > 1)) return SMIRK_ERR_BAD_ARG;
    }
    if (!visual_size_ok(S)) return SMIRK_ERR_UNSUPPORTED;
    const int64_t cell = S + SMIRK_VISUAL_PADDING;
    int64_t H = -1, W = 0;
    for (int c = 0; c < ncols; ++c) {
        const SmirkVisualColumn& d = cols[c];
        const int64_t n = d.nsrc == 4 ? (int64_t)B * d.nrow : B;
        const int64_t xm = d.nrow < n ? d.nrow : n, ym = (n + xm - 1) / xm;
        const int64_t h = n == 1 ? S : ym * cell + SMIRK_VISUAL_PADDING, w = n == 1 ? S : xm * cell + SMIRK_VISUAL_PADDING;
        if (h >= (1ll << 20) || W + w >= (1ll << 20)) return SMIRK_ERR_UNSUPPORTED;      // keeps n (S + 2) < 2^32 for the kernel's division by S + 2
        if (H >= 0 && h != H) return SMIRK_ERR_UNSUPPORTED;
        H = h;
        G.start[c] = (int32_t)W; G.count[c] = (int32_t)n; G.xmaps[c] = (int32_t)xm;
        W += w;
    }
    G.start[ncols] = (int32_t)W;
    if ((double)H * (double)W * 3.0 >= 2147483648.0 - 16.0) return SMIRK_ERR_UNSUPPORTED;
    G.H = (int32_t)H; G.W = (int32_t)W;
    G.bytes = smirk_align_up((size_t)H * (size_t)W * 3, 16);
    return SMIRK_OK;
}

extern "C" int smirk_visual_abi_version(void) { return SMIRK_VISUAL_ABI_VERSION; }

extern "C" int smirk_visual_sheet_size(const SmirkVisualColumn* cols, int ncols, int B, int S, int32_t* H, int32_t* W, size_t* bytes) {
    if (!H || !W || !bytes) return SMIRK_ERR_BAD_ARG;
    VisualGeometry G;
    const int rc = visual_geometry(cols, ncols, B, S, G);
    if (rc != SMIRK_OK) return rc;
    *H = G.H; *W = G.W; *bytes = G.bytes;
    return SMIRK_OK;
}

extern "C" size_t smirk_visual_workspace_bytes(int B, int S) {
    if (B <= 0 || !visual_size_ok(S)) return 0;
    return smirk_align_up((size_t)B * S * S, 256);
}

// ---- the overlay map ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void visual_clear_kernel(uint4* __restrict__ map, uint32_t nvec) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nvec) map[i] = make_uint4(0u, 0u, 0u, 0u);
}

// blockIdx.y = layer: the layer's pointer and counts are scalar loads from the kernel arguments
__global__ __launch_bounds__(256) void visual_dots_kernel(SmirkVisualDots dots, int B, int S, float centre, uint32_t* __restrict__ map) {
    const int layer = blockIdx.y;
    const float* lm = dots.lm[layer];
    const int rows = dots.rows[layer], npts = dots.npts[layer];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (!lm || i >= (uint32_t)B * (uint32_t)npts) return;
    const uint32_t b = i / (uint32_t)npts, k = i - b * (uint32_t)npts;
    const float* p = lm + ((size_t)b * rows + k) * 2;
    const float px = p[0] * centre + centre, py = p[1] * centre + centre;           // utils.py:68, two roundings each
    if (!(fabsf(px) < 1.0e9f) || !(fabsf(py) < 1.0e9f)) return;                      // non-finite: skipped; anything this far out cannot reach the cell either
    const int cx = (int)px, cy = (int)py;                                            // int(): toward zero
    const uint32_t bit = 1u << layer;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int x = cx + (t == 1 ? -1 : t == 2 ? 1 : 0), y = cy + (t == 3 ? -1 : t == 4 ? 1 : 0);
        if (x < 0 || y < 0 || x >= S || y >= S) continue;
        const size_t at = ((size_t)b * S + y) * S + x;
        atomicOr(map + (at >> 2), bit << (8u * (uint32_t)(at & 3)));
    }
}

// ---- the sheet ---------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t visual_level(float v) {                          // base_trainer.py:157-159: * 255.0, clip, astype(uint8); NaN -> 0
    const float t = v * 255.0f;
    return t == t ? (uint32_t)fminf(fmaxf(t, 0.0f), 255.0f) : 0u;
}

// the three sheet bytes (byte 0 in bits 0-7) of pixel (xl, y) of a column; 0 on padding
__device__ __forceinline__ uint32_t visual_pixel(const SmirkVisualColumn& d, int count, int xmaps, float fy, float fx, int B, int S, uint32_t magic, int bgr,
                                                 uint32_t xl, uint32_t y, const uint8_t* __restrict__ overlay) {
    uint32_t n = 0, iy = y, ix = xl, cx = 0, cy = 0;
    if (count != 1) {
        if (y < SMIRK_VISUAL_PADDING || xl < SMIRK_VISUAL_PADDING) return 0u;
        const uint32_t gy = y - SMIRK_VISUAL_PADDING, gx = xl - SMIRK_VISUAL_PADDING, cell = (uint32_t)S + SMIRK_VISUAL_PADDING;
        cy = __umulhi(gy, magic); cx = __umulhi(gx, magic);
        iy = gy - cy * cell; ix = gx - cx * cell;
        n = cy * (uint32_t)xmaps + cx;
        if (iy >= (uint32_t)S || ix >= (uint32_t)S || n >= (uint32_t)count) return 0u;
    }
    const int sy = min((int)floorf((float)iy * fy), d.Hs - 1), sx = min((int)floorf((float)ix * fx), d.Ws - 1);     // F.interpolate, mode nearest
    const float* s = d.src[0];
    uint32_t img = n;
    if (d.nsrc == 4) {                                                               // xmaps = 4 Ke: row = b, cell = (ke, which)
        const uint32_t which = cx & 3u;
        s = which == 0 ? d.src[0] : which == 1 ? d.src[1] : which == 2 ? d.src[2] : d.src[3];
        img = (cx >> 2) * (uint32_t)B + cy;
    }
    const size_t plane = (size_t)d.Hs * d.Ws, step = d.channels == 3 ? plane : 0;
    const size_t at = (size_t)img * d.channels * plane + (size_t)sy * d.Ws + sx;
    float r = s[at], g = s[at + step], b = s[at + 2 * step];
    if (d.blend) {                                                                   // base_trainer.py:134-135
        const float* q = d.blend;
        const float r1 = q[at] * d.w_blend, g1 = q[at + step] * d.w_blend, b1 = q[at + 2 * step] * d.w_blend;
        r = r * d.w_src + r1; g = g * d.w_src + g1; b = b * d.w_src + b1;
    }
    if (d.landmarks) {
        const uint32_t o = overlay[((size_t)n * S + iy) * S + ix];
        if (o) {                                                                     // the highest layer drawn here
            const uint32_t top = 31u - (uint32_t)__clz((int)o);
            r = top >= 1u ? 1.0f : 0.0f; g = (top == 0u || top == 3u) ? 1.0f : 0.0f; b = top >= 2u ? 1.0f : 0.0f;
        } else {                                                                     // utils.py:72 then :88
            r = (float)visual_level(r) / 255.0f; g = (float)visual_level(g) / 255.0f; b = (float)visual_level(b) / 255.0f;
        }
    }
    const uint32_t lr = visual_level(r), lg = visual_level(g), lb = visual_level(b);
    return bgr ? (lb | (lg << 8) | (lr << 16)) : (lr | (lg << 8) | (lb << 16));
}

__global__ __launch_bounds__(256) void visual_sheet_kernel(VisualSheetArgs a, const uint8_t* __restrict__ overlay, uint4* __restrict__ sheet) {
    const uint32_t chunk = blockIdx.x * 256u + threadIdx.x;
    if (chunk >= a.nchunks) return;
    const uint32_t byte0 = chunk * 16u, p0 = byte0 / 3u, ch0 = byte0 - p0 * 3u;
    uint32_t x[VISUAL_SLOTS], y[VISUAL_SLOTS], rgb[VISUAL_SLOTS];
    y[0] = p0 / (uint32_t)a.W; x[0] = p0 - y[0] * (uint32_t)a.W;
#pragma unroll
    for (int j = 1; j < VISUAL_SLOTS; ++j) {                                         // W >= SMIRK_VISUAL_MIN_SIZE > VISUAL_SLOTS: at most one wrap
        const bool wrap = x[j - 1] + 1u == (uint32_t)a.W;
        x[j] = wrap ? 0u : x[j - 1] + 1u; y[j] = y[j - 1] + (wrap ? 1u : 0u);
    }
#pragma unroll
    for (int j = 0; j < VISUAL_SLOTS; ++j) {
        rgb[j] = 0u;
        if (p0 + (uint32_t)j >= a.npixels) x[j] = 0xffffffffu;                       // the tail after the last pixel: in no column, stays 0
    }
    for (int c = 0; c < a.ncols; ++c) {                                              // uniform: every a.*[c] is a scalar load
        const uint32_t xs = (uint32_t)a.start[c], xe = (uint32_t)a.start[c + 1];
        bool any = false;
#pragma unroll
        for (int j = 0; j < VISUAL_SLOTS; ++j) any |= x[j] >= xs && x[j] < xe;
        if (!__any(any)) continue;
#pragma unroll
        for (int j = 0; j < VISUAL_SLOTS; ++j)
            if (x[j] >= xs && x[j] < xe)
                rgb[j] = visual_pixel(a.col[c], a.count[c], a.xmaps[c], a.fy[c], a.fx[c], a.B, a.S, a.magic, a.bgr, x[j] - xs, y[j], overlay);
    }
    // eighteen bytes in five words, then the sixteen that start at channel ch0
    const uint32_t w0 = rgb[0] | (rgb[1] << 24), w1 = (rgb[1] >> 8) | (rgb[2] << 16), w2 = (rgb[2] >> 16) | (rgb[3] << 8), w3 = rgb[4] | (rgb[5] << 24),
                   w4 = rgb[5] >> 8;
    sheet[chunk] = make_uint4(__builtin_amdgcn_alignbyte(w1, w0, ch0), __builtin_amdgcn_alignbyte(w2, w1, ch0), __builtin_amdgcn_alignbyte(w3, w2, ch0),
                              __builtin_amdgcn_alignbyte(w4, w3, ch0));
}

// ---- entries -----------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int smirk_visual_dots(const SmirkVisualDots* dots, int B, int S, float centre, void* ws, size_t ws_bytes, void* stream) {
    if (!dots || !ws || B <= 0 || !(fabsf(centre) <= 3.0e38f) || ((uintptr_t)ws & 255u)) return SMIRK_ERR_BAD_ARG;
    int most = 0;
    for (int l = 0; l < SMIRK_VISUAL_LAYERS; ++l) {
        if (dots->rows[l] < 0 || dots->npts[l] < 0 || dots->npts[l] > dots->rows[l] || ((uintptr_t)dots->lm[l] & 3u)) return SMIRK_ERR_BAD_ARG;
        if (dots->lm[l] && dots->npts[l] > most) most = dots->npts[l];
    }
    if (!visual_size_ok(S) || most > SMIRK_VISUAL_MAX_POINTS) return SMIRK_ERR_UNSUPPORTED;
    const size_t need = smirk_visual_workspace_bytes(B, S);
    if ((double)B * most >= 2147483648.0 || need / 16 >= (1ull << 32)) return SMIRK_ERR_UNSUPPORTED;
    if (ws_bytes < need) return SMIRK_ERR_WORKSPACE;
    const uint32_t nvec = (uint32_t)(need / 16);
    smirk_prof_next(nullptr, 0.0, (double)need);
    SMIRK_LAUNCH(visual_clear_kernel, dim3((nvec + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, (uint4*)ws, nvec);
    if (most > 0) {
        double pts = 0.0;
        for (int l = 0; l < SMIRK_VISUAL_LAYERS; ++l) pts += dots->lm[l] ? (double)B * dots->npts[l] : 0.0;
        smirk_prof_next(nullptr, 4.0 * pts, pts * (8.0 + 5.0 * 4.0));
        SMIRK_LAUNCH(visual_dots_kernel, dim3(((uint32_t)B * (uint32_t)most + 255u) / 256u, SMIRK_VISUAL_LAYERS), dim3(256), 0, (hipStream_t)stream, *dots, B, S, centre,
                     (uint32_t*)ws);
    }
    return smirk_launch_status();
}

extern "C" int smirk_visual_sheet(const SmirkVisualColumn* cols, int ncols, int B, int S, int bgr, const void* ws, size_t ws_bytes, uint8_t* sheet,
                                  size_t sheet_bytes, void* stream) {
    VisualSheetArgs a = {};
    VisualGeometry G;
    const int rc = visual_geometry(cols, ncols, B, S, G);
    if (rc != SMIRK_OK) return rc;
    if (!sheet || ((uintptr_t)sheet & 255u)) return SMIRK_ERR_BAD_ARG;
    bool marked = false;
    double read = 0.0;
    for (int c = 0; c < ncols; ++c) {
        const SmirkVisualColumn& d = cols[c];
        for (int k = 0; k < d.nsrc; ++k)
            if (!d.src[k] || ((uintptr_t)d.src[k] & 3u)) return SMIRK_ERR_BAD_ARG;
        if (d.blend && (d.nsrc != 1 || d.landmarks || ((uintptr_t)d.blend & 3u))) return SMIRK_ERR_BAD_ARG;
        if (d.blend && !(fabsf(d.w_src) <= 3.0e38f && fabsf(d.w_blend) <= 3.0e38f)) return SMIRK_ERR_BAD_ARG;
        marked |= d.landmarks != 0;
        read += (double)G.count[c] * S * S * (4.0 * d.channels * (d.blend ? 2 : 1) + (d.landmarks ? 1.0 : 0.0));
        a.col[c] = d;
        a.col[c].landmarks = d.landmarks != 0;
        a.count[c] = G.count[c]; a.xmaps[c] = G.xmaps[c];
        a.fy[c] = (float)d.Hs / (float)S; a.fx[c] = (float)d.Ws / (float)S;
    }
    if (marked && (!ws || ((uintptr_t)ws & 255u))) return SMIRK_ERR_BAD_ARG;
    if (sheet_bytes < G.bytes || (marked && ws_bytes < smirk_visual_workspace_bytes(B, S))) return SMIRK_ERR_WORKSPACE;
    for (int c = 0; c <= ncols; ++c) a.start[c] = G.start[c];
    a.ncols = ncols; a.B = B; a.S = S; a.H = G.H; a.W = G.W; a.bgr = bgr != 0;
    const uint32_t cell = (uint32_t)S + SMIRK_VISUAL_PADDING;
    a.magic = (uint32_t)(((1ull << 32) + cell - 1) / cell);
    a.npixels = (uint32_t)G.H * (uint32_t)G.W;
    a.nchunks = (uint32_t)(G.bytes / 16);
    smirk_prof_next(nullptr, 0.0, read + (double)G.bytes);
    SMIRK_LAUNCH(visual_sheet_kernel, dim3((a.nchunks + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a, (const uint8_t*)ws, (uint4*)sheet);
    return smirk_launch_status();
}
