// The trainer's batch preparation (reference: datasets/base_dataset.py:124-215 prepare_data; include/smirk_data.h): decoded uint8 BGR frames of
// mixed resolutions + landmark arrays -> img, landmarks_fan, flag_landmarks_fan, landmarks_mp, mask, img_mica on the device.  The law of every function below is
// restated in numpy integers / float64 in tests/data_law.py; this unit is compiled with -ffp-contract=off so that every product and sum rounds as written there.
//
//   data_params_kernel      one workgroup per frame: crop similarity, every draw and coin (data_rng.h), ShiftScaleRotate matrix + inverse, ArcFace similarity,
//                           the landmark outputs and the truncated hull points
//   data_crop_kernel        one thread per output pixel: the 224 x 224 crop (arithmetic of warp_affine_u8_kernel, video.hip) and the 112 x 112 MICA warp
//   data_stats_kernel       one workgroup per frame: point-wise lookup table (needs the mean grey), CLAHE tile histograms in LDS -> 64 x 256 table bytes
//   data_colour_kernel      one thread per pixel: lookup table, saturation, hue, CLAHE apply, RGB shift
//   data_blur_noise_kernel  one thread per pixel: box blur (reflect-101), Gaussian noise
//   data_resample_kernel    one thread per pixel: ShiftScaleRotate of image and mask, / 255, HWC -> NCHW
// All streaming except stats; the hull mask in between is smirk_hull_mask of video.hip, unchanged.
#include "common.h"
#include "data_rng.h"
#include "../../include/smirk_data.h"

#define DATA_LUT_BYTES 256
#define DATA_CLAHE_BYTES (SMIRK_DATA_CLAHE_TILES * SMIRK_DATA_CLAHE_TILES * 256)
#define DATA_COIN(c, t) (((c) >> (t)) & 1)

struct DataLayout { size_t params, hullpts, crop, stage_a, stage_b, hull, lut, clahe, total; };

static bool data_layout(int N, int S, int train, DataLayout& L) {
    if (N <= 0 || S <= 0 || S % SMIRK_DATA_CLAHE_TILES != 0 || S > SMIRK_DATA_MAX_SIZE) return false;
    size_t o = 0;
    const size_t n = (size_t)N, px = (size_t)S * S;
    auto take = [&](size_t bytes) { const size_t at = o; o = smirk_align_up(o + bytes, 256); return at; };
    L.params = take(n * sizeof(SmirkDataParams));
    L.hullpts = take(n * SMIRK_DATA_MAX_POINTS * 2 * sizeof(float));
    L.crop = L.stage_a = L.stage_b = L.hull = L.lut = L.clahe = 0;
    if (train) {
        L.crop = take(n * px * 3);
        L.stage_a = take(n * px * 3);
        L.stage_b = take(n * px * 3);
        L.hull = take(n * px * sizeof(float));
        L.lut = take(n * DATA_LUT_BYTES);
        L.clahe = take(n * DATA_CLAHE_BYTES);
    }
    L.total = o;
    return true;
}

// SMIRK_OK, or the refusal every entry shares for (N, S, workspace)
static int data_check(int N, int S, int train, const void* ws, size_t ws_bytes, DataLayout& L) {
    if (N <= 0 || S <= 0 || !ws) return SMIRK_ERR_BAD_ARG;
    if (S % SMIRK_DATA_CLAHE_TILES != 0 || S > SMIRK_DATA_MAX_SIZE) return SMIRK_ERR_UNSUPPORTED;
    if (!data_layout(N, S, train, L)) return SMIRK_ERR_BAD_ARG;
    if (ws_bytes < L.total) return SMIRK_ERR_WORKSPACE;
    return SMIRK_OK;
}

extern "C" int smirk_data_abi_version(void) { return SMIRK_DATA_ABI_VERSION; }
extern "C" size_t smirk_data_workspace_bytes(int N, int S, int train) { DataLayout L; return data_layout(N, S, train, L) ? L.total : 0; }
extern "C" size_t smirk_data_hull_points_offset(int N, int S, int train) { DataLayout L; return data_layout(N, S, train, L) ? L.hullpts : 0; }
extern "C" size_t smirk_data_hull_offset(int N, int S, int train) { DataLayout L; return data_layout(N, S, train, L) ? L.hull : 0; }

// ---- integer / float64 helpers shared by the kernels (tests/data_law.py, same names) ---------------------------------------------------------------------------
__device__ __forceinline__ double clip255(double v) { return fmin(fmax(v, 0.0), 255.0); }
__device__ __forceinline__ int trunc_u8(double v) { return (int)clip255(v); }
__device__ __forceinline__ int rint_u8(double v) { return (int)rint(clip255(v)); }
__device__ __forceinline__ int grey_u8(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }
__device__ __forceinline__ double data_uniform(uint32_t x, double lo, double hi) { return lo + (hi - lo) * data_u01(x); }

// ColorJitter saturation then hue on one pixel (8-bit HSV computed in float64)
__device__ __forceinline__ void jitter_sat_hue(int& r, int& g, int& b, double fs, double hue) {
    const double gr = (double)grey_u8(r, g, b);
    r = rint_u8(fs * r + (1.0 - fs) * gr); g = rint_u8(fs * g + (1.0 - fs) * gr); b = rint_u8(fs * b + (1.0 - fs) * gr);
    const int v = max(r, max(g, b)), mn = min(r, min(g, b)), d = v - mn;
    const int s8 = v > 0 ? (int)rint(255.0 * d / (double)v) : 0;
    double h = 0.0;
    if (d != 0) {
        if (v == r) h = 60.0 * (g - b) / (double)d;
        else if (v == g) h = 120.0 + 60.0 * (b - r) / (double)d;
        else h = 240.0 + 60.0 * (r - g) / (double)d;
        if (h < 0.0) h += 360.0;
    }
    int h8 = (int)rint(h / 2.0);
    if (h8 >= 180) h8 -= 180;
    double t = h8 + hue * 180.0;
    t = t - 180.0 * floor(t / 180.0);
    if (t >= 180.0) t -= 180.0;
    h8 = (int)t;
    const double hh = (2 * h8) / 60.0, sec = floor(hh), f = hh - sec, s = s8 / 255.0, vv = (double)v;
    const double p = vv * (1.0 - s), q = vv * (1.0 - s * f), u = vv * (1.0 - s * (1.0 - f));
    const int k = (int)sec;
    const double rr = (k == 0 || k == 5) ? vv : (k == 1 ? q : (k == 4 ? u : p));
    const double gg = (k == 1 || k == 2) ? vv : (k == 0 ? u : (k == 3 ? q : p));
    const double bb = (k == 3 || k == 4) ? vv : (k == 2 ? u : (k == 5 ? q : p));
    r = rint_u8(rr); g = rint_u8(gg); b = rint_u8(bb);
}

__device__ __forceinline__ double srgb_to_linear(int i) {
    const double u = i / 255.0;
    return u <= 0.04045 ? u / 12.92 : pow((u + 0.055) / 1.055, 2.4);
}
__device__ __forceinline__ double lab_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }
__device__ __forceinline__ double lab_finv(double t) { const double t3 = t * t * t; return t3 > 0.008856 ? t3 : (t - 16.0 / 116.0) / 7.787; }
__device__ __forceinline__ double linear_to_srgb(double c) { return c <= 0.0031308 ? 12.92 * c : 1.055 * pow(c, 1.0 / 2.4) - 0.055; }

// 8-bit L of a pixel given the linear values of its channels
__device__ __forceinline__ int lab_l8(double R, double G, double B, double& fy) {
    const double Y = 0.212671 * R + 0.715160 * G + 0.072169 * B;
    fy = lab_f(Y);
    return rint_u8(2.55 * (Y > 0.008856 ? 116.0 * fy - 16.0 : 903.3 * Y));
}

// ---- params --------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void data_params_kernel(const double* __restrict__ lmk_mp, const int32_t* __restrict__ n_mp, int Lmax,
                                                          const double* __restrict__ lmk_fan, const uint8_t* __restrict__ flag_fan,
                                                          const int32_t* __restrict__ mp_index, int n_index, int S, double scale_lo, double scale_hi,
                                                          SmirkDataAugment aug, int train, uint64_t seed, uint64_t offset, float* __restrict__ out_fan,
                                                          float* __restrict__ out_mp, uint8_t* __restrict__ out_flag, SmirkDataParams* __restrict__ params,
                                                          float* __restrict__ hullpts) {
    __shared__ double red[4][256];
    __shared__ double s_m[12];                       // crop_fwd (s, tx, ty: 0..2), ssr_fwd 3..8
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(n_mp[f], 1), Lmax);
    const double* mp = lmk_mp + (size_t)f * Lmax * 2;
    const double* fan = lmk_fan + (size_t)f * SMIRK_DATA_FAN_POINTS * 2;
    double left = 1e300, right = -1e300, top = 1e300, bottom = -1e300;
    for (int i = tid; i < n; i += 256) {
        const double x = mp[2 * i], y = mp[2 * i + 1];
        left = fmin(left, x); right = fmax(right, x); top = fmin(top, y); bottom = fmax(bottom, y);
    }
    red[0][tid] = left; red[1][tid] = right; red[2][tid] = top; red[3][tid] = bottom;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] = fmin(red[0][tid], red[0][tid + o]); red[1][tid] = fmax(red[1][tid], red[1][tid + o]);
            red[2][tid] = fmin(red[2][tid], red[2][tid + o]); red[3][tid] = fmax(red[3][tid], red[3][tid + o]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        SmirkDataParams* P = params + f;
        left = red[0][0]; right = red[1][0]; top = red[2][0]; bottom = red[3][0];
        const uint64_t base = offset + (uint64_t)DATA_FRAME_COUNTERS * (uint64_t)f;
        const DataDraw d0 = data_philox(base + 0, DATA_STREAM_FRAME, seed), d1 = data_philox(base + 1, DATA_STREAM_FRAME, seed),
                       d2 = data_philox(base + 2, DATA_STREAM_FRAME, seed), d3 = data_philox(base + 3, DATA_STREAM_FRAME, seed),
                       d4 = data_philox(base + 4, DATA_STREAM_FRAME, seed), d5 = data_philox(base + 5, DATA_STREAM_FRAME, seed),
                       d6 = data_philox(base + 6, DATA_STREAM_FRAME, seed);
        // crop_face: the box of the mediapipe points enlarged by `scale`, mapped onto [0, S - 1]^2
        const double scale = train ? data_uniform(d0.x0, scale_lo, scale_hi) : scale_lo;
        const double old_size = (right - left + bottom - top) / 2;
        const double cx = right - (right - left) / 2.0, cy = bottom - (bottom - top) / 2.0;
        double sz = floor(old_size * scale);                                     // int(): the product is positive
        sz = fmin(fmax(sz, 1.0), 1073741824.0);
        const double s = (double)(S - 1) / sz, si = sz / (double)(S - 1);
        const double x0 = cx - sz / 2.0, y0 = cy - sz / 2.0, tx = -s * x0, ty = -s * y0;
        P->crop_fwd[0] = s; P->crop_fwd[1] = 0.0; P->crop_fwd[2] = tx; P->crop_fwd[3] = 0.0; P->crop_fwd[4] = s; P->crop_fwd[5] = ty;
        P->crop_inv[0] = si; P->crop_inv[1] = 0.0; P->crop_inv[2] = x0; P->crop_inv[3] = 0.0; P->crop_inv[4] = si; P->crop_inv[5] = y0;
        P->scale = scale;
        s_m[0] = s; s_m[1] = tx; s_m[2] = ty;
        // the augmentation's coins and draws
        int coins = 0, k = 3;
        double m[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0}, mi[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        double alpha = 1.0, beta = 0.0, gamma = 1.0, jb = 1.0, jc = 1.0, js = 1.0, jh = 0.0, clip = 1.0, sr = 0.0, sg = 0.0, sb = 0.0, sigma = 0.0;
        double angle = 0.0, zoom = 1.0, dx = 0.0, dy = 0.0;
        if (train) {
            coins |= (data_u01(d0.x1) < aug.p[0]) << 0;
            alpha = 1.0 + data_uniform(d0.x2, -aug.contrast_limit, aug.contrast_limit);
            beta = data_uniform(d0.x3, -aug.brightness_limit, aug.brightness_limit);
            coins |= (data_u01(d1.x0) < aug.p[1]) << 1;
            gamma = data_uniform(d1.x1, aug.gamma_lo, aug.gamma_hi) / 100.0;
            coins |= (data_u01(d1.x2) < aug.p[2]) << 2;
            jb = 1.0 + data_uniform(d1.x3, -aug.cj_brightness, aug.cj_brightness);
            jc = 1.0 + data_uniform(d2.x0, -aug.cj_contrast, aug.cj_contrast);
            js = 1.0 + data_uniform(d2.x1, -aug.cj_saturation, aug.cj_saturation);
            jh = data_uniform(d2.x2, -aug.cj_hue, aug.cj_hue);
            coins |= (data_u01(d2.x3) < aug.p[3]) << 3;
            clip = data_uniform(d3.x0, aug.clahe_lo, aug.clahe_hi);
            coins |= (data_u01(d3.x1) < aug.p[4]) << 4;
            sr = data_uniform(d3.x2, -aug.rgb_shift, aug.rgb_shift);
            sg = data_uniform(d3.x3, -aug.rgb_shift, aug.rgb_shift);
            sb = data_uniform(d4.x0, -aug.rgb_shift, aug.rgb_shift);
            coins |= (data_u01(d4.x1) < aug.p[5]) << 5;
            k = 3 + 2 * (int)(((uint64_t)d4.x2 * (uint64_t)((aug.blur_max - 1) / 2)) >> 32);
            coins |= (data_u01(d4.x3) < aug.p[6]) << 6;
            sigma = sqrt(data_uniform(d5.x0, aug.noise_var_lo, aug.noise_var_hi));
            coins |= (data_u01(d5.x1) < aug.p[7]) << 7;
            angle = data_uniform(d5.x2, -aug.rotate_limit, aug.rotate_limit);
            zoom = 1.0 + data_uniform(d5.x3, -aug.scale_limit, aug.scale_limit);
            dx = data_uniform(d6.x0, -aug.shift_limit, aug.shift_limit);
            dy = data_uniform(d6.x1, -aug.shift_limit, aug.shift_limit);
            if (DATA_COIN(coins, SMIRK_DATA_SHIFT_SCALE_ROTATE)) {
                // cv2.getRotationMatrix2D((c, c), angle, zoom) with the shift added to its translation
                const double rad = angle * (3.141592653589793 / 180.0), c = (double)(S - 1) / 2.0;
                const double a = zoom * cos(rad), b = zoom * sin(rad);
                m[0] = a; m[1] = b; m[2] = ((1.0 - a) * c - b * c) + dx * (double)S;
                m[3] = -b; m[4] = a; m[5] = (b * c + (1.0 - a) * c) + dy * (double)S;
                const double det = a * a + b * b, ia = a / det, ib = b / det;
                mi[0] = ia; mi[1] = -ib; mi[2] = -(mi[0] * m[2] + mi[1] * m[5]);
                mi[3] = ib; mi[4] = ia; mi[5] = -(mi[3] * m[2] + mi[4] * m[5]);
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) { P->ssr_fwd[i] = m[i]; P->ssr_inv[i] = mi[i]; s_m[3 + i] = m[i]; }
        P->bc_alpha = alpha; P->bc_beta = beta; P->gamma = gamma; P->cj[0] = jb; P->cj[1] = jc; P->cj[2] = js; P->cj[3] = jh; P->clahe_clip = clip;
        P->rgb_shift[0] = sr; P->rgb_shift[1] = sg; P->rgb_shift[2] = sb; P->noise_sigma = sigma;
        P->ssr_angle = angle; P->ssr_scale = zoom; P->ssr_dx = dx; P->ssr_dy = dy;
        P->coins = coins; P->blur_k = k; P->_pad = 0;
        // estimate_norm: least-squares similarity of five points of the UNCROPPED FAN landmarks onto the ArcFace template, closed form about the centroids
        int flag = flag_fan[f] ? 1 : 0;
        double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (flag) {
            const double sx[5] = {(fan[2 * 36] + fan[2 * 39]) / 2, (fan[2 * 42] + fan[2 * 45]) / 2, fan[2 * 32], fan[2 * 48], fan[2 * 54]};
            const double sy[5] = {(fan[2 * 36 + 1] + fan[2 * 39 + 1]) / 2, (fan[2 * 42 + 1] + fan[2 * 45 + 1]) / 2, fan[2 * 32 + 1], fan[2 * 48 + 1], fan[2 * 54 + 1]};
            const double tx5[5] = {(double)38.2946f, (double)73.5318f, (double)56.0252f, (double)41.5493f, (double)70.7299f};
            const double ty5[5] = {(double)51.6963f, (double)51.5014f, (double)71.7366f, (double)92.3655f, (double)92.2041f};
            const double msx = ((((sx[0] + sx[1]) + sx[2]) + sx[3]) + sx[4]) / 5.0, msy = ((((sy[0] + sy[1]) + sy[2]) + sy[3]) + sy[4]) / 5.0;
            const double mdx = ((((tx5[0] + tx5[1]) + tx5[2]) + tx5[3]) + tx5[4]) / 5.0, mdy = ((((ty5[0] + ty5[1]) + ty5[2]) + ty5[3]) + ty5[4]) / 5.0;
            double na = 0.0, nb = 0.0, den = 0.0;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const double xs = sx[i] - msx, ys = sy[i] - msy, xd = tx5[i] - mdx, yd = ty5[i] - mdy;
                na += xs * xd + ys * yd; nb += xs * yd - ys * xd; den += xs * xs + ys * ys;
            }
            if (den > 0.0) {
                const double a = na / den, b = nb / den;
                const double ftx = mdx - (a * msx - b * msy), fty = mdy - (b * msx + a * msy);
                const double det = a * a + b * b;
                if (det > 0.0) {
                    const double ia = a / det, ib = b / det;
                    q[0] = ia; q[1] = ib; q[2] = -(ia * ftx + ib * fty);
                    q[3] = -ib; q[4] = ia; q[5] = -(-ib * ftx + ia * fty);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) P->mica_inv[i] = q[i];
        P->flag_fan = flag;
        out_flag[f] = (uint8_t)flag;
    }
    __syncthreads();
    const double s = s_m[0], tx = s_m[1], ty = s_m[2];
    const double m0 = s_m[3], m1 = s_m[4], m2 = s_m[5], m3 = s_m[6], m4 = s_m[7], m5 = s_m[8];
    const float fS = (float)S;
    // create_mask's points: every cropped mediapipe point truncated toward zero (rows past n repeat point 0: the hull does not change)
    float* hp = hullpts + (size_t)f * Lmax * 2;
    for (int i = tid; i < Lmax; i += 256) {
        const int j = i < n ? i : 0;
        const double x = s * mp[2 * j] + tx, y = s * mp[2 * j + 1] + ty;
        hp[2 * i] = (float)(int)fmin(fmax(x, -16777216.0), 16777216.0); hp[2 * i + 1] = (float)(int)fmin(fmax(y, -16777216.0), 16777216.0);
    }
    for (int i = tid; i < n_index + SMIRK_DATA_FAN_POINTS; i += 256) {
        const bool is_mp = i < n_index;
        const int j = is_mp ? min(max(mp_index[i], 0), n - 1) : i - n_index;
        const double* src = is_mp ? mp + 2 * j : fan + 2 * j;
        const double x = s * src[0] + tx, y = s * src[1] + ty;
        const double xa = (m0 * x + m1 * y) + m2, ya = (m3 * x + m4 * y) + m5;
        float vx = (float)xa, vy = (float)ya;
        vx = vx / fS; vx = vx * 2.0f; vx = vx - 1.0f;
        vy = vy / fS; vy = vy * 2.0f; vy = vy - 1.0f;
        float* o = is_mp ? out_mp + ((size_t)f * n_index + i) * 2 : out_fan + ((size_t)f * SMIRK_DATA_FAN_POINTS + j) * 2;
        o[0] = vx; o[1] = vy;
    }
}

static bool data_bad_p(double p) { return !(p >= 0.0 && p <= 1.0); }
static bool data_bad_sym(double l, double cap) { return !(l >= 0.0 && l <= cap); }
static bool data_bad_range(double lo, double hi, double min_lo) { return !(lo >= min_lo && lo <= hi && hi < 1e300); }

static bool data_augment_ok(const SmirkDataAugment* a) {
    for (int t = 0; t < SMIRK_DATA_TRANSFORMS; ++t)
        if (data_bad_p(a->p[t])) return false;
    if (data_bad_sym(a->brightness_limit, 1e6) || data_bad_sym(a->contrast_limit, 1e6)) return false;
    if (data_bad_range(a->gamma_lo, a->gamma_hi, 0.0) || !(a->gamma_lo > 0.0)) return false;
    if (data_bad_sym(a->cj_brightness, 1.0) || data_bad_sym(a->cj_contrast, 1.0) || data_bad_sym(a->cj_saturation, 1.0) || data_bad_sym(a->cj_hue, 0.5)) return false;
    if (data_bad_range(a->clahe_lo, a->clahe_hi, 1.0)) return false;
    if (data_bad_sym(a->rgb_shift, 255.0)) return false;
    if (data_bad_range(a->noise_var_lo, a->noise_var_hi, 0.0)) return false;
    if (data_bad_sym(a->shift_limit, 1.0) || data_bad_sym(a->rotate_limit, 360.0) || !(a->scale_limit >= 0.0 && a->scale_limit < 1.0)) return false;
    if (a->blur_max != 3 && a->blur_max != 5 && a->blur_max != 7) return false;
    return true;
}

extern "C" int smirk_data_params(const double* lmk_mp, const int32_t* n_mp, int Lmax, const double* lmk_fan, const uint8_t* flag_fan, const int32_t* mp_index,
                                 int n_index, int N, int S, double scale_lo, double scale_hi, const SmirkDataAugment* aug, uint64_t seed, uint64_t offset,
                                 float* landmarks_fan_out, float* landmarks_mp_out, uint8_t* flag_fan_out, void* ws, size_t ws_bytes, void* stream) {
    if (!lmk_mp || !n_mp || !lmk_fan || !flag_fan || !mp_index || !landmarks_fan_out || !landmarks_mp_out || !flag_fan_out) return SMIRK_ERR_BAD_ARG;
    if (Lmax < 1 || Lmax > SMIRK_DATA_MAX_POINTS || n_index < 1 || n_index > SMIRK_DATA_MAX_POINTS) return SMIRK_ERR_BAD_ARG;
    if (!(scale_lo > 0.0 && scale_lo <= scale_hi && scale_hi < 1e300)) return SMIRK_ERR_BAD_ARG;
    if (aug && !data_augment_ok(aug)) return SMIRK_ERR_BAD_ARG;
    DataLayout L;
    const int rc = data_check(N, S, aug != nullptr, ws, ws_bytes, L);
    if (rc != SMIRK_OK) return rc;
    SmirkDataAugment a = {};
    if (aug) a = *aug;
    char* w = (char*)ws;
    SMIRK_LAUNCH(data_params_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, lmk_mp, n_mp, Lmax, lmk_fan, flag_fan, mp_index, n_index, S, scale_lo, scale_hi,
                 a, aug ? 1 : 0, seed, offset, landmarks_fan_out, landmarks_mp_out, flag_fan_out, (SmirkDataParams*)(w + L.params), (float*)(w + L.hullpts));
    return smirk_launch_status();
}

// ---- crop + MICA warp ------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double frame_px(const uint8_t* img, int rows, int cols, double r, double c, int ch) {
    if (r < 0 || r >= rows || c < 0 || c >= cols) return 0.0;
    return (double)img[((size_t)(int)r * cols + (int)c) * 3 + ch];
}

__global__ __launch_bounds__(256) void data_crop_kernel(const uint8_t* __restrict__ frames, size_t frames_bytes, const SmirkDataFrame* __restrict__ table, int S,
                                                        const SmirkDataParams* __restrict__ params, float* __restrict__ img_f32, uint8_t* __restrict__ crop_u8,
                                                        float* __restrict__ img_mica, int crop_blocks) {
    const int f = blockIdx.y;
    const SmirkDataFrame fr = table[f];
    const SmirkDataParams* P = params + f;
    // a descriptor that reaches past the packed buffer reads as a black frame
    const bool ok = fr.H > 0 && fr.W > 0 && fr.offset <= frames_bytes && (size_t)fr.H * fr.W * 3 <= frames_bytes - fr.offset;
    const int Hs = ok ? fr.H : 0, Ws = ok ? fr.W : 0;
    const uint8_t* src = frames + (ok ? fr.offset : 0);
    if ((int)blockIdx.x < crop_blocks) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i >= S * S) return;
        const int row = i / S, col = i % S;
        const double* M = P->crop_inv;
        const double x = M[0] * col + M[1] * row + M[2];
        const double y = M[3] * col + M[4] * row + M[5];
        const double minr = floor(y), minc = floor(x), maxr = ceil(y), maxc = ceil(x);
        const double dr = y - minr, dc = x - minc;
        const size_t plane = (size_t)S * S;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double top = (1 - dc) * frame_px(src, Hs, Ws, minr, minc, ch) + dc * frame_px(src, Hs, Ws, minr, maxc, ch);
            const double bot = (1 - dc) * frame_px(src, Hs, Ws, maxr, minc, ch) + dc * frame_px(src, Hs, Ws, maxr, maxc, ch);
            const uint8_t v = (uint8_t)((1 - dr) * top + dr * bot);                  // astype(np.uint8): truncation
            const int oc = 2 - ch;                                                   // cv2.cvtColor(BGR2RGB)
            if (crop_u8) crop_u8[((size_t)f * plane + i) * 3 + oc] = v;
            else img_f32[((size_t)f * 3 + oc) * plane + i] = (float)v / 255.0f;
        }
    } else {
        const int Q = SMIRK_DATA_MICA_SIZE;
        const int i = (blockIdx.x - crop_blocks) * 256 + threadIdx.x;
        if (i >= Q * Q) return;
        const int row = i / Q, col = i % Q;
        float* o = img_mica + (size_t)f * 3 * Q * Q + i;
        if (!P->flag_fan) { o[0] = 0.f; o[Q * Q] = 0.f; o[2 * Q * Q] = 0.f; return; }
        const double* M = P->mica_inv;
        const double x = M[0] * col + M[1] * row + M[2];
        const double y = M[3] * col + M[4] * row + M[5];
        const double y0 = floor(y), x0 = floor(x), fy = y - y0, fx = x - x0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double p00 = frame_px(src, Hs, Ws, y0, x0, ch) / 255.0, p01 = frame_px(src, Hs, Ws, y0, x0 + 1, ch) / 255.0;
            const double p10 = frame_px(src, Hs, Ws, y0 + 1, x0, ch) / 255.0, p11 = frame_px(src, Hs, Ws, y0 + 1, x0 + 1, ch) / 255.0;
            const double v = (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11);
            o[(size_t)(2 - ch) * Q * Q] = (float)v;
        }
    }
}

extern "C" int smirk_data_crop(const uint8_t* frames, size_t frames_bytes, const SmirkDataFrame* table, int N, int S, int train, float* img, float* img_mica,
                               void* ws, size_t ws_bytes, void* stream) {
    if (!frames || !table || !img_mica || frames_bytes == 0 || (!train && !img)) return SMIRK_ERR_BAD_ARG;
    DataLayout L;
    const int rc = data_check(N, S, train, ws, ws_bytes, L);
    if (rc != SMIRK_OK) return rc;
    char* w = (char*)ws;
    const int cb = (S * S + 255) / 256, mb = (SMIRK_DATA_MICA_SIZE * SMIRK_DATA_MICA_SIZE + 255) / 256;
    SMIRK_LAUNCH(data_crop_kernel, dim3(cb + mb, N), dim3(256), 0, (hipStream_t)stream, frames, frames_bytes, table, S, (const SmirkDataParams*)(w + L.params),
                 train ? (float*)nullptr : img, train ? (uint8_t*)(w + L.crop) : (uint8_t*)nullptr, img_mica, cb);
    return smirk_launch_status();
}

// ---- stats: lookup table + CLAHE tables --------------------------------------------------------------------------------------------------------------------------
#define DATA_STATS_THREADS 512
#define DATA_HIST_STRIDE 257                       // one tile's 256 bins + 1: the per-tile pass walks 32 tiles with one thread each
__global__ __launch_bounds__(DATA_STATS_THREADS) void data_stats_kernel(int S, const SmirkDataParams* __restrict__ params, const uint8_t* __restrict__ crop,
                                                                        uint8_t* __restrict__ lut_out, uint8_t* __restrict__ clahe_out) {
    __shared__ uint8_t lut_a[256], lut[256];
    __shared__ double lin[256];
    __shared__ unsigned hist[32 * DATA_HIST_STRIDE];
    __shared__ unsigned long long s_sum;
    const int f = blockIdx.x, tid = threadIdx.x, px = S * S;
    const SmirkDataParams* P = params + f;
    const int coins = P->coins;
    const uint8_t* img = crop + (size_t)f * px * 3;
    if (tid == 0) s_sum = 0ull;
    if (tid < 256) {
        int v = tid;
        if (DATA_COIN(coins, SMIRK_DATA_BRIGHTNESS_CONTRAST)) v = trunc_u8(v * P->bc_alpha + P->bc_beta * 255.0);
        if (DATA_COIN(coins, SMIRK_DATA_GAMMA)) v = trunc_u8(pow(v / 255.0, P->gamma) * 255.0);
        lut_a[tid] = (uint8_t)v;
    }
    __syncthreads();
    const bool jitter = DATA_COIN(coins, SMIRK_DATA_COLOR_JITTER);
    if (jitter) {                                   // the contrast pivots on int(mean grey + 0.5) of the image entering ColorJitter
        unsigned long long part = 0ull;
        for (int i = tid; i < px; i += DATA_STATS_THREADS) part += (unsigned)grey_u8(lut_a[img[3 * i]], lut_a[img[3 * i + 1]], lut_a[img[3 * i + 2]]);
        atomicAdd(&s_sum, part);
        __syncthreads();
        if (tid < 256) {
            const int m = (int)((double)s_sum / (double)px + 0.5);
            int v = trunc_u8(lut_a[tid] * P->cj[0]);
            v = trunc_u8(v * P->cj[1] + (1.0 - P->cj[1]) * m);
            lut[tid] = (uint8_t)v;
        }
    } else if (tid < 256) lut[tid] = lut_a[tid];
    __syncthreads();
    if (tid < 256) lut_out[(size_t)f * DATA_LUT_BYTES + tid] = lut[tid];
    if (!DATA_COIN(coins, SMIRK_DATA_CLAHE)) return;
    if (tid < 256) lin[tid] = srgb_to_linear(tid);
    const int T = SMIRK_DATA_CLAHE_TILES, th = S / T, area = th * th, half_px = px / 2;
    const double fs = P->cj[2], hue = P->cj[3];
    for (int half = 0; half < 2; ++half) {
        for (int i = tid; i < 32 * DATA_HIST_STRIDE; i += DATA_STATS_THREADS) hist[i] = 0u;
        __syncthreads();
        for (int i = half * half_px + tid; i < (half + 1) * half_px; i += DATA_STATS_THREADS) {
            int r = lut[img[3 * i]], g = lut[img[3 * i + 1]], b = lut[img[3 * i + 2]];
            if (jitter) jitter_sat_hue(r, g, b, fs, hue);
            double fy;
            const int l8 = lab_l8(lin[r], lin[g], lin[b], fy);
            const int row = i / S, col = i % S, tile = (row / th - half * (T / 2)) * T + col / th;
            atomicAdd(&hist[tile * DATA_HIST_STRIDE + l8], 1u);
        }
        __syncthreads();
        if (tid < 32) {                             // cv::CLAHE: clip, redistribute the excess, cumulative table
            unsigned* h = hist + tid * DATA_HIST_STRIDE;
            const int clip = max((int)(P->clahe_clip * area / 256.0), 1);
            int clipped = 0;
            for (int i = 0; i < 256; ++i) {
                const int c = (int)h[i];
                if (c > clip) { clipped += c - clip; h[i] = (unsigned)clip; }
            }
            const int batch = clipped / 256;
            int resid = clipped - batch * 256;
            for (int i = 0; i < 256; ++i) h[i] += (unsigned)batch;
            if (resid != 0) {
                const int step = max(256 / resid, 1);
                for (int i = 0; i < 256 && resid > 0; i += step, --resid) h[i] += 1u;
            }
            uint8_t* o = clahe_out + ((size_t)f * T * T + half * 32 + tid) * 256;
            int sum = 0;
            for (int i = 0; i < 256; ++i) { sum += (int)h[i]; o[i] = (uint8_t)rint_u8(sum * 255.0 / (double)area); }
        }
        __syncthreads();
    }
}

extern "C" int smirk_data_stats(int N, int S, void* ws, size_t ws_bytes, void* stream) {
    DataLayout L;
    const int rc = data_check(N, S, 1, ws, ws_bytes, L);
    if (rc != SMIRK_OK) return rc;
    char* w = (char*)ws;
    SMIRK_LAUNCH(data_stats_kernel, dim3(N), dim3(DATA_STATS_THREADS), 0, (hipStream_t)stream, S, (const SmirkDataParams*)(w + L.params),
                 (const uint8_t*)(w + L.crop), (uint8_t*)(w + L.lut), (uint8_t*)(w + L.clahe));
    return smirk_launch_status();
}

// ---- colour: the point-wise chain ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void data_colour_kernel(int S, const SmirkDataParams* __restrict__ params, const uint8_t* __restrict__ crop,
                                                          const uint8_t* __restrict__ lut_in, const uint8_t* __restrict__ clahe_in, uint8_t* __restrict__ out) {
    __shared__ uint8_t lut[256];
    __shared__ double lin[256];
    const int f = blockIdx.y, tid = threadIdx.x, px = S * S;
    const SmirkDataParams* P = params + f;
    const int coins = P->coins;
    const bool clahe = DATA_COIN(coins, SMIRK_DATA_CLAHE);
    lut[tid] = lut_in[(size_t)f * DATA_LUT_BYTES + tid];
    if (clahe) lin[tid] = srgb_to_linear(tid);
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    if (i >= px) return;
    const uint8_t* p = crop + ((size_t)f * px + i) * 3;
    int r = lut[p[0]], g = lut[p[1]], b = lut[p[2]];
    if (DATA_COIN(coins, SMIRK_DATA_COLOR_JITTER)) jitter_sat_hue(r, g, b, P->cj[2], P->cj[3]);
    if (clahe) {
        // RGB -> 8-bit Lab (D65), float64
        const double R = lin[r], G = lin[g], B = lin[b];
        const double X = ((0.412453 * R + 0.357580 * G) + 0.180423 * B) / 0.950456, Z = ((0.019334 * R + 0.119193 * G) + 0.950227 * B) / 1.088754;
        double fy;
        const int l8 = lab_l8(R, G, B, fy);
        const int a8 = rint_u8(500.0 * (lab_f(X) - fy) + 128.0), b8 = rint_u8(200.0 * (fy - lab_f(Z)) + 128.0);
        // bilinear blend of the four neighbouring tiles' tables
        const int T = SMIRK_DATA_CLAHE_TILES, th = S / T, row = i / S, col = i % S;
        const double tyf = row / (double)th - 0.5, txf = col / (double)th - 0.5;
        const double ty0 = floor(tyf), tx0 = floor(txf), ya = tyf - ty0, xa = txf - tx0;
        const int ty1 = max((int)ty0, 0), ty2 = min((int)ty0 + 1, T - 1), tx1 = max((int)tx0, 0), tx2 = min((int)tx0 + 1, T - 1);
        const uint8_t* tab = clahe_in + (size_t)f * DATA_CLAHE_BYTES + l8;
        const double v11 = tab[(ty1 * T + tx1) * 256], v12 = tab[(ty1 * T + tx2) * 256], v21 = tab[(ty2 * T + tx1) * 256], v22 = tab[(ty2 * T + tx2) * 256];
        const int l8n = rint_u8((v11 * (1.0 - xa) + v12 * xa) * (1.0 - ya) + (v21 * (1.0 - xa) + v22 * xa) * ya);
        // 8-bit Lab -> RGB
        const double Lv = l8n / 2.55, av = a8 - 128.0, bv = b8 - 128.0;
        double Y, gy;
        if (Lv > 7.9996248) { gy = (Lv + 16.0) / 116.0; Y = gy * gy * gy; }
        else { Y = Lv / 903.3; gy = 7.787 * Y + 16.0 / 116.0; }
        const double Xn = lab_finv(gy + av / 500.0) * 0.950456, Zn = lab_finv(gy - bv / 200.0) * 1.088754;
        const double Rl = (3.240479 * Xn - 1.53715 * Y) - 0.498535 * Zn, Gl = (-0.969256 * Xn + 1.875991 * Y) + 0.041556 * Zn,
                     Bl = (0.055648 * Xn - 0.204043 * Y) + 1.057311 * Zn;
        r = rint_u8(255.0 * linear_to_srgb(Rl)); g = rint_u8(255.0 * linear_to_srgb(Gl)); b = rint_u8(255.0 * linear_to_srgb(Bl));
    }
    if (DATA_COIN(coins, SMIRK_DATA_RGB_SHIFT)) { r = trunc_u8(r + P->rgb_shift[0]); g = trunc_u8(g + P->rgb_shift[1]); b = trunc_u8(b + P->rgb_shift[2]); }
    uint8_t* o = out + ((size_t)f * px + i) * 3;
    o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
}

extern "C" int smirk_data_colour(int N, int S, void* ws, size_t ws_bytes, void* stream) {
    DataLayout L;
    const int rc = data_check(N, S, 1, ws, ws_bytes, L);
    if (rc != SMIRK_OK) return rc;
    char* w = (char*)ws;
    SMIRK_LAUNCH(data_colour_kernel, dim3((S * S + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, S, (const SmirkDataParams*)(w + L.params),
                 (const uint8_t*)(w + L.crop), (const uint8_t*)(w + L.lut), (const uint8_t*)(w + L.clahe), (uint8_t*)(w + L.stage_a));
    return smirk_launch_status();
}

// ---- finish: blur + noise, then the ShiftScaleRotate resample ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ __launch_bounds__(256) void data_blur_noise_kernel(int S, const SmirkDataParams* __restrict__ params, const uint8_t* __restrict__ in,
                                                              uint64_t seed, uint64_t offset, uint8_t* __restrict__ out) {
    const int f = blockIdx.y, px = S * S, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    const SmirkDataParams* P = params + f;
    const int coins = P->coins, row = i / S, col = i % S;
    const uint8_t* img = in + (size_t)f * px * 3;
    int r, g, b;
    if (DATA_COIN(coins, SMIRK_DATA_BLUR)) {
        const int k = P->blur_k, h = k / 2;
        int sr = 0, sg = 0, sb = 0;
        for (int dy = -h; dy <= h; ++dy) {
            const uint8_t* line = img + (size_t)reflect101(row + dy, S) * S * 3;
            for (int dx = -h; dx <= h; ++dx) {
                const uint8_t* p = line + reflect101(col + dx, S) * 3;
                sr += p[0]; sg += p[1]; sb += p[2];
            }
        }
        const double kk = (double)(k * k);
        r = rint_u8(sr / kk); g = rint_u8(sg / kk); b = rint_u8(sb / kk);
    } else { r = img[3 * i]; g = img[3 * i + 1]; b = img[3 * i + 2]; }
    if (DATA_COIN(coins, SMIRK_DATA_GAUSS_NOISE)) {
        const DataDraw d = data_philox(offset + (uint64_t)f * (uint64_t)px + (uint64_t)i, DATA_STREAM_PIXEL, seed);
        double zr, zg, zb, unused;
        data_normal2(d.x0, d.x1, zr, zg);
        data_normal2(d.x2, d.x3, zb, unused);
        const double sigma = P->noise_sigma;
        r = trunc_u8(r + sigma * zr); g = trunc_u8(g + sigma * zg); b = trunc_u8(b + sigma * zb);
    }
    uint8_t* o = out + ((size_t)f * px + i) * 3;
    o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
}

__device__ __forceinline__ double stage_px(const uint8_t* img, int S, double r, double c, int ch) {
    if (r < 0 || r >= S || c < 0 || c >= S) return 0.0;
    return (double)img[((size_t)(int)r * S + (int)c) * 3 + ch];
}

__global__ __launch_bounds__(256) void data_resample_kernel(int S, const SmirkDataParams* __restrict__ params, const uint8_t* __restrict__ in,
                                                            const float* __restrict__ hull, float* __restrict__ img_out, float* __restrict__ mask_out) {
    const int f = blockIdx.y, px = S * S, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    const double* M = params[f].ssr_inv;
    const int row = i / S, col = i % S;
    const double x = (M[0] * col + M[1] * row) + M[2], y = (M[3] * col + M[4] * row) + M[5];
    const double x0 = floor(x), y0 = floor(y), fx = x - x0, fy = y - y0;
    const uint8_t* img = in + (size_t)f * px * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double p00 = stage_px(img, S, y0, x0, ch), p01 = stage_px(img, S, y0, x0 + 1, ch), p10 = stage_px(img, S, y0 + 1, x0, ch),
                     p11 = stage_px(img, S, y0 + 1, x0 + 1, ch);
        const int v = rint_u8((1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11));      // the constant border takes part
        img_out[((size_t)f * 3 + ch) * px + i] = (float)v / 255.0f;
    }
    const double sx = floor(x + 0.5), sy = floor(y + 0.5);                                                       // mask: nearest on 1 - hull, border 0
    const bool inside = sx >= 0 && sx < S && sy >= 0 && sy < S;
    mask_out[(size_t)f * px + i] = inside ? hull[(size_t)f * px + (size_t)(int)sy * S + (int)sx] : 1.0f;
}

extern "C" int smirk_data_finish(int N, int S, uint64_t seed, uint64_t offset, float* img, float* mask, void* ws, size_t ws_bytes, void* stream) {
    if (!img || !mask) return SMIRK_ERR_BAD_ARG;
    DataLayout L;
    const int rc = data_check(N, S, 1, ws, ws_bytes, L);
    if (rc != SMIRK_OK) return rc;
    char* w = (char*)ws;
    const dim3 grid((S * S + 255) / 256, N);
    SMIRK_LAUNCH(data_blur_noise_kernel, grid, dim3(256), 0, (hipStream_t)stream, S, (const SmirkDataParams*)(w + L.params), (const uint8_t*)(w + L.stage_a), seed,
                 offset, (uint8_t*)(w + L.stage_b));
    SMIRK_LAUNCH(data_resample_kernel, grid, dim3(256), 0, (hipStream_t)stream, S, (const SmirkDataParams*)(w + L.params), (const uint8_t*)(w + L.stage_b),
                 (const float*)(w + L.hull), img, mask);
    return smirk_launch_status();
}
