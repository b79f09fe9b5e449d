// Loss head of the trainer's first path for MI355X (gfx950): the landmark terms, the regularisers and the L1 reconstruction term of smirk_trainer.py:56-72,
// 97-101, their weighted total (:134-154) and its gradient; the four cycle terms (:304-313) are row terms of the same kind.  Two launches forward, one
// backward, all on the caller's stream, with no host synchronisation, no allocation, no copy and no atomics.
//   loss_partial_kernel     one workgroup per chunk of SMIRK_LOSS_CHUNK items (row term: elements of the rows x cols slice; image term: pixels, a thread reads
//                           all C planes of its pixels, so the channel mean `loss_img` costs no extra pass).  d = pred - target in fp32 as torch computes it, d^2 or
//                           |d| summed in float64: per thread in item order, across the wave by a fixed butterfly, across the four waves in wave order.  The
//                           chunk -> partial mapping depends on the term shapes only, never on the CU count.
//   loss_finalise_kernel    one wave per term: the lanes count the flagged rows (integers: exact in any order), lane 0 adds the term's partials in index order,
//                           divides by the participating count and stores the fp32 term; thread 0 then stores total = sum of weight * term (float64, rounded once).
//   loss_backward_kernel    one workgroup per chunk of the FULL gradient extent (rows x row_stride: zeros outside `cols` and in unflagged rows, so the caller may
//                           hand in uninitialised memory).  The upstream gradient is read from a device pointer; a workgroup of a flagged term recounts the flags
//                           (B bytes) instead of a launch that would publish the count.  Squared terms: g * w * 2 (pred - target) / n in float64, rounded once
//                           (the correctly rounded gradient: the float64 law's own); image term: +-(g * w / n) by the sign of d, 0 at d = 0.
// These kernels are bandwidth- (image term: 2 reads + at most 1.33 writes per element) and latency-class (everything else).
#include <limits.h>

#include "common.h"

#define LOSS_BLOCK 256
#define LOSS_ITEMS (SMIRK_LOSS_CHUNK / LOSS_BLOCK)                                  // items per thread and chunk
static_assert(SMIRK_LOSS_CHUNK % (4 * LOSS_BLOCK) == 0, "a chunk is a whole number of 16-byte vectors per thread");

struct LossTermDev {
    const float *pred, *target;
    const uint8_t* flags;
    float *loss_img, *grad;
    int rows, row_stride, cols, kind, C, HW;
    int chunk0;                                                                    // first chunk (= partial index, forward) of this term; chunk0 of term k + 1 ends it
    float weight;
};
struct LossArgs {
    LossTermDev t[SMIRK_LOSS_MAX_TERMS + 1];                                       // t[n].chunk0 = total number of chunks
    int n;
};

__device__ __forceinline__ int loss_find_term(const LossArgs& a, int chunk) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < SMIRK_LOSS_MAX_TERMS; ++j) k += (int)(j < a.n && chunk >= a.t[j].chunk0);
    return k;
}

// sum over the workgroup in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double loss_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// rows of a flagged term that take part (every thread of the workgroup gets the count)
__device__ __forceinline__ int loss_block_flag_count(const uint8_t* flags, int rows, int* red) {
    int c = 0;
    for (int r = threadIdx.x; r < rows; r += LOSS_BLOCK) c += (int)(flags[r] != 0);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(LOSS_BLOCK) void loss_partial_kernel(LossArgs a, double* __restrict__ partials) {
    __shared__ double red[LOSS_BLOCK / 64];
    const int chunk = blockIdx.x;
    const int k = loss_find_term(a, chunk);
    const LossTermDev& T = a.t[k];
    const int local = chunk - T.chunk0;
    double acc = 0.0;
    if (T.kind == SMIRK_LOSS_SQUARE) {
        const int n = T.rows * T.cols;
#pragma unroll 4
        for (int i = 0; i < LOSS_ITEMS; ++i) {
            const int e = local * SMIRK_LOSS_CHUNK + i * LOSS_BLOCK + (int)threadIdx.x;
            if (e >= n) break;
            const int r = e / T.cols, c = e - r * T.cols;
            if (T.flags && !T.flags[r]) continue;
            const size_t at = (size_t)r * T.row_stride + c;
            const float d = T.pred[at] - (T.target ? T.target[at] : 0.0f);
            acc += (double)d * (double)d;
        }
    } else {
        const int HW = T.HW, C = T.C, npix = T.rows * HW;
        if ((HW & 3) == 0) {                                                       // every plane starts on a 16-byte boundary: one f32x4 per plane and thread
            const int nq = npix >> 2, qhw = HW >> 2;
#pragma unroll 2
            for (int i = 0; i < LOSS_ITEMS / 4; ++i) {
                const int q = local * (SMIRK_LOSS_CHUNK / 4) + i * LOSS_BLOCK + (int)threadIdx.x;
                if (q >= nq) break;
                const int b = q / qhw, o = (q - b * qhw) << 2;
                const size_t base = (size_t)b * C * HW + o;
                double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
                for (int ch = 0; ch < C; ++ch) {
                    const f32x4 p = *(const f32x4*)(T.pred + base + (size_t)ch * HW);
                    const f32x4 t = *(const f32x4*)(T.target + base + (size_t)ch * HW);
                    s0 += (double)fabsf(p.x - t.x); s1 += (double)fabsf(p.y - t.y);
                    s2 += (double)fabsf(p.z - t.z); s3 += (double)fabsf(p.w - t.w);
                }
                acc += (s0 + s1) + (s2 + s3);
                if (T.loss_img) {
                    f32x4 m;
                    m.x = (float)(s0 / (double)C); m.y = (float)(s1 / (double)C); m.z = (float)(s2 / (double)C); m.w = (float)(s3 / (double)C);
                    *(f32x4*)(T.loss_img + (size_t)b * HW + o) = m;
                }
            }
        } else {
#pragma unroll 2
            for (int i = 0; i < LOSS_ITEMS; ++i) {
                const int p = local * SMIRK_LOSS_CHUNK + i * LOSS_BLOCK + (int)threadIdx.x;
                if (p >= npix) break;
                const int b = p / HW, o = p - b * HW;
                const size_t base = (size_t)b * C * HW + o;
                double s = 0.0;
                for (int ch = 0; ch < C; ++ch) s += (double)fabsf(T.pred[base + (size_t)ch * HW] - T.target[base + (size_t)ch * HW]);
                acc += s;
                if (T.loss_img) T.loss_img[(size_t)b * HW + o] = (float)(s / (double)C);
            }
        }
    }
    const double sum = loss_block_sum(acc, red);
    if (threadIdx.x == 0) partials[chunk] = sum;
}

// participating element count of term T given the number of flagged rows (all rows when the term has no flags)
__device__ __forceinline__ double loss_count(const LossTermDev& T, int flagged) {
    if (T.kind == SMIRK_LOSS_ABS_IMAGE) return (double)T.rows * (double)T.C * (double)T.HW;
    return (double)(T.flags ? flagged : T.rows) * (double)T.cols;
}

__global__ __launch_bounds__(64 * SMIRK_LOSS_MAX_TERMS) void loss_finalise_kernel(LossArgs a, const double* __restrict__ partials, float* __restrict__ out_terms,
                                                                                  float* __restrict__ out_total) {
    __shared__ double term[SMIRK_LOSS_MAX_TERMS];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (k < a.n) {                                                                 // wave-uniform
        const LossTermDev& T = a.t[k];
        int flagged = 0;
        if (T.flags) {
            for (int r = lane; r < T.rows; r += 64) flagged += (int)(T.flags[r] != 0);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) flagged += __shfl_xor(flagged, o, 64);
        }
        if (lane == 0) {
            const int c1 = a.t[k + 1].chunk0;
            double s = 0.0;
            for (int c = T.chunk0; c < c1; ++c) s += partials[c];                  // index order
            const double n = loss_count(T, flagged);
            const double v = n > 0.0 ? s / n : 0.0;
            term[k] = v;
            out_terms[k] = (float)v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int j = 0; j < a.n; ++j) tot += (double)a.t[j].weight * term[j];
        *out_total = (float)tot;
    }
}

__global__ __launch_bounds__(LOSS_BLOCK) void loss_backward_kernel(LossArgs a, const float* __restrict__ grad_total) {
    __shared__ int red[LOSS_BLOCK / 64];
    const int chunk = blockIdx.x;
    const int k = loss_find_term(a, chunk);
    const LossTermDev& T = a.t[k];
    const int local = chunk - T.chunk0;
    const int flagged = T.flags ? loss_block_flag_count(T.flags, T.rows, red) : 0;
    const double n = loss_count(T, flagged);
    const double gw = (double)grad_total[0] * (double)T.weight;
    if (T.kind == SMIRK_LOSS_SQUARE) {
        const double scale = n > 0.0 ? 2.0 * gw / n : 0.0;                         // the product below is taken in float64 and rounded once: these terms are a
        const int total = T.rows * T.row_stride;                                   // few KB, and their gradients enter the ill-conditioned backward of the chain
#pragma unroll 4
        for (int i = 0; i < LOSS_ITEMS; ++i) {
            const int e = local * SMIRK_LOSS_CHUNK + i * LOSS_BLOCK + (int)threadIdx.x;
            if (e >= total) break;
            const int r = e / T.row_stride, c = e - r * T.row_stride;
            float g = 0.0f;
            if (n > 0.0 && c < T.cols && (!T.flags || T.flags[r])) g = (float)(scale * ((double)T.pred[e] - (T.target ? (double)T.target[e] : 0.0)));
            T.grad[e] = g;
        }
    } else {
        const float scale = (float)(gw / n);                                       // n >= 1: validated on the host
        const int HW = T.HW, C = T.C, npix = T.rows * HW;
        if ((HW & 3) == 0) {
            const int nq = npix >> 2, qhw = HW >> 2;
#pragma unroll 2
            for (int i = 0; i < LOSS_ITEMS / 4; ++i) {
                const int q = local * (SMIRK_LOSS_CHUNK / 4) + i * LOSS_BLOCK + (int)threadIdx.x;
                if (q >= nq) break;
                const int b = q / qhw, o = (q - b * qhw) << 2;
                const size_t base = (size_t)b * C * HW + o;
                for (int ch = 0; ch < C; ++ch) {
                    const f32x4 p = *(const f32x4*)(T.pred + base + (size_t)ch * HW);
                    const f32x4 t = *(const f32x4*)(T.target + base + (size_t)ch * HW);
                    const float d0 = p.x - t.x, d1 = p.y - t.y, d2 = p.z - t.z, d3 = p.w - t.w;
                    f32x4 g;                                                       // sign(0) = 0, like torch's l1_loss backward
                    g.x = d0 > 0.0f ? scale : d0 < 0.0f ? -scale : 0.0f; g.y = d1 > 0.0f ? scale : d1 < 0.0f ? -scale : 0.0f;
                    g.z = d2 > 0.0f ? scale : d2 < 0.0f ? -scale : 0.0f; g.w = d3 > 0.0f ? scale : d3 < 0.0f ? -scale : 0.0f;
                    *(f32x4*)(T.grad + base + (size_t)ch * HW) = g;
                }
            }
        } else {
#pragma unroll 2
            for (int i = 0; i < LOSS_ITEMS; ++i) {
                const int p = local * SMIRK_LOSS_CHUNK + i * LOSS_BLOCK + (int)threadIdx.x;
                if (p >= npix) break;
                const int b = p / HW, o = p - b * HW;
                const size_t base = (size_t)b * C * HW + o;
                for (int ch = 0; ch < C; ++ch) {
                    const float d = T.pred[base + (size_t)ch * HW] - T.target[base + (size_t)ch * HW];
                    T.grad[base + (size_t)ch * HW] = d > 0.0f ? scale : d < 0.0f ? -scale : 0.0f;
                }
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------------
static inline bool loss_misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }

// items a term is chunked over: forward = participating candidates (row term) or pixels; backward = the full gradient extent (row term) or pixels
static inline long long loss_items(const SmirkLossTerm& t, bool backward) {
    if (t.kind == SMIRK_LOSS_ABS_IMAGE) return (long long)t.rows * t.HW;
    return (long long)t.rows * (backward ? t.row_stride : t.cols);
}
static inline long long loss_chunks(long long items) { return (items + SMIRK_LOSS_CHUNK - 1) / SMIRK_LOSS_CHUNK; }

static int loss_validate(const SmirkLossTerm* terms, int n_terms) {
    if (!terms || n_terms < 1 || n_terms > SMIRK_LOSS_MAX_TERMS) return SMIRK_ERR_BAD_ARG;
    for (int k = 0; k < n_terms; ++k) {
        const SmirkLossTerm& t = terms[k];
        if (!t.pred || t.rows < 1 || t.cols < 1 || t.row_stride < 1 || t.cols > t.row_stride) return SMIRK_ERR_BAD_ARG;
        if (t.kind != SMIRK_LOSS_SQUARE && t.kind != SMIRK_LOSS_ABS_IMAGE) return SMIRK_ERR_BAD_ARG;
        if (loss_misaligned(t.pred) || loss_misaligned(t.target) || loss_misaligned(t.grad) || loss_misaligned(t.loss_img)) return SMIRK_ERR_BAD_ARG;
        if (t.kind == SMIRK_LOSS_ABS_IMAGE) {
            if (t.C < 1 || t.HW < 1 || !t.target || t.row_flags) return SMIRK_ERR_BAD_ARG;
            if ((long long)t.C * t.HW != (long long)t.row_stride || t.cols != t.row_stride) return SMIRK_ERR_BAD_ARG;
        } else if (t.loss_img) {
            return SMIRK_ERR_BAD_ARG;
        }
    }
    for (int k = 0; k < n_terms; ++k)
        if ((long long)terms[k].rows * terms[k].row_stride > (long long)INT_MAX - SMIRK_LOSS_CHUNK) return SMIRK_ERR_UNSUPPORTED;   // the last chunk's indices stay ints
    return SMIRK_OK;
}

extern "C" size_t smirk_loss_workspace_bytes(const SmirkLossTerm* terms, int n_terms) {
    if (loss_validate(terms, n_terms) != SMIRK_OK) return 0;
    long long chunks = 0;
    for (int k = 0; k < n_terms; ++k) chunks += loss_chunks(loss_items(terms[k], false));
    return smirk_align_up((size_t)chunks * sizeof(double), 256);
}

// -> number of chunks; terms without a gradient pointer get none in the backward layout
static int loss_fill(LossArgs& a, const SmirkLossTerm* terms, int n_terms, bool backward) {
    long long chunk = 0;
    a.n = n_terms;
    for (int k = 0; k <= n_terms; ++k) {
        LossTermDev& d = a.t[k];
        d = LossTermDev{};
        d.chunk0 = (int)chunk;
        if (k == n_terms) break;
        const SmirkLossTerm& t = terms[k];
        d.pred = t.pred; d.target = t.target; d.flags = t.row_flags; d.loss_img = t.loss_img; d.grad = t.grad;
        d.rows = t.rows; d.row_stride = t.row_stride; d.cols = t.cols; d.kind = t.kind; d.C = t.C; d.HW = t.HW; d.weight = t.weight;
        if (!backward || t.grad) chunk += loss_chunks(loss_items(t, backward));
    }
    return (int)chunk;
}

static double loss_bytes(const SmirkLossTerm* terms, int n_terms, bool backward) {
    double b = 0.0;
    for (int k = 0; k < n_terms; ++k) {
        const SmirkLossTerm& t = terms[k];
        if (backward && !t.grad) continue;
        const double slice = (double)t.rows * t.cols * sizeof(float) * (t.target ? 2.0 : 1.0) + (t.row_flags ? (double)t.rows : 0.0);
        if (backward) b += slice + (double)t.rows * t.row_stride * sizeof(float);
        else b += slice + (t.loss_img ? (double)t.rows * t.HW * sizeof(float) : 0.0);
    }
    return b;
}

extern "C" int smirk_loss_forward(const SmirkLossTerm* terms, int n_terms, float* out_terms, float* out_total, void* ws, size_t ws_bytes, void* stream) {
    if (!out_terms || !out_total || !ws || loss_misaligned(ws)) return SMIRK_ERR_BAD_ARG;
    const int bad = loss_validate(terms, n_terms);
    if (bad != SMIRK_OK) return bad;
    if (ws_bytes < smirk_loss_workspace_bytes(terms, n_terms)) return SMIRK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    LossArgs a;
    const int chunks = loss_fill(a, terms, n_terms, false);
    double* partials = (double*)ws;
    smirk_prof_next(nullptr, 0.0, loss_bytes(terms, n_terms, false) + (double)chunks * sizeof(double));
    SMIRK_LAUNCH(loss_partial_kernel, dim3((unsigned)chunks), dim3(LOSS_BLOCK), 0, st, a, partials);
    smirk_prof_next(nullptr, 0.0, (double)chunks * sizeof(double) + (n_terms + 1) * sizeof(float));
    SMIRK_LAUNCH(loss_finalise_kernel, dim3(1), dim3(64 * SMIRK_LOSS_MAX_TERMS), 0, st, a, (const double*)partials, out_terms, out_total);
    return smirk_launch_status();
}

extern "C" int smirk_loss_backward(const SmirkLossTerm* terms, int n_terms, const float* grad_total, void* ws, size_t ws_bytes, void* stream) {
    if (!grad_total || !ws || loss_misaligned(ws)) return SMIRK_ERR_BAD_ARG;
    const int bad = loss_validate(terms, n_terms);
    if (bad != SMIRK_OK) return bad;
    if (ws_bytes < smirk_loss_workspace_bytes(terms, n_terms)) return SMIRK_ERR_WORKSPACE;
    LossArgs a;
    const int chunks = loss_fill(a, terms, n_terms, true);
    if (chunks == 0) return SMIRK_OK;                                              // no term asks for a gradient
    smirk_prof_next(nullptr, 0.0, loss_bytes(terms, n_terms, true));
    SMIRK_LAUNCH(loss_backward_kernel, dim3((unsigned)chunks), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, a, grad_total);
    return smirk_launch_status();
}
