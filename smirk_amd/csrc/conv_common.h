// Shared pieces of the convolution kernels (conv.hip and the conv_*.hip units it dispatches to) and of the training units (wgrad.hip, train.hip,
// train_encoder.hip): argument block, GEMM-row -> pixel map, the split-fp16 conversions and the 8-channel group access, the XOR-swizzled LDS operand image,
// the operand-size predicate of the buffer-addressed loads, the grid of a grid-stride launch and the cross-unit launcher prototypes.
// See conv.hip for the design notes.
#pragma once
#include "common.h"

#define CV_BK 32

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

struct ConvArgs {
    SmirkConvDesc d;
    const float *in0, *in1, *w, *scale, *shift, *residual;   // F16X3: in0/in1/w/residual/out are split-fp16 tensors viewed as dwords
    float* out;
    int M, N, K, Cin;
    float* stats;  // train mode (BatchNorm statistics from the accumulators): per-tile partial column sums [rows][N][2] = (sum z, sum z^2) in fp32, or nullptr.
                   // Whoever fixes a launch's geometry states its row count next to it (conv_dispatch_one, smirk_conv3x3_ring64_launch); the fixed-order fp64
                   // reduction over the rows is bn_finalize_partials_kernel (train.hip)
    int psh;       // GEMM rows enumerate each image in (2^psh x 2^psh)-pixel patches (tile-major): a BM-row tile is then a compact 2-D
                   // patch whose 3x3 halo is ~1.3x its area instead of 3 full image rows — the im2col re-reads stay in L1/L2
};

// GEMM row -> (image, y, x).  Inside an image rows are ordered patch-major; any bijection is valid because every output
// address is computed from (b, y, x).
__device__ __forceinline__ void row_to_pixel(int m, int HoWo, int Wo, int psh, int& b, int& oy, int& ox) {
    b = m / HoWo;
    const int rem = m - b * HoWo;
    const int t = rem >> (2 * psh), in = rem & ((1 << (2 * psh)) - 1);
    const int tpr = Wo >> psh, ty = t / tpr, tx = t - ty * tpr;
    oy = (ty << psh) + (in >> psh);
    ox = (tx << psh) + (in & ((1 << psh) - 1));
}

__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = (i < 0) ? -i : i;
    return (i >= n) ? (2 * n - 2 - i) : i;
}

// 8 fp32 values -> split-fp16 group: out_hi = fp16(v), out_lo = fp16((v - hi) * 2^11)
__device__ __forceinline__ void split8(const float* v, half8& hi, half8& lo) {
    smirk_range_audit8(v);
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
        smirk_half2 h, l;
        smirk_split2(v[q], v[q + 1], h, l);
        hi[q] = h.x; hi[q + 1] = h.y; lo[q] = l.x; lo[q + 1] = l.y;
    }
}
// split WITHOUT an audit: for values that are the maximum / a copy of values audited a few lines earlier (the fused 2 x 2 max-pool outputs)
__device__ __forceinline__ void split8_noaudit(const float* v, half8& hi, half8& lo) {
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
        smirk_half2 h, l;
        smirk_split2(v[q], v[q + 1], h, l);
        hi[q] = h.x; hi[q + 1] = h.y; lo[q] = l.x; lo[q + 1] = l.y;
    }
}
// the same split for the hot epilogues: the range audit goes into the lane's running maximum (SmirkRangeAcc, common.h), tested once per kernel
template <typename RA>
__device__ __forceinline__ void split8(const float* v, half8& hi, half8& lo, RA& ra) {
    ra.see8(v);
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
        smirk_half2 h, l;
        smirk_split2(v[q], v[q + 1], h, l);
        hi[q] = h.x; hi[q + 1] = h.y; lo[q] = l.x; lo[q + 1] = l.y;
    }
}
__device__ __forceinline__ float join1(_Float16 hi, _Float16 lo) { return (float)hi + (float)lo * (1.0f / 2048.0f); }
// one 8-channel split16 group (hi halves, then lo halves) <-> 8 fp32 values: the access of every streaming kernel of the training units
__device__ __forceinline__ void load_group(const float* p, float* v) {
    const half8 hi = *(const half8*)p, lo = *(const half8*)(p + 4);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = join1(hi[q], lo[q]);
}
__device__ __forceinline__ void store_group(float* p, const float* v) {
    half8 hi, lo;
    split8(v, hi, lo);
    *(half8*)p = hi;
    *(half8*)(p + 4) = lo;
}


// LDS operand image: [rows][32 dwords] (one 128-byte K chunk per row), written by global_load_lds_dwordx4 — 64 lanes x 16 B =
// 8 consecutive rows per wave instruction, lane-linear, so no padding is possible.  Bank conflicts are removed by an XOR
// swizzle applied on the SOURCE side (which 16-byte piece of the row a lane fetches) and on the read side:
// physical piece = logical piece ^ ((row >> 1) & 7)  => the 16 rows of a ds_read_b128 lane group hit 16 distinct 16-byte slots.
__device__ __forceinline__ int lds_piece(int row, int piece) { return row * 32 + ((piece ^ ((row >> 1) & 7)) << 2); }


// XCD-aware tile id: hardware places block id on XCD id%8; give each XCD a contiguous run of logical tiles
__device__ __forceinline__ int xcd_logical(int id, int nblk) {
    const int xcd = id & 7, slot = id >> 3;
    const int q = nblk >> 3, r = nblk & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// grid of a grid-stride kernel with 256 threads per block: one thread per item, at most `cap` blocks
static inline unsigned blocks_for(size_t items, unsigned cap) {
    const size_t g = (items + 255) / 256;
    return (unsigned)(g > cap ? cap : (g ? g : 1));
}
// Buffer-addressed operand DMA (`buffer_load_dwordx4 ... offen lds`) reaches a tensor through 32-bit byte offsets and a 32-bit num_records: the tensor must
// end below 2 GiB.  `dwords` = its size in 4-byte elements (fp32, or split-fp16 pairs).
#define CONV_BUF_LIMIT (1ll << 31)
static inline bool conv_fits32(long long dwords) { return dwords * 4 < CONV_BUF_LIMIT; }
// both activation sources of a layer
static inline bool conv_inputs_fit32(const SmirkConvDesc& d) {
    const long long px = (long long)d.B * d.H * d.W;
    return conv_fits32(px * d.C0) && conv_fits32(px * d.C1);
}
// in0 / in1 / w of an implicit GEMM
static inline bool conv_operands_fit32(const ConvArgs& a) { return conv_inputs_fit32(a.d) && conv_fits32((long long)a.N * a.K); }

// the launch profiler's algorithmic work of an implicit GEMM (common.h smirk_prof_next): 2 M N K flop; every operand, the output and the residual once
static inline void conv_prof_next(const char* name, const ConvArgs& a) {
    if (!g_smirk_prof_on) return;
    const double px = (double)a.d.B * a.d.H * a.d.W;
    smirk_prof_next(name, 2.0 * a.M * a.N * a.K, 4.0 * (px * a.Cin + (double)a.M * a.N + (double)a.N * a.K + (a.residual ? (double)a.M * a.N : 0.0)));
}

// The kernel families conv_dispatch_one (conv.hip) tries before conv_igemm_kernel, in this order.  A family that writes ConvArgs::stats has its partial-row
// count computed by whoever fixes its launch geometry.
// conv_ring.hip: 16 x 16 patches, weights streamed through an LDS ring, two workgroups per CU (Cout = 64 at 112 x 112), optional fused 2 x 2 max-pool
bool smirk_conv3x3_ring64_eligible(const SmirkConvDesc* d, bool has_residual);
int smirk_conv3x3_ring64_launch(const SmirkConvDesc* d, const void* in0, const void* in1, const void* w, const float* scale, const float* shift, void* out,
                                void* pooled, hipStream_t st, float* stats = nullptr, int* stats_rows = nullptr, bool x1 = false);
bool smirk_conv3x3_ring64_x1_eligible(const SmirkConvDesc* d, bool has_residual);      // x1: the one-MFMA form (the generator's f16x1 inference arithmetic), Cout = 64 only
// conv_upcat.hip: a decoder level's ConvTranspose2d(2c -> c, k2 s2) composed into the 3x3 convolution over cat(up, skip) (c = 32 / 64, split-fp16 only); the
// composed weights and the 16 shift rows are rebuilt per call into caller-provided workspace
bool smirk_conv3x3_upcat_eligible(int c, int H, int W);
size_t smirk_conv3x3_upcat_weff_bytes(int c);
size_t smirk_conv3x3_upcat_shift_bytes(int c);
int smirk_conv3x3_upcat_launch(int c, const void* d, const void* e, const SmirkConvLayer* up, const SmirkConvLayer* conv, void* out, int B, int H, int W,
                               void* weff, void* shift4, hipStream_t st, bool x1 = false);      // x1: c = 64 only
// conv.hip, for the generator's plan alone (network.hip): the dispatcher in the f16x1 inference arithmetic, where a layer may also take the one-MFMA ring kernel
// (the public smirk_conv_igemm_f16x1 keeps choosing what the training path was measured with), and the pool-fused entry in either arithmetic
int smirk_conv_dispatch_gen_x1(const SmirkConvDesc* d, const void* in0, const void* in1, const void* w, const float* scale, const float* shift, const void* residual,
                               void* out, void* stream);
int smirk_conv3x3_pool_launch(const SmirkConvDesc* d, const void* in0, const void* in1, const void* w, const float* scale, const float* shift, void* out,
                              void* pooled, void* stream, bool x1);
// conv_patch.hip: persistent halo-patch kernel for the large-image / few-channel 3x3 layers (split-fp16 only)
bool smirk_conv3x3_patch_eligible(const SmirkConvDesc* d, bool has_residual);
int smirk_conv3x3_patch_launch(const SmirkConvDesc* d, const void* in0, const void* in1, const void* w, const float* scale,
                               const float* shift, void* out, hipStream_t st, const float* fw, const float* fb, float* fout,
                               int fcout);
// conv.hip: what smirk_conv3x3_pool_f16x3 (conv + BN + ReLU + 2 x 2 max-pool on the ring kernel) and smirk_conv3x3_tail_f16x3 (conv + BN + ReLU + 1x1 conv + sigmoid on
// the patch kernel) serve; each entry answers SMIRK_ERR_UNSUPPORTED exactly where its predicate says no
bool smirk_conv3x3_pool_supported(const SmirkConvDesc* d);
bool smirk_conv3x3_tail_supported(const SmirkConvDesc* d, int fcout);
// conv_halo.hip: the ping-pong schedule with the A operand staged once per channel chunk (one pixel halo serves all nine taps); 256-row tiles x 4 wave rows
#define HS_BM 256
#define HS_WGM 4
bool smirk_conv_halo_eligible(const ConvArgs& a);
int smirk_conv_halo_launch(const ConvArgs& a, hipStream_t st, bool x1);
// conv_halo.hip: decoder levels with c = 128 / 256 output channels (split-fp16 only), ConvTranspose2d(2c -> c, k2 s2) composed into the level's first 3x3 convolution as
// TWO launches: conv_halo_up_kernel (2 x 2 coarse taps per output parity class -> partial', stored at the fine pixels) and the ordinary 3x3 convolution over the skip
// tensor with partial' as its residual.  smirk_updeep_compose rebuilds weff / shift16 / wskip of up to two levels in ONE launch, once per forward.
struct SmirkUpdeepLevel {
    int c;                                  // output channels of the level
    const SmirkConvLayer *up, *conv;        // the ConvTranspose2d layer (shift = bias) and the first 3x3 layer over cat(up, skip) with its folded BatchNorm
    void *weff, *shift16, *wskip;           // workspace of smirk_updeep_{weff,shift,wskip}_bytes(c)
};
size_t smirk_updeep_weff_bytes(int c);
size_t smirk_updeep_shift_bytes(int c);
size_t smirk_updeep_wskip_bytes(int c);
bool smirk_updeep_eligible(int B, int H, int W, int c);                 // H x W: the FINE image; both launches pass smirk_conv_halo_eligible with their own M
int smirk_updeep_compose(const SmirkUpdeepLevel* lv, int nlv, hipStream_t st);
int smirk_updeep_coarse_launch(const SmirkUpdeepLevel* lv, const void* d, void* partial, int B, int H, int W, bool x1, hipStream_t st);   // x1: conv_halo_up_x1_kernel
// conv_pp.hip: 8-wave ping-pong kernel (256 x 128 tile, 3-stage ring) for the deep split-fp16 3x3 layers
bool smirk_conv_pp_eligible(const ConvArgs& a);
int smirk_conv_pp_launch(const ConvArgs& a, hipStream_t st);
