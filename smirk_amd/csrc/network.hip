// Whole-network entries of libsmirk_hip.so: ONE host call enqueues every layer of a module's forward on the caller's stream.
//
//   smirk_generator_forward   SmirkGenerator.forward   (src/smirk_generator.py:51-86; _block :88-119; ResnetBlock :121-178)
//   smirk_backbone_forward    one sub-encoder of SmirkEncoder.forward: timm MobileNetV3-minimal features[-1] -> GAP -> Linear (+ clamps)
//                             (src/smirk_encoder.py:34-45, :66-73, :95-110; backbone per SURVEY.md App. A)
//
// Both halves of this file have the same frame.  Which kernel serves a convolution is decided by the dispatchers of conv.hip / conv_patch.hip / encoder_ops.hip /
// encoder_head.hip / mbconv*.hip; which ENTRY serves a level of the generator or a block of a backbone is decided here, once per call, by a pure plan function:
//                  plan                                        forward: a walk over the plan      bytes of the plan                   the plan, device-free
//   generator      plan_generator (+ gen_chain_count)          smirk_generator_forward[_packed]   smirk_generator_workspace_bytes     smirk_generator_plan
//   backbone       backbone_plan (backbone_block_family)       smirk_backbone_forward             smirk_backbone_workspace_bytes      smirk_backbone_plan
// A plan reads the weights' shape fields, the call's sizes and the kernels' own `*_supported` / `*_eligible` statements; it follows no pointer.  The forwards launch
// what the plan says and return what a launch returns.  What moves here is the host-side walk (~60 launches for the generator, ~35-50 per backbone): from Python +
// ctypes (~15 ms per 128-frame step, more than the GPU time of the step) to straight C++ (a few hundred microseconds), and the activation memory from the
// framework's allocator to a caller-provided workspace that is laid out once:
//   * U-Net skip tensors e1..e4 have fixed slots,
//   * everything else rotates through three scratch slots sized for the largest temporary (a layer reads at most two temporaries —
//     input and residual — and writes one).
// No allocation, no synchronisation; every pointer is a device pointer except the weight structs (host structs of device pointers).
#include <sys/syscall.h>
#include <unistd.h>
#include <stdlib.h>

#include "conv_common.h"
#include "../../include/smirk_handoff.h"
#include "../../include/smirk_generator_plan.h"
#include "../../include/smirk_generator_arith.h"

namespace {

struct Arena {
    char* base;
    size_t off;
    void* take(size_t bytes) {
        off = smirk_align_up(off, 256);
        void* p = base ? base + off : nullptr;
        off += bytes;
        return p;
    }
};

// three rotating scratch slots; pick() returns a slot that holds neither `a` nor `b`
struct Rot {
    void* slot[3];
    void* pick(const void* a, const void* b) const {
        for (int i = 0; i < 3; ++i)
            if (slot[i] != a && slot[i] != b) return slot[i];
        return nullptr;
    }
};

inline size_t act_bytes(int B, int H, int W, int C) { return (size_t)B * H * W * C * 4; }

// arith: the SMIRK_PRECISION_* value of the layer (the generator: gen_level_arith; the backbones: their weights' precision)
int conv_call(int arith, const SmirkConvDesc& d, const void* in0, const void* in1, const SmirkConvLayer& L, const void* residual, void* out,
              void* stream) {
    if (arith == SMIRK_PRECISION_F16X1) return smirk_conv_dispatch_gen_x1(&d, in0, in1, L.w, L.scale, L.shift, residual, out, stream);
    return arith == SMIRK_PRECISION_F16X3 ? smirk_conv_igemm_f16x3(&d, in0, in1, L.w, L.scale, L.shift, residual, out, stream)
                 : smirk_conv_igemm_f32(&d, (const float*)in0, (const float*)in1, (const float*)L.w, L.scale, L.shift, (const float*)residual,
                                        (float*)out, stream);
}

SmirkConvDesc desc3x3(int B, int H, int W, int c0, int c1, int cout, bool reflect, bool relu) {
    SmirkConvDesc d;
    d.B = B; d.H = H; d.W = W; d.C0 = c0; d.C1 = c1; d.Cout = cout; d.KH = d.KW = 3; d.stride = 1; d.pad_t = d.pad_l = 1;
    d.Ho = H; d.Wo = W; d.pad_mode = reflect ? SMIRK_PAD_REFLECT : SMIRK_PAD_ZERO; d.act = relu ? SMIRK_ACT_RELU : SMIRK_ACT_NONE;
    d.out_mode = SMIRK_OUT_NHWC;
    return d;
}

SmirkConvDesc desc1x1(int B, int H, int W, int cin, int cout, bool relu, bool convt) {
    SmirkConvDesc d;
    d.B = B; d.H = H; d.W = W; d.C0 = cin; d.C1 = 0; d.Cout = cout; d.KH = d.KW = 1; d.stride = 1; d.pad_t = d.pad_l = 0;
    d.Ho = H; d.Wo = W; d.pad_mode = SMIRK_PAD_ZERO; d.act = relu ? SMIRK_ACT_RELU : SMIRK_ACT_NONE;
    d.out_mode = convt ? SMIRK_OUT_CONVT2X2 : SMIRK_OUT_NHWC;
    return d;
}

#define TRY(expr)                      \
    do {                               \
        const int rc_ = (expr);        \
        if (rc_ != SMIRK_OK) return rc_; \
    } while (0)

// ---- the arithmetic of a level ------------------------------------------------------------------------------------------------------------------------------------
// SMIRK_PRECISION_F16X1 (inference only) keeps the split16 storage of F16X3 everywhere — weight images, workspace, pack / pool / hand-off kernels, range
// audit — and issues ONE fp16 MFMA per product block, on the hi halves, in every convolution of the levels l >= GEN_X1_FROM: both encoder convolutions, the
// ConvTranspose2d or its composed form, both decoder convolutions, and (level 4) the bottleneck and the ResNet blocks.  Levels below run exactly the launches of F16X3.
// A layer's arithmetic is a function of the precision and its level ALONE (never of the batch, the chains, taps or a kernel switch): where a kernel family has no
// one-MFMA form (enc1_fused, the 32-channel conv_upcat, the patch kernels, conv_pp) the plan sends the layer to one that has (conv_halo_x1_kernel,
// conv_halo_up_x1_kernel, the 64-channel conv3x3_ring / conv3x3_upcat kernels in X1, conv_igemm_kernel<..., X1>), never to the three-MFMA form.
// 1: every level-1 layer (112^2 x 64 at 224^2: ring, pool-fused ring, upcat) measured 1.39-1.79x faster in its one-MFMA form at 128 and at 1024 frames, the
// levels below 1.5-2.2x (profiles/x1_per_launch_x3_vs_x1.txt).  Level 0 (224^2 x 32: enc1_fused, patch, fused tail) is not bound by the matrix pipe.
constexpr int GEN_X1_FROM = 1;

bool gen_split(const SmirkGeneratorWeights* w) { return w->precision == SMIRK_PRECISION_F16X3 || w->precision == SMIRK_PRECISION_F16X1; }

// level 0..3, 4 = bottleneck + ResNet blocks -> SMIRK_PRECISION_*: what the forward hands to conv_call and what smirk_generator_arith reports
int gen_level_arith(const SmirkGeneratorWeights* w, int level) {
    return w->precision == SMIRK_PRECISION_F16X1 ? (level >= GEN_X1_FROM ? SMIRK_PRECISION_F16X1 : SMIRK_PRECISION_F16X3) : w->precision;
}
bool gen_level_x1(const SmirkGeneratorWeights* w, int level) { return gen_level_arith(w, level) == SMIRK_PRECISION_F16X1; }

bool gen_args_ok(const SmirkGeneratorWeights* w, int B, int H, int W) {
    if (!w || B <= 0 || H <= 0 || W <= 0 || H % 16 || W % 16) return false;
    if (w->res_blocks < 0 || w->res_blocks > SMIRK_GEN_MAX_RES || w->features <= 0 || w->out_channels <= 0 || w->out_channels > 4) return false;
    if (gen_split(w)) return w->features % 8 == 0 && w->cin_pad == 8 && w->in_channels <= 8;
    return w->precision == SMIRK_PRECISION_F32 && w->features % 8 == 0 && w->cin_pad % 4 == 0 && w->cin_pad >= w->in_channels;
}

// ---- how many sub-batch chains run the deep part of the network ---------------------------------------------------------------------------------------------------
// The layers at H/4 and below rarely fill whole rounds of workgroups on the 256 CUs (14 x 14 x 512: 196 B / 256 tiles x 4 = 1.53 rounds at 128 frames = 2 rounds
// of time, 3.06 -> 4 at 256; the 28 x 28 and 56 x 56 layers likewise), and each waits for the one before it.  Frames are independent, so the SECTION — encoder4,
// bottleneck, ResNet blocks, decoder4 (levels l >= GEN_SECTION_FROM) — runs as TWO (optionally three) sub-batch chains on as many streams (the caller's and
// library-owned side streams, forked / joined with events): while one chain's layer drains its partial last round the other chain's workgroups take the free CUs.
// Bit-identical results (batch invariance, tests/test_scale_gpu.py run with it forced).  Measured with the RCCL gather enqueued, same box (profiles/r04l_, r04m_,
// r04n_): +3.2 % at 128 frames per pass, +4.5 % at 256, +1.2 % at 1024 for the H/8 + H/16 part -> taken when > 5 % of a 14 x 14 layer's last round would idle.
// $SMIRK_GEN_SPLIT_CHAINS=0 / 2 / 3 selects the number of chains (the A/B switch of tests/test_generator_gpu.py).  The section starts at H/8: starting it at H/4
// measured 8,801 vs 8,857 faces/s at 128 frames, 9,406 vs 9,473 at 256, 9,872 vs 9,782 at 1024 (profiles/r04n_chain_from.txt; the 56 x 56 layers fill their rounds) and
// the switch for it left the library.  Batches below 16 frames are never split by the heuristic (a fork / join costs more than the idle part of their only round).
constexpr int GEN_SECTION_FROM = 3;

// The WISH, a pure function: taps copy whole tensors and the launch profiler times launches on ONE stream, so either keeps one chain; `forced` is the switch's value.
int gen_chain_count(int features, int B, int H, int W, bool taps, bool profiling, int forced, int cus) {
    if (B < 2 || taps || profiling) return 1;
    const double rounds = ((double)B * (H >> 4) * (W >> 4) / 256.0) * ((features << 4) / 128.0) / cus;      // 256 x 128 tiles of a 14 x 14 layer per CU
    const double full = (double)(long long)(rounds + 0.999999);
    int n = B >= 16 && full > 0 && (full - rounds) / full > 0.05 ? 2 : 1;
    if (forced) n = forced;
    return n > B ? B : n;
}

int gen_chain_wish(const SmirkGeneratorWeights* w, int B, int H, int W, bool taps) {
    return gen_chain_count(w->features, B, H, W, taps, g_smirk_prof_on, smirk_switch(SMIRK_SW_GEN_SPLIT_CHAINS), smirk_device_cus());
}

// The GRANT.  Side streams and the fork / join events are owned per HOST THREAD and device (thread_local): two threads driving the same device neither race on the
// lazy creation nor record / wait on each other's events; created once, reused by every forward of that thread (re-recording an event only affects later waits).
// RAII: a host thread that ends releases its side streams and events (a thread pool of short-lived workers leaked 2 streams + 3 events per thread; advisor r05).
// The destructor runs at thread exit; work still queued on a side stream completes first (hipStreamDestroy defers the release until the stream drains).
struct ChainResources {
    hipStream_t side[64][2] = {};
    hipEvent_t ev[64][3] = {};
    ~ChainResources() {
        // the MAIN thread's thread_locals are destroyed inside exit(), where the HIP runtime may already be shutting down: the process exit reclaims them
        if ((long)syscall(SYS_gettid) == (long)getpid()) return;
        int cur = 0;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        for (int d = 0; d < 64; ++d) {
            bool any = false;
            for (int k = 0; k < 2; ++k) any = any || side[d][k];
            for (int k = 0; k < 3; ++k) any = any || ev[d][k];
            if (!any) continue;
            if (hipSetDevice(d) != hipSuccess) { (void)hipGetLastError(); continue; }
            for (int k = 0; k < 2; ++k) if (side[d][k]) (void)hipStreamDestroy(side[d][k]);
            for (int k = 0; k < 3; ++k) if (ev[d][k]) (void)hipEventDestroy(ev[d][k]);
        }
        if (have) (void)hipSetDevice(cur);
        (void)hipGetLastError();
    }
};

struct ChainGrant {
    int n;                                                          // `want`, or 1: no fork
    hipStream_t side[2];
    hipEvent_t fork, join[2];
};

// `want` chains with their streams and events, or ONE chain: while `stream` is being captured (or cannot say), without a current device, or when an event or a
// stream cannot be created.
ChainGrant grant_chains(int want, hipStream_t stream) {
    ChainGrant g = {1, {nullptr, nullptr}, nullptr, {nullptr, nullptr}};
    if (want < 2) return g;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return g; }
    thread_local ChainResources res;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return g; }
    for (int k = 0; k < 3; ++k)
        if (!res.ev[dev][k] && hipEventCreateWithFlags(&res.ev[dev][k], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); res.ev[dev][k] = nullptr; return g; }
    for (int k = 0; k + 1 < want; ++k) {
        if (!res.side[dev][k] && hipStreamCreateWithFlags(&res.side[dev][k], hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); res.side[dev][k] = nullptr; return g; }
        g.side[k] = res.side[dev][k];
    }
    g.fork = res.ev[dev][0]; g.join[0] = res.ev[dev][1]; g.join[1] = res.ev[dev][2];
    g.n = want;
    return g;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------------------------------------
// Everything a generator forward decides before it launches (DESIGN.md 28 has the family table): a pure function of the weights' SHAPE fields, the sources' channel
// counts (0 + 0: the packed entry), the batch, the image size, whether taps are wanted and the chain count it is granted.  It follows no pointer (`ws` only becomes
// addresses); the kernel switches reach it through the kernels' own `*_supported` / `*_eligible` statements, which are not restated here.  `r` is what
// smirk_generator_plan reports (include/smirk_generator_plan.h describes every field); r.input = -1 stands for the fp32 pair of sources that no pack kernel serves.
// Levels l = 0..3 work at H >> l x W >> l with features << l channels (encoder l + 1, decoder l + 1).
struct GenPlan {
    SmirkGeneratorPlanReport r;
    bool fast;                                                      // split-fp16 with 32 features: what every specialised generator kernel is written for
    void *x, *e[4];                                                 // packed network input [B][H][W][cin_pad], skip tensors
    Rot rot;
    void *upcat_w[2], *upcat_s[2];                                  // levels 0 / 1 (index = l): composed weights and shift rows (conv_upcat.hip), rebuilt by every forward
    void *updeep_w[2], *updeep_s[2], *updeep_k[2];                  // levels 2 / 3 (index = l - 2): composed coarse-tap weights, shift rows, skip-half conv rows (conv_halo.hip)
};

GenPlan plan_generator(const SmirkGeneratorWeights* w, int Ca, int Cb, int B, int H, int W, bool taps, int nchain, void* ws) {
    GenPlan p = {};
    SmirkGeneratorPlanReport& r = p.r;
    const bool split = gen_split(w);
    const int f = w->features;
    p.fast = split && f == 32;
    r.input = Ca == 0 && Cb == 0 ? SMIRK_GEN_INPUT_PACKED : split ? SMIRK_GEN_INPUT_SPLIT_PACK : Cb == 0 ? SMIRK_GEN_INPUT_NHWC_PAD
              : Ca == 3 && Cb == 3 && w->cin_pad == 8 ? SMIRK_GEN_INPUT_PACK_F32 : -1;
    r.nchain = nchain;
    r.section_from = GEN_SECTION_FROM;
    for (int k = 0; k < nchain; ++k) {                              // chain k owns frames [B k / n, B (k + 1) / n)
        r.chain_b0[k] = (int)((long long)B * k / nchain);
        r.chain_nb[k] = (int)((long long)B * (k + 1) / nchain) - r.chain_b0[k];
    }
    for (int l = 0; l < 4; ++l) {
        const int h = H >> l, wd = W >> l, c = f << l;
        const bool whole = l < GEN_SECTION_FROM;                    // above the section: one launch sequence for the whole batch
        const bool x3 = split && !gen_level_x1(w, l);               // enc1_fused and the 32-channel conv_upcat exist in the three-MFMA form only
        const SmirkConvDesc conv2 = desc3x3(B, h, wd, c, 0, c, false, true);
        r.enc[l] = l == 0 && x3 && smirk_enc1_fused_supported(w->cin_pad, f, h, wd) ? SMIRK_GEN_ENC_ENC1_FUSED
                   : whole && split && smirk_conv3x3_pool_supported(&conv2) ? SMIRK_GEN_ENC_CONV_POOLFUSED : SMIRK_GEN_ENC_CONV_CONV_POOL;
        // Levels 0 / 1 compose their weights inside their own entry.  Levels 2 / 3: the composed weights exist only where the WHOLE batch is eligible (ONE launch builds
        // them ahead of the fork, for every chain to read); a chain takes UPDEEP where they exist and its own frames are eligible, so a batch whose level tensor passes
        // 2 GiB runs PAIR in every chain.
        const bool composed = l >= 2 && p.fast && smirk_updeep_eligible(B, h, wd, c);
        if (composed) r.compose_mask |= 1 << l;
        for (int k = 0; k < SMIRK_GEN_MAX_CHAINS; ++k) {
            if (k >= (whole ? 1 : nchain)) r.dec[l][k] = -1;
            else if (l < 2) r.dec[l][k] = p.fast && (x3 || c == 64) && smirk_conv3x3_upcat_eligible(c, h, wd) ? SMIRK_GEN_DEC_UPCAT : SMIRK_GEN_DEC_PAIR;
            else r.dec[l][k] = composed && smirk_updeep_eligible(whole ? B : r.chain_nb[k], h, wd, c) ? SMIRK_GEN_DEC_UPDEEP : SMIRK_GEN_DEC_PAIR;
        }
    }
    const SmirkConvDesc last = desc3x3(B, H, W, f, 0, f, false, true);
    r.fused_tail = p.fast && !gen_level_x1(w, 0) && !taps && H >= 64 && smirk_conv3x3_tail_supported(&last, w->out_channels);
    // Workspace: the layout depends on neither switches, taps nor chains (callers size and cache workspaces from smirk_generator_workspace_bytes).
    Arena a{(char*)ws, 0};
    p.x = a.take(act_bytes(B, H, W, w->cin_pad));
    for (int l = 0; l < 4; ++l) p.e[l] = a.take(act_bytes(B, H >> l, W >> l, f << l));
    for (int i = 0; i < 3; ++i) p.rot.slot[i] = a.take(act_bytes(B, H, W, f));      // the largest temporary: enc1conv1 out, up1, dec1conv1 out
    for (int l = 0; l < 2 && p.fast; ++l) {
        p.upcat_w[l] = a.take(smirk_conv3x3_upcat_weff_bytes(f << l));
        p.upcat_s[l] = a.take(smirk_conv3x3_upcat_shift_bytes(f << l));
    }
    for (int l = 2; l < 4 && p.fast; ++l) {
        p.updeep_w[l - 2] = a.take(smirk_updeep_weff_bytes(f << l));
        p.updeep_s[l - 2] = a.take(smirk_updeep_shift_bytes(f << l));
        p.updeep_k[l - 2] = a.take(smirk_updeep_wskip_bytes(f << l));
    }
    r.workspace_bytes = smirk_align_up(a.off, 256);
    return p;
}

// ---- the emitters: one level's launches on `nb` frames, every pointer already resolved by the caller (whole-batch tensors, or a chain's views) -----------------------
int pool2x2(bool split, const void* in, void* out, int nb, int h, int wd, int c, void* strm) {
    return split ? smirk_maxpool2x2_split16(in, out, nb, h, wd, c, strm) : smirk_maxpool2x2_nhwc((const float*)in, (float*)out, nb, h, wd, c, strm);
}

void tap_copy(void* tap, const void* src, size_t bytes, void* strm) {
    if (tap) (void)hipMemcpyAsync(tap, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)strm);
}

// the slots an encoder level writes, in the order the families have always picked them (which slot a tensor lands in is part of "same bits, same overlap")
void encoder_slots(const Rot& rot, int family, const void* in, void*& t1, void*& pooled) {
    t1 = family == SMIRK_GEN_ENC_ENC1_FUSED ? nullptr : rot.pick(in, nullptr);
    pooled = family == SMIRK_GEN_ENC_CONV_POOLFUSED ? rot.pick(t1, nullptr) : rot.pick(nullptr, nullptr);
}

// encoder level l (smirk_generator.py:52-59): in [h][wd][cin] -> conv -> t1 -> conv -> skip [h][wd][c] -> pool -> pooled
int encoder_level(const SmirkGeneratorWeights* w, int family, int l, int nb, int h, int wd, int cin, const void* in, void* t1, void* skip, void* pooled, void* tap,
                  void* strm) {
    const bool split = gen_split(w);
    const int c = w->features << l, arith = gen_level_arith(w, l);
    const SmirkConvLayer *c1 = &w->enc[l][0], *c2 = &w->enc[l][1];
    const SmirkConvDesc d1 = desc3x3(nb, h, wd, cin, 0, c, false, true), d2 = desc3x3(nb, h, wd, c, 0, c, false, true);
    switch (family) {
        case SMIRK_GEN_ENC_ENC1_FUSED:
            TRY(smirk_enc1_fused_split16(in, c1->w, c1->scale, c1->shift, c2->w, c2->scale, c2->shift, skip, pooled, nb, h, wd, strm));
            break;
        case SMIRK_GEN_ENC_CONV_POOLFUSED:
            TRY(conv_call(arith, d1, in, nullptr, *c1, nullptr, t1, strm));
            TRY(smirk_conv3x3_pool_launch(&d2, t1, nullptr, c2->w, c2->scale, c2->shift, skip, pooled, strm, arith == SMIRK_PRECISION_F16X1));
            break;
        default:                                                    // SMIRK_GEN_ENC_CONV_CONV_POOL
            TRY(conv_call(arith, d1, in, nullptr, *c1, nullptr, t1, strm));
            TRY(conv_call(arith, d2, t1, nullptr, *c2, nullptr, skip, strm));
            break;
    }
    tap_copy(tap, skip, act_bytes(nb, h, wd, c), strm);
    return family == SMIRK_GEN_ENC_CONV_CONV_POOL ? pool2x2(split, skip, pooled, nb, h, wd, c, strm) : SMIRK_OK;
}

SmirkUpdeepLevel updeep_level(const SmirkGeneratorWeights* w, const GenPlan& p, int l) {
    return SmirkUpdeepLevel{w->features << l, &w->up[3 - l], &w->dec[3 - l][0], p.updeep_w[l - 2], p.updeep_s[l - 2], p.updeep_k[l - 2]};
}

void decoder_slots(const Rot& rot, int family, const void* coarse, void*& tmp, void*& out) {
    tmp = family == SMIRK_GEN_DEC_UPCAT ? nullptr : rot.pick(coarse, nullptr);
    out = rot.pick(family == SMIRK_GEN_DEC_UPCAT ? coarse : tmp, nullptr);
}

// the first half of decoder level l (smirk_generator.py:65-75): ConvTranspose2d k2 s2 of coarse [h/2][wd/2][2c], cat with skip [h][wd][c], conv -> out [h][wd][c];
// tmp holds `up` (PAIR) or the coarse launch's partial sums (UPDEEP)
int decoder_level(const SmirkGeneratorWeights* w, const GenPlan& p, int family, int l, int nb, int h, int wd, const void* coarse, const void* skip, void* tmp,
                  void* out, void* strm) {
    const int c = w->features << l, arith = gen_level_arith(w, l);
    const SmirkConvLayer &up = w->up[3 - l], &conv = w->dec[3 - l][0];
    switch (family) {
        case SMIRK_GEN_DEC_UPCAT:
            return smirk_conv3x3_upcat_launch(c, coarse, skip, &up, &conv, out, nb, h, wd, p.upcat_w[l], p.upcat_s[l], (hipStream_t)strm, arith == SMIRK_PRECISION_F16X1);
        case SMIRK_GEN_DEC_UPDEEP: {                                // launch 2 is the ordinary 3x3 convolution over the skip tensor with launch 1's output as its residual
            const SmirkUpdeepLevel u = updeep_level(w, p, l);
            TRY(smirk_updeep_coarse_launch(&u, coarse, tmp, nb, h, wd, arith == SMIRK_PRECISION_F16X1, (hipStream_t)strm));
            const SmirkConvLayer half{u.wskip, conv.scale, conv.shift};
            return conv_call(arith, desc3x3(nb, h, wd, c, 0, c, false, true), skip, nullptr, half, tmp, out, strm);
        }
        default:                                                    // SMIRK_GEN_DEC_PAIR
            TRY(conv_call(arith, desc1x1(nb, h / 2, wd / 2, 2 * c, c, false, true), coarse, nullptr, up, nullptr, tmp, strm));
            return conv_call(arith, desc3x3(nb, h, wd, c, c, c, false, true), tmp, skip, conv, nullptr, out, strm);
    }
}

}  // namespace

extern "C" size_t smirk_generator_workspace_bytes(const SmirkGeneratorWeights* w, int B, int H, int W) {
    if (!gen_args_ok(w, B, H, W)) return 0;
    return plan_generator(w, 0, 0, B, H, W, false, 1, nullptr).r.workspace_bytes;
}

extern "C" int smirk_genplan_abi_version(void) { return SMIRK_GENPLAN_ABI_VERSION; }

extern "C" int smirk_genarith_abi_version(void) { return SMIRK_GENARITH_ABI_VERSION; }

extern "C" int smirk_generator_arith(const SmirkGeneratorWeights* w, int32_t* x1_from, int32_t level_arith[4], int32_t* deep_arith) {
    if (!w || !x1_from || !level_arith || !deep_arith || (!gen_split(w) && w->precision != SMIRK_PRECISION_F32)) return SMIRK_ERR_BAD_ARG;
    *x1_from = GEN_X1_FROM;
    for (int l = 0; l < 4; ++l) level_arith[l] = gen_level_arith(w, l);
    *deep_arith = gen_level_arith(w, 4);
    return SMIRK_OK;
}

extern "C" int smirk_generator_plan(const SmirkGeneratorWeights* w, int Ca, int Cb, int B, int H, int W, int with_taps, SmirkGeneratorPlanReport* report) {
    if (!gen_args_ok(w, B, H, W) || !report) return SMIRK_ERR_BAD_ARG;
    const bool packed = Ca == 0 && Cb == 0;
    if (packed ? !gen_split(w) : (Ca <= 0 || Cb < 0 || Ca + Cb != w->in_channels)) return SMIRK_ERR_BAD_ARG;
    *report = plan_generator(w, Ca, Cb, B, H, W, with_taps != 0, gen_chain_wish(w, B, H, W, with_taps != 0), nullptr).r;
    return report->input < 0 ? SMIRK_ERR_UNSUPPORTED : SMIRK_OK;
}

// The one body of the two whole-network entries, a walk over the plan: smirk_generator_forward packs cat(a, b) into the workspace first,
// smirk_generator_forward_packed (include/smirk_handoff.h) hands in `packed`, the same tensor written by masking_handoff_kernel, and the pack step is left out.
static int generator_forward_body(const SmirkGeneratorWeights* w, const float* a, int Ca, const float* b, int Cb, const void* packed, float* y, int B, int H,
                                  int W, void* const* taps, void* ws, size_t ws_bytes, void* stream) {
    const int wish = gen_chain_wish(w, B, H, W, taps != nullptr);
    GenPlan p = plan_generator(w, Ca, Cb, B, H, W, taps != nullptr, wish, ws);
    if (ws_bytes < p.r.workspace_bytes) return SMIRK_ERR_WORKSPACE;
    if (p.r.input < 0) return SMIRK_ERR_UNSUPPORTED;
    const ChainGrant cg = grant_chains(wish, (hipStream_t)stream);
    if (cg.n != wish) p = plan_generator(w, Ca, Cb, B, H, W, taps != nullptr, cg.n, ws);
    const SmirkGeneratorPlanReport& r = p.r;
    const bool split = gen_split(w);
    const int f = w->features, L0 = GEN_SECTION_FROM, deep = gen_level_arith(w, 4);
    auto tap = [&](int i) { return taps ? taps[i] : nullptr; };

    // ---- cat + NCHW -> NHWC (+ split) of the network input (smirk_trainer.py:94, demo.py:167), and the composed weights of the deep decoder levels ------------------
    switch (r.input) {
        case SMIRK_GEN_INPUT_PACKED: break;                         // already in the network's input format
        case SMIRK_GEN_INPUT_SPLIT_PACK: TRY(smirk_pack_generator_input_split16(a, Ca, b, Cb, p.x, B, H, W, stream)); break;
        case SMIRK_GEN_INPUT_NHWC_PAD: TRY(smirk_nchw_to_nhwc_pad(a, (float*)p.x, B, Ca, H, W, w->cin_pad, stream)); break;
        default: TRY(smirk_pack_generator_input(a, b, (float*)p.x, B, H, W, stream)); break;
    }
    if (r.compose_mask) {
        SmirkUpdeepLevel todo[2];
        int n = 0;
        for (int l = 2; l < 4; ++l)
            if (r.compose_mask & (1 << l)) todo[n++] = updeep_level(w, p, l);
        TRY(smirk_updeep_compose(todo, n, (hipStream_t)stream));
    }
    // ---- encoder levels above the section, whole batch --------------------------------------------------------------------------------------------------------------
    const void* cur = packed ? packed : p.x;
    for (int l = 0; l < L0; ++l) {
        void *t1, *pl;
        encoder_slots(p.rot, r.enc[l], cur, t1, pl);
        TRY(encoder_level(w, r.enc[l], l, B, H >> l, W >> l, l ? f << (l - 1) : w->cin_pad, cur, t1, p.e[l], pl, tap(l), stream));
        cur = pl;
    }
    // ---- the section (smirk_generator.py:56-68, :121-178), once per chain ---------------------------------------------------------------------------------------------
    // Memory: temporaries rotate through the three scratch slots, each sized for the largest tensor of the network (B x H x W x f elements = 4x the largest tensor of
    // this section).  The chains run at different paces and would otherwise put tensors of DIFFERENT shapes (so different frame offsets) into one slot at the same
    // time: chain k keeps its temporaries in QUARTER k + 1 of every slot, indexed from frame 0; only the tensors that cross the section's boundary use the whole-batch
    // layout — its input (the pooled tensor of the level above), the skip tensors, its output — which all lie inside quarter 0 with frame ranges that are disjoint
    // between the chains; the output never shares a slot with the input (one chain may finish while another still reads its input frames).
    const size_t quarter = (act_bytes(B, H, W, f) / 4) & ~(size_t)255;
    const int h16 = H >> 4, w16 = W >> 4, c16 = f << 4;
    auto section = [&](int k, void* strm, const void* in, const void*& out) -> int {
        const int b0 = r.chain_b0[k], nb = r.chain_nb[k];
        const size_t priv = r.nchain > 1 ? quarter * (size_t)(k + 1) : 0;
        auto N = [&](const void* base, int h, int wd, int c) { return (char*)base + act_bytes(b0, h, wd, c); };     // this chain's frames of a whole-batch tensor
        auto P = [&](const void* base) { return (char*)base + priv; };                                               // a chain-private temporary
        const void* cur = N(in, H >> L0, W >> L0, f << (L0 - 1));
        const void* cur_slot = in;
        for (int l = L0; l < 4; ++l) {
            const int h = H >> l, wd = W >> l, c = f << l;
            void *t1, *pl;
            encoder_slots(p.rot, r.enc[l], cur_slot, t1, pl);
            TRY(encoder_level(w, r.enc[l], l, nb, h, wd, c / 2, cur, P(t1), N(p.e[l], h, wd, c), P(pl), tap(l), strm));   // (taps => one chain over the whole batch)
            cur = P(pl); cur_slot = pl;
        }
        void* b1 = p.rot.pick(cur_slot, nullptr);                   // bottleneck
        TRY(conv_call(deep, desc3x3(nb, h16, w16, c16 / 2, 0, c16, false, true), cur, nullptr, w->enc[4][0], nullptr, P(b1), strm));
        void* b2 = p.rot.pick(b1, nullptr);
        TRY(conv_call(deep, desc3x3(nb, h16, w16, c16, 0, c16, false, true), P(b1), nullptr, w->enc[4][1], nullptr, P(b2), strm));
        tap_copy(tap(4), b2, act_bytes(B, h16, w16, c16), strm);
        const void* dc = b2;                                        // ResNet blocks: reflect pad, conv-BN-ReLU, reflect pad, conv-BN, + x
        for (int i = 0; i < w->res_blocks; ++i) {
            void* t = p.rot.pick(dc, nullptr);
            TRY(conv_call(deep, desc3x3(nb, h16, w16, c16, 0, c16, true, true), P(dc), nullptr, w->res[i][0], nullptr, P(t), strm));
            void* o = p.rot.pick(dc, t);
            TRY(conv_call(deep, desc3x3(nb, h16, w16, c16, 0, c16, true, false), P(t), nullptr, w->res[i][1], P(dc), P(o), strm));
            dc = o;
        }
        tap_copy(tap(5), dc, act_bytes(B, h16, w16, c16), strm);
        for (int l = 3; l >= L0; --l) {                             // decoder levels of the section; the last one writes the whole-batch layout
            const int h = H >> l, wd = W >> l, c = f << l;
            void *tmp, *d1;
            decoder_slots(p.rot, r.dec[l][k], dc, tmp, d1);
            TRY(decoder_level(w, p, r.dec[l][k], l, nb, h, wd, P(dc), N(p.e[l], h, wd, c), P(tmp), P(d1), strm));
            const bool last = l == L0;
            void* d2 = last ? p.rot.pick(d1, in) : p.rot.pick(d1, nullptr);
            TRY(conv_call(gen_level_arith(w, l), desc3x3(nb, h, wd, c, 0, c, false, true), P(d1), nullptr, w->dec[3 - l][1], nullptr, last ? N(d2, h, wd, c) : P(d2), strm));
            tap_copy(tap(6 + (3 - l)), d2, act_bytes(B, h, wd, c), strm);
            dc = d2;
        }
        out = dc;
        return SMIRK_OK;
    };
    const void* dcur = nullptr;
    if (r.nchain > 1) {
        int rc = hipEventRecord(cg.fork, (hipStream_t)stream) == hipSuccess ? SMIRK_OK : SMIRK_ERR_LAUNCH;
        bool forked[2] = {false, false};
        for (int k = r.nchain - 1; rc == SMIRK_OK && k >= 0; --k) {   // chain 0 runs on the caller's stream, enqueued last
            hipStream_t st_k = k == 0 ? (hipStream_t)stream : cg.side[k - 1];
            if (k > 0 && hipStreamWaitEvent(st_k, cg.fork, 0) != hipSuccess) { rc = SMIRK_ERR_LAUNCH; break; }
            if (k > 0) forked[k - 1] = true;
            rc = section(k, (void*)st_k, cur, dcur);
            if (rc == SMIRK_OK && k > 0 && hipEventRecord(cg.join[k - 1], st_k) != hipSuccess) rc = SMIRK_ERR_LAUNCH;
        }
        for (int k = 0; rc == SMIRK_OK && k + 1 < r.nchain; ++k)
            if (hipStreamWaitEvent((hipStream_t)stream, cg.join[k], 0) != hipSuccess) rc = SMIRK_ERR_LAUNCH;
        if (rc != SMIRK_OK) {
            // a chain failed part-way: whatever was enqueued on the side streams still reads / writes the caller's workspace.  The caller's stream must not run
            // ahead of it (the workspace may be reused or freed in stream order), so the side streams are drained before the error is returned.
            for (int k = 0; k < 2; ++k)
                if (forked[k]) (void)hipStreamSynchronize(cg.side[k]);
            return rc;
        }
    } else {
        TRY(section(0, stream, cur, dcur));
    }
    // ---- decoder levels above the section, whole batch, and the network tail ----------------------------------------------------------------------------------------
    for (int l = L0 - 1; l >= 0; --l) {
        const int h = H >> l, wd = W >> l, c = f << l;              // output resolution of this level
        void *tmp, *t1;
        decoder_slots(p.rot, r.dec[l][0], dcur, tmp, t1);
        TRY(decoder_level(w, p, r.dec[l][0], l, B, h, wd, dcur, p.e[l], tmp, t1, stream));
        const SmirkConvLayer& c2 = w->dec[3 - l][1];
        const SmirkConvDesc d2 = desc3x3(B, h, wd, c, 0, c, false, true);
        if (l == 0 && r.fused_tail) return smirk_conv3x3_tail_f16x3(&d2, t1, nullptr, c2.w, c2.scale, c2.shift, w->final_w, w->final_b, y, w->out_channels, stream);
        void* t2 = p.rot.pick(t1, nullptr);
        TRY(conv_call(gen_level_arith(w, l), d2, t1, nullptr, c2, nullptr, t2, stream));
        tap_copy(tap(6 + (3 - l)), t2, act_bytes(B, h, wd, c), stream);
        dcur = t2;
    }
    return split ? smirk_conv1x1_sigmoid_nchw_split16(dcur, w->final_w, w->final_b, y, B, H, W, f, w->out_channels, stream)
                 : smirk_conv1x1_sigmoid_nchw((const float*)dcur, w->final_w, w->final_b, y, B, H, W, f, w->out_channels, stream);
}

extern "C" int smirk_generator_forward(const SmirkGeneratorWeights* w, const float* a, int Ca, const float* b, int Cb, float* y, int B, int H,
                                       int W, void* const* taps, void* ws, size_t ws_bytes, void* stream) {
    if (!gen_args_ok(w, B, H, W) || !a || !y || !ws || Ca <= 0 || Cb < 0 || Ca + Cb != w->in_channels || (Cb > 0 && !b)) return SMIRK_ERR_BAD_ARG;
    if (!w->final_w || !w->final_b) return SMIRK_ERR_BAD_ARG;
    return generator_forward_body(w, a, Ca, b, Cb, nullptr, y, B, H, W, taps, ws, ws_bytes, stream);
}

extern "C" int smirk_generator_forward_packed(const SmirkGeneratorWeights* w, const void* packed, float* y, int B, int H, int W, void* const* taps, void* ws,
                                              size_t ws_bytes, void* stream) {
    if (!gen_args_ok(w, B, H, W) || !gen_split(w) || !packed || !y || !ws) return SMIRK_ERR_BAD_ARG;
    if (!w->final_w || !w->final_b) return SMIRK_ERR_BAD_ARG;
    return generator_forward_body(w, nullptr, 0, nullptr, 0, packed, y, B, H, W, taps, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// MobileNetV3-minimal backbone + pooled linear head
// ------------------------------------------------------------------------------------------------------------------------------------
namespace {

bool backbone_args_ok(const SmirkBackboneWeights* w, int B, int H, int W) {
    if (!w || B <= 0 || H < 32 || W < 32 || w->n_blocks <= 0 || w->n_blocks > SMIRK_BACKBONE_MAX_BLOCKS || w->n_out < 0) return false;
    if (w->precision != SMIRK_PRECISION_F16X3 && w->precision != SMIRK_PRECISION_F32) return false;
    if (w->n_out > 0 && (!w->head_w || !w->head_b)) return false;                    // n_out == 0: features only, no head
    return w->stem.w && w->stem.scale && w->stem.shift && w->stem_cout > 0;
}

// The backbone's A/B switches (switches.h) as values: the entries read them once per call, so a test may set and unset them between calls.
struct BackboneSwitches {
    bool no_image, no_tile, no_fused, no_head;
};

BackboneSwitches backbone_switches() {
    return {smirk_switch(SMIRK_SW_DISABLE_MBCONV_IMAGE) != 0, smirk_switch(SMIRK_SW_DISABLE_MBCONV_TILE) != 0, smirk_switch(SMIRK_SW_DISABLE_MBCONV_FUSED) != 0,
            smirk_switch(SMIRK_SW_DISABLE_ENCODER_HEAD_FUSED) != 0};
}

// Which kernel family serves one block on an h x w input: the first row of this table whose condition holds (DESIGN.md 19 lists what every block of the two
// backbones takes).  Rows 2-4 are for InvertedResidual blocks in the split-fp16 precision, unless $SMIRK_DISABLE_MBCONV_FUSED; each `*_supported` is the kernel's own
// statement of what it serves and is not restated here.
//   1  CONV1X1        ConvBnAct 1x1: one implicit-GEMM launch
//   2  MBCONV_IMAGE   smirk_mbconv_image_supported (stride 1: one wave per 2 x 14 halo band, or whole images per workgroup), unless $SMIRK_DISABLE_MBCONV_IMAGE, and unless
//                     $SMIRK_DISABLE_MBCONV_TILE keeps a block that row 4 also serves on the 8 x 8-tile kernel
//   3  MBCONV_S2      stride 2, no residual, smirk_mbconv_s2_supported: one wave per output tile
//   4  MBCONV_TILE    smirk_mbconv_supported: 8 x 8 output tiles.  The FALLBACK of rows 2 and 3 — feature maps of more than 224 pixels with a side that is no multiple of 14, and the
//                     IMAGE / TILE switches; at 224 x 224 no block of either backbone reaches it by default
//   5  DS_UNFUSED     DepthwiseSeparable: depthwise, pointwise.  Never fused: it has no expanded tensor to keep on chip (202 vs 200 us at stride 1, 97 vs 66 at
//      IR_UNFUSED     stride 2).  InvertedResidual: pointwise, depthwise, pointwise
int backbone_block_family(const SmirkMbBlock& b, int h, int w, bool split, const BackboneSwitches& sw) {
    if (b.kind == 2) return SMIRK_BACKBONE_CONV1X1;
    if (b.kind == 1 && split && !sw.no_fused) {
        const bool tile = smirk_mbconv_supported(b.cin, b.mid, b.cout, b.stride);
        if (!sw.no_image && !(sw.no_tile && tile) && smirk_mbconv_image_supported(h, w, b.cin, b.mid, b.cout, b.stride)) return SMIRK_BACKBONE_MBCONV_IMAGE;
        if (b.stride == 2 && !b.skip && smirk_mbconv_s2_supported(b.cin, b.mid, b.cout)) return SMIRK_BACKBONE_MBCONV_S2;
        if (tile) return SMIRK_BACKBONE_MBCONV_TILE;
    }
    return b.kind == 0 ? SMIRK_BACKBONE_DS_UNFUSED : SMIRK_BACKBONE_IR_UNFUSED;
}

// Everything smirk_backbone_forward decides before it launches: a pure function of the weights' SHAPE fields, the batch, the image size and the switch values (no
// pointer target, no environment, no device).  The workspace is three rotating slots sized for the largest activation any schedule of these blocks reads or writes —
// the unfused temporaries included, because a switch may turn fusion off on the next call with the same workspace — and the pooled vectors of the head.
struct BackbonePlan {
    bool ok;                                            // false: the channels do not chain (stem_cout -> blocks -> feat_ch)
    struct Block { int family, h, w, ho, wo; } blk[SMIRK_BACKBONE_MAX_BLOCKS];    // blk[0].family == SMIRK_BACKBONE_HEAD_FUSED: stem + block 0 in one launch
    size_t slot_off[3], pooled_off, total;
};

BackbonePlan backbone_plan(const SmirkBackboneWeights* w, int B, int H, int W, const BackboneSwitches& sw) {
    BackbonePlan p;
    p.ok = false;
    const bool split = w->precision == SMIRK_PRECISION_F16X3;
    int h = (H + 1) / 2, wd = (W + 1) / 2, c = w->stem_cout;
    size_t m = (size_t)B * h * wd * c;                   // largest activation, in elements
    for (int i = 0; i < w->n_blocks; ++i) {
        const SmirkMbBlock& b = w->blocks[i];
        if (b.cin != c || b.stride < 1) return p;
        const int ho = (h + b.stride - 1) / b.stride, wo = (wd + b.stride - 1) / b.stride;
        const size_t in_mid = (size_t)B * h * wd * b.mid, out_mid = (size_t)B * ho * wo * b.mid, out = (size_t)B * ho * wo * b.cout;
        if (b.kind == 1 && in_mid > m) m = in_mid;
        if (b.kind != 2 && out_mid > m) m = out_mid;
        if (out > m) m = out;
        p.blk[i] = {backbone_block_family(b, h, wd, split, sw), h, wd, ho, wo};
        h = ho; wd = wo; c = b.cout;
    }
    if (c != w->feat_ch) return p;
    p.ok = true;
    const SmirkMbBlock& b0 = w->blocks[0];
    if (split && !sw.no_head && smirk_encoder_head_supported(w->stem_cout, b0.kind, b0.cin, b0.mid, b0.cout, b0.stride, b0.skip))
        p.blk[0].family = SMIRK_BACKBONE_HEAD_FUSED;    // encoder_head.hip: the 16-channel 112 x 112 tensors between stem and block 0 never reach HBM
    size_t off = 0;
    for (int i = 0; i < 3; ++i) { p.slot_off[i] = smirk_align_up(off, 256); off = p.slot_off[i] + m * 4; }
    p.pooled_off = smirk_align_up(off, 256);
    p.total = smirk_align_up(p.pooled_off + (size_t)B * w->feat_ch * 4, 256);
    return p;
}

}  // namespace

extern "C" size_t smirk_backbone_workspace_bytes(const SmirkBackboneWeights* w, int B, int H, int W) {
    if (!backbone_args_ok(w, B, H, W)) return 0;
    const BackbonePlan p = backbone_plan(w, B, H, W, BackboneSwitches{});          // (the layout does not depend on the switches)
    return p.ok ? p.total : 0;
}

extern "C" int smirk_backbone_plan(const SmirkBackboneWeights* w, int B, int H, int W, int* family, int cap) {
    if (!backbone_args_ok(w, B, H, W) || cap < 0 || (cap > 0 && !family)) return SMIRK_ERR_BAD_ARG;
    const BackbonePlan p = backbone_plan(w, B, H, W, backbone_switches());
    if (!p.ok) return SMIRK_ERR_BAD_ARG;
    for (int i = 0; i < w->n_blocks && i < cap; ++i) family[i] = p.blk[i].family;
    return w->n_blocks;
}

extern "C" int smirk_backbone_forward(const SmirkBackboneWeights* w, const float* img, int B, int H, int W, float* out, void* feat_out,
                                      void* ws, size_t ws_bytes, void* stream) {
    if (!backbone_args_ok(w, B, H, W) || !img || !ws || (w->n_out > 0 && !out) || (w->n_out == 0 && !feat_out)) return SMIRK_ERR_BAD_ARG;
    const BackbonePlan p = backbone_plan(w, B, H, W, backbone_switches());
    if (!p.ok) return SMIRK_ERR_BAD_ARG;
    if (ws_bytes < p.total) return SMIRK_ERR_WORKSPACE;
    const bool split = w->precision == SMIRK_PRECISION_F16X3;
    Rot rot;
    for (int i = 0; i < 3; ++i) rot.slot[i] = (char*)ws + p.slot_off[i];
    float* pooled = (float*)((char*)ws + p.pooled_off);
    auto pointwise = [&](const void* in, int hh, int ww, int cin, int cout, const SmirkConvLayer& L, bool relu, const void* res, void* o) {
        return conv_call(w->precision, desc1x1(B, hh, ww, cin, cout, relu, false), in, nullptr, L, res, o, stream);
    };
    auto depthwise = [&](const void* in, int hh, int ww, int c, int stride, const SmirkConvLayer& L, void* o) {
        return split ? smirk_dwconv3x3_split16(in, (const float*)L.w, L.scale, L.shift, o, B, hh, ww, c, stride, 1, stream)
                     : smirk_dwconv3x3((const float*)in, (const float*)L.w, L.scale, L.shift, (float*)o, B, hh, ww, c, stride, 1, stream);
    };
    void* x = nullptr;                                  // the current activation: none yet where the fused head reads the image itself
    if (p.blk[0].family != SMIRK_BACKBONE_HEAD_FUSED) {
        x = rot.slot[0];
        TRY(split ? smirk_stem_conv_s2_split16(img, (const float*)w->stem.w, w->stem.scale, w->stem.shift, x, B, H, W, w->stem_cout, stream)
                  : smirk_stem_conv_s2(img, (const float*)w->stem.w, w->stem.scale, w->stem.shift, (float*)x, B, H, W, w->stem_cout, stream));
    }
    for (int i = 0; i < w->n_blocks; ++i) {
        const SmirkMbBlock& b = w->blocks[i];
        const BackbonePlan::Block& q = p.blk[i];
        const void* res = b.skip ? x : nullptr;
        void* t = rot.pick(x, nullptr);                 // the two slots that do not hold x: temporaries of the unfused sequences, one of them the output
        void* u = rot.pick(x, t);
        void* o = t;
        switch (q.family) {
            case SMIRK_BACKBONE_HEAD_FUSED:
                TRY(smirk_encoder_head_fused_split16(img, (const float*)w->stem.w, w->stem.scale, w->stem.shift, (const float*)b.dw.w, b.dw.scale, b.dw.shift,
                                                     b.pw.w, b.pw.scale, b.pw.shift, b.skip ? 1 : 0, o, B, H, W, b.stride, stream));
                break;
            case SMIRK_BACKBONE_CONV1X1:
                TRY(pointwise(x, q.h, q.w, b.cin, b.cout, b.pw, true, nullptr, o));
                break;
            case SMIRK_BACKBONE_MBCONV_IMAGE:
                TRY(smirk_mbconv_image_split16(x, b.pw.w, b.pw.scale, b.pw.shift, (const float*)b.dw.w, b.dw.scale, b.dw.shift, b.pwl.w, b.pwl.scale, b.pwl.shift,
                                               b.skip ? 1 : 0, o, B, q.h, q.w, b.cin, b.mid, b.cout, stream));
                break;
            case SMIRK_BACKBONE_MBCONV_S2:
                TRY(smirk_mbconv_s2_split16(x, b.pw.w, b.pw.scale, b.pw.shift, (const float*)b.dw.w, b.dw.scale, b.dw.shift, b.pwl.w, b.pwl.scale, b.pwl.shift,
                                            o, B, q.h, q.w, b.cin, b.mid, b.cout, stream));
                break;
            case SMIRK_BACKBONE_MBCONV_TILE:
                TRY(smirk_mbconv_fused_split16(x, b.pw.w, b.pw.scale, b.pw.shift, (const float*)b.dw.w, b.dw.scale, b.dw.shift, b.pwl.w, b.pwl.scale, b.pwl.shift,
                                               b.skip ? 1 : 0, o, B, q.h, q.w, b.cin, b.mid, b.cout, b.stride, stream));
                break;
            case SMIRK_BACKBONE_DS_UNFUSED:             // dw + BN + ReLU -> pw + BN (+ x)
                o = u;
                TRY(depthwise(x, q.h, q.w, b.cin, b.stride, b.dw, t));
                TRY(pointwise(t, q.ho, q.wo, b.cin, b.cout, b.pw, false, res, o));
                break;
            default:                                    // SMIRK_BACKBONE_IR_UNFUSED: pw + BN + ReLU -> dw + BN + ReLU -> pwl + BN (+ x)
                TRY(pointwise(x, q.h, q.w, b.cin, b.mid, b.pw, true, nullptr, t));
                TRY(depthwise(t, q.h, q.w, b.mid, b.stride, b.dw, u));
                TRY(pointwise(u, q.ho, q.wo, b.mid, b.cout, b.pwl, false, res, o));
                break;
        }
        x = o;
    }
    const int hw = p.blk[w->n_blocks - 1].ho * p.blk[w->n_blocks - 1].wo, c = w->feat_ch;
    if (feat_out) (void)hipMemcpyAsync(feat_out, x, (size_t)B * hw * c * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (w->n_out == 0) return SMIRK_OK;
    TRY(split ? smirk_gap_linear_split16(x, w->head_w, w->head_b, out, pooled, B, hw, c, w->n_out, stream)
              : smirk_gap_linear((const float*)x, w->head_w, w->head_b, out, pooled, B, hw, c, w->n_out, stream));
    if (w->clamp_n_exp >= 0) TRY(smirk_expression_clamps(out, B, w->clamp_n_exp, stream));
    return SMIRK_OK;
}
