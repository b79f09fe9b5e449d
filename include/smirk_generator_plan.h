/* smirk_generator_plan.h — extension table of libsmirk_hip.so for ONE query: what a whole-network generator entry (smirk_generator_forward of smirk_hip.h,
 * smirk_generator_forward_packed of smirk_handoff.h) would launch for a given call, answered from plan_generator (csrc/network.hip) without touching device memory.
 * It is for tests and tools; nothing on the hot path calls it.
 *
 * It is versioned on its own (the version function below): the tables of smirk_hip.h, smirk_mica.h, smirk_emotion.h, smirk_optim.h and smirk_handoff.h and their
 * versions do not move when an entry is added here.
 */
#ifndef SMIRK_GENERATOR_PLAN_H
#define SMIRK_GENERATOR_PLAN_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_GENPLAN_ABI_VERSION 1

int smirk_genplan_abi_version(void);

/* How the network input reaches its packed NHWC form. */
enum SmirkGenInput {
    SMIRK_GEN_INPUT_PACKED = 0,         /* the packed entry: the caller's tensor is the network input, no launch */
    SMIRK_GEN_INPUT_SPLIT_PACK = 1,     /* split-fp16: smirk_pack_generator_input_split16 */
    SMIRK_GEN_INPUT_NHWC_PAD = 2,       /* fp32, one source: smirk_nchw_to_nhwc_pad */
    SMIRK_GEN_INPUT_PACK_F32 = 3        /* fp32, 3 + 3 channels on cin_pad 8: smirk_pack_generator_input */
};

/* The launches of one encoder level (two convolutions -> skip tensor, 2 x 2 max-pool). */
enum SmirkGenEncoder {
    SMIRK_GEN_ENC_ENC1_FUSED = 0,       /* smirk_enc1_fused_split16: the whole level in one launch */
    SMIRK_GEN_ENC_CONV_POOLFUSED = 1,   /* a convolution, then smirk_conv3x3_pool_f16x3 */
    SMIRK_GEN_ENC_CONV_CONV_POOL = 2    /* three launches */
};

/* The launches of a decoder level's ConvTranspose2d + first convolution over cat(up, skip); the level's second convolution (or the fused tail) follows. */
enum SmirkGenDecoder {
    SMIRK_GEN_DEC_UPCAT = 0,            /* conv_upcat.hip: composed into one convolution (its weights are composed by a launch of their own just before) */
    SMIRK_GEN_DEC_UPDEEP = 1,           /* conv_halo.hip: conv_halo_up_kernel, then the skip-half convolution with its output as the residual */
    SMIRK_GEN_DEC_PAIR = 2              /* ConvTranspose2d, then the two-source convolution */
};

#define SMIRK_GEN_MAX_CHAINS 3

/* Levels are indexed by l = 0..3: level l works at H >> l x W >> l with features << l channels (encoder1..4, decoder1..4).  Levels l >= section_from run inside the
 * section that is split into sub-batch chains; chain k owns frames [chain_b0[k], chain_b0[k] + chain_nb[k]). */
typedef struct SmirkGeneratorPlanReport {
    int32_t input;                             /* SmirkGenInput */
    int32_t nchain;                            /* the chains a forward on a stream that is not being captured gets (1: no fork) */
    int32_t chain_b0[SMIRK_GEN_MAX_CHAINS], chain_nb[SMIRK_GEN_MAX_CHAINS];
    int32_t section_from;
    int32_t enc[4];                            /* SmirkGenEncoder per level */
    int32_t dec[4][SMIRK_GEN_MAX_CHAINS];      /* SmirkGenDecoder per level and chain; whole-batch levels use [l][0]; -1 elsewhere */
    int32_t compose_mask;                      /* bit l: smirk_updeep_compose builds level l's composed weights (one launch for all set bits, ahead of the fork) */
    int32_t fused_tail;                        /* 1: smirk_conv3x3_tail_f16x3 ends the network; 0: decoder1's second convolution, then smirk_conv1x1_sigmoid_nchw* */
    uint64_t workspace_bytes;                  /* what smirk_generator_workspace_bytes returns */
} SmirkGeneratorPlanReport;

/* The plan of a call of smirk_generator_forward with sources of Ca and Cb channels — or, with Ca == 0 and Cb == 0, of smirk_generator_forward_packed — on B frames of H x W,
 * with or without taps, under the environment switches as they are now.  Only the shape fields of `w` are read (precision, features, cin_pad, in_channels,
 * out_channels, res_blocks); no pointer is followed.
 * SMIRK_ERR_BAD_ARG where the entry itself would refuse the shape (the conditions of smirk_generator_workspace_bytes returning 0, Ca + Cb != in_channels, the packed
 * entry with another precision than split-fp16, report == NULL); SMIRK_ERR_UNSUPPORTED for an fp32 pair of sources that is not 3 + 3 channels on cin_pad 8. */
int smirk_generator_plan(const SmirkGeneratorWeights* w, int Ca, int Cb, int B, int H, int W, int with_taps, SmirkGeneratorPlanReport* report);

#ifdef __cplusplus
}
#endif
#endif
