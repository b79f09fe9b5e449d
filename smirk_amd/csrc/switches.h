// Environment switches of libsmirk_hip.so: the one place that names them and the one place that reads them (smirk_switch, capi.hip).
// Each one chooses between kernel families for the same operation (A/B tests, integrators' bisection); every one is read on every call, so a test may set
// and unset it between calls.
//
// variable                          values: what smirk_switch() returns, what it selects                                  default         used by
// SMIRK_IGEMM_HALO                  "0": 0, deep 3x3 convolutions stay off conv_halo_kernel; anything else ("a..."          1               tests/test_conv_gpu.py
//                                   included): 1, every eligible geometry on conv_halo_kernel.  "0" also puts the      tests/test_updeep_gpu.py
//                                   generator's decoder levels 3 / 4 back on their two launches (ConvTranspose, then
//                                   the convolution over cat(up, skip)) instead of conv_halo_up_kernel + the skip-half
//                                   convolution (their eligibility is conv_halo's)
// SMIRK_IGEMM_PP                    "0": 0, conv_pp_kernel off; "a...": 2, conv_pp_kernel for every eligible shape         1 (<= 16x16     tests/test_conv_gpu.py
//                                   (not only images of at most 256 pixels); anything else: 1                             images)
// SMIRK_CONV_RING                   "0": 0, the 64-output-channel ring kernels off (round-3 kernels) and the generator's   1               tests/test_conv_gpu.py,
//                                   decoder levels 1 / 2 back on their two launches (ConvTranspose, then the convolution                  tests/test_upcat_gpu.py
//                                   over cat(up, skip)) instead of conv3x3_upcat_kernel; anything else: 1
// SMIRK_DISABLE_PATCH_KERNEL        set (any value, "0" too): 1, neither the patch nor the ring convolution kernels        0               (integrators)
// SMIRK_DISABLE_ENC1_FUSED          set (any value): 1, smirk_enc1_fused_supported answers 0                              0               tests/test_conv_gpu.py
// The next four reach backbone_plan (network.hip) as one struct of values; its priority table says what each takes away:
// SMIRK_DISABLE_MBCONV_IMAGE        set (any value): 1, no image-resident MBConv kernel in the encoder backbone           0               tests/test_encoder_gpu.py,
// SMIRK_DISABLE_MBCONV_TILE         set (any value): 1, blocks that mbconv_fused_kernel (8 x 8 tiles) also serves stay    0               tests/test_backbone_
//                                   on it instead of the image-resident kernel: the 24-48-channel stride-1 blocks                         dispatch_{cpu,gpu}.py
// SMIRK_DISABLE_MBCONV_FUSED        set (any value): 1, no fused MBConv kernels (separate expand / depthwise / project)   0
// SMIRK_DISABLE_ENCODER_HEAD_FUSED  set (any value): 1, stem and first block of the backbone as separate launches         0
// SMIRK_GEN_SPLIT_CHAINS            the number of the generator's H/8 + H/16 sub-batch chains: "0": 1, "3": 3, else 2     0 (unset):      tests/test_generator_gpu.py,
//                                                                                                                         heuristic       bench.py
// SMIRK_WGRAD_F16                   atoi(value): 0 exact-fp32 weight-gradient kernel, 1 / 2 split-fp16 x3 with 1 / 2       2               tests/test_train_ops_gpu.py
//                                   chunks per barrier (+16: alternative LDS transpose lane geometry, diagnostic);                        (through smirk_conv_wgrad_
//                                   smirk_conv_wgrad_set_mode overrides it                                                                set_mode)
//
// Switches read by the Python package, not here: SMIRK_AMD_*_PRECISION, SMIRK_ENCODER_SERIAL, SMIRK_ENCODER_TRAIN_SERIAL, SMIRK_BN_STATS_UNFUSED,
// SMIRK_F16X3_RANGE_CHECK, SMIRK_HIP_LIBRARY, and
// SMIRK_DISABLE_MASKING_HANDOFF     set (any value): masking.demo_masked_image_packed, and with it the hull_mask= path of the pipelines, keeps the six separate
//                                   launches (rendered mask, two max pools, patch-centre field, composition, the generator's pack) instead of
//                                   masking_handoff_kernel + smirk_generator_forward_packed; same output bits (tests/test_masking_handoff_gpu.py,
//                                   tests/test_generator_packed_gpu.py).  The choice between the two is made where the tensors are allocated, in Python, so the
//                                   variable is read there and is not a member of the enum below.
// SMIRK_DISABLE_TRAIN_HANDOFF       set (any value): masking.train_masked_image_packed, and with it cycle.render_second_path / second_path_packed and
//                                   first_path.forward_first_path, keeps the separate utilities (two point samplings, transfer_pixels, rendered mask, masking,
//                                   the generator's own cat + pack) instead of sample_transfer_points_kernel + train_masking_handoff_kernel +
//                                   SmirkGenerator.forward_pair_packed; same output bits (tests/test_train_handoff_gpu.py).  Read in Python, like the one above.
#pragma once

#define SMIRK_WGRAD_F16_DEFAULT 2

enum SmirkSwitch {
    SMIRK_SW_IGEMM_HALO,
    SMIRK_SW_IGEMM_PP,
    SMIRK_SW_CONV_RING,
    SMIRK_SW_DISABLE_PATCH_KERNEL,
    SMIRK_SW_DISABLE_ENC1_FUSED,
    SMIRK_SW_DISABLE_MBCONV_IMAGE,
    SMIRK_SW_DISABLE_MBCONV_TILE,
    SMIRK_SW_DISABLE_MBCONV_FUSED,
    SMIRK_SW_DISABLE_ENCODER_HEAD_FUSED,
    SMIRK_SW_GEN_SPLIT_CHAINS,
    SMIRK_SW_WGRAD_F16,
    SMIRK_SW_COUNT
};

int smirk_switch(SmirkSwitch s);
