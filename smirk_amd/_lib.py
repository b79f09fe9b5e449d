"""ctypes binding of libsmirk_hip.so (C ABI declared in include/smirk_hip.h).

There is NO fallback: if the shared object is missing or a tensor is not on the HIP device the call raises.
torch is used for device memory and streams only; every pointer handed to the library is `tensor.data_ptr()`.
"""
import ctypes as C
import os
import struct

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libsmirk_hip.so")
LIB_PATH = os.environ.get("SMIRK_HIP_LIBRARY", LIB_PATH)      # tuning aid: A/B a differently-built libsmirk_hip.so in one gpurun
ABI_VERSION = 17
PACK_DEPTHWISE, PACK_STEM, PACK_CONVT2X2 = -3, -27, -2          # SmirkPackJob.KH markers (include/smirk_hip.h SMIRK_PACK_*)
SMIRK_OK, SMIRK_ERR_BAD_ARG, SMIRK_ERR_WORKSPACE, SMIRK_ERR_LAUNCH, SMIRK_ERR_UNSUPPORTED = 0, -1, -2, -3, -4      # include/smirk_hip.h

_p = C.c_void_p
_i = C.c_int
_sz = C.c_size_t


class SmirkFlameModel(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("V", "VP", "F", "n_shape", "n_exp", "KP", "n_static", "n_dyn", "n_lut",
                                         "n_full", "n_mp", "_pad")] + \
               [(n, _p) for n in ("dirs", "v_template", "lbs_weights", "jdirs", "jtemplate", "l_eyelid", "r_eyelid",
                                  "faces", "static_faces", "static_bary", "dyn_faces", "dyn_bary", "full_faces",
                                  "full_bary", "mp_faces", "mp_bary")]


class SmirkRenderMesh(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("V", "Vf", "Ff", "nnz")] + \
               [(n, _p) for n in ("keep", "faces", "nrm_ptr", "nrm_face", "nrm_corner")]


class SmirkConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "W", "C0", "C1", "Cout", "KH", "KW", "stride", "pad_t", "pad_l",
                                         "Ho", "Wo", "pad_mode", "act", "out_mode")]


class SmirkConvLayer(C.Structure):
    _fields_ = [("w", _p), ("scale", _p), ("shift", _p)]


GEN_MAX_RES, BACKBONE_MAX_BLOCKS = 16, 24
PRECISION_F32, PRECISION_F16X3, PRECISION_F16X1 = 0, 1, 2             # F16X1: the generator's whole-network entries only (include/smirk_generator_arith.h)
BACKBONE_FAMILIES = ("HEAD_FUSED", "CONV1X1", "MBCONV_IMAGE", "MBCONV_S2", "MBCONV_TILE", "DS_UNFUSED", "IR_UNFUSED")   # enum SmirkBackboneFamily, by code


class SmirkGeneratorWeights(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_channels", "out_channels", "features", "res_blocks", "precision", "cin_pad")] + \
               [("enc", SmirkConvLayer * 2 * 5), ("res", SmirkConvLayer * 2 * GEN_MAX_RES), ("up", SmirkConvLayer * 4),
                ("dec", SmirkConvLayer * 2 * 4), ("final_w", _p), ("final_b", _p)]


class SmirkMbBlock(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "stride", "cin", "mid", "cout", "skip")] + \
               [("pw", SmirkConvLayer), ("dw", SmirkConvLayer), ("pwl", SmirkConvLayer)]


class SmirkBackboneWeights(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_blocks", "precision", "n_out", "clamp_n_exp", "stem_cout", "feat_ch")] + \
               [("stem", SmirkConvLayer), ("blocks", SmirkMbBlock * BACKBONE_MAX_BLOCKS), ("head_w", _p), ("head_b", _p)]


class SmirkProfileRecord(C.Structure):
    _fields_ = [("kernel", C.c_char * 120), ("flop", C.c_double), ("bytes", C.c_double), ("ms", C.c_float), ("_pad", C.c_int32)]


LOSS_MAX_TERMS, LOSS_CHUNK = 8, 4096                            # include/smirk_hip.h SMIRK_LOSS_MAX_TERMS, SMIRK_LOSS_CHUNK
LOSS_SQUARE, LOSS_ABS_IMAGE = 0, 1                               # SmirkLossTerm.kind
VGG_TAPS, VGG_L1_CHUNK = 4, 4096                                 # include/smirk_hip.h SMIRK_VGG_TAPS, SMIRK_VGG_L1_CHUNK (8-channel groups of a half per partial)


class SmirkLossTerm(C.Structure):
    _fields_ = [("pred", _p), ("target", _p), ("row_flags", _p)] + \
               [(n, C.c_int32) for n in ("rows", "row_stride", "cols", "kind", "C", "HW")] + \
               [("weight", C.c_float), ("loss_img", _p), ("grad", _p)]


PAD_ZERO, PAD_REFLECT = 0, 1
ACT_NONE, ACT_RELU = 0, 1
OUT_NHWC, OUT_CONVT2X2 = 0, 1

_SIGS = {
    "smirk_strerror": (C.c_char_p, [_i]),
    "smirk_abi_version": (_i, []),
    "smirk_range_flag_peek": (C.c_uint, []),
    "smirk_range_flag_clear": (None, []),
    "smirk_flame_workspace_bytes": (_sz, [C.POINTER(SmirkFlameModel), _i]),
    "smirk_flame_forward": (_i, [C.POINTER(SmirkFlameModel), _i, _p, _i, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                 _p, _p, _sz, _p]),
    "smirk_flame_backward_workspace_bytes": (_sz, [C.POINTER(SmirkFlameModel), _i]),
    "smirk_flame_backward": (_i, [C.POINTER(SmirkFlameModel), _p, _i, _p, _i, _p, _i] + [_p] * 5 + [_p, _p] + [_p] * 4 + [_p] * 7 +
                             [_p, _sz, _p]),
    "smirk_vertices2landmarks": (_i, [_p, _i, _i, _p, _p, _p, _i, _p, _p]),
    "smirk_render_workspace_bytes": (_sz, [C.POINTER(SmirkRenderMesh), _i, _i, _i]),
    "smirk_render_forward": (_i, [C.POINTER(SmirkRenderMesh), _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "smirk_vertex_normals": (_i, [C.POINTER(SmirkRenderMesh), _i, _p, _p, _p]),
    "smirk_mask_face_weights": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "smirk_sample_faces": (_i, [_p, _i, _i, _i, C.c_uint64, C.c_uint64, _p, _p, _p]),
    "smirk_points_to_pixels": (_i, [_p, _i, _i, _i, _p, _p]),
    "smirk_maxpool_sq": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "smirk_bernoulli_field": (_i, [_p, _sz, C.c_float, C.c_uint64, C.c_uint64, _p]),
    "smirk_masking_compose": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, C.c_uint64, C.c_uint64, _p, _p]),
    "smirk_render_backward_workspace_bytes": (_sz, [C.POINTER(SmirkRenderMesh), _i, _i, _i]),
    "smirk_render_backward": (_i, [C.POINTER(SmirkRenderMesh), _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "smirk_project_landmarks_backward": (_i, [_p, _p, _p, _i, _i, _p, _p, _p]),
    "smirk_encoder_head_supported": (_i, [_i] * 7),
    "smirk_encoder_head_fused_split16": (_i, [_p] * 10 + [_i, _p] + [_i] * 4 + [_p]),
    "smirk_mbconv_image_supported": (_i, [_i] * 6),
    "smirk_mbconv_image_split16": (_i, [_p] * 10 + [_i, _p] + [_i] * 6 + [_p]),
    "smirk_mbconv_lds_bytes": (_sz, [_i, _i, _i, _i]),
    "smirk_mbconv_supported": (_i, [_i, _i, _i, _i]),
    "smirk_mbconv_fused_split16": (_i, [_p] * 10 + [_i, _p] + [_i] * 7 + [_p]),
    "smirk_mbconv_s2_supported": (_i, [_i, _i, _i]),
    "smirk_mbconv_s2_split16": (_i, [_p] * 11 + [_i] * 6 + [_p]),
    "smirk_warp_affine_u8": (_i, [_p, _i, _i, _i, _p, _i, _i, _i, _p, _p, _p]),
    "smirk_resize_linear_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "smirk_f32_nchw_to_u8_grid": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p]),
    "smirk_u8_hwc_to_f32_nchw": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "smirk_interp_bilinear_f32": (_i, [_p, _i, _i, _i, _i, _i, _p, _p]),
    "smirk_hull_mask": (_i, [_p, _i, _i, _i, _i, _i, _p, _p]),
    "smirk_rendered_mask": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "smirk_scatter_points_mask": (_i, [_p, _p, _i, _i, _i, _i, _p, _p]),
    "smirk_transfer_pixels": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p]),
    "smirk_project_landmarks": (_i, [_p, _p, _i, _i, _p, _p]),
    "smirk_conv_igemm_f32": (_i, [C.POINTER(SmirkConvDesc), _p, _p, _p, _p, _p, _p, _p, _p]),
    "smirk_conv_igemm_f16x3": (_i, [C.POINTER(SmirkConvDesc), _p, _p, _p, _p, _p, _p, _p, _p]),
    "smirk_conv_igemm_f16x1": (_i, [C.POINTER(SmirkConvDesc), _p, _p, _p, _p, _p, _p, _p, _p]),
    "smirk_conv3x3_tail_f16x3": (_i, [C.POINTER(SmirkConvDesc), _p, _p, _p, _p, _p, _p, _p, _p, _i, _p]),
    "smirk_conv3x3_pool_f16x3": (_i, [C.POINTER(SmirkConvDesc), _p, _p, _p, _p, _p, _p, _p, _p]),
    "smirk_enc1_fused_supported": (_i, [_i, _i, _i, _i]),
    "smirk_enc1_fused_split16": (_i, [_p] * 9 + [_i, _i, _i, _p]),
    "smirk_f32_to_split16": (_i, [_p, _p, _sz, _p]),
    "smirk_split16_to_f32": (_i, [_p, _p, _sz, _p]),
    "smirk_maxpool2x2_split16": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "smirk_split16_range_check": (_i, [_p, _sz, C.c_float, _p, _p]),
    "smirk_pack_generator_input_split16": (_i, [_p, _i, _p, _i, _p, _i, _i, _i, _p]),
    "smirk_conv1x1_sigmoid_nchw_split16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "smirk_maxpool2x2_nhwc": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "smirk_nchw_to_nhwc_pad": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "smirk_pack_generator_input": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "smirk_conv1x1_sigmoid_nchw": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "smirk_stem_conv_s2": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_dwconv3x3": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "smirk_gap_linear": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_stem_conv_s2_split16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_dwconv3x3_split16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "smirk_gap_linear_split16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_expression_clamps": (_i, [_p, _i, _i, _p]),
    "smirk_generator_workspace_bytes": (_sz, [C.POINTER(SmirkGeneratorWeights), _i, _i, _i]),
    "smirk_generator_forward": (_i, [C.POINTER(SmirkGeneratorWeights), _p, _i, _p, _i, _p, _i, _i, _i, C.POINTER(_p), _p, _sz, _p]),
    "smirk_backbone_workspace_bytes": (_sz, [C.POINTER(SmirkBackboneWeights), _i, _i, _i]),
    "smirk_backbone_forward": (_i, [C.POINTER(SmirkBackboneWeights), _p, _i, _i, _i, _p, _p, _p, _sz, _p]),
    "smirk_backbone_plan": (_i, [C.POINTER(SmirkBackboneWeights), _i, _i, _i, C.POINTER(C.c_int), _i]),
    "smirk_train_reduce_workspace_bytes": (_sz, [_i]),
    "smirk_conv_stats_rows_max": (_sz, [C.POINTER(SmirkConvDesc)]),
    "smirk_conv_igemm_stats_split16": (_i, [C.POINTER(SmirkConvDesc), _p, _p, _p, _p, _p, C.POINTER(C.c_int), _i, _p]),
    "smirk_bn_train_forward_partials_split16": (_i, [_p, _sz, _i, _p, _p, _p, _i, C.c_float, C.c_float, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p]),
    "smirk_dwconv3x3_stats_split16": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, C.POINTER(C.c_int), _p]),
    "smirk_bn_train_forward_split16": (_i, [_p, _sz, _i, _p, _p, _p, _i, C.c_float, C.c_float, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "smirk_bn_train_backward_split16": (_i, [_p, _p, _sz, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p, _sz, _p]),
    "smirk_bn_eval_forward_split16": (_i, [_p, _sz, _i, _p, _p, _p, _p, _p, _i, C.c_float, _p, _p, _p, _p]),
    "smirk_bn_eval_backward_split16": (_i, [_p, _p, _sz, _i, _p, _p, _p, _p, _p, _i, _p, _p]),
    "smirk_colsum_split16": (_i, [_p, _sz, _i, _p, _p, _sz, _p]),
    "smirk_maxpool2x2_backward_split16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_reflect_pad1_backward_split16": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_space_to_depth2_split16": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "smirk_conv1x1_sigmoid_backward_split16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "smirk_conv_wgrad_set_mode": (_i, [_i]),
    "smirk_conv_wgrad_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "smirk_conv_wgrad_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "smirk_conv_wgrad_f16x1": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "smirk_conv_wgrad_param": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "smirk_conv_wgrad_x1_fallbacks": (C.c_ulonglong, []),
    "smirk_pack_conv_weights_batch_split16": (_i, [_p, _i, C.c_ulonglong, _p]),
    "smirk_pack_conv_weights_split16": (_i, [_p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "smirk_stem_conv_s2_raw_split16": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_stem_conv_s2_wgrad_workspace_bytes": (_sz, [_i]),
    "smirk_stem_conv_s2_wgrad_split16": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "smirk_stem_conv_s2_dgrad_split16": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_dwconv3x3_dgrad_split16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "smirk_dwconv3x3_wgrad_workspace_bytes": (_sz, [_i]),
    "smirk_dwconv3x3_wgrad_split16": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "smirk_dwconv3x3_wgrad_param_split16": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "smirk_gap_linear_backward_split16": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_dwconv3x3_eval_backward_split16": (_i, [_p] * 8 + [_i] * 5 + [_p]),
    "smirk_relu_scale_backward_split16": (_i, [_p, _p, _p, _p, C.c_longlong, _i, _p]),
    "smirk_profile_start": (_i, []),
    "smirk_profile_stop": (_i, [C.POINTER(SmirkProfileRecord), _i]),
    "smirk_random_point_budget": (_i, [_p, _i, _i, C.c_float, C.c_uint64, C.c_uint64, _p]),
    "smirk_cycle_augment_workspace_bytes": (_sz, [_i]),
    "smirk_cycle_augment": (_i, [_p] * 6 + [_i] * 6 + [_p, _p, _p, _i, C.c_uint64, C.c_uint64] + [_p] * 6 + [_p, _p, _sz, _p]),
    "smirk_loss_workspace_bytes": (_sz, [C.POINTER(SmirkLossTerm), _i]),
    "smirk_loss_forward": (_i, [C.POINTER(SmirkLossTerm), _i, _p, _p, _p, _sz, _p]),
    "smirk_loss_backward": (_i, [C.POINTER(SmirkLossTerm), _i, _p, _p, _sz, _p]),
    "smirk_vgg_prepare_split16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "smirk_vgg_prepare_backward_split16": (_i, [_p, _p, _p, _i, _i, _i, C.c_float, _p]),
    "smirk_vgg_l1_workspace_bytes": (_sz, [C.POINTER(C.c_longlong), _i]),
    "smirk_vgg_l1_partials_split16": (_i, [_p, _i, _i, C.POINTER(C.c_longlong), _i, _p, _sz, _p]),
    "smirk_vgg_l1_finalise": (_i, [C.POINTER(C.c_longlong), _i, _p, _sz, _p, _p, _p]),
    "smirk_vgg_relu_tap_backward_split16": (_i, [_p, _p, _p, _p, _p, C.c_longlong, _i, C.c_float, _p]),
}
EXPORTS = tuple(_SIGS)

# The extension table of include/smirk_mica.h (the frozen MICA network of the pre-training stage): the same shared object, its own version.  The main table
# above, ABI_VERSION and include/smirk_hip.h do not move when an entry is added here.
MICA_ABI_VERSION = 1
MICA_FC_MAX_B, MICA_HEAD_LAYERS, MICA_HEAD_MAX_DIM = 64, 5, 1024   # include/smirk_mica.h SMIRK_MICA_FC_MAX_B, SMIRK_MICA_HEAD_LAYERS, SMIRK_MICA_HEAD_MAX_DIM


class SmirkMicaLinear(C.Structure):
    _fields_ = [("w", _p), ("b", _p), ("n_in", C.c_int32), ("n_out", C.c_int32)]


class SmirkMicaHead(C.Structure):
    _fields_ = [("layer", SmirkMicaLinear * MICA_HEAD_LAYERS)]


MICA_SIGS = {
    "smirk_mica_abi_version": (_i, []),
    "smirk_mica_prepare_split16": (_i, [_p, _p, _i, _i, _i, _p]),
    "smirk_mica_affine_prelu_split16": (_i, [_p, _p, _p, _p, _p, C.c_longlong, _i, _p]),
    "smirk_mica_fc_workspace_bytes": (_sz, [_i, _i, _i]),
    "smirk_mica_fc_split16": (_i, [_p, _p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    "smirk_mica_head": (_i, [_p, C.POINTER(SmirkMicaHead), _p, _i, _p]),
}
MICA_EXPORTS = tuple(MICA_SIGS)

# The extension table of include/smirk_emotion.h (the frozen emotion network of the first path): again the same shared object and a version of its own.
EMOTION_ABI_VERSION = 1
EMOTION_STEM_COUT, EMOTION_STEM_K, EMOTION_STEM_KPAD = 64, 147, 160   # include/smirk_emotion.h SMIRK_EMOTION_STEM_COUT, _STEM_K, _STEM_KPAD
EMOTION_METRICS = {"l2": 0, "l1": 1, "cos": 2}                        # SMIRK_EMOTION_L2, _L1, _COS
EMOTION_SIGS = {
    "smirk_emotion_abi_version": (_i, []),
    "smirk_emotion_stem_split16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "smirk_emotion_stem_dgrad_split16": (_i, [_p, _p, _p, C.c_float, _p, _i, _i, _i, _p]),
    "smirk_emotion_maxpool_split16": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "smirk_emotion_maxpool_backward_split16": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "smirk_emotion_dilate2_split16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "smirk_emotion_head_forward_split16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "smirk_emotion_head_backward_split16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, C.c_float, _p]),
}
EMOTION_EXPORTS = tuple(EMOTION_SIGS)

# The extension table of include/smirk_optim.h (the trainer's optimiser stage: clip_grad_norm_ and Adam as multi-tensor kernels): the same shared object, a
# version of its own.
OPTIM_ABI_VERSION = 1
OPTIM_CHUNK = 4096                                                     # include/smirk_optim.h SMIRK_OPTIM_CHUNK
OPTIM_KIND_NORM, OPTIM_KIND_SCALE, OPTIM_KIND_ADAM = 1, 2, 4           # SMIRK_OPTIM_KIND_*


class SmirkOptimTensor(C.Structure):
    _fields_ = [("param", _p), ("exp_avg", _p), ("exp_avg_sq", _p), ("numel", C.c_longlong), ("first_chunk", C.c_int32), ("_pad", C.c_int32)]


class SmirkOptimStep(C.Structure):
    _fields_ = [("grad", _p), ("step_size", C.c_float), ("bias_correction2_sqrt", C.c_float)]


_ll = C.c_longlong
OPTIM_SIGS = {
    "smirk_optim_abi_version": (_i, []),
    "smirk_optim_plan": (_i, [C.POINTER(SmirkOptimTensor), C.POINTER(SmirkOptimStep), _i, _i, C.POINTER(_ll)]),
    "smirk_optim_chunk_map": (_i, [C.POINTER(SmirkOptimTensor), _i, _p, _ll]),
    "smirk_optim_grad_norm_workspace_bytes": (_sz, [_ll]),
    "smirk_optim_grad_norm": (_i, [_p, _p, _p, _i, _ll, C.c_float, _p, _sz, _p, _p]),
    "smirk_optim_scale_grads": (_i, [_p, _p, _p, _i, _ll, _p, _p]),
    "smirk_optim_adam_step": (_i, [_p, _p, _p, _i, _ll, C.c_double, C.c_double, C.c_double, _p, _p]),
}
OPTIM_EXPORTS = tuple(OPTIM_SIGS)

# The extension table of include/smirk_handoff.h (masking -> generator hand-off of the inference path: one launch for masked_img and the generator's packed
# input, and the generator entry that starts from it): the same shared object, a version of its own.
HANDOFF_ABI_VERSION = 1
HANDOFF_SIGS = {
    "smirk_handoff_abi_version": (_i, []),
    "smirk_masking_handoff": (_i, [_p, _p, _p, _ll, _p, _i, _i, _i, C.c_float, C.c_uint64, C.c_uint64, C.c_uint64, _p, _p, _p]),
    "smirk_generator_forward_packed": (_i, [C.POINTER(SmirkGeneratorWeights), _p, _p, _i, _i, _i, C.POINTER(_p), _p, _sz, _p]),
}
HANDOFF_EXPORTS = tuple(HANDOFF_SIGS)

# The extension table of include/smirk_train_handoff.h (sampled points -> generator input of the two training paths: one launch for the points of the source frame
# and its Ke target frames, one for the transfer, masked_img and the generator's packed input): the same shared object, a version of its own.
TRAIN_HANDOFF_ABI_VERSION = 1
RENDERED_RULES = ("nonzero", "positive")                               # SMIRK_RENDERED_RULE_*, by code
TRAIN_HANDOFF_SIGS = {
    "smirk_train_handoff_abi_version": (_i, []),
    "smirk_sample_transfer_points": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, C.c_uint64, C.c_uint64, _p, _p, _p, _p, _p, _p, _p]),
    "smirk_train_masking_handoff": (_i, [_p, _p, _p, _ll, _p, _p, _i, _i, _i, _i, _i, _i, C.c_float, C.c_uint64, C.c_uint64, C.c_uint64, _p, _p, _p]),
}
TRAIN_HANDOFF_EXPORTS = tuple(TRAIN_HANDOFF_SIGS)

# The extension table of include/smirk_generator_plan.h (what a whole-network generator entry would launch, answered by generator_plan without touching device
# memory; for tests and tools, nothing on the hot path calls it): the same shared object, a version of its own.
GENPLAN_ABI_VERSION = 1
GEN_MAX_CHAINS = 3                                                     # include/smirk_generator_plan.h SMIRK_GEN_MAX_CHAINS
GEN_INPUTS = ("PACKED", "SPLIT_PACK", "NHWC_PAD", "PACK_F32")          # enum SmirkGenInput, by code
GEN_ENCODER_FAMILIES = ("ENC1_FUSED", "CONV_POOLFUSED", "CONV_CONV_POOL")   # enum SmirkGenEncoder, by code
GEN_DECODER_FAMILIES = ("UPCAT", "UPDEEP", "PAIR")                     # enum SmirkGenDecoder, by code


class SmirkGeneratorPlanReport(C.Structure):
    _fields_ = [("input", C.c_int32), ("nchain", C.c_int32), ("chain_b0", C.c_int32 * GEN_MAX_CHAINS), ("chain_nb", C.c_int32 * GEN_MAX_CHAINS),
                ("section_from", C.c_int32), ("enc", C.c_int32 * 4), ("dec", C.c_int32 * GEN_MAX_CHAINS * 4), ("compose_mask", C.c_int32),
                ("fused_tail", C.c_int32), ("workspace_bytes", C.c_uint64)]


GENPLAN_SIGS = {
    "smirk_genplan_abi_version": (_i, []),
    "smirk_generator_plan": (_i, [C.POINTER(SmirkGeneratorWeights), _i, _i, _i, _i, _i, _i, C.POINTER(SmirkGeneratorPlanReport)]),
}
GENPLAN_EXPORTS = tuple(GENPLAN_SIGS)

# The extension table of include/smirk_generator_arith.h (which arithmetic every level of the generator runs in under the weights' precision, answered by the
# function the forward asks; for tests and tools): the same shared object, a version of its own.
GENARITH_ABI_VERSION = 1
GEN_ARITH = ("F32", "F16X3", "F16X1")                                  # SMIRK_PRECISION_*, by code
GENARITH_SIGS = {
    "smirk_genarith_abi_version": (_i, []),
    "smirk_generator_arith": (_i, [C.POINTER(SmirkGeneratorWeights), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}
GENARITH_EXPORTS = tuple(GENARITH_SIGS)

# The extension table of include/smirk_data.h (the trainer's batch preparation: decoded frames + landmark arrays -> the batch dict on the device): the same shared
# object, a version of its own.
DATA_ABI_VERSION = 1
DATA_MAX_POINTS, DATA_FAN_POINTS, DATA_MICA_SIZE, DATA_MAX_SIZE = 1024, 68, 112, 2040   # include/smirk_data.h SMIRK_DATA_MAX_POINTS, _FAN_POINTS, _MICA_SIZE, _MAX_SIZE
DATA_TRANSFORMS = ("brightness_contrast", "gamma", "color_jitter", "clahe", "rgb_shift", "blur", "gauss_noise", "shift_scale_rotate")   # enum SmirkDataTransform, by code


class SmirkDataAugment(C.Structure):
    _fields_ = [("p", C.c_double * 8)] + \
               [(n, C.c_double) for n in ("brightness_limit", "contrast_limit", "gamma_lo", "gamma_hi", "cj_brightness", "cj_contrast", "cj_saturation", "cj_hue",
                                          "clahe_lo", "clahe_hi", "rgb_shift", "noise_var_lo", "noise_var_hi", "shift_limit", "scale_limit", "rotate_limit")] + \
               [("blur_max", C.c_int32), ("_pad", C.c_int32)]


class SmirkDataFrame(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("H", C.c_int32), ("W", C.c_int32)]


class SmirkDataParams(C.Structure):
    _fields_ = [(n, C.c_double * 6) for n in ("crop_fwd", "crop_inv", "ssr_fwd", "ssr_inv", "mica_inv")] + \
               [(n, C.c_double) for n in ("scale", "bc_alpha", "bc_beta", "gamma")] + [("cj", C.c_double * 4), ("clahe_clip", C.c_double), ("rgb_shift", C.c_double * 3)] + \
               [(n, C.c_double) for n in ("noise_sigma", "ssr_angle", "ssr_scale", "ssr_dx", "ssr_dy")] + \
               [(n, C.c_int32) for n in ("coins", "blur_k", "flag_fan", "_pad")]


DATA_SIGS = {
    "smirk_data_abi_version": (_i, []),
    "smirk_data_workspace_bytes": (_sz, [_i, _i, _i]),
    "smirk_data_hull_points_offset": (_sz, [_i, _i, _i]),
    "smirk_data_hull_offset": (_sz, [_i, _i, _i]),
    "smirk_data_params": (_i, [_p, _p, _i, _p, _p, _p, _i, _i, _i, C.c_double, C.c_double, C.POINTER(SmirkDataAugment), C.c_uint64, C.c_uint64, _p, _p, _p, _p, _sz, _p]),
    "smirk_data_crop": (_i, [_p, _sz, _p, _i, _i, _i, _p, _p, _p, _sz, _p]),
    "smirk_data_stats": (_i, [_i, _i, _p, _sz, _p]),
    "smirk_data_colour": (_i, [_i, _i, _p, _sz, _p]),
    "smirk_data_finish": (_i, [_i, _i, C.c_uint64, C.c_uint64, _p, _p, _p, _sz, _p]),
}
DATA_EXPORTS = tuple(DATA_SIGS)

# The extension table of include/smirk_visual.h (the trainer's visualisation sheet: fp32 panels on the device -> one uint8 sheet): the same shared object, a version
# of its own.
VISUAL_ABI_VERSION = 1
VISUAL_MAX_COLUMNS, VISUAL_MAX_POINTS, VISUAL_LAYERS = 16, 1024, 4     # include/smirk_visual.h SMIRK_VISUAL_MAX_COLUMNS, _MAX_POINTS, _LAYERS
VISUAL_MIN_SIZE, VISUAL_MAX_SIZE, VISUAL_PADDING = 8, 4096, 2           # SMIRK_VISUAL_MIN_SIZE, _MAX_SIZE, _PADDING


class SmirkVisualColumn(C.Structure):
    _fields_ = [("src", _p * 4), ("blend", _p), ("w_src", C.c_float), ("w_blend", C.c_float)] + \
               [(n, C.c_int32) for n in ("nsrc", "channels", "Hs", "Ws", "nrow", "landmarks")]


class SmirkVisualDots(C.Structure):
    _fields_ = [("lm", _p * 4), ("rows", C.c_int32 * 4), ("npts", C.c_int32 * 4)]


VISUAL_SIGS = {
    "smirk_visual_abi_version": (_i, []),
    "smirk_visual_sheet_size": (_i, [C.POINTER(SmirkVisualColumn), _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_sz)]),
    "smirk_visual_workspace_bytes": (_sz, [_i, _i]),
    "smirk_visual_dots": (_i, [C.POINTER(SmirkVisualDots), _i, _i, C.c_float, _p, _sz, _p]),
    "smirk_visual_sheet": (_i, [C.POINTER(SmirkVisualColumn), _i, _i, _i, _i, _p, _sz, _p, _sz, _p]),
}
VISUAL_EXPORTS = tuple(VISUAL_SIGS)

# The extension table of include/smirk_jpeg.h (baseline JPEG encoding of uint8 pictures on the device): the same shared object, a version of its own.
JPEG_ABI_VERSION = 1
JPEG_HEADER_BYTES, JPEG_MCU_MAX_BYTES, JPEG_MAX_DIM = 629, 1245, 65535      # include/smirk_jpeg.h SMIRK_JPEG_HEADER_BYTES, _MCU_MAX_BYTES, _MAX_DIM
JpegQuantTables = (C.c_uint8 * 64) * 2

JPEG_SIGS = {
    "smirk_jpeg_abi_version": (_i, []),
    "smirk_jpeg_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "smirk_jpeg_max_bytes": (_sz, [_i, _i, _i, _i]),
    "smirk_jpeg_quant_tables": (_i, [_i, C.POINTER(JpegQuantTables)]),
    "smirk_jpeg_encode_u8": (_i, [_p, _i, _i, _i, _i, C.POINTER(JpegQuantTables), _i, _p, _sz, _p, _sz, _p, _p]),
}
JPEG_EXPORTS = tuple(JPEG_SIGS)

_LIB = None


class SmirkHipError(RuntimeError):
    pass


def lib():
    """The loaded library; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SmirkHipError(f"{LIB_PATH} not found: build it with `python -m smirk_amd.build` "
                                "(smirk_amd has no CPU / eager fallback)")
        L = C.CDLL(LIB_PATH)
        for table in (_SIGS, MICA_SIGS, EMOTION_SIGS, OPTIM_SIGS, HANDOFF_SIGS, TRAIN_HANDOFF_SIGS, GENPLAN_SIGS, GENARITH_SIGS, DATA_SIGS, VISUAL_SIGS, JPEG_SIGS):
            for name, (res, args) in table.items():
                fn = getattr(L, name)       # AttributeError => header / library mismatch
                fn.restype, fn.argtypes = res, args
        if L.smirk_abi_version() != ABI_VERSION or L.smirk_mica_abi_version() != MICA_ABI_VERSION or L.smirk_emotion_abi_version() != EMOTION_ABI_VERSION or \
                L.smirk_optim_abi_version() != OPTIM_ABI_VERSION or L.smirk_handoff_abi_version() != HANDOFF_ABI_VERSION or \
                L.smirk_genplan_abi_version() != GENPLAN_ABI_VERSION or L.smirk_genarith_abi_version() != GENARITH_ABI_VERSION or L.smirk_data_abi_version() != DATA_ABI_VERSION or \
                L.smirk_visual_abi_version() != VISUAL_ABI_VERSION or L.smirk_train_handoff_abi_version() != TRAIN_HANDOFF_ABI_VERSION or \
                L.smirk_jpeg_abi_version() != JPEG_ABI_VERSION:
            raise SmirkHipError("libsmirk_hip.so ABI version mismatch; rebuild")
        _LIB = L
    return _LIB


def check(code):
    if code != 0:
        raise SmirkHipError(f"libsmirk_hip: {lib().smirk_strerror(code).decode()} ({code})")


def raise_if_range_tripped(where, synchronize=False):
    """The split-fp16 storage format carries |x| < 65520 only (its `hi` half is an fp16).  Every kernel that writes it audits what it stores and sets one sticky
    host-pinned word (include/smirk_hip.h smirk_range_flag_peek); this reads that word — a plain host load, no device synchronisation unless asked for — and
    raises once it is set.  The modules call it at the START of every forward, so an overflow in call N is reported by call N + 1 at the latest (or by
    smirk_amd.check_numerics(), which synchronises first).  The reference computes in fp32 and has no such limit: a checkpoint whose activations leave the
    fp16 range must run SmirkGenerator.precision = "f32" (exact-fp32 kernels) instead."""
    if synchronize:
        torch.cuda.synchronize()
    L = lib()
    if L.smirk_range_flag_peek():
        L.smirk_range_flag_clear()
        raise SmirkHipError(f"{where}: an activation left the range of the split-fp16 storage format (|x| >= 65520, or a non-finite input) in a kernel that ran "
                            "before this call — its output and everything computed from it are invalid (inf / NaN).  Badly scaled weights or inputs; the exact-fp32 "
                            "generator kernels (SmirkGenerator.precision = 'f32') have no such limit.  The flag has been cleared.")


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype=torch.float32, allow_none=False):
    """Device pointer of a contiguous tensor of the expected dtype that lives on the HIP device."""
    if t is None:
        if allow_none:
            return None
        raise SmirkHipError("missing tensor argument")
    if not t.is_cuda:
        raise SmirkHipError("smirk_amd runs on the MI355X HIP device only: got a CPU tensor (no CPU fallback exists)")
    if t.dtype != dtype:
        raise SmirkHipError(f"expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise SmirkHipError("expected a contiguous tensor")
    return C.c_void_p(t.data_ptr())


def as_f32c(t):
    """float32 contiguous view/copy (device-side plumbing only)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def aligned16(t):
    """as_f32c on a 16-byte boundary: an offset view is cloned, because the kernels read 16-byte vectors"""
    t = as_f32c(t)
    return t.clone() if t.data_ptr() % 16 else t


def second_backward(function, held):
    """the error of a backward pass over a tape that the first one released"""
    return RuntimeError(f"{function}.backward called a second time: the tape of {held} is released after the first backward pass "
                        "(retain_graph=True is not supported by the HIP training path; run the forward again)")


def profile_start():
    """Arm the library's launch profiler (include/smirk_hip.h): every kernel it launches from now on is bracketed by HIP events on its stream."""
    check(lib().smirk_profile_start())


def profile_stop(cap=8192):
    """-> [(kernel name as instantiated, algorithmic flop, algorithmic bytes, milliseconds)] for every launch since profile_start()."""
    buf = (SmirkProfileRecord * cap)()
    n = lib().smirk_profile_stop(buf, cap)
    if n < 0:
        check(n)
    return [(buf[i].kernel.decode(), buf[i].flop, buf[i].bytes, buf[i].ms) for i in range(min(n, cap))]


def conv_layer(w, scale=None, shift=None):
    """SmirkConvLayer from packed device tensors (the caller keeps them alive)."""
    l = SmirkConvLayer()
    l.w = w.data_ptr() if w is not None else None
    l.scale = scale.data_ptr() if scale is not None else None
    l.shift = shift.data_ptr() if shift is not None else None
    return l


_DESC_PACK = struct.Struct("=16i").pack
assert C.sizeof(SmirkConvDesc) == 64 and all(t is C.c_int32 for _, t in SmirkConvDesc._fields_)      # what _DESC_PACK lays out: sixteen int32, no padding


def conv_desc(B, H, W, c0, cout, k=1, *, c1=0, stride=1, pad=None, out_hw=None, reflect=False, relu=False, convt=False):
    """SmirkConvDesc of a k x k convolution over an NHWC input [B, H, W, c0 (+ c1 of a second source)].  `pad` defaults to (k - 1) // 2 on both axes and the
    output size to (H + 2 pad - k) // stride + 1; `out_hw` overrides it (the full correlation of a reflect-padded layer's data gradient: pad 2, (H + 2, W + 2))."""
    pad = (k - 1) // 2 if pad is None else pad
    ho, wo = ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1) if out_hw is None else out_hw
    # The values follow SmirkConvDesc._fields_.  This runs once per convolution launch, ~600 times per training step: timeit of the construction alone (CPython
    # 3.10, same values) gives 0.36 us for pack + copy, 0.67 us for sixteen named field stores and 1.18 us for the keyword constructor.
    return SmirkConvDesc.from_buffer_copy(_DESC_PACK(B, H, W, c0, c1, cout, k, k, stride, pad, pad, ho, wo, PAD_REFLECT if reflect else PAD_ZERO,
                                                     ACT_RELU if relu else ACT_NONE, OUT_CONVT2X2 if convt else OUT_NHWC))


def conv_launch(entry, d, st, x0, w, x1=None, scale=None, shift=None, residual=None, out=None):
    """One call of a smirk_conv_igemm_* entry on the stream `st`: -> out, [B, 2H, 2W, Cout] for the 2 x 2 transposed-convolution store and [B, Ho, Wo, Cout]
    otherwise, allocated here unless the caller passes it."""
    if out is None:
        out = torch.empty((d.B, 2 * d.H, 2 * d.W, d.Cout) if d.out_mode == OUT_CONVT2X2 else (d.B, d.Ho, d.Wo, d.Cout), device=x0.device)
    check(entry(d, ptr(x0), ptr(x1, allow_none=True), ptr(w), ptr(scale, allow_none=True), ptr(shift, allow_none=True), ptr(residual, allow_none=True), ptr(out), st))
    return out


def version_key(tensors):
    """what a cache of images derived from `tensors` is keyed on: a re-allocation moves data_ptr, an in-place update moves torch's version counter"""
    return tuple((t.data_ptr(), t._version) for t in tensors)


class SmirkPackJob(C.Structure):
    """include/smirk_hip.h SmirkPackJob"""
    _fields_ = [("w", C.c_void_p), ("fwd", C.c_void_p), ("dgrad", C.c_void_p), ("Cout", C.c_int32), ("cin_total", C.c_int32), ("cin_off", C.c_int32),
                ("Cin", C.c_int32), ("KH", C.c_int32), ("cin_pad", C.c_int32), ("start", C.c_ulonglong)]


class _LoudCut(torch.autograd.Function):
    """Identity whose backward raises: attached to the output of a forward that has no backward implementation whenever autograd would
    otherwise record a (silently broken) graph through it.  Forward-only callers (demo.py runs without torch.no_grad()) are unaffected."""

    @staticmethod
    def forward(ctx, what, y, *deps):
        ctx.what = what
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        raise NotImplementedError(f"{ctx.what} has no backward on the HIP path: gradients cannot flow through it "
                                  "(run it under torch.no_grad(), or detach its inputs)")


def loud_cut(what, y, deps):
    """y if autograd is off or nothing in `deps` requires grad; otherwise y with a grad_fn that raises when back-propagated through."""
    if not torch.is_grad_enabled():
        return y
    deps = [t for t in deps if torch.is_tensor(t) and t.requires_grad]
    return _LoudCut.apply(what, y, *deps) if deps else y


class Workspace:
    """Grow-only byte scratch buffers owned by a module, one per (device, stream): the library never allocates, and two streams that run
    the same module concurrently (OverlappedPipeline, the encoder's side streams) must not share scratch memory."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes, device, stream=None):
        if torch.device(device).type != "cuda":
            raise SmirkHipError("smirk_amd runs on the MI355X HIP device only: got a CPU tensor / module (no CPU fallback exists)")
        key = (device, torch.cuda.current_stream(device).cuda_stream if stream is None else stream)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self.bufs[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return buf
