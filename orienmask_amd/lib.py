"""ctypes binding of liborienmask_hip.so (C ABI declared in include/orienmask_hip.h).

The HIP library IS the product: there is no CPU or eager-PyTorch fallback.  If the shared
object is missing or does not export a declared symbol, loading raises immediately.
"""
import contextlib
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liborienmask_hip.so")

OM_MAX_SCALES = 3
OM_MAX_ANCHORS = 9
OM_STATUS_SPLIT_RANGE = 1      # include/orienmask_hip.h: bits of the forward's status word
OM_STATUS_SK_TIMEOUT = 2


class LayerInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64),
                ("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("cout_pad", ctypes.c_int32),
                ("ksize", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("has_bn", ctypes.c_int32), ("leaky", ctypes.c_int32), ("wino_planes", ctypes.c_int32),
                ("w_off", ctypes.c_int64), ("scale_off", ctypes.c_int64), ("shift_off", ctypes.c_int64),
                ("wino_off", ctypes.c_int64), ("wino_alt_off", ctypes.c_int64), ("w16_off", ctypes.c_int64),
                ("wsplit_off", ctypes.c_int64), ("wsplit_scale_off", ctypes.c_int64),
                ("wsplit_direct_off", ctypes.c_int64), ("wsplit_direct_scale_off", ctypes.c_int64)]


class PostCfg(ctypes.Structure):
    _fields_ = [("num_scales", ctypes.c_int32),
                ("grid_h", ctypes.c_int32 * OM_MAX_SCALES), ("grid_w", ctypes.c_int32 * OM_MAX_SCALES),
                ("image_h", ctypes.c_int32), ("image_w", ctypes.c_int32),
                ("anchors_per_scale", ctypes.c_int32),
                ("anchor_w", ctypes.c_float * OM_MAX_ANCHORS), ("anchor_h", ctypes.c_float * OM_MAX_ANCHORS),
                ("anchor_mask", (ctypes.c_int32 * 3) * OM_MAX_SCALES),
                ("num_classes", ctypes.c_int32),
                ("conf_thresh", ctypes.c_float), ("nms_thresh", ctypes.c_float),
                ("nms_pre", ctypes.c_int32), ("nms_post", ctypes.c_int32),
                ("orien_thresh", ctypes.c_float),
                ("bbox_pix_stride", ctypes.c_int32),
                ("nms_semantics", ctypes.c_int32), ("nms_normalized", ctypes.c_int32),
                ("anchors_of_scale", ctypes.c_int32 * OM_MAX_SCALES)]


class RleImage(ctypes.Structure):
    """include/orienmask_hip.h: om_rle_image"""
    _fields_ = [("mask", ctypes.c_void_p), ("K", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("crop_top", ctypes.c_int32), ("crop_down", ctypes.c_int32), ("crop_left", ctypes.c_int32),
                ("crop_right", ctypes.c_int32), ("hflip", ctypes.c_int32), ("vflip", ctypes.c_int32),
                ("orig_h", ctypes.c_int32), ("orig_w", ctypes.c_int32)]


class VisImage(ctypes.Structure):
    """include/orienmask_hip.h: om_vis_image"""
    _fields_ = [("image", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_float", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("keep", ctypes.c_void_p), ("colors", ctypes.c_void_p), ("boxes", ctypes.c_void_p),
                ("n_keep", ctypes.c_int32), ("Hn", ctypes.c_int32), ("Wn", ctypes.c_int32),
                ("crop_left", ctypes.c_int32), ("crop_right", ctypes.c_int32), ("crop_top", ctypes.c_int32),
                ("crop_down", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("with_mask", ctypes.c_int32), ("draw_boxes", ctypes.c_int32), ("alpha", ctypes.c_float)]


OM_LOSS_MAX_CLASSES = 2047      # include/orienmask_hip.h: the loss's limits and result vector layout
OM_LOSS_MAX_GT = 1024
OM_LOSS_TERMS = 7
OM_LOSS_METRICS = 8
OM_LOSS_SCALE_FLOATS = OM_LOSS_TERMS + 2 * OM_LOSS_METRICS
OM_LOSS_FLAG_OFF = OM_MAX_SCALES * OM_LOSS_SCALE_FLOATS
OM_LOSS_RESULT_FLOATS = OM_LOSS_FLAG_OFF + 1
OM_LOSS_FLAG_NONFINITE_WH = 1
OM_LOSS_FLAG_TOO_MANY_GT = 2
OM_LOSS_FLAG_BAD_CLASS = 4
# include/orienmask_hip.h: the counter block of om_loss_accumulate, in float64 elements (the two status words are int64)
OM_COUNTER_MAX_KEYS = 1 + 2 * (OM_MAX_SCALES + 1) * OM_LOSS_METRICS
OM_COUNTER_STAGE_OFF = 0
OM_COUNTER_EPOCH_OFF = 2 * OM_COUNTER_MAX_KEYS
OM_COUNTER_FLAG_OFF = 4 * OM_COUNTER_MAX_KEYS
OM_COUNTER_STEP_OFF = OM_COUNTER_FLAG_OFF + 1
OM_COUNTER_BLOCK_DOUBLES = OM_COUNTER_FLAG_OFF + 2
OM_COUNTER_FLAG_NONFINITE_LOSS = 256


class LossCfg(ctypes.Structure):
    """include/orienmask_hip.h: om_loss_cfg"""
    _fields_ = [("num_scales", ctypes.c_int32),
                ("grid_h", ctypes.c_int32 * OM_MAX_SCALES), ("grid_w", ctypes.c_int32 * OM_MAX_SCALES),
                ("image_h", ctypes.c_int32), ("image_w", ctypes.c_int32),
                ("anchors_of_scale", ctypes.c_int32 * OM_MAX_SCALES),
                ("anchor_mask", (ctypes.c_int32 * 3) * OM_MAX_SCALES),
                ("num_anchors_total", ctypes.c_int32),
                ("anchor_w", ctypes.c_float * OM_MAX_ANCHORS), ("anchor_h", ctypes.c_float * OM_MAX_ANCHORS),
                ("num_classes", ctypes.c_int32),
                ("center_region", ctypes.c_float), ("valid_region", ctypes.c_float),
                ("label_smooth", ctypes.c_float), ("label_on", ctypes.c_float),
                ("obj_ignore_threshold", ctypes.c_float),
                ("weight", (ctypes.c_float * OM_LOSS_TERMS) * OM_MAX_SCALES),
                ("bbox_stride", (ctypes.c_int64 * 4) * OM_MAX_SCALES),
                ("orien_stride", (ctypes.c_int64 * 3) * OM_MAX_SCALES)]


OM_VIS_MAX_KEPT = 512
OM_VIS_BATCH = 16
OM_PRE_BATCH = 16               # include/orienmask_hip.h: om_preprocess_batch, images per launch and the flags of a geom row
OM_PRE_U8 = 1
OM_PRE_BGR = 2
# include/orienmask_hip.h: the JPEG decoder -- images per launch set, the int32 words of an info record, the int64 words of a
# descriptor row, the reasons a stream is left to a host reader, the bound on |coefficient * quantiser| of the int32 IDCT
OM_JPEG_BATCH = 16
OM_JPEG_COEF_BOUND = 1170
OM_JPEG_INFO_WORDS = 32
OM_JPEG_I_WIDTH, OM_JPEG_I_HEIGHT, OM_JPEG_I_NCOMP, OM_JPEG_I_SUPPORTED, OM_JPEG_I_REASON = 0, 1, 2, 3, 4
OM_JPEG_I_HMAX, OM_JPEG_I_VMAX, OM_JPEG_I_RESTART, OM_JPEG_I_BLOCKS, OM_JPEG_I_COMP = 5, 6, 7, 8, 10
OM_JPEG_COMP_WORDS = 6
OM_JPEG_DESC_WORDS = 8
(OM_JPEG_R_NONE, OM_JPEG_R_PROGRESSIVE, OM_JPEG_R_ARITHMETIC, OM_JPEG_R_LOSSLESS, OM_JPEG_R_PRECISION, OM_JPEG_R_FRAME,
 OM_JPEG_R_QUANT16, OM_JPEG_R_COMPONENTS, OM_JPEG_R_ADOBE, OM_JPEG_R_SAMPLING, OM_JPEG_R_SCANS, OM_JPEG_R_DNL,
 OM_JPEG_R_ORIENTATION, OM_JPEG_R_SIZE, OM_JPEG_R_RANGE) = range(15)

_vp, _i, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t

# symbol -> (restype, argtypes); must list every function include/orienmask_hip.h declares
SIGNATURES = {
    "om_version": (_i, []),
    "om_last_error": (ctypes.c_char_p, []),
    "om_model_create": (_i, [ctypes.POINTER(_vp), _i, _i]),
    "om_model_create_variant": (_i, [ctypes.POINTER(_vp), _i, _i, _i]),
    "om_model_destroy": (None, [_vp]),
    "om_model_num_layers": (_i, [_vp]),
    "om_model_layer_info": (_i, [_vp, _i, ctypes.POINTER(LayerInfo)]),
    "om_model_weight_floats": (_sz, [_vp]),
    "om_model_load_weights": (_i, [_vp, _vp, _sz, _i]),
    "om_model_weight_split_words": (_sz, [_vp]),
    "om_model_load_weights_split": (_i, [_vp, _vp, _sz]),
    "om_model_set_precision": (_i, [_vp, _i]),
    "om_model_get_precision": (_i, [_vp]),
    "om_model_set_latency_cells": (_i, [_vp, ctypes.c_longlong]),
    "om_model_set_latency_ksplit": (_i, [_vp, _i]),
    "om_model_attach_postprocess": (_i, [_vp, ctypes.POINTER(PostCfg), _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t]),
    "om_model_set_upsample_on_read": (_i, [_vp, _i]),
    "om_conv2d_split": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "om_conv2d_split_k": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "om_conv2d_winograd24_split": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp, _vp]),
    "om_set_stem_fusion": (_i, [_i, _i]),
    "om_get_stem_fusion": (_i, [_i]),
    "om_get_conv3x3_f16_variant": (_i, []),
    "om_set_conv3x3_f16_variant": (_i, [_i]),
    "om_conv2d_wino14_split": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "om_conv2d_wino14_blocks": (_i, [_i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_longlong)]),
    "om_conv2d_wino14_wide_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "om_conv2d_wino14_wide": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp, _vp]),
    "om_set_wino14_wide": (_i, [_i]),
    "om_get_wino14_wide": (_i, []),
    "om_forward_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "om_forward_status_offset": (_sz, [_vp, _i, _i, _i]),
    "om_forward": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "om_layer_tile": (_i, [_vp, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                           ctypes.POINTER(ctypes.c_int)]),
    "om_model_weight_halfs": (_sz, [_vp]),
    "om_model_load_weights_f16": (_i, [_vp, _vp, _sz]),
    "om_forward_f16_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "om_forward_f16": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "om_layer_tile_f16": (_i, [_vp, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                               ctypes.POINTER(ctypes.c_int)]),
    "om_conv2d_f16": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _i, _vp]),
    "om_conv2d_stem_f16": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "om_conv2d_winograd_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "om_conv2d_winograd": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "om_layer_output_view": (_i, [_vp, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int),
                                  ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "om_model_keep_activations": (_i, [_vp, _i]),
    "om_conv2d_winograd24_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "om_conv2d_winograd24": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "om_profile_enable": (_i, [_vp, _i]),
    "om_profile_enable_layers": (_i, [_vp, ctypes.c_char_p, _i]),
    "om_profile_read": (_i, [_vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), _i,
                             ctypes.POINTER(ctypes.c_int)]),
    "om_conv2d": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "om_conv2d_mode": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _vp]),
    "om_conv2d_stem": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "om_conv2d_stem2_split": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "om_conv2d_stem3_split": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "om_conv2d_stem2_f16": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _vp]),
    "om_conv2d_split_gather": (_i, [_i, ctypes.POINTER(_vp), ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), _i, _i, _i,
                                    _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "om_preprocess": (_i, [_vp, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                           _i, _i, _i, _i, _f, _vp, _vp]),
    "om_preprocess_batch": (_i, [ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_int32), _i, ctypes.POINTER(ctypes.c_float),
                                 ctypes.POINTER(ctypes.c_float), _i, _i, _f, _vp, _vp]),
    "om_jpeg_info": (_i, [_vp, _sz, ctypes.POINTER(ctypes.c_int32)]),
    "om_jpeg_entropy_decode": (_i, [_vp, _sz, _vp, _sz, _vp, ctypes.POINTER(ctypes.c_int32)]),
    "om_jpeg_workspace_bytes": (_sz, [ctypes.POINTER(ctypes.c_int64), _i]),
    "om_jpeg_decode_batch": (_i, [ctypes.POINTER(ctypes.c_int64), _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "om_pad_nchw": (_i, [_vp, ctypes.c_longlong, _i, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "om_postprocess_workspace_bytes": (_sz, [ctypes.POINTER(PostCfg), _i]),
    "om_postprocess": (_i, [ctypes.POINTER(PostCfg), _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "om_postprocess_detect": (_i, [ctypes.POINTER(PostCfg), _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "om_postprocess_assemble": (_i, [ctypes.POINTER(PostCfg), _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "om_postprocess_candidates": (_i, [ctypes.POINTER(PostCfg), _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "om_postprocess_masks": (_i, [ctypes.POINTER(PostCfg), _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "om_recover_bbox": (_i, [_vp, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), _i, _i, _i, _i,
                             _vp, _vp]),
    "om_recover_masks_rle": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "om_recover_masks_rle_strings": (_i, [_vp, _i, _vp, _i, _vp, _vp, ctypes.c_longlong, _vp, _vp, _vp, _vp]),
    "om_visualize_workspace_bytes": (_sz, [_vp, _i]),
    "om_visualize": (_i, [_vp, _i, _vp, _sz, _vp]),
    "om_cocoeval_workspace_bytes": (_sz, [ctypes.c_longlong, _i]),
    "om_cocoeval_masks": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_longlong, _vp, _sz, _vp]),
    "om_cocoeval_mask_stats": (_i, [_i, ctypes.c_longlong, _vp, _vp, _vp]),
    "om_cocoeval_mask_iou": (_i, [_i, _vp, _vp, _i, _vp, _vp, ctypes.c_longlong, _vp, _vp, _vp]),
    "om_cocoeval_bbox_iou": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "om_cocoeval_match": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "om_segm_decode_workspace_bytes": (_sz, [ctypes.c_longlong, _i]),
    "om_segm_decode": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_longlong, _vp, _sz, _vp, _vp]),
    "om_post_kernel_occupancy": (_i, [_i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "om_nms_workspace_bytes": (_sz, [_i]),
    "om_nms": (_i, [_vp, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "om_nms_ex": (_i, [_vp, _i, _f, _i, _vp, _vp, _vp, _sz, _vp]),
    "om_ref_math": (_i, [_vp, ctypes.c_longlong, _i, _i, _vp, _vp]),
    "om_loss_workspace_bytes": (_sz, [ctypes.POINTER(LossCfg), _i, _i]),
    "om_loss": (_i, [ctypes.POINTER(LossCfg), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "om_loss_targets": (_i, [ctypes.POINTER(LossCfg), ctypes.POINTER(_vp), _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                             _vp, _vp, _vp, _vp, _sz, _vp]),
    "om_loss_accumulate": (_i, [_vp, _i, ctypes.POINTER(_f), _i, ctypes.c_longlong, _vp, _vp, _vp]),
    "om_augment_workspace_bytes": (_sz, [_i]),
    "om_augment": (_i, [_vp, _i, _vp, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "om_loss_backward": (_i, [ctypes.POINTER(LossCfg), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, _vp, _vp, _i, _vp, _vp, _sz, _vp,
                              ctypes.POINTER(_f), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp]),
    "om_sgd_step": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "om_sgd_clip_step": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _f, _i, ctypes.c_longlong, _vp]),
    "om_sgd_ema_step": (_i, [_vp, _vp, _i, _vp, _i, _vp, _f, _vp]),
    "om_sgd_clip_ema_step": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _f, _i, ctypes.c_longlong, _vp, _vp, ctypes.c_double, _i,
                                  _vp]),
    "om_ema_swap": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "om_adam_step": (_i, [_vp, _vp, _i, _vp, _i, _vp, _f, _vp]),
    "om_adam_clip_step": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _i, ctypes.c_longlong, _vp, _vp, ctypes.c_double,
                               _i, _vp]),
    "om_adam_ema_swap": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "om_bn_act_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "om_bn_act_forward": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, ctypes.c_double, ctypes.c_double, _f, _vp, _vp, _vp, _vp,
                               _vp, _sz, _vp]),
    "om_bn_act_backward": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "om_bn_sync_stats": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "om_bn_sync_forward": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _f, _vp, _vp,
                                _vp, _vp, _vp, _vp]),
    "om_bn_sync_backward_sums": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "om_bn_sync_backward_dx": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _i, _vp, _vp, _vp]),
    "om_conv2d_grad_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "om_conv2d_grad_input": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "om_conv2d_grad_weight": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "om_conv2d_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "om_conv2d_frozen_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_double, _f, _vp, _vp, _vp]),
    "om_conv2d_bf16_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "om_conv2d_bf16_frozen_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_double, _f, _vp, _vp,
                                           _vp]),
    "om_conv2d_bf16_grad_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "om_conv2d_bf16_grad_input": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _sz, _vp]),
    "om_conv2d_bf16_grad_weight": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "om_route_concat_forward": (_i, [ctypes.POINTER(_vp), ctypes.POINTER(_i), ctypes.POINTER(_i), _i, _i, _i, _i, _vp, _vp]),
    "om_route_concat_backward": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i), _i, _i, _i, _i, ctypes.POINTER(_vp), _vp]),
}
# the bf16-activation forms: the same arguments, the activation pointers bf16
for _name in ("om_bn_act_forward", "om_bn_act_backward", "om_bn_sync_stats", "om_bn_sync_forward", "om_bn_sync_backward_sums",
              "om_bn_sync_backward_dx", "om_route_concat_forward", "om_route_concat_backward"):
    SIGNATURES[_name + "_bf16"] = SIGNATURES[_name]

_lib = None


class OrienMaskHipError(RuntimeError):
    pass


def load():
    """Load the HIP library once; raise loudly if it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OrienMaskHipError(
            "%s not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C orienmask_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    # torch first (this module's own import): its wheel bundles a HIP runtime, and the process must end up with ONE runtime -- the one whose streams and device
    # pointers the callers hand to this library.  Loaded the other way round (this library before torch) the library binds to
    # /opt/rocm's runtime, torch initialises its own, and every launch fails with "no ROCm-capable device is detected".
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise OrienMaskHipError("%s does not export %s" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().om_last_error()
        raise OrienMaskHipError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else "?"))


def require_cuda_tensor(t, name, dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise OrienMaskHipError("%s must be a tensor on an MI355X device (got %s); this path has no CPU fallback"
                                % (name, getattr(t, "device", type(t))))
    if dtype is not None and t.dtype != dtype:
        raise OrienMaskHipError("%s must be %s, got %s" % (name, dtype, t.dtype))


def current_stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ------------------------------------------------------------------------------------------------- the one call path
_NO_SWITCH = contextlib.nullcontext()


def on_device(dev):
    """The launches go to the tensors' device: switch only when it is not the current one (the switch costs as much as a
    launch).  Also the guard of a block of several launches with events or copies; `launch` inside it then switches nothing."""
    return _NO_SWITCH if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def raw_args(args):
    """The arguments as ctypes takes them under argtypes: a tensor becomes its data_ptr() (a view's own address); ints, floats,
    None, ctypes objects and addresses computed by the caller pass through untouched.  Nothing is validated."""
    return [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]


def _entry(name):
    if name not in SIGNATURES:
        raise OrienMaskHipError("%s is not an entry point of %s" % (name, LIB_PATH))
    return getattr(load(), name)


def launch(name, dev, *args, stream=None):
    """Call entry point `name`, whose last parameter is om_stream, with `dev` current: `args` through raw_args, then the stream --
    `dev`'s current torch stream, or `stream` (a torch.cuda.Stream or a raw pointer).  A nonzero status raises check(rc, name)."""
    fn = _entry(name)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    elif isinstance(stream, torch.cuda.Stream):
        stream = stream.cuda_stream
    with on_device(dev):
        rc = fn(*raw_args(args), stream)
    check(rc, name)


def call(name, *args):
    """launch without a device or a stream: the host-side entry points that return a status."""
    check(_entry(name)(*raw_args(args)), name)


def workspace_bytes(name, *args):
    """A size query whose 0 means refusal: raises with the library's message, as check(-1, name) does."""
    n = _entry(name)(*args)
    if n == 0:
        check(-1, name)
    return n
