"""ctypes binding of libppyolo_hip.so (the C ABI declared in include/ppyolo_hip.h).

`cffi` is not installed in this image, so the thin C-ABI layer is
bound with the stdlib.  There is NO fallback: if the shared library is missing the
import of any op raises, and every call checks the C return code.
"""
import collections
import ctypes
import functools
import os
from ctypes import c_double, c_float, c_int, c_longlong, c_size_t, c_ulonglong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PPYOLO_HIP_LIB') or os.path.join(_HERE, 'lib', 'libppyolo_hip.so')     # (override: experiments)

OK = 0
ERR_UNSUPPORTED = -2      # PPY_ERR_UNSUPPORTED (include/ppyolo_hip.h)
ACT = {None: 0, 'relu': 1, 'leaky': 2}
NORM_ACT = dict(ACT, mish=3)      # PPY_ACT_MISH: ppy_group_norm_f32 only (the convolution entry points reject it)
GN_MAX_CHUNKS = 128               # PPY_GN_MAX_CHUNKS
MERGE_METRIC = {'iou': 0, 'ios': 1}                                              # PPY_MERGE_IOU / PPY_MERGE_IOS
MERGE_MAX_ROWS, MERGE_RANK_MAX, MERGE_CHUNK, MERGE_MAX_KEEP = 8192, 1024, 64, 1024      # PPY_MERGE_* (include/ppyolo_hip.h)
TRACK_FREE, TRACK_NEW, TRACK_TRACKED, TRACK_LOST = 0, 1, 2, 3                    # PPY_TRACK_FREE .. PPY_TRACK_LOST
TRACK_MAX_TRACKS, TRACK_MAX_ROWS = 1024, 1024                                    # PPY_TRACK_MAX_TRACKS, PPY_TRACK_MAX_ROWS


class PPYoloHipError(RuntimeError):
    pass


_lib = None


class ConvCfgInfo(ctypes.Structure):
    """ppy_conv_cfg_info (include/ppyolo_hip.h)."""
    _fields_ = [(f, c_int) for f in ('family', 'local', 'operands', 'bm', 'bn', 'stages', 'splitk_mode', 'reads_presplit',
                                     'writes_presplit', 'bn_stats', 'stats_twin')]


class JpegInfo(ctypes.Structure):
    """ppy_jpeg_info_t (include/ppyolo_hip.h)."""
    _fields_ = [('status', c_int), ('width', c_int), ('height', c_int), ('out_width', c_int), ('out_height', c_int),
                ('orientation', c_int), ('components', c_int), ('h_samp', c_int * 3), ('v_samp', c_int * 3),
                ('blocks_w', c_int * 3), ('blocks_h', c_int * 3), ('restart_interval', c_int), ('coef_bytes', c_longlong),
                ('reason', ctypes.c_char * 64), ('progressive', c_int)]


JPEG_ACCEPT = {'progressive': 1, 'multiscan': 2, 'sampling': 4}      # PPY_JPEG_ACCEPT_* (include/ppyolo_hip.h)


class JpegScan(ctypes.Structure):
    """ppy_jpeg_scan_t (include/ppyolo_hip.h): the header of a scan record."""
    _fields_ = [('components', c_int), ('mcus_w', c_int), ('mcus_h', c_int), ('restart_interval', c_int), ('h_samp', c_int * 3),
                ('v_samp', c_int * 3), ('blocks_w', c_int * 3), ('segments', c_int), ('mcus', c_int), ('reserved', c_int),
                ('coef_offset', c_longlong * 3), ('coef_elems', c_longlong), ('table_offset', ctypes.c_uint),
                ('segment_offset', ctypes.c_uint), ('data_offset', ctypes.c_uint), ('data_bytes', ctypes.c_uint),
                ('record_bytes', ctypes.c_uint), ('reserved2', ctypes.c_uint)]


JPEG_SUBSEQ_MIN, JPEG_SUBSEQ_MAX, JPEG_SUBSEQ_DEFAULT = 8, 4096, 32      # PPY_JPEG_SUBSEQ_* (include/ppyolo_hip.h)


class JpegDesc(ctypes.Structure):
    """ppy_jpeg_desc_t (include/ppyolo_hip.h)."""
    _fields_ = [('width', c_int), ('height', c_int), ('components', c_int), ('orientation', c_int), ('h_samp', c_int * 3),
                ('v_samp', c_int * 3), ('blocks_w', c_int * 3), ('blocks_h', c_int * 3), ('coef_offset', c_longlong * 3),
                ('coef_bytes', c_longlong), ('coef_base', c_longlong), ('quant', (ctypes.c_ushort * 64) * 3)]


class JpegEncParams(ctypes.Structure):
    """ppy_jpeg_enc_params_t (include/ppyolo_hip.h)."""
    _fields_ = [('quality', c_int), ('h_samp', c_int), ('v_samp', c_int), ('restart_interval', c_int)]


class JpegEncDesc(ctypes.Structure):
    """ppy_jpeg_enc_desc_t (include/ppyolo_hip.h)."""
    _fields_ = [('src', c_void_p), ('row_stride', c_longlong), ('width', c_int), ('height', c_int), ('components', c_int),
                ('restart_interval', c_int), ('h_samp', c_int * 3), ('v_samp', c_int * 3), ('blocks_w', c_int * 3),
                ('blocks_h', c_int * 3), ('real_w', c_int * 3), ('real_h', c_int * 3), ('mcus_w', c_int), ('mcus_h', c_int),
                ('blocks', c_longlong), ('segments', c_longlong), ('coef_offset', c_longlong * 3), ('coef_bytes', c_longlong),
                ('coef_base', c_longlong), ('scan_capacity', c_longlong), ('ws_bytes', c_longlong), ('ws_base', c_longlong)]


class JpegEncSizes(ctypes.Structure):
    """ppy_jpeg_enc_sizes_t (include/ppyolo_hip.h)."""
    _fields_ = [('table_bytes', c_size_t), ('coef_bytes', c_size_t), ('ws_bytes', c_size_t), ('out_bytes', c_size_t)]


class PngDesc(ctypes.Structure):
    """ppy_png_desc_t (include/ppyolo_hip.h)."""
    _fields_ = [('width', c_int), ('height', c_int), ('bit_depth', c_int), ('colour_type', c_int), ('interlace', c_int),
                ('palette_entries', c_int), ('scan_offset', c_longlong), ('scan_bytes', c_longlong), ('palette', ctypes.c_ubyte * 768)]


class DrawImage(ctypes.Structure):
    """ppy_draw_image_t (include/ppyolo_hip.h)."""
    _fields_ = [('base', c_void_p), ('pitch', c_longlong), ('h', c_int), ('w', c_int)]


class PilImage(ctypes.Structure):
    """ppy_pil_image_t (include/ppyolo_hip.h)."""
    _fields_ = [('base', c_void_p), ('pitch', c_longlong), ('h', c_int), ('w', c_int)]


class TrackParams(ctypes.Structure):
    """ppy_track_params_t (include/ppyolo_hip.h)."""
    _fields_ = [('high_thresh', c_float), ('low_thresh', c_float), ('new_thresh', c_float), ('match_thresh', c_float * 3),
                ('max_lost', c_int), ('class_agnostic', c_int)]


PIL_FILTERS = {0: 'nearest', 1: 'lanczos', 2: 'bilinear', 3: 'bicubic', 4: 'box', 5: 'hamming'}      # Pillow's codes (ppy_pil_resize_plan)

DRAW_MAX_ROWS, DRAW_NAME_MAX = 1024, 64      # K and name length ppy_draw_detections_u8 takes (include/ppyolo_hip.h)

_PROTOS = {
    'ppy_version': (c_int, []),
    'ppy_error_string': (ctypes.c_char_p, [c_int]),
    'ppy_last_hip_error': (ctypes.c_char_p, []),
    'ppy_note_hip_error': (None, [c_int]),
    'ppy_conv2d_split_weights_bf16x3': (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p]),
    'ppy_conv2d_split_weights_f16x2': (c_int, [c_void_p, c_int, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ppy_conv2d_bn_act_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_void_p, c_void_p, c_void_p, c_int] + [c_int] * 13
                              + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_conv2d_bn_act_split_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_int, c_void_p, c_void_p, c_void_p, c_int] + [c_int] * 13
                                    + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p]),
    'ppy_conv2d_workspace_bytes': (c_size_t, [c_int] * 11),
    'ppy_conv2d_bn_partials_bytes': (c_size_t, [ctypes.c_longlong, c_int]),
    'ppy_conv2d_train_fwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int] + [c_int] * 10
                                 + [c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_int), c_void_p]),
    'ppy_bn_train_stats_merge_f32': (c_int, [c_void_p, c_size_t, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ppy_conv1x1_expand_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int]
                               + [c_int] * 7 + [c_void_p, c_void_p, c_void_p]),
    'ppy_conv3x3_maxpool_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int] + [c_int] * 6 + [c_void_p, c_void_p, c_void_p]),
    'ppy_conv1x1_stats_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'ppy_conv1x1_bn_apply_f32': (c_int, [c_void_p, c_int] + [c_void_p] * 8 + [c_int, c_void_p, c_int] + [c_int] * 7 + [c_void_p, c_void_p, c_void_p]),
    'ppy_conv2d_num_configs': (c_int, []),
    'ppy_conv2d_config_info': (c_int, [c_int, ctypes.POINTER(ConvCfgInfo)]),
    'ppy_conv2d_stream_first_config': (c_int, []),
    'ppy_conv2d_patch_first_config': (c_int, []),
    'ppy_conv2d_ws_first_config': (c_int, []),
    'ppy_conv2d_small_first_config': (c_int, []),
    'ppy_conv2d_pick': (c_int, [c_int] * 9 + [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'ppy_conv2d_dgrad_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int] + [c_int] * 11 + [c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_conv2d_dgrad_workspace_bytes': (c_size_t, [c_int] * 11),
    'ppy_train_prepare_weights_f16x2': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    'ppy_conv2d_dgrad_prepared_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int] + [c_int] * 10
                                      + [c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_conv2d_wgrad_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p] + [c_int] * 9 + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_conv2d_wgrad_workspace_bytes': (c_size_t, [c_int] * 9),
    'ppy_bn_train_workspace_bytes': (c_size_t, [c_int, c_int]),
    'ppy_bn_train_stats_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_size_t, c_void_p]),
    'ppy_bn_train_apply_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                        c_int, c_int, c_int, c_void_p, c_void_p]),
    'ppy_bn_train_bwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                      c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_act_bwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_longlong, c_int, c_int, c_void_p]),
    'ppy_upsample2x_bwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'ppy_spp_bwd_workspace_bytes': (c_size_t, [c_int] * 4),
    'ppy_spp_bwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                 c_void_p]),
    'ppy_dropblock_workspace_bytes': (c_size_t, [c_int] * 4),
    'ppy_dropblock_mask_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_ulonglong, c_void_p, c_size_t,
                                        c_void_p]),
    'ppy_dropblock_apply_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_longlong, c_int, c_void_p]),
    'ppy_sgd_momentum_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_longlong, c_float, c_float, c_float, c_int, c_void_p]),
    'ppy_avgpool2x2_bwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_int] + [c_int] * 4 + [c_void_p]),
    'ppy_maxpool3x3s2_bwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int] + [c_int] * 4 + [c_void_p]),
    'ppy_zero_insert_f32': (c_int, [c_void_p, c_int, c_void_p, c_int] + [c_int] * 7 + [c_void_p]),
    'ppy_ema_update_f32': (c_int, [c_void_p, c_void_p, c_longlong, c_float, c_float, c_void_p]),
    'ppy_add_inplace_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_longlong, c_int, c_void_p]),
    'ppy_upsample2x_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'ppy_channel_sum_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_yolov3_loss_workspace_bytes': (c_size_t, [c_int] * 3),
    'ppy_yolov3_loss_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_float), c_int, c_int, c_int, c_int, c_int,
                                     c_double, c_double, c_double, c_int, c_int, c_double, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                     c_size_t, c_void_p]),
    'ppy_stem_conv3x3s2_nchw_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                             c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'ppy_stem_conv3x3s2_nchw_x3_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                                c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'ppy_preprocess_u8_f32': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p]),
    'ppy_pil_resize_plan_bytes': (c_size_t, [c_int, ctypes.POINTER(PilImage), c_int, c_int, c_int]),
    'ppy_pil_resize_plan': (c_int, [c_int, ctypes.POINTER(PilImage), c_int, c_int, c_int, c_void_p, c_size_t, ctypes.POINTER(c_size_t),
                                    ctypes.c_char_p]),
    'ppy_pil_resize_u8': (c_int, [c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]),
    'ppy_preprocess_pil_u8_f32': (c_int, [c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_void_p]),
    'ppy_pil_crop_plan_bytes': (c_int, [c_int, ctypes.POINTER(PilImage), c_int, c_int, c_int, c_int, c_int, ctypes.c_float, c_int,
                                        ctypes.POINTER(c_size_t), ctypes.POINTER(c_int), ctypes.c_char_p]),
    'ppy_pil_crop_rows_u8': (c_int, [c_int, ctypes.POINTER(PilImage), c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, ctypes.c_float,
                                     c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ppy_pil_crop_list_u8': (c_int, [c_int, ctypes.POINTER(PilImage), c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                     c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ppy_augment_render_f32': (c_int, [c_void_p, c_longlong, c_int, c_int, c_void_p, ctypes.POINTER(c_double), c_int, c_void_p,
                                        c_void_p]),
    'ppy_augment_canvas': (c_int, [c_void_p, c_longlong, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'ppy_augment_render_src_f32': (c_int, [c_void_p, c_longlong, c_int, c_int, c_void_p, ctypes.POINTER(c_double), c_int, c_void_p,
                                            c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_longlong), ctypes.POINTER(c_int),
                                            ctypes.POINTER(c_int), c_void_p]),
    'ppy_augment_canvas_src': (c_int, [c_void_p, c_longlong, c_int, c_int, c_int, c_int, c_void_p, c_int, ctypes.POINTER(c_void_p),
                                        ctypes.POINTER(c_longlong), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p]),
    'ppy_augment_targets_f32': (c_int, [c_void_p, c_longlong, c_void_p, c_void_p, c_int, c_void_p]),
    'ppy_cocoeval_workspace_bytes': (c_size_t, [c_longlong] + [c_int] * 6),
    'ppy_cocoeval_records_f32': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    'ppy_cocoeval_bbox': (c_int, [c_void_p, c_void_p, c_longlong, c_int, c_int] + [c_void_p] * 6 + [c_int, c_int, c_void_p, c_int, c_void_p,
                                  c_int, c_void_p, c_int, c_void_p, ctypes.POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_size_t, c_void_p]),
    'ppy_maxpool3x3s2_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'ppy_avgpool2x2_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'ppy_spp_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                            c_void_p]),
    'ppy_dcnv2_sample_f32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p] + [c_int] * 8 + [c_void_p]),
    'ppy_dcnv2_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                              c_void_p, c_int] + [c_int] * 10 + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_dcnv2_workspace_bytes': (c_size_t, [c_int] * 9),
    'ppy_dcnv2_num_configs': (c_int, []),
    'ppy_dcnv2_backward_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]
                               + [c_int] * 7 + [c_void_p, c_size_t, c_void_p]),
    'ppy_dcnv2_backward_workspace_bytes': (c_size_t, [c_int] * 7),
    'ppy_yolo_decode_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_float), c_int,
                                    c_double, c_int, c_double, c_int, c_void_p, c_void_p, c_int, c_int, c_float,
                                    c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'ppy_yolo_decode_levels_f32': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                           c_int, c_double, c_int, c_double, c_int, c_void_p, c_void_p, c_int, c_float,
                                           c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'ppy_matrix_nms_f32': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float,
                                   c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    'ppy_matrix_nms_workspace_bytes': (c_size_t, [c_int]),
    'ppy_multiclass_nms_f32': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                       c_float, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p]),
    'ppy_multiclass_nms_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'ppy_merge_views_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'ppy_merge_views_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(c_int), c_void_p, c_int, c_int, c_float, c_float,
                                    c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, ctypes.c_char_p, c_void_p]),
    'ppy_fuse_views_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'ppy_fuse_views_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(c_int), c_void_p, ctypes.POINTER(c_float), c_void_p,
                                   c_int, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                   ctypes.c_char_p, c_void_p]),
    'ppy_track_state_bytes': (c_size_t, [c_int, c_int]),
    'ppy_track_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'ppy_track_update_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(TrackParams), c_void_p, c_size_t, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, ctypes.c_char_p, c_void_p]),
    'ppy_nms_candidates_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                       c_int, c_void_p]),
    'ppy_conv3x3_conv1x1_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int, c_void_p, c_int, c_void_p, c_int] + [c_int] * 6 + [c_float, c_float, c_void_p, c_void_p]),
    'ppy_lane_stream_create': (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(ctypes.c_uint32), c_int]),
    'ppy_lane_stream_destroy': (c_int, [c_void_p]),
    'ppy_jpeg_info': (c_int, [c_void_p, c_size_t, ctypes.POINTER(JpegInfo)]),
    'ppy_jpeg_entropy_decode': (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, ctypes.POINTER(JpegDesc), c_void_p]),
    'ppy_jpeg_info_ex': (c_int, [c_void_p, c_size_t, ctypes.c_uint, ctypes.POINTER(JpegInfo)]),
    'ppy_jpeg_entropy_decode_ex': (c_int, [c_void_p, c_size_t, ctypes.c_uint, c_void_p, c_size_t, ctypes.POINTER(JpegDesc), c_void_p]),
    'ppy_jpeg_workspace_bytes': (c_size_t, [c_int, ctypes.POINTER(JpegDesc)]),
    'ppy_jpeg_table_bytes': (c_size_t, [c_int]),
    'ppy_jpeg_pack_table': (c_int, [c_int, ctypes.POINTER(JpegDesc), ctypes.POINTER(c_void_p), ctypes.POINTER(c_longlong), c_int,
                                    c_void_p, c_size_t]),
    'ppy_jpeg_reconstruct_u8': (c_int, [c_int, ctypes.POINTER(JpegDesc), c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    'ppy_jpeg_scan_bytes': (c_size_t, [c_void_p, c_size_t, ctypes.POINTER(c_longlong)]),
    'ppy_jpeg_scan_prepare': (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, ctypes.POINTER(c_size_t), ctypes.POINTER(JpegDesc), c_void_p]),
    'ppy_jpeg_entropy_plan_bytes': (c_size_t, [c_int, c_longlong]),
    'ppy_jpeg_entropy_plan': (c_int, [c_int, ctypes.POINTER(JpegDesc), c_void_p, c_size_t, ctypes.POINTER(c_longlong), c_int, c_void_p,
                                      c_size_t, ctypes.POINTER(c_size_t)]),
    'ppy_jpeg_entropy_device': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_jpeg_entropy_twin': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t]),
    'ppy_jpeg_reason_string': (ctypes.c_char_p, [c_int]),
    'ppy_jpeg_enc_quant': (c_int, [c_int, c_void_p, c_void_p]),
    'ppy_jpeg_enc_header_bytes': (c_size_t, [c_int, c_int]),
    'ppy_jpeg_enc_header': (c_int, [ctypes.POINTER(JpegEncParams), c_int, c_int, c_int, c_void_p, c_size_t, ctypes.POINTER(c_size_t), c_void_p]),
    'ppy_jpeg_enc_scan_capacity': (c_size_t, [c_longlong, c_longlong]),
    'ppy_jpeg_enc_layout': (c_int, [ctypes.POINTER(JpegEncParams), c_int, ctypes.POINTER(JpegEncDesc), ctypes.POINTER(JpegEncSizes), c_void_p]),
    'ppy_jpeg_enc_pack_table': (c_int, [ctypes.POINTER(JpegEncParams), c_int, ctypes.POINTER(JpegEncDesc), c_void_p, c_size_t]),
    'ppy_jpeg_enc_coefficients': (c_int, [c_int, ctypes.POINTER(JpegEncDesc), c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_jpeg_enc_scan_device': (c_int, [c_int, ctypes.POINTER(JpegEncDesc), c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p,
                                         c_void_p, c_size_t, c_void_p]),
    'ppy_jpeg_enc_scan_host': (c_int, [ctypes.POINTER(JpegEncDesc), c_void_p, c_size_t, c_void_p, c_size_t, ctypes.POINTER(c_size_t), c_void_p]),
    'ppy_png_table_bytes': (c_size_t, [c_int]),
    'ppy_png_pack_table': (c_int, [c_int, ctypes.POINTER(PngDesc), ctypes.POINTER(c_void_p), ctypes.POINTER(c_longlong), c_void_p, c_size_t]),
    'ppy_png_workspace_bytes': (c_size_t, [c_int, ctypes.POINTER(PngDesc)]),
    'ppy_png_reconstruct_u8': (c_int, [c_int, ctypes.POINTER(PngDesc), c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    'ppy_draw_detections_u8': (c_int, [c_int, ctypes.POINTER(DrawImage), c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_int,
                                       c_void_p, c_void_p, ctypes.POINTER(c_int), c_void_p, c_void_p]),
    'ppy_group_norm_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_float, c_int, c_void_p, c_int, c_void_p, c_int, c_int]
                           + [c_int] * 4 + [c_void_p, c_size_t, c_void_p]),
    'ppy_mish_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'ppy_group_norm_train_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_float, c_int, c_void_p, c_int, c_void_p, c_int]
                                 + [c_int] * 4 + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'ppy_group_norm_bwd_workspace_bytes': (c_size_t, [c_int] * 5),
    'ppy_group_norm_bwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                       c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int] + [c_int] * 4 + [c_void_p, c_size_t, c_void_p]),
    'ppy_affine_act_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int] + [c_int] * 4 + [c_void_p]),
    'ppy_affine_bwd_workspace_bytes': (c_size_t, [c_int] * 4),
    'ppy_affine_bwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                   c_void_p, c_void_p, c_int] + [c_int] * 4 + [c_void_p, c_size_t, c_void_p]),
    'ppy_mish_bwd_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int] + [c_int] * 4 + [c_void_p]),
}


def exported_symbols():
    """Every entry point include/ppyolo_hip.h declares."""
    return sorted(_PROTOS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PPYoloHipError(
                'libppyolo_hip.so not found at %s -- build it with `python -c "import __graft_entry__ as g; '
                'g.build()"` (hipcc, gfx950). There is no CPU / PyTorch fallback for the HIP path.' % LIB_PATH)
        # PyTorch-ROCm ships its own libamdhip64; the process must hold ONE HIP runtime, the one torch initialises
        # (device memory and streams come from torch).  Loading this library first binds it to the system runtime
        # instead, and its launches then fail with hipErrorNoDevice -- so make sure torch's is mapped before dlopen.
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=''):
    if rc != OK:
        msg = lib().ppy_error_string(rc).decode()
        if rc == -4:                  # PPY_ERR_LAUNCH: say which HIP error it was
            msg += ' [%s]' % lib().ppy_last_hip_error().decode()
        raise PPYoloHipError('%s failed: %s (code %d)' % (what or 'libppyolo_hip call', msg, rc))


# ppy_conv_cfg_info as Python reads it: enums by name (in the header's order; `operands` as engine.math_mode names them), flags as bools
CFG_FAMILIES = ('fp32', 'bf16x3', 'f16x2', 'f16x2_slab', 'f16x2_tall', 'stream', 'patch', 'ws', 'ws_pre', 'kparity', 'small')
CFG_OPERANDS = ('fp32', 'bf16x3', 'f16x2')
CFG_SPLITK = ('none', 'workspace', 'workgroup')
ConvCfg = collections.namedtuple('ConvCfg', 'id family local operands bm bn stages splitk_mode reads_presplit writes_presplit bn_stats stats_twin')


@functools.lru_cache(None)
def conv_cfgs():
    """What every conv cfg id is and can do (ppy_conv2d_config_info): a list of ConvCfg indexed by id, read from the library once."""
    out = []
    for cfg in range(lib().ppy_conv2d_num_configs()):
        d = ConvCfgInfo()
        check(lib().ppy_conv2d_config_info(cfg, ctypes.byref(d)), 'ppy_conv2d_config_info')
        out.append(ConvCfg(cfg, CFG_FAMILIES[d.family], d.local, CFG_OPERANDS[d.operands], d.bm, d.bn, d.stages, CFG_SPLITK[d.splitk_mode],
                           bool(d.reads_presplit), bool(d.writes_presplit), bool(d.bn_stats), d.stats_twin))
    return out


def conv_cfg(cfg):
    """The ConvCfg of one explicit id (the library's own choice, cfg < 0, has no descriptor)."""
    if not 0 <= cfg < len(conv_cfgs()):
        raise PPYoloHipError('no conv cfg id %d' % cfg)
    return conv_cfgs()[cfg]
