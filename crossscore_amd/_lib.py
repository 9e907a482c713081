"""ctypes binding of libcrossscore_hip.so (include/crossscore_hip.h).  Fails loudly when the library is
missing: there is no CPU or eager fallback for the hot path."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcrossscore_hip.so")

CS_OK, CS_ERR_BAD_ARG, CS_ERR_UNSUPPORTED, CS_ERR_STATE, CS_ERR_HIP = range(5)
# cs_op_metric_map_u16 modes (CS_METRIC_*): the GT map's load_content conversion, by (metric type, metric min)
METRIC_SSIM_M1_1, METRIC_SSIM_0_1, METRIC_MAE, METRIC_MSE = range(4)
PNG_GRAY16, PNG_RGB8 = 0, 1  # cs_op_png_encode kinds (CS_PNG_*)
PNG_DYNAMIC, PNG_ADAPTIVE_FILTER = 1, 2  # cs_op_png_encode_ex flags (CS_PNG_*)
# status words of cs_op_png_decode (CS_PNGDEC_*)
(PNGDEC_OK, PNGDEC_BAD_CRC, PNGDEC_BAD_ADLER, PNGDEC_BAD_ZLIB_HEADER, PNGDEC_BAD_BLOCK_TYPE, PNGDEC_BAD_STORED_LEN, PNGDEC_BAD_CODE, PNGDEC_BAD_SYMBOL,
 PNGDEC_BAD_DISTANCE, PNGDEC_STREAM_SHORT, PNGDEC_STREAM_LONG, PNGDEC_BAD_FILTER, PNGDEC_INPUT_EXHAUSTED, PNGDEC_HEADER_MISMATCH,
 PNGDEC_BAD_FRAMING) = range(15)
JPEG_GRAY, JPEG_444, JPEG_422, JPEG_420 = range(4)  # cs_jpeg_info.sampling (CS_JPEG_*)
# status words of cs_op_jpeg_decode (CS_JPGDEC_*)
(JPGDEC_OK, JPGDEC_BAD_FRAMING, JPGDEC_HEADER_MISMATCH, JPGDEC_BAD_TABLE, JPGDEC_BAD_CODE, JPGDEC_BAD_SYMBOL, JPGDEC_INPUT_EXHAUSTED,
 JPGDEC_BAD_RESTART) = range(8)
JPGDEC_BAD_SCAN = 8  # cs_op_jpeg_decode_ex with JPEG_PROGRESSIVE only (CS_JPGDEC_BAD_SCAN)
JPEG_PROGRESSIVE = 1  # flag of cs_jpeg_probe_ex / cs_jpeg_decode_workspace_bytes_ex / cs_op_jpeg_decode_ex (CS_JPEG_PROGRESSIVE)
GTMAP_SSIM, GTMAP_MAE = 0, 1  # cs_op_gt_metric_map_u8 kinds (CS_GTMAP_*)

# CsEpilogue (csrc/cs_common.h)
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2  # cs_set_weight_typed
(EPI_BIAS_F16, EPI_BIAS_GELU_F16, EPI_BIAS_RELU_F16, EPI_BIAS_LEAKY_F16, EPI_RESID_F32, EPI_PATCH_F32, EPI_HEAD_SCORE,
 EPI_LN_F16, EPI_LN_GELU_F16, EPI_RESID_F32_LN) = range(10)


class CsConfig(C.Structure):
    _fields_ = [
        ("hidden", C.c_int), ("enc_layers", C.c_int), ("enc_heads", C.c_int), ("mlp_ratio", C.c_int),
        ("patch", C.c_int), ("pos_grid", C.c_int), ("pe_h", C.c_int), ("pe_w", C.c_int),
        ("dec_layers", C.c_int), ("dec_heads", C.c_int), ("do_self_attn", C.c_int), ("do_short_cut", C.c_int),
        ("act", C.c_int), ("pow_p", C.c_float), ("enc_chunk_images", C.c_int), ("ln_fold", C.c_int), ("lanes", C.c_int), ("pos_interp_legacy", C.c_int), ("enc_fused", C.c_int),
        ("operand_dtype", C.c_int), ("pe_interp_mode", C.c_int), ("skip_finite_check", C.c_int), ("swiglu", C.c_int),
    ]


class CsU8Image(C.Structure):
    """cs_u8_image: one decoded uint8 HWC image on the device and its resize / crop geometry (cs_forward_u8)."""
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("row_bytes", C.c_int), ("rs_h", C.c_int), ("rs_w", C.c_int),
                ("crop_y", C.c_int), ("crop_x", C.c_int)]


class CsPngInfo(C.Structure):
    """cs_png_info: what cs_png_probe reads from a file's framing and IHDR."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("color_type", C.c_int), ("bit_depth", C.c_int), ("interlace", C.c_int), ("kind", C.c_int),
                ("num_idat", C.c_int), ("idat_bytes", C.c_ulonglong)]


class CsJpegInfo(C.Structure):
    """cs_jpeg_info: what cs_jpeg_probe reads from a file's marker segments."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("components", C.c_int), ("sampling", C.c_int), ("restart_interval", C.c_int),
                ("entropy_offset", C.c_ulonglong)]


class CsJpegScanInfo(C.Structure):
    """cs_jpeg_scan_info: what cs_jpeg_probe_ex adds to cs_jpeg_info."""
    _fields_ = [("process", C.c_int), ("scans", C.c_int), ("entropy_offset", C.c_ulonglong)]


SHEET_FILL, SHEET_IMAGE, SHEET_BLEND, SHEET_RAMP, SHEET_FRAME, SHEET_TEXT = range(6)  # cs_sheet_panel.kind (CS_SHEET_*)
SHEET_MAX_PANELS, SHEET_MAX_SIDE = 48, 4096  # CS_SHEET_MAX_*


class CsSheetPanel(C.Structure):
    """cs_sheet_panel: one panel of cs_op_sheet_compose."""
    _fields_ = [("kind", C.c_int), ("dst_y", C.c_int), ("dst_x", C.c_int), ("dst_h", C.c_int), ("dst_w", C.c_int),
                ("src", C.c_void_p), ("src_h", C.c_int), ("src_w", C.c_int), ("src_row_bytes", C.c_int),
                ("src2", C.c_void_p), ("src2_h", C.c_int), ("src2_w", C.c_int), ("src2_row_bytes", C.c_int),
                ("rgb", C.c_uint8 * 3), ("param", C.c_int), ("text", C.c_char * 16)]


# every symbol include/crossscore_hip.h declares: name -> (restype, argtypes)
_vp, _i, _f, _ll, _sz = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_size_t
_fp = C.POINTER(C.c_float)
SYMBOLS = {
    "cs_create": (_vp, [C.POINTER(CsConfig)]),
    "cs_destroy": (None, [_vp]),
    "cs_last_error": (C.c_char_p, []),
    "cs_set_weight": (_i, [_vp, C.c_char_p, _vp, _i, _i, C.POINTER(C.c_int64)]),
    "cs_set_weight_typed": (_i, [_vp, C.c_char_p, _vp, _i, _i, _i, C.POINTER(C.c_int64)]),
    "cs_num_weights": (_i, [_vp]),
    "cs_weight_name": (C.c_char_p, [_vp, _i]),
    "cs_finalize": (_i, [_vp]),
    "cs_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "cs_encode_references": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "cs_forward_cached": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "cs_forward_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _fp, _fp, _vp, _vp, _i, _vp, _vp]),
    "cs_encode_references_u8": (_i, [_vp, _vp, _i, _i, _i, _fp, _fp, _vp, _vp]),
    "cs_forward_cached_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _fp, _fp, _vp, _vp, _i, _vp, _vp]),
    "cs_u8_input_supported": (_i, [_vp, _vp, _i, _i]),
    "cs_op_token_descriptors": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "cs_op_descriptor_centre": (_i, [_vp, _i, _i, _vp, _vp]),
    "cs_op_descriptor_unit": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "cs_op_select_references": (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "cs_op_gather_tokens": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "cs_forward_select": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "cs_forward_select_u8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _fp, _fp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "cs_op_group_descriptors": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "cs_op_select_references_grouped": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "cs_op_gather_tokens_ex": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _i]),
    "cs_forward_select_grouped": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "cs_forward_select_grouped_u8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _fp, _fp, _vp, _vp, _i, _vp, _vp,
                                          _vp, _vp]),
    "cs_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "cs_nonfinite_count": (_i, [_vp, C.POINTER(C.c_longlong)]),
    "cs_forward_stats": (_i, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_char_p, _sz]),
    "cs_debug_set_op_operand_dtype": (_i, [_i]),
    "cs_debug_capture": (_i, [_vp, _i]),
    "cs_debug_read": (_i, [_vp, C.c_char_p, _vp, _sz, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), _vp]),
    "cs_profile_enable": (_i, [_vp, _i]),
    "cs_profile_read": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "cs_profile_read_bytes": (_i, [_vp, _i, C.POINTER(C.c_double)]),
    "cs_op_gemm": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _f,
                        _vp, _vp, _i, _vp, _i, _vp, _f, _vp]),
    "cs_op_head_score": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "cs_op_attention": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _ll, _ll, _ll, _ll, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "cs_op_attention_weights": (_i, [_vp, _vp, _i, _i, _ll, _ll, _i, _i, _i, _i, _i, _f, _vp, _i, _vp, _vp]),
    "cs_op_reference_use": (_i, [_vp, _vp, _i, _i, _ll, _ll, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cs_request_reference_use": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cs_op_layernorm": (_i, [_vp, _i, _i, _vp, _vp, _f, _vp, _vp, _vp]),
    "cs_op_ln_finalize": (_i, [_vp, _i, _i, _i, _i, _f, _vp, _vp]),
    "cs_op_silu_mul": (_i, [_vp, _i, _i, _i, _vp]),
    "cs_op_im2col": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "cs_op_patch_embed": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "cs_op_patch_embed_fused": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "cs_op_patch_embed_fused_u8": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "cs_debug_patch_fused_enable": (None, [_i]),
    "cs_set_lanes": (_i, [_vp, _i]),
    "cs_redraw_lane_streams": (_i, [_vp]),
    "cs_debug_stream_probe_log": (None, [_i]),
    "cs_op_pos_bicubic": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "cs_op_pos_bicubic_ex": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "cs_op_pe_bilinear": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "cs_op_pe_interp": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "cs_op_score_to_gray16": (_i, [_vp, C.c_longlong, _i, _vp, _vp]),
    "cs_op_score_to_rgb": (_i, [_vp, C.c_longlong, C.c_float, C.c_float, _vp, _vp, _vp]),
    "cs_png_bound": (_sz, [_i, _i, _i]),
    "cs_png_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "cs_op_png_encode": (_i, [_vp, _i, _i, _i, _i, _ll, _vp, _sz, _vp, _vp, _vp]),
    "cs_op_png_encode_ex": (_i, [_vp, _i, _i, _i, _i, _ll, _vp, _sz, _vp, _vp, _vp, _i]),
    "cs_png_probe": (_i, [_vp, _sz, _vp, _vp, _i]),
    "cs_png_decode_workspace_bytes": (_sz, [_i, _i, _i, _i, _sz]),
    "cs_op_png_decode": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _vp, _ll, _vp, _vp, _vp]),
    "cs_jpeg_probe": (_i, [_vp, _sz, _vp]),
    "cs_jpeg_decode_workspace_bytes": (_sz, [_i, _i, _i, _sz]),
    "cs_op_jpeg_decode": (_i, [_vp, _vp, _vp, _sz, _i, _i, _i, _vp, _ll, _vp, _vp, _vp]),
    "cs_jpeg_probe_ex": (_i, [_vp, _sz, _i, _vp, _vp]),
    "cs_jpeg_decode_workspace_bytes_ex": (_sz, [_i, _i, _i, _sz, _i]),
    "cs_op_jpeg_decode_ex": (_i, [_vp, _vp, _vp, _sz, _i, _i, _i, _vp, _ll, _vp, _vp, _i, _vp]),
    "cs_debug_jpeg_scan_levels": (None, [_i]),
    "cs_op_denorm_to_rgb8": (_i, [_vp, _i, _i, _i, _fp, _fp, _vp, _vp]),
    "cs_op_metric_map_u16": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "cs_op_gt_metric_map_u8": (_i, [_vp, _vp, _i, _i, _i, _ll, _i, _vp, _i, _vp]),
    "cs_op_metric_map_sums_u16": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _vp, _vp]),
    "cs_op_gt_metric_sums_u8": (_i, [_vp, _vp, _i, _i, _i, _ll, _vp, _vp]),
    "cs_score_gt_workspace_bytes": (_sz, [_i, _i, _i]),
    "cs_op_score_gt_stats": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "cs_score_pool_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "cs_op_score_pool_f32": (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int32), _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cs_op_score_pool_u16": (_i, [_vp, _i, _i, _i, _i, _ll, C.POINTER(C.c_int32), _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cs_op_sheet_compose": (_i, [C.POINTER(CsSheetPanel), _i, _vp, _i, _i, _vp]),
    "cs_op_preprocess_u8": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_float), C.POINTER(C.c_float), _vp, _vp, _vp]),
    "cs_op_pack_f16": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "cs_op_streams_overlap": (_i, [_vp, _vp, _vp]),
    "cs_op_ln_fold_consts": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "cs_gemm_column_tiles": (_i, [_i]),
    "cs_debug_gemm256_enable": (None, [_i]),
    "cs_debug_gemm256_kmin": (None, [_i]),
    "cs_debug_gemm_grid": (None, [_i]),
    "cs_debug_panel_impl": (None, [_i]),
    "cs_panel_supported": (_i, [_i, _i]),
    "cs_panel_image_bytes": (_sz, [_i]),
    "cs_op_panel_pack": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cs_op_linear_layernorm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _vp]),
    "cs_op_linear_layernorm_linear": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "cs_debug_rowln_enable": (None, [_i]),
    "cs_op_encoder_panel": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp]),
    # head fit (csrc/headfit.hip)
    "cs_head_fit_supported": (_i, [_i, _i]),
    "cs_head_fit_row_tile": (_i, []),
    "cs_head_fit_row_chunk": (_i, []),
    "cs_head_fit_g_columns": (_i, []),
    "cs_head_backward_workspace_bytes": (_sz, [_i, _i, _i]),
    "cs_gemm_tn_workspace_bytes": (_sz, [_i, _i, _i]),
    "cs_op_head_grad_z": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _i, _vp, _vp, _vp, _vp]),
    "cs_debug_op_head_grad_z_tap": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "cs_op_gemm_tn": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _f, _i, _vp, _i, _vp, _vp, _vp]),
    "cs_op_head_backward": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, C.c_double, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cs_head_backward": (_i, [_vp, _vp, _i, _i, _i, C.c_double, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cs_debug_head_inputs": (_i, [_vp, _vp, _vp, _i, _vp]),
    "cs_op_adamw": (_i, [_vp, _vp, _vp, _vp, _ll, _f, _f, _f, _f, _f, _i, _vp, _vp]),
    "cs_set_head_weights": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    # tail fit (csrc/tailfit.hip)
    "cs_tail_fit_supported": (_i, [_i, _i]),
    "cs_tail_fit_ln_row_tile": (_i, []),
    "cs_ln_backward_workspace_bytes": (_sz, [_i, _i]),
    "cs_tail_backward_workspace_bytes": (_sz, [_i, _i, _i]),
    "cs_op_ln_backward": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _f, _i, _f, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "cs_op_tail_backward": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _f, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _f,
                                 C.c_double, _i] + [_vp] * 13),
    "cs_fit_tail_keep": (_i, [_vp, _i]),
    "cs_tail_backward": (_i, [_vp, _vp, _i, _i, _i, C.c_double, _i] + [_vp] * 12),
    "cs_debug_tail_inputs": (_i, [_vp, _vp, _vp, _i, _vp]),
    "cs_set_tail_weights": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # attention backward (csrc/attnbwd.hip)
    "cs_attention_backward_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "cs_attention_backward_tiles": (_i, [_i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cs_op_attention_backward": (_i, [_vp] * 6 + [_i] * 5 + [_ll] * 5 + [_i] * 5 + [_f, _vp, _i, _ll, _vp, _i, _ll, _vp, _i, _ll, _vp, _vp]),
    # cross-attention fit (csrc/crossfit.hip)
    "cs_cross_fit_supported": (_i, [_i, _i, _i]),
    "cs_cross_backward_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "cs_op_cross_backward": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i,
                                  _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _f, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _f,
                                  C.c_double, _i] + [_vp] * 19),
    "cs_fit_cross_keep": (_i, [_vp, _i]),
    "cs_cross_backward": (_i, [_vp, _vp, _i, _i, _i, C.c_double, _i] + [_vp] * 18),
    "cs_debug_cross_inputs": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "cs_set_cross_weights": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # whole-layer fit (csrc/layerfit.hip)
    "cs_layer_fit_supported": (_i, [_i, _i, _i, _i]),
    "cs_layer_backward_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "cs_op_layer_backward": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp,
                                  _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i,
                                  _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _f, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _f,
                                  C.c_double, _i] + [_vp] * 25),
    "cs_fit_layer_keep": (_i, [_vp, _i]),
    "cs_layer_backward": (_i, [_vp, _vp, _i, _i, _i, C.c_double, _i] + [_vp] * 24),
    "cs_debug_layer_inputs": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "cs_set_layer_weights": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_lib = None


class CrossScoreHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """dlopen the in-tree library and bind every declared symbol.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CrossScoreHipError(
            f"{LIB_PATH} is missing: build it with `python -m crossscore_amd.build` (hipcc --offload-arch=gfx950). "
            "The CrossScore hot path has no CPU/eager fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().cs_last_error().decode("utf-8", "replace")


def check(rc: int) -> None:
    """Maps library status codes to the exceptions the reference raises for the same conditions:
    ValueError for bad shapes / configs (regression_layer.py:37, check_config.py:23-28, image.py:15 assert),
    RuntimeError for state and HIP errors (load_state_dict / CUDA errors)."""
    if rc == CS_OK:
        return
    msg = last_error()
    if rc in (CS_ERR_BAD_ARG,):
        raise ValueError(msg)
    if rc == CS_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise CrossScoreHipError(msg)
