"""ctypes binding of libhps.so (C ABI: include/hps.h).

PyTorch is only plumbing here: tensors own device memory, ``data_ptr()`` and the current HIP stream
are handed to the library.  There is no CPU implementation behind these calls -- if the library or a
HIP device is missing the call fails loudly.

``dev_library()`` is a context manager for tests / tests/dev only: inside it every call goes to libhps_dev.so
(include/hps_dev.h: the product code plus earlier kernel generations, alternate variants, tuning switches).
"""
import contextlib
import ctypes
import os

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libhps.so")
DEV_LIB_PATH = os.path.join(_PKG_DIR, "libhps_dev.so")

_c = ctypes
_P = _c.c_void_p
_I = _c.c_int

# name -> argtypes (restype is always int unless listed in _RESTYPES)
_PROTOTYPES = {
    "hps_version": [],
    "hps_last_error": [],
    "hps_stream_create_cu_partition": [_I, _I, _c.POINTER(_P)],
    "hps_stream_destroy": [_P],
    "hps_smpl_pose_prep": [_P, _P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _P],
    "hps_smpl_blend": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "hps_smpl_lbs": [_P, _I, _P, _P, _P, _I, _I, _P, _P, _I, _I, _P],
    "hps_smpl_mesh_fused": [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P],
    "hps_smpl_mesh_fused_picks": [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P],
    "hps_smpl_mesh_fused_shared_shape": [_P] * 8 + [_I, _I, _P] + [_I] * 5 + [_P, _P, _I, _P],
    "hps_smpl_split_bf16x3_bytes": [_I, _I],
    "hps_smpl_split_bf16x3_mesh_tile": [],
    "hps_smpl_split_bf16x3": [_P, _I, _I, _I, _I, _P, _P],
    "hps_smpl_mesh_fused_shared_shape_bf16x3": [_P] * 8 + [_I, _I, _P] + [_I] * 4 + [_P, _P, _I, _P],
    "hps_smpl_v_shaped": [_P, _I, _P, _I, _P, _P, _I, _I, _P],
    "hps_smpl_mesh_fused_np": [_I],
    "hps_smpl_lbs_backward": [_P, _I, _P, _P, _P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "hps_smpl_blend_backward": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "hps_smpl_pose_prep_backward": [_P, _P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _I, _P],
    "hps_smpl_joints": [_P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _I, _P],
    "hps_vertex_uncertainty": [_P, _P, _I, _I, _I, _P],
    "hps_joints_and_uncertainty": [_P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P],
    "hps_query_workspace": [_I, _c.c_int64, _c.c_int64, _c.c_int64],
    "hps_mf_sample": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _c.c_float, _c.c_float, _P, _P, _P, _c.c_uint64,
                      _c.c_int64, _P, _I, _P, _P, _P, _P],
    "hps_infer_assemble": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "hps_quat_to_rotmat": [_P, _P, _I, _P],
    "hps_rot6d_to_rotmat": [_P, _P, _I, _P],
    "hps_batch_rodrigues": [_P, _P, _I, _P],
    "hps_linear": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "hps_head_trunk": [_P] + [_I] + [_P] * 14 + [_I] * 7 + [_P],
    "hps_head_joint_level": [_P, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _c.c_float, _P, _P, _I, _I, _P],
    "hps_head_joint_level_svd": [_P, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _c.c_float, _P, _P, _P, _P, _I, _I, _I, _P],
    "hps_svd3_packed": [_P, _P, _I, _I, _P],
    "hps_host_svd3_emulated": [_P, _P, _I, _I],
    "hps_host_svd_flavor": [],
    "hps_host_svd3_packed": [_P, _P, _I, _I],
    "hps_host_bind_lapack": [_c.c_char_p],
    "hps_head_svd_finish": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "hps_canny_edges": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _c.c_float, _I, _P],
    "hps_canny_edge_map": [_P, _P, _I, _P, _c.c_int64, _I, _I, _I, _I, _c.c_float, _I, _P],
    "hps_proxy_rep": [_P, _P, _P, _P, _I, _I, _I, _I, _c.c_float, _P],
    "hps_pointset_errors": [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "hps_heatmaps_to_joints2d": [_P, _P, _P, _I, _I, _I, _c.c_float, _P],
    "hps_sample_joints2d_error": [_P, _P, _I, _P, _P, _P, _c.c_float, _P, _I, _I, _P],
    "hps_conv2d_bn_act_pad": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P],
    "hps_conv2d_bn_act_pad_down": [_P] * 9 + [_I] * 14 + [_P, _P],
    "hps_bottleneck_expand_down": [_P] * 9 + [_I] * 12 + [_P],
    "hps_conv3x3_winograd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P],
    "hps_conv3x3_winograd_workspace": [_I, _I, _I, _I, _I],
    "hps_stem_phase_frames_bytes": [_I, _I, _I],
    "hps_stem_phase_split": [_P, _P, _I, _I, _I, _I, _P],
    "hps_proxy_rep_phase_frames": [_P, _P, _P, _P, _I, _I, _I, _I, _c.c_float, _P],
    "hps_stem_winograd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "hps_stem_pool_side_bytes": [_I, _I, _I],
    "hps_stem_winograd_pooled": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "hps_stem_winograd_pooled_nchw": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "hps_sums_f64": [_P, _P, _P, _I, _c.c_double, _P, _P, _P, _P],
    "hps_sizeof_enc_op": [],
    "hps_encoder_run": [_P, _I, _P],
    "hps_head_pose_levels": [_P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _c.c_float, _P, _P, _P, _P, _P, _P,
                             _P, _P, _I, _I, _I, _I, _P],
    "hps_nchw_to_padded_nhwc": [_P, _P, _I, _I, _I, _I, _I, _P],
    "hps_nchw_to_padded_nhwc_generic": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "hps_maxpool3x3s2_pad": [_P, _P, _I, _I, _I, _I, _I, _P],
    "hps_global_avgpool_pad": [_P, _P, _I, _I, _I, _I, _I, _P],
    "hps_mf_log_norm_const": [_P, _I, _P, _P, _P, _P],
    "hps_mf_nll": [_P, _P, _P, _P, _P, _I, _c.c_double, _P, _P, _P, _P, _P],
    "hps_mf_loss_forward": [_P, _P, _P, _P],
    "hps_mf_loss_backward": [_P, _P, _P, _P],
    "hps_head_forward_refine": [_P, _I] + [_P] * 9 + [_I] + [_P] * 6 + [_c.c_float] + [_P] * 13 + [_I] * 7 + [_P],
    "hps_head_pose_levels_backward": [_P, _I, _I, _P, _P, _I] + [_P] * 21 + [_I, _I, _I, _P],
    "hps_head_pose_levels_backward_factors": [_P, _I, _I, _P, _P, _I] + [_P] * 23 + [_I, _I, _I, _P],
    "hps_mf_sample_keep_quat": [_P, _P, _P, _I, _I, _I, _I, _c.c_float, _c.c_float, _P, _P, _P, _c.c_uint64, _c.c_int64, _I, _P, _P, _P, _P],
    "hps_mf_sample_backward": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _c.c_float, _P, _P, _P, _P],
    "hps_head_trunk_backward": [_P, _I] + [_P] * 20 + [_I] * 7 + [_P],
    "hps_rot6d_to_rotmat_backward": [_P, _P, _P, _I, _P],
    "hps_conv_wgrad": [_P] * 4 + [_I] * 12 + [_P],
    "hps_conv_wgrad_slice_pixels": [_I, _I],
    "hps_conv_wgrad_workspace": [_I] * 9,
    "hps_conv_dgrad": [_P] * 4 + [_I] * 12 + [_P],
    "hps_conv1x1_dgrad": [_P] * 4 + [_I] * 9 + [_P],
    "hps_conv1x1_wgrad": [_P] * 4 + [_I] * 9 + [_P],
    "hps_conv1x1_wgrad_slice_pixels": [_I, _I],
    "hps_conv1x1_wgrad_workspace": [_I] * 6,
    "hps_relu_gate_pad": [_P] * 4 + [_I] * 6 + [_P],
    "hps_relu_gate_workspace": [_I] * 4,
    "hps_maxpool3x3s2_backward": [_P] * 3 + [_I] * 5 + [_P],
    "hps_global_avgpool_backward": [_P] * 2 + [_I] * 5 + [_P],
    "hps_bn_batch_stats": [_P] * 4 + [_I] * 5 + [_P],
    "hps_bn_batch_stats_workspace": [_I] * 4,
    "hps_bn_train_fold": [_P] * 5 + [_c.c_double, _c.c_double, _c.c_longlong] + [_P] * 5 + [_I, _P],
    "hps_bn_apply_act_pad": [_P] * 5 + [_I] * 7 + [_P],
    "hps_bn_train_backward_sums": [_P] * 7 + [_I] * 7 + [_P],
    "hps_bn_train_backward_sums_workspace": [_I] * 4,
    "hps_bn_train_backward_dz": [_P] * 7 + [_I] * 7 + [_P],
    "hps_seg_bbox_affine": [_P, _c.c_int64, _P, _I, _I, _I, _I, _c.c_float, _P, _P, _P, _P, _P, _P],
    "hps_train_crop_augment": [_P, _c.c_int64, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "hps_train_joints2d": [_P, _P, _P, _P, _P, _I, _I, _c.c_float, _I, _I, _P, _P, _P, _P, _P],
    "hps_sizeof_adam_entry": [],
    "hps_adam_step": [_P, _I, _P, _I, _P],
    "hps_sizeof_refresh_op": [],
    "hps_weights_refresh": [_P, _I, _P],
    "hps_sizeof_render_args": [],
    "hps_render": [_P, _P],
    "hps_sizeof_silhouette_args": [],
    "hps_silhouette_iou": [_P, _P],
    "hps_sizeof_train_metrics_args": [],
    "hps_train_metrics_update": [_P, _P],
    "hps_sizeof_vis_views_args": [],
    "hps_vis_views": [_P, _P],
    "hps_sizeof_vis_compose_args": [],
    "hps_vis_compose": [_P, _P],
    "hps_sizeof_vis_uncrop_args": [],
    "hps_vis_uncrop": [_P, _P],
    "hps_sizeof_png_encode_args": [],
    "hps_png_bound": [_I, _I, _I],
    "hps_png_segment_rows": [_I, _I, _I],
    "hps_png_encode": [_P, _P],
    "hps_sizeof_jpeg_header": [],
    "hps_sizeof_jpeg_decode_args": [],
    "hps_jpeg_parse": [_P, _c.c_int64, _P],
    "hps_jpeg_decode": [_P, _P],
    "hps_sizeof_jpeg_encode_args": [],
    "hps_jpeg_encode_bound": [_I, _I, _I, _I],
    "hps_jpeg_encode": [_P, _P],
    "hps_sizeof_c16_problem": [],
    "hps_conv2d_bn_act_c16": [_P, _I, _P],
    "hps_hrnet_pack_input": [_P, _P, _I, _I, _I, _I, _I, _P],
    "hps_hrnet_unpack_output": [_P, _P, _I, _I, _I, _I, _I, _P],
    "hps_sizeof_hrnet_fuse_args": [],
    "hps_hrnet_fuse": [_P, _P],
    "hps_sizeof_hrnet_op": [],
    "hps_hrnet_run": [_P, _I, _P],
    "hps_sizeof_predict_boxes_args": [],
    "hps_predict_boxes": [_P, _P],
    "hps_sizeof_crop_bilinear_args": [],
    "hps_crop_bilinear": [_P, _P],
    "hps_sizeof_hrnet_keypoints_args": [],
    "hps_hrnet_keypoints": [_P, _P],
    "hps_sizeof_texture_gather_args": [],
    "hps_texture_gather": [_P, _P],
    "hps_sizeof_resize_bilinear_u8_args": [],
    "hps_resize_bilinear_u8": [_P, _P],
    "hps_sizeof_eval_crop_u8_args": [],
    "hps_eval_crop_u8": [_P, _P],
    "hps_keypoints_scale_round": [_P, _P, _P, _P, _I, _I, _P],
    "hps_sizeof_eval_heatmaps_args": [],
    "hps_eval_heatmaps": [_P, _P],
    "hps_sizeof_det_transform_args": [],
    "hps_det_transform": [_P, _P],
    "hps_det_subsample2": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "hps_sizeof_det_rpn_decode_args": [],
    "hps_det_rpn_decode": [_P, _P],
    "hps_sizeof_det_nms_args": [],
    "hps_det_nms": [_P, _P],
    "hps_sizeof_det_roi_align_args": [],
    "hps_det_roi_align": [_P, _P],
    "hps_det_roi_align_halo": [_P, _I, _P],
    "hps_sizeof_det_box_decode_args": [],
    "hps_det_box_decode": [_P, _P],
    "hps_sizeof_det_gather_args": [],
    "hps_det_gather": [_P, _P],
    "hps_sizeof_det_mask_predict_args": [],
    "hps_det_mask_predict": [_P, _P],
    "hps_sizeof_det_paste_masks_args": [],
    "hps_det_paste_masks": [_P, _P],
}
_RESTYPES = {"hps_last_error": _c.c_char_p, "hps_smpl_split_bf16x3_bytes": _c.c_size_t, "hps_query_workspace": _c.c_int64, "hps_conv3x3_winograd_workspace": _c.c_size_t,
             "hps_stem_phase_frames_bytes": _c.c_size_t, "hps_stem_pool_side_bytes": _c.c_size_t,
             "hps_conv_wgrad_workspace": _c.c_size_t, "hps_conv1x1_wgrad_workspace": _c.c_size_t, "hps_relu_gate_workspace": _c.c_size_t,
             "hps_bn_batch_stats_workspace": _c.c_size_t, "hps_bn_train_backward_sums_workspace": _c.c_size_t,
             "hps_png_bound": _c.c_int64, "hps_jpeg_encode_bound": _c.c_int64}

EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

_lib = None
_dev_lib = None
_use_dev = False


class EncOp(_c.Structure):
    """include/hps.h: hps_enc_op."""
    _fields_ = [("kind", _I), ("x", _P), ("w", _P), ("scale", _P), ("shift", _P), ("residual", _P), ("y", _P),
                ("splitk_ws", _P)] + [(n, _I) for n in ("B", "H", "W", "ipad", "Cin", "Cout", "KH", "KW", "stride", "pad", "opad",
                                                       "relu", "row_mode", "variant", "ksplit")] + [
                    ("w_down", _P), ("scale_down", _P), ("shift_down", _P), ("y_down", _P), ("x_down", _P), ("ipad_down", _I), ("Cin_down", _I)]


class MfLossArgs(_c.Structure):
    """include/hps.h: hps_mf_loss_args (struct_bytes = ctypes.sizeof(MfLossArgs); the library rejects any other value)."""
    _fields_ = [("struct_bytes", _I), ("reduction", _I)] + [
        (n, _c.c_int64) for n in ("n_pose", "shape_B", "n_shape", "j2d_B", "Ns", "K", "n_glob", "n_verts", "n_joints3d")] + [
        ("img_wh", _c.c_double), ("overreg", _c.c_double), ("weights", _c.c_double * 6)] + [
        (n, _P) for n in ("pose_F", "pose_U", "pose_S", "pose_V", "shape_loc", "shape_scale", "joints2d", "glob_rotmats", "verts",
                          "joints3d", "t_pose_rotmats", "t_shape", "t_joints2d", "t_joints2d_vis", "t_glob_rotmats", "t_verts",
                          "t_joints3d", "g_pose_F", "g_pose_S", "g_shape_loc", "g_shape_scale", "g_joints2d", "g_glob_rotmats",
                          "g_verts", "g_joints3d")]


class AdamEntry(_c.Structure):
    """include/hps.h: hps_adam_entry."""
    _fields_ = [("param", _P), ("grad", _P), ("exp_avg", _P), ("exp_avg_sq", _P), ("numel", _c.c_int64)] + [
        (n, _c.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "bias_correction1", "bias_correction2_sqrt")] + [
        ("decoupled", _I), ("reserved", _I)]


class RefreshOp(_c.Structure):
    """include/hps.h: hps_refresh_op."""
    _fields_ = [("kind", _I), ("scale_dim", _I), ("src", _P), ("dst", _P), ("dst2", _P), ("aux0", _P), ("aux1", _P), ("aux2", _P),
                ("eps", _c.c_double), ("n", _I * 4), ("sstride", _I * 4), ("dstride", _I * 4)]


class RenderArgs(_c.Structure):
    """include/hps.h: hps_render_args (struct_bytes = ctypes.sizeof(RenderArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "H", "W", "num_verts", "num_dp_verts", "num_faces", "projection", "tex_h", "tex_w",
                                  "cam_t_stride", "scale_stride")] + [("light_stride", _I * 4)] + [
        (n, _P) for n in ("vertices", "verts_map", "faces", "vf_offsets", "vf_faces", "verts_iuv", "verts_uv", "cam_t", "scale",
                          "light_location", "ambient", "diffuse", "specular", "texture", "verts_features", "workspace", "iuv", "rgb",
                          "depth", "pix_to_face", "bary", "iuv_train")]


class SilhouetteArgs(_c.Structure):
    """include/hps.h: hps_silhouette_args (struct_bytes = ctypes.sizeof(SilhouetteArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "M", "W", "group", "num_verts", "num_dp_verts", "num_faces", "projection", "flip_x_pi",
                                  "cam_t_stride", "scale_stride")] + [
        (n, _P) for n in ("vertices", "verts_map", "faces", "verts_iuv", "cam_t", "scale", "target", "workspace", "counts", "mask_out")]


class TrainMetricsArgs(_c.Structure):
    """include/hps.h: hps_train_metrics_args (struct_bytes = ctypes.sizeof(TrainMetricsArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "P", "J", "K", "N", "batch_size", "mask", "split", "num_status")] + [
        ("img_wh", _c.c_float)] + [
        (n, _P) for n in ("pred_verts", "target_verts", "pred_reposed", "target_reposed", "pred_joints3d", "target_joints3d",
                          "pred_joints2d", "target_joints2d", "pred_joints2d_samples", "vis", "loss", "status", "workspace", "sums")]


class VisView(_c.Structure):
    """include/hps.h: hps_vis_view."""
    _fields_ = [("vertices", _P), ("var", _P), ("yaw", _I), ("camera", _I)]


class VisViewsArgs(_c.Structure):
    """include/hps.h: hps_vis_views_args (struct_bytes = ctypes.sizeof(VisViewsArgs); the library rejects any other value)."""
    _fields_ = [("struct_bytes", _I), ("num_views", _I), ("num_verts", _I), ("constant", _c.c_float), ("fixed_cam_t", _c.c_float * 3),
                ("fixed_scale", _c.c_float), ("cam_z", _c.c_float), ("views", _c.POINTER(VisView))] + [
        (n, _P) for n in ("lut", "cam", "out_vertices", "out_colours", "out_cam_t", "out_scale")]


class VisPanel(_c.Structure):
    """include/hps.h: hps_vis_panel."""
    _fields_ = [(n, _I) for n in ("kind", "row", "col", "render")]


class VisComposeArgs(_c.Structure):
    """include/hps.h: hps_vis_compose_args (struct_bytes = ctypes.sizeof(VisComposeArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "rows", "cols", "wh", "num_panels", "num_renders", "D", "proxy_channels", "num_joints")] + [
        ("panels", _c.POINTER(VisPanel))] + [(n, _P) for n in ("rgb", "iuv", "crop", "proxy", "joints", "out")]


class VisUncropArgs(_c.Structure):
    """include/hps.h: hps_vis_uncrop_args (struct_bytes = ctypes.sizeof(VisUncropArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "H", "W", "wh")] + [
        (n, _P) for n in ("rgb", "iplane", "image", "bbox_centre", "bbox_wh", "out")]


PNG_MAX_IMAGES = 8


class PngImage(_c.Structure):
    """include/hps.h: hps_png_image."""
    _fields_ = [("pixels", _P), ("H", _I), ("W", _I), ("C", _I), ("strategy", _I), ("out", _P), ("capacity", _c.c_int64), ("length", _P),
                ("workspace", _P)]


class PngEncodeArgs(_c.Structure):
    """include/hps.h: hps_png_encode_args (struct_bytes = ctypes.sizeof(PngEncodeArgs); the library rejects any other value)."""
    _fields_ = [("struct_bytes", _I), ("num_images", _I), ("image", PngImage * PNG_MAX_IMAGES)]


class JpegHuff(_c.Structure):
    """include/hps.h: hps_jpeg_huff."""
    _fields_ = [("bits", _c.c_uint8 * 16), ("vals", _c.c_uint8 * 256)]


class JpegHeader(_c.Structure):
    """include/hps.h: hps_jpeg_header (struct_bytes = ctypes.sizeof(JpegHeader); written by hps_jpeg_parse)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "width", "height", "ncomp", "hs", "vs", "restart_interval", "scan_offset", "scan_length",
                                  "num_blocks", "num_intervals", "file_bytes")] + [
        ("quant", (_c.c_uint8 * 64) * 3), ("dc", JpegHuff * 3), ("ac", JpegHuff * 3)]


class JpegImage(_c.Structure):
    """include/hps.h: hps_jpeg_image."""
    _fields_ = [(n, _P) for n in ("data", "header", "header_dev", "out", "workspace")]


class JpegDecodeArgs(_c.Structure):
    """include/hps.h: hps_jpeg_decode_args (struct_bytes = ctypes.sizeof(JpegDecodeArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "num_images", "mode", "subseq_bits")] + [("status", _P), ("rounds", _P),
                                                                                         ("image", JpegImage * 64)]


JPEG_MAX_DIM, JPEG_MAX_SCAN_BYTES, JPEG_NOT_FOR_DEVICE = 8192, 1 << 22, 1
JPEG_ENC_MAX_IMAGES = 8


class JpegEncImage(_c.Structure):
    """include/hps.h: hps_jpeg_enc_image."""
    _fields_ = [("pixels", _P), ("H", _I), ("W", _I), ("C", _I), ("quality", _I), ("sampling", _I), ("reserved", _I), ("out", _P),
                ("capacity", _c.c_int64), ("length", _P), ("workspace", _P)]


class JpegEncodeArgs(_c.Structure):
    """include/hps.h: hps_jpeg_encode_args (struct_bytes = ctypes.sizeof(JpegEncodeArgs); the library rejects any other value)."""
    _fields_ = [("struct_bytes", _I), ("num_images", _I), ("image", JpegEncImage * JPEG_ENC_MAX_IMAGES)]


JPEG_RGB, JPEG_NATIVE, JPEG_GREY = 0, 1, 2
JPEG_ST_MARKERS, JPEG_ST_CODE, JPEG_ST_OVERRUN, JPEG_ST_SHORT = 1, 2, 4, 8


class C16Problem(_c.Structure):
    """include/hps.h: hps_c16_problem."""
    _fields_ = [(n, _P) for n in ("x", "w", "scale", "shift", "residual", "y")] + [
        (n, _I) for n in ("B", "H", "W", "ipad", "Cin", "Cout", "K", "stride", "opad", "relu")]


class HrnetFuseArgs(_c.Structure):
    """include/hps.h: hps_hrnet_fuse_args."""
    _fields_ = [("term", _P * 4), ("shift", _I * 4), ("pad", _I * 4), ("n_terms", _I), ("y", _P)] + [
        (n, _I) for n in ("opad", "B", "H", "W", "C", "relu")]


class HrnetOp(_c.Structure):
    """include/hps.h: hps_hrnet_op."""
    _fields_ = [("kind", _I), ("n_problems", _I), ("conv", C16Problem * 4), ("fuse", HrnetFuseArgs), ("x", _P), ("y", _P)] + [
        (n, _I) for n in ("B", "H", "W", "C", "P")]


FRONTEND_MAX_IMAGES, FRONTEND_RECORD_FLOATS = 64, 12
FRONTEND_SRC_HWC_U8, FRONTEND_SRC_CHW_F32 = 0, 1


class BoxImage(_c.Structure):
    """include/hps.h: hps_box_image."""
    _fields_ = [("boxes", _P), ("labels", _P), ("scores", _P), ("n", _I), ("H", _I), ("W", _I), ("reserved", _I)]


class PredictBoxesArgs(_c.Structure):
    """include/hps.h: hps_predict_boxes_args (struct_bytes = ctypes.sizeof(PredictBoxesArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "out_w", "out_h", "hrnet_aspect_fix")] + [
        ("threshold", _c.c_float), ("scale_factor", _c.c_float), ("records", _P), ("image", BoxImage * FRONTEND_MAX_IMAGES)]


class CropImage(_c.Structure):
    """include/hps.h: hps_crop_image."""
    _fields_ = [("src", _P), ("H", _I), ("W", _I), ("kind", _I), ("reserved", _I)]


class CropBilinearArgs(_c.Structure):
    """include/hps.h: hps_crop_bilinear_args (struct_bytes = ctypes.sizeof(CropBilinearArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "out_w", "out_h")] + [("mean", _c.c_float * 3), ("std", _c.c_float * 3)] + [
        (n, _P) for n in ("records", "raw", "normalised")] + [("image", CropImage * FRONTEND_MAX_IMAGES)]


class HrnetKeypointsArgs(_c.Structure):
    """include/hps.h: hps_hrnet_keypoints_args (struct_bytes = ctypes.sizeof(HrnetKeypointsArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "K", "h", "w")] + [("factor", _c.c_float), ("vis_threshold", _c.c_float),
                                                                          ("always_visible", _c.c_uint32)] + [
        (n, _P) for n in ("heatmaps", "records", "joints_hrnet", "confs", "joints_crop", "visib")]


class TextureGatherArgs(_c.Structure):
    """include/hps.h: hps_texture_gather_args (struct_bytes = ctypes.sizeof(TextureGatherArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "Ht", "Wt", "n_grey", "n_nongrey")] + [(n, _P) for n in ("grey", "nongrey", "out")] + [
        ("is_grey", _I * FRONTEND_MAX_IMAGES), ("idx", _I * FRONTEND_MAX_IMAGES)]


class U8Image(_c.Structure):
    """include/hps.h: hps_u8_image."""
    _fields_ = [("src", _P), ("H", _I), ("W", _I)]


class ResizeBilinearU8Args(_c.Structure):
    """include/hps.h: hps_resize_bilinear_u8_args (struct_bytes = ctypes.sizeof(ResizeBilinearU8Args))."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "out_w", "out_h")] + [("out", _P), ("image", U8Image * FRONTEND_MAX_IMAGES)]


class EvalCropImage(_c.Structure):
    """include/hps.h: hps_eval_crop_image."""
    _fields_ = [("rgb", _P), ("seg", _P), ("H", _I), ("W", _I), ("centre_v", _c.c_double), ("centre_h", _c.c_double), ("side", _c.c_double)]


class EvalCropU8Args(_c.Structure):
    """include/hps.h: hps_eval_crop_u8_args (struct_bytes = ctypes.sizeof(EvalCropU8Args))."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "out_wh", "K")] + [("scale_factor", _c.c_double)] + [
        (n, _P) for n in ("keypoints", "rgb", "seg", "joints", "positions")] + [("image", EvalCropImage * FRONTEND_MAX_IMAGES)]


class EvalHeatmapsArgs(_c.Structure):
    """include/hps.h: hps_eval_heatmaps_args (struct_bytes = ctypes.sizeof(EvalHeatmapsArgs))."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "K", "wh", "use_threshold")] + [("std", _c.c_float), ("always_visible", _c.c_uint32),
                                                                                       ("threshold", _c.c_double)] + [
        (n, _P) for n in ("positions", "keypoints", "out")]


DET_MAX_IMAGES, DET_MAX_ANCHORS, DET_MAX_LEVELS, DET_NMS_MAX_BOXES = 64, 8, 4, 2048


class DetImage(_c.Structure):
    """include/hps.h: hps_det_image."""
    _fields_ = [("src", _P), ("H", _I), ("W", _I), ("oh", _I), ("ow", _I)]


class DetTransformArgs(_c.Structure):
    """include/hps.h: hps_det_transform_args (struct_bytes = ctypes.sizeof(DetTransformArgs); the library rejects any other value)."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "FH", "FW", "P")] + [("mean", _c.c_float * 3), ("std", _c.c_float * 3), ("y", _P),
                                                                            ("image", DetImage * DET_MAX_IMAGES)]


class DetRpnDecodeArgs(_c.Structure):
    """include/hps.h: hps_det_rpn_decode_args."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "h", "w", "A", "k", "n_out", "out_offset")] + [
        (n, _c.c_float) for n in ("stride_h", "stride_w", "min_size")] + [("base", (_c.c_float * 4) * DET_MAX_ANCHORS)] + [
        (n, _P) for n in ("deltas", "index", "logits", "boxes", "scores")] + [("size", (_I * 2) * DET_MAX_IMAGES)]


class DetNmsArgs(_c.Structure):
    """include/hps.h: hps_det_nms_args."""
    _fields_ = [("struct_bytes", _I), ("G", _I), ("N", _I), ("thresh", _c.c_float)] + [(n, _P) for n in ("boxes", "order", "scores", "keep_scores")]


class DetLevel(_c.Structure):
    """include/hps.h: hps_det_level."""
    _fields_ = [("x", _P), ("h", _I), ("w", _I), ("pad", _I), ("scale", _c.c_float)]


class DetRoiAlignArgs(_c.Structure):
    """include/hps.h: hps_det_roi_align_args."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "R", "C", "bins", "n_levels")] + [("level", DetLevel * DET_MAX_LEVELS)] + [
        (n, _P) for n in ("boxes", "scores", "y")]


class DetBoxDecodeArgs(_c.Structure):
    """include/hps.h: hps_det_box_decode_args."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "R", "NC")] + [("score_thresh", _c.c_float), ("min_size", _c.c_float)] + [
        (n, _P) for n in ("logits", "deltas", "proposals", "prop_scores", "boxes", "scores", "probs")] + [("size", (_I * 2) * DET_MAX_IMAGES)]


class DetGatherArgs(_c.Structure):
    """include/hps.h: hps_det_gather_args."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "B", "D", "R", "NC")] + [
        (n, _P) for n in ("top_scores", "top_index", "order", "boxes", "out_boxes", "out_labels", "out_scores", "counts")] + [
        ("size", (_I * 4) * DET_MAX_IMAGES)]


DET_MASK_BINS, DET_MASK_CHANNELS, DET_MASK_SIZE = 14, 256, 28


class DetMaskPredictArgs(_c.Structure):
    """include/hps.h: hps_det_mask_predict_args."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "K", "NC")] + [
        (n, _P) for n in ("x", "wd", "bd", "wl", "bl", "labels", "scores", "probs", "logits")]


class DetPasteMasksArgs(_c.Structure):
    """include/hps.h: hps_det_paste_masks_args."""
    _fields_ = [(n, _I) for n in ("struct_bytes", "n", "H", "W", "binary")] + [("threshold", _c.c_float)] + [(n, _P) for n in ("probs", "boxes", "out")]


C16_MAX_PROBLEMS, HRNET_MAX_TERMS = 4, 4
HRNET_PACK, HRNET_CONV, HRNET_FUSE, HRNET_UNPACK = 0, 1, 2, 3
VIS_MAX_VIEWS, VIS_MAX_CELLS = 32, 32
VIS_PANEL_RENDER, VIS_PANEL_RENDER_OVER_CROP, VIS_PANEL_CROP, VIS_PANEL_PROXY = 0, 1, 2, 3
TRAIN_METRICS_NSLOT = 14
RENDER_PERSPECTIVE, RENDER_ORTHOGRAPHIC = 0, 1
ADAM_CHUNK = 4096
REFRESH_PERMUTE, REFRESH_FOLD, REFRESH_WINO_U, REFRESH_STEM_U = 0, 1, 2, 3
MF_REDUCTION_MEAN, MF_REDUCTION_SUM = 0, 1
ENC_RELAYOUT, ENC_CONV, ENC_MAXPOOL, ENC_AVGPOOL, ENC_CONV_WINOGRAD, ENC_STEM_SPLIT, ENC_STEM_WINOGRAD, ENC_RELAYOUT_GENERIC = 0, 1, 2, 3, 4, 5, 6, 7
ENC_STEM_WINOGRAD_POOLED, ENC_STEM_WINOGRAD_POOLED_NCHW, ENC_CONV_DOWN, ENC_EXPAND_DOWN = 8, 9, 10, 11
# op kind -> (entry point, the hps_enc_op fields that are its arguments in front of the stream): the switch of csrc/composite.hip
ENC_ENTRY = {kind: (entry, tuple(fields.split())) for kind, entry, fields in (
    (ENC_RELAYOUT, "hps_nchw_to_padded_nhwc", "x y B Cin H W opad"),
    (ENC_RELAYOUT_GENERIC, "hps_nchw_to_padded_nhwc_generic", "x y B Cin Cout H W KW opad"),
    (ENC_CONV, "hps_conv2d_bn_act_pad", "x w scale shift residual y B H W ipad Cin Cout KH KW stride pad opad relu row_mode variant ksplit splitk_ws"),
    (ENC_CONV_DOWN, "hps_conv2d_bn_act_pad_down", "x w scale shift y w_down scale_down shift_down y_down B H W ipad Cin Cout KH KW stride pad opad "
                                                  "relu variant ksplit splitk_ws"),
    (ENC_EXPAND_DOWN, "hps_bottleneck_expand_down", "x w scale shift x_down w_down scale_down shift_down y B H W stride ipad ipad_down opad Cin Cin_down "
                                                    "Cout variant ksplit"),
    (ENC_CONV_WINOGRAD, "hps_conv3x3_winograd", "x w scale shift residual y B H W ipad Cin Cout opad relu splitk_ws"),
    (ENC_STEM_SPLIT, "hps_stem_phase_split", "x y B Cin H W"),
    (ENC_STEM_WINOGRAD, "hps_stem_winograd", "x w scale shift y B H W opad relu"),
    (ENC_STEM_WINOGRAD_POOLED, "hps_stem_winograd_pooled", "x w scale shift y splitk_ws B H W opad relu"),
    (ENC_STEM_WINOGRAD_POOLED_NCHW, "hps_stem_winograd_pooled_nchw", "x w scale shift y splitk_ws B H W opad relu"),
    (ENC_MAXPOOL, "hps_maxpool3x3s2_pad", "x y B H W Cin opad"),
    (ENC_AVGPOOL, "hps_global_avgpool_pad", "x y B H W Cin ipad"))}
SVD_HOST, SVD_DEVICE, SVD_DEVICE_FMA = 0, 1, 2
SVD_ROUNDING_REFERENCE, SVD_ROUNDING_FMA = 0, 1
HEAD_WIDE_WORKGROUPS = 0x100


class HpsError(RuntimeError):
    pass


def _open(path, prototypes, what):
    if not os.path.exists(path):
        raise HpsError(
            "%s is missing (%s). Build it with `python -m hierarchicalprobabilistic3dhuman_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path." % (what, path))
    lib = ctypes.CDLL(path)
    for name, argtypes in prototypes.items():
        fn = getattr(lib, name)          # AttributeError if the build is stale: fail loudly
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, _I)
    # the head's host SVD uses the MKL sgesdd_ PyTorch itself links (same routine as the reference's torch.svd)
    torch_cpu = os.path.join(os.path.dirname(torch.__file__), "lib", "libtorch_cpu.so")
    if os.path.exists(torch_cpu):
        lib.hps_host_bind_lapack(torch_cpu.encode())
    return lib


def load(dev=False):
    """dlopen libhps.so (dev=True: libhps_dev.so) and attach prototypes; raises if the library has not been built."""
    global _lib, _dev_lib
    if dev:
        if _dev_lib is None:
            _dev_lib = _open(DEV_LIB_PATH, dict(_PROTOTYPES, **_dev_prototypes()), "libhps_dev.so")
        return _dev_lib
    if _lib is None:
        _lib = _open(LIB_PATH, _PROTOTYPES, "libhps.so")
    return _lib


def _dev_prototypes():
    """ctypes prototypes of the dev library's extra entry points (include/hps_dev.h).  They are test infrastructure and live on the
    tests' side of the tree -- tests/devlib.py, loaded here by path -- together with the helpers that call them; the package itself
    names no hps_dev_* symbol."""
    import importlib.util
    path = os.path.join(os.path.dirname(_PKG_DIR), "tests", "devlib.py")
    if not os.path.exists(path):
        raise HpsError("libhps_dev.so is test infrastructure: its prototypes live in tests/devlib.py, which is missing (%s)" % path)
    spec = importlib.util.spec_from_file_location("hps_tests_devlib_prototypes", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.DEV_PROTOTYPES


@contextlib.contextmanager
def dev_library():
    """Route every call inside the block to libhps_dev.so (tests and tests/dev only)."""
    global _use_dev
    prev, _use_dev = _use_dev, True
    try:
        yield load(dev=True)
    finally:
        _use_dev = prev


def require_device(t, what="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HpsError(
            "%s must live on a HIP (MI355X) device; this package has no CPU path "
            "(the CPU oracle under oracle/ is test infrastructure only)" % what)
    if t.device.index != torch.cuda.current_device():
        # kernels are launched on the CURRENT device's current stream (stream()): a tensor of another device would be
        # addressed from the wrong GPU.  The reference's `device` arguments become torch.cuda.set_device(device).
        raise HpsError("%s lives on cuda:%d but the current device is cuda:%d; call torch.cuda.set_device(%d) "
                       "(or use `with torch.cuda.device(...)`) before calling into libhps"
                       % (what, t.device.index, torch.cuda.current_device(), t.device.index))


def ptr(t, dtype=torch.float32, what="tensor"):
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    require_device(t, what)
    if t.dtype != dtype:
        raise HpsError("%s: expected %s, got %s" % (what, dtype, t.dtype))
    if not t.is_contiguous():
        raise HpsError("%s must be contiguous" % what)
    return _P(t.data_ptr())


def iptr(t, what="index tensor"):
    return ptr(t, torch.int32, what)


def stream():
    return _P(torch.cuda.current_stream().cuda_stream)


def cu_partition_stream(first_cu, num_cus):
    """torch stream restricted to CUs [first_cu, first_cu + num_cus) of every XCD (include/hps.h: hps_stream_create_cu_partition).
    The stream lives as long as the process (a handful are ever created: one pair per InferencePipeline)."""
    s = _P()
    call("hps_stream_create_cu_partition", int(first_cu), int(num_cus), _c.byref(s))
    if not _partition_streams:
        import atexit
        atexit.register(_destroy_partition_streams)
    _partition_streams.append(s.value)
    return torch.cuda.ExternalStream(s.value)


_partition_streams = []


def _destroy_partition_streams():
    """At interpreter exit: drain and destroy the CU-partition streams this process created (a tool that hooks the runtime's teardown --
    rocprofv3 -- otherwise finds live streams it never saw created by hipStreamCreate and crashes in its own finaliser)."""
    try:
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        lib = load()
        while _partition_streams:
            lib.hps_stream_destroy(_P(_partition_streams.pop()))
    except Exception:
        pass


_svd_flavor = None
_svd_flavor_exact = None


def svd_flavor():
    """Rounding flavour (include/hps.h: HPS_SVD_ROUNDING_*) of the in-kernel SVD that reproduces THIS host's LAPACK (the MKL
    sgesdd_ behind torch.svd) bit for bit -- calibrated once per process by hps_host_svd_flavor.  If neither flavour matches
    (another LAPACK build), the reference-BLAS rounding is used and a warning says so."""
    global _svd_flavor, _svd_flavor_exact
    if _svd_flavor is None:
        fl = load(dev=_use_dev).hps_host_svd_flavor()
        _svd_flavor_exact = fl in (SVD_ROUNDING_REFERENCE, SVD_ROUNDING_FMA)
        if not _svd_flavor_exact:
            import warnings
            warnings.warn("libhps: neither rounding flavour of the in-kernel 3x3 SVD reproduces this host's LAPACK sgesdd bit for "
                          "bit; using reference rounding (expect about one differently signed singular-vector pair in 10^4 "
                          "matrices relative to torch.svd on this host; svd_mode='host' is exact)")
            fl = SVD_ROUNDING_REFERENCE
        _svd_flavor = fl
    return _svd_flavor


def svd_flavor_is_exact():
    """True when the calibrated flavour reproduces this host's LAPACK bit for bit (the normal case with PyTorch's MKL)."""
    svd_flavor()
    return bool(_svd_flavor_exact)


def call(name, *args):
    lib = load(dev=_use_dev)
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.hps_last_error()
        raise HpsError("%s failed (code %d): %s" % (name, rc, msg.decode() if msg else ""))


def issue_enc_op(op):
    """One hps_enc_op through its own public entry point (ENC_ENTRY), on the current stream."""
    entry, fields = ENC_ENTRY[op.kind]
    call(entry, *[getattr(op, f) for f in fields], stream())


def run_enc_ops(ops, first, count, composite=True):
    """ops[first:first + count] of an EncOp array on the current stream: one hps_encoder_run call across the C ABI, or
    (``composite`` False, the cross-check of csrc/composite.hip's argument mapping) op by op through the public entry points."""
    if not composite:
        for i in range(first, first + count):
            issue_enc_op(ops[i])
    elif first == 0:
        call("hps_encoder_run", ops, count, stream())
    else:
        call("hps_encoder_run", _c.cast(_c.byref(ops, first * _c.sizeof(EncOp)), _c.POINTER(EncOp)), count, stream())


WS_CONV_SPLITK, WS_SMPL_MP, WS_SMPL_XT, WS_SMPL_A, WS_SMPL_VPOSED, WS_HEAD_F, WS_HEAD_USV = range(7)
WS_MF_LOSS = 8
WS_SMPL_LBS_BWD, WS_SMPL_BLEND_BWD = 9, 10
WS_HEAD_LEVELS_BWD, WS_HEAD_TRUNK_BWD = 11, 12
WS_SEG_BBOX = 13
WS_RENDER = 14
WS_SILHOUETTE = 15
WS_TRAIN_METRICS = 16
WS_PNG = 17
WS_JPEG = 18
WS_JPEG_ENC = 19


def jpeg_ws_dims(h):
    """include/hps.h: HPS_WS_JPEG_D1 / _D2 -- hps_query_workspace's three dimensions for a parsed header."""
    return (int(h.scan_length), int(h.width) + (int(h.height) << 32),
            int(h.ncomp) + (int(h.hs) << 8) + (int(h.vs) << 16) + (int(h.restart_interval) << 32))


def jpeg_enc_d2(C, sampling):
    """include/hps.h: HPS_WS_JPEG_ENC_D2 -- channels and sampling in hps_query_workspace's third dimension."""
    return int(C) + (int(sampling) << 8)


def silhouette_d2(num_faces, W):
    """include/hps.h: HPS_WS_SILHOUETTE_D2 -- the face count and the image side in hps_query_workspace's third dimension."""
    return int(num_faces) + (int(W) << 32)


def query_workspace(what, d0=0, d1=0, d2=0):
    """include/hps.h: hps_query_workspace -- bytes (HPS_WS_SMPL_MP: a count) of a caller-provided scratch buffer."""
    n = load(dev=_use_dev).hps_query_workspace(int(what), int(d0), int(d1), int(d2))
    if n < 0:
        raise HpsError("hps_query_workspace(%d, %d, %d, %d) failed" % (what, d0, d1, d2))
    return int(n)


def f32c(t):
    """fp32 contiguous view/copy on the same device."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()
