"""ctypes binding of ``libdvmvs_hip.so`` (the C ABI declared in ``include/dvmvs_hip.h``).

The library is the only implementation of the hot path: there is no CPU or eager-PyTorch fallback.  If it has not
been built (``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C deep-video-mvs_amd/csrc``) every op
raises ``RuntimeError`` on first use.
"""
import ctypes
import os
import threading

# PyTorch-ROCm ships its own libamdhip64.so.  It must be in the process BEFORE libdvmvs_hip.so is dlopen'ed so that the
# library's DT_NEEDED libamdhip64.so.7 resolves to that already-loaded copy: two HIP runtimes in one process do not
# share streams or device memory (symptom: "no ROCm-capable device is detected" from the second one).  The same holds for
# libMIOpen.so.1 (dvmvs_conv_bias_act_fwd): the process has ONE MIOpen, the one torch's convolutions use.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DVMVS_HIP_LIB", os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libdvmvs_hip.so")))

ABI_VERSION = 11
MAX_MEASUREMENTS = 8
MAX_DEPTH_LEVELS = 256
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1

_c_fp = ctypes.c_void_p          # device pointer to float
_c_fpp = ctypes.POINTER(ctypes.c_void_p)  # host array of device pointers
_c_int = ctypes.c_int
_c_dbl = ctypes.c_double
_c_stream = ctypes.c_void_p
_c_f3 = ctypes.POINTER(ctypes.c_float)    # host array of floats

# name -> (restype, argtypes); must list every symbol the header declares (checked by tests/test_capi_symbols.py)
SIGNATURES = {
    "dvmvs_abi_version": (_c_int, []),
    "dvmvs_build_arch": (ctypes.c_char_p, []),
    "dvmvs_error_string": (ctypes.c_char_p, [_c_int]),
    "dvmvs_trace_marker": (_c_int, [_c_stream]),
    "dvmvs_host_pointer_device_visible": (_c_int, [ctypes.c_void_p]),
    "dvmvs_cost_volume_workspace_bytes": (ctypes.c_size_t, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "dvmvs_sweep_matrices": (_c_int, [_c_fp, _c_fpp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_stream]),
    "dvmvs_cost_volume_fwd": (_c_int, [_c_fp, _c_fpp, _c_fp, _c_fp, _c_fp,
                                       _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                       _c_dbl, _c_dbl, _c_int, _c_int, _c_int, _c_fp, ctypes.c_size_t, _c_stream]),
    "dvmvs_sweep_plan_stats": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dbl, _c_dbl, _c_int,
                                        ctypes.POINTER(ctypes.c_longlong)]),
    "dvmvs_sweep_select_variant": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dbl, _c_dbl]),
    "dvmvs_sweep_work_list_bytes": (ctypes.c_size_t, [_c_int, _c_int, _c_int, _c_int]),
    "dvmvs_sweep_work_list": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dbl, _c_dbl, _c_int, _c_fp, ctypes.c_size_t]),
    "dvmvs_sweep_plan": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dbl, _c_dbl, _c_int, _c_fp, ctypes.c_size_t]),
    "dvmvs_sweep_plan6": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dbl, _c_dbl, _c_fp, ctypes.c_size_t]),
    "dvmvs_nchw_to_nhwc": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_copy_batch": (_c_int, [_c_fpp, _c_fpp, ctypes.POINTER(ctypes.c_longlong), _c_int, _c_stream]),
    "dvmvs_sweep_mfma_estimate": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dbl, _c_dbl, ctypes.POINTER(ctypes.c_double)]),
    "dvmvs_cost_volume_planned_fwd": (_c_int, [_c_fp, _c_fpp, _c_fp, _c_fp, _c_fp,
                                               _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                               _c_dbl, _c_dbl, _c_int, _c_int, _c_int, _c_fp, ctypes.c_size_t, _c_fp, _c_stream]),
    "dvmvs_cost_volume_bwd": (_c_int, [_c_fp, _c_fp, _c_fpp, _c_fp, _c_fp, _c_fp, _c_fpp,
                                       _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                       _c_dbl, _c_dbl, _c_stream]),
    "dvmvs_hidden_warp_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_hidden_warp_bwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_relative_pose": (_c_int, [_c_fp, _c_fp, _c_fp, _c_int, _c_stream]),
    "dvmvs_lstm_gates_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_lstm_gates_bwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_lstm_gates_partials_fwd": (_c_int, [_c_fp, _c_int, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_bottleneck_conv_packed_bytes": (ctypes.c_size_t, [_c_int, _c_int]),
    "dvmvs_bottleneck_conv_pack": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_stream]),
    "dvmvs_bottleneck_conv_splits": (_c_int, [_c_int] * 6),
    "dvmvs_bottleneck_conv_fwd": (_c_int, [_c_fp, _c_fp, _c_fp] + [_c_int] * 6 + [_c_stream]),
    "dvmvs_bottleneck_conv_up2x_fwd": (_c_int, [_c_fp, _c_fp, _c_fp] + [_c_int] * 5 + [_c_stream]),
    "dvmvs_direct_conv_tile": (_c_int, [_c_int] * 7),
    "dvmvs_direct_conv_shape": (_c_int, [_c_int] * 7),
    "dvmvs_direct_conv_packed_bytes": (ctypes.c_size_t, [_c_int] * 4),
    "dvmvs_direct_conv_pack": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_direct_conv_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, _c_int, _c_fp, _c_fp, ctypes.c_longlong] + [_c_int] * 8 + [_c_stream]),
    "dvmvs_direct_conv_dual_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, _c_int, _c_fp, _c_fp, ctypes.c_longlong, _c_fp] + [_c_int] * 8 + [_c_stream]),
    "dvmvs_pointwise_conv_supported": (_c_int, [_c_int] * 7),
    "dvmvs_pointwise_conv_packed_bytes": (ctypes.c_size_t, [_c_int] * 2),
    "dvmvs_pointwise_conv_pack": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_stream]),
    "dvmvs_pointwise_conv_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, _c_int, _c_fp, ctypes.c_longlong] + [_c_int] * 7 + [_c_stream]),
    "dvmvs_conv_head_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, ctypes.c_longlong] + [_c_int] * 5 + [ctypes.c_float, ctypes.c_float, _c_stream]),
    "dvmvs_partial_sums_bias_act_fwd": (_c_int, [_c_fp, _c_int, _c_fp, ctypes.c_longlong, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_depth_reproject_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int,
                                           _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_bias_act_fwd": (_c_int, [_c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                    ctypes.c_float, ctypes.c_float, _c_stream]),
    "dvmvs_bias_act_inplace": (_c_int, [_c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_conv_bias_act_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong] + [_c_int] * 9 + [_c_stream]),
    "dvmvs_upsample2x_fwd": (_c_int, [_c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_upsample2x_pair_fwd": (_c_int, [_c_fp, _c_fp, ctypes.c_longlong, _c_int, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_upsample2x_bwd": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_depthwise_conv_bwd_workspace_bytes": (ctypes.c_size_t, [_c_int] * 6),
    "dvmvs_depthwise_conv_bwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_depth_reproject_lowres_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_depth_reproject_estimate_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_tsdf_integrate": (_c_int, [_c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                      ctypes.c_float, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, ctypes.c_float, ctypes.c_float, _c_stream]),
    "dvmvs_marching_cubes_workspace_bytes": (ctypes.c_size_t, [_c_int, _c_int, _c_int]),
    "dvmvs_marching_cubes_count": (_c_int, [_c_fp, _c_int, _c_int, _c_int, ctypes.c_float, _c_fp, ctypes.c_size_t, _c_fp, _c_stream]),
    "dvmvs_marching_cubes_emit": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                           ctypes.c_float, ctypes.c_float, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong,
                                           ctypes.c_longlong, _c_stream]),
    "dvmvs_depthwise_conv_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                          _c_stream]),
    "dvmvs_rgb_sweep_fwd": (_c_int, [_c_fp, _c_fpp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                     _c_dbl, _c_dbl, _c_int, _c_int, _c_int, _c_stream]),
    "dvmvs_gp_filter_step": (_c_int, [_c_fp, _c_fp, _c_fp, _c_int, _c_dbl, _c_dbl, _c_dbl, _c_dbl, _c_dbl, _c_dbl, _c_int, _c_stream]),
    "dvmvs_dps_volume_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dbl, _c_stream]),
    "dvmvs_dps_regress_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dbl, _c_stream]),
    "dvmvs_preprocess_rgb_fwd": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_longlong, _c_int, _c_int, _c_int, _c_int,
                                          ctypes.c_longlong, _c_dbl, _c_f3, _c_f3, _c_int, _c_stream]),
    "dvmvs_preprocess_depth_fwd": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dbl, _c_stream]),
    "dvmvs_depth_errors_workspace_bytes": (ctypes.c_size_t, [_c_int, ctypes.c_longlong]),
    "dvmvs_depth_errors_fwd": (_c_int, [_c_fp, _c_fp, _c_int, ctypes.c_longlong, ctypes.c_float, _c_fp, _c_fp, _c_fp, _c_stream]),
    "dvmvs_tsdf_raycast_mask_bytes": (ctypes.c_size_t, [_c_int, _c_int, _c_int]),
    "dvmvs_tsdf_raycast_mask": (_c_int, [_c_fp, _c_fp, _c_int, _c_int, _c_int, _c_fp, _c_stream]),
    "dvmvs_tsdf_raycast_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_float, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_float, _c_fp, _c_fp, _c_fp, _c_stream]),
    "dvmvs_tsdf_integrate_frames_workspace_bytes": (ctypes.c_size_t, [_c_int]),
    "dvmvs_tsdf_integrate_frames": (_c_int, [_c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                             ctypes.c_float, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float,
                                             _c_f3, ctypes.c_float, _c_fp, _c_fp, _c_stream]),
    "dvmvs_nearest_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong]),
    "dvmvs_nearest_query_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_longlong]),
    "dvmvs_nearest_build": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_size_t, _c_stream]),
    "dvmvs_nearest_distance_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, ctypes.c_size_t, _c_fp, _c_fp,
                                            _c_stream]),
    "dvmvs_distance_metrics_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, ctypes.c_float, _c_fp, _c_fp, _c_stream]),
    "dvmvs_consistency_matrices": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_stream]),
    "dvmvs_depth_consistency_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int,
                                             ctypes.c_float, ctypes.c_float, _c_int, _c_int, _c_stream]),
    "dvmvs_surface_sample_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong]),
    "dvmvs_surface_sample_count": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_dbl, _c_fp, ctypes.c_size_t, _c_fp, _c_stream]),
    "dvmvs_surface_sample_emit": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_dbl, ctypes.c_uint, _c_fp, ctypes.c_longlong,
                                           _c_fp, _c_fp, _c_stream]),
    "dvmvs_voxel_downsample_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong]),
    "dvmvs_voxel_keys": (_c_int, [_c_fp, ctypes.c_longlong, ctypes.c_float, _c_fp, ctypes.c_size_t, _c_fp, _c_stream]),
    "dvmvs_voxel_downsample_count": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, ctypes.c_size_t, _c_fp, _c_stream]),
    "dvmvs_voxel_downsample_emit": (_c_int, [ctypes.c_longlong, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, _c_stream]),
    "dvmvs_mesh_raster_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong] * 4),
    "dvmvs_mesh_raster_cameras": (_c_int, [_c_fp, _c_fp, _c_int, _c_stream]),
    "dvmvs_mesh_raster_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float,
                                       ctypes.c_float, _c_int, _c_int, _c_fp, ctypes.c_size_t, _c_fp, _c_fp, _c_fp, _c_stream]),
    "dvmvs_mesh_visibility_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float,
                                           ctypes.c_float, _c_fp, _c_stream]),
    "dvmvs_icp_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong, _c_int]),
    "dvmvs_icp_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, ctypes.c_size_t, ctypes.c_float, _c_int, _c_int,
                               _c_dbl, ctypes.POINTER(ctypes.c_double), _c_fp, ctypes.c_size_t, _c_stream]),
    "dvmvs_transform_points_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_stream]),
    "dvmvs_mesh_components_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_longlong]),
    "dvmvs_mesh_components_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, ctypes.c_size_t, _c_fp, _c_fp, _c_fp, _c_fp,
                                           _c_fp, _c_stream]),
    "dvmvs_mesh_filter_count": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                                         ctypes.c_longlong, _c_int, _c_fp, ctypes.c_size_t, _c_fp, _c_stream]),
    "dvmvs_mesh_filter_emit": (_c_int, [_c_fp] * 8 + [ctypes.c_longlong] * 4 + [_c_int, _c_fp, ctypes.c_size_t, ctypes.c_longlong,
                                                                                ctypes.c_longlong] + [_c_fp] * 6 + [_c_stream]),
    "dvmvs_knn_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, ctypes.c_size_t, _c_int, ctypes.c_float, _c_int,
                               _c_fp, _c_fp, _c_stream]),
    "dvmvs_radius_count_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, ctypes.c_size_t, ctypes.c_float, _c_int,
                                        _c_int, _c_fp, _c_stream]),
    "dvmvs_outlier_statistics_fwd": (_c_int, [_c_fp, _c_fp, ctypes.c_longlong, _c_int, _c_dbl, _c_fp, _c_fp, _c_fp, _c_stream]),
    "dvmvs_point_normals_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_int, _c_fp, ctypes.c_longlong, _c_fp,
                                         _c_fp, _c_fp, _c_fp, _c_stream]),
    "dvmvs_icp_plane_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong, _c_int]),
    "dvmvs_icp_plane_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, ctypes.c_size_t, ctypes.c_float,
                                     _c_int, _c_dbl, ctypes.POINTER(ctypes.c_double), _c_fp, ctypes.c_size_t, _c_stream]),
    "dvmvs_implicit_band_fwd": (_c_int, [_c_fp, ctypes.c_longlong] + [ctypes.c_float] * 4 + [_c_int] * 3 + [ctypes.c_float, _c_fp, _c_stream]),
    "dvmvs_implicit_nodes_fwd": (_c_int, [_c_fp, ctypes.c_longlong] + [ctypes.c_float] * 4 + [_c_int] * 3 + [_c_fp, _c_stream]),
    "dvmvs_implicit_values_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_int, ctypes.c_float, _c_int,
                                           _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_stream]),
    "dvmvs_implicit_trim_fwd": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_int, _c_int, _c_int, _c_fp, _c_fp,
                                         _c_stream]),
    "dvmvs_mesh_simplify_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_longlong]),
    "dvmvs_voxel_downsample_runs": (_c_int, [ctypes.c_longlong, _c_fp, _c_fpp, _c_fpp]),
    "dvmvs_mesh_simplify_keys": (_c_int, [_c_fp, ctypes.c_longlong, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_size_t, _c_fp, _c_fp,
                                          _c_fp, _c_stream]),
    "dvmvs_mesh_simplify_pair_keys": (_c_int, [_c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_stream]),
    "dvmvs_mesh_simplify_count": (_c_int, [_c_fp, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_dbl, _c_int] + [_c_fp] * 10
                                  + [ctypes.c_size_t, _c_fp, _c_stream]),
    "dvmvs_mesh_simplify_emit": (_c_int, [ctypes.c_longlong, ctypes.c_longlong, _c_fp, ctypes.c_size_t, ctypes.c_longlong, ctypes.c_longlong]
                                 + [_c_fp] * 6 + [_c_stream]),
    "dvmvs_mesh_smooth_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_longlong]),
    "dvmvs_mesh_smooth_keys": (_c_int, [_c_fp, ctypes.c_longlong, ctypes.c_longlong, _c_fp, _c_fp, _c_stream]),
    "dvmvs_mesh_smooth_rows": (_c_int, [_c_fp, ctypes.c_longlong, ctypes.c_longlong, _c_fp, ctypes.c_size_t, _c_stream]),
    "dvmvs_mesh_smooth_rows_export": (_c_int, [ctypes.c_longlong, ctypes.c_longlong, _c_fp, ctypes.c_size_t, _c_fp, _c_fp, _c_fp, _c_stream]),
    "dvmvs_mesh_smooth_steps": (_c_int, [_c_fp, ctypes.c_longlong, ctypes.c_longlong, _c_int, _c_int, _c_dbl, _c_dbl, _c_int, _c_int, _c_fp,
                                         ctypes.c_size_t, _c_fp, _c_stream]),
    "dvmvs_mesh_smooth_normals": (_c_int, [_c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_size_t,
                                           _c_fp, _c_stream]),
    "dvmvs_sparse_mark": (_c_int, [_c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float,
                                   ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _c_int, _c_stream]),
    "dvmvs_sparse_assign": (_c_int, [_c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, _c_stream]),
    "dvmvs_sparse_integrate": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_float, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float, _c_f3,
                                        ctypes.c_float, _c_int, _c_stream]),
    "dvmvs_sparse_gather": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                     _c_int, _c_stream]),
    "dvmvs_sparse_neighbours": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_stream]),
    "dvmvs_sparse_extract_count": (_c_int, [_c_fp, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_stream]),
    "dvmvs_sparse_extract_scan": (_c_int, [_c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_stream]),
    "dvmvs_sparse_extract_emit": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                           ctypes.c_float, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, ctypes.c_longlong, _c_stream]),
    "dvmvs_sparse_raycast_index": (_c_int, [_c_fp, _c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_stream]),
    "dvmvs_sparse_raycast_flags": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_stream]),
    "dvmvs_sparse_raycast_fwd": (_c_int, [_c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_int, _c_int,
                                          _c_int, _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _c_int,
                                          _c_fp, _c_fp, _c_int, _c_int, _c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, _c_fp, _c_fp,
                                          _c_fp, _c_stream]),
}

# Added to the header without a new ABI number (the number is pinned at 11): a library built before the addition passes the version
# check below and only lacks these symbols, so their absence is reported as what it is.
ADDED_WITHIN_ABI = ("dvmvs_preprocess_rgb_fwd", "dvmvs_preprocess_depth_fwd")
# ... and the second addition under the same number (depth evaluation), checked the same way
ADDED_WITHIN_ABI_DEPTH_ERRORS = ("dvmvs_depth_errors_workspace_bytes", "dvmvs_depth_errors_fwd")
# ... and the third (ray-casting a TSDF volume)
ADDED_WITHIN_ABI_TSDF_RAYCAST = ("dvmvs_tsdf_raycast_mask_bytes", "dvmvs_tsdf_raycast_mask", "dvmvs_tsdf_raycast_fwd")
# ... and the fourth (fusing a batch of frames into a TSDF volume)
ADDED_WITHIN_ABI_TSDF_FUSE = ("dvmvs_tsdf_integrate_frames_workspace_bytes", "dvmvs_tsdf_integrate_frames")
# ... and the fifth (nearest-point distances between point clouds and the 3-D reconstruction metrics)
ADDED_WITHIN_ABI_NEAREST = ("dvmvs_nearest_workspace_bytes", "dvmvs_nearest_query_workspace_bytes", "dvmvs_nearest_build",
                            "dvmvs_nearest_distance_fwd", "dvmvs_distance_metrics_fwd")
# ... and the sixth (filtering depth maps by multi-view geometric consistency)
ADDED_WITHIN_ABI_CONSISTENCY = ("dvmvs_consistency_matrices", "dvmvs_depth_consistency_fwd")
# ... and the seventh (point sets for the 3-D metrics: surface sampling and voxel down-sampling)
ADDED_WITHIN_ABI_SURFACE_SAMPLE = ("dvmvs_surface_sample_workspace_bytes", "dvmvs_surface_sample_count", "dvmvs_surface_sample_emit",
                                   "dvmvs_voxel_downsample_workspace_bytes", "dvmvs_voxel_keys", "dvmvs_voxel_downsample_count",
                                   "dvmvs_voxel_downsample_emit")
# ... and the eighth (rasterising a triangle mesh to depth maps; vertex visibility)
ADDED_WITHIN_ABI_MESH_RASTER = ("dvmvs_mesh_raster_workspace_bytes", "dvmvs_mesh_raster_cameras", "dvmvs_mesh_raster_fwd",
                                "dvmvs_mesh_visibility_fwd")
# ... and the ninth (registering a point cloud to another by trimmed ICP)
ADDED_WITHIN_ABI_REGISTRATION = ("dvmvs_icp_workspace_bytes", "dvmvs_icp_fwd", "dvmvs_transform_points_fwd")
# ... and the tenth (which workgroup shape of the direct convolution a problem runs with)
ADDED_WITHIN_ABI_DIRECT_CONV_SHAPE = ("dvmvs_direct_conv_shape",)
# ... and the eleventh (connected components of a triangle mesh and their removal by size)
ADDED_WITHIN_ABI_MESH_COMPONENTS = ("dvmvs_mesh_components_workspace_bytes", "dvmvs_mesh_components_fwd", "dvmvs_mesh_filter_count",
                                    "dvmvs_mesh_filter_emit")
# ... and the twelfth (the k nearest neighbours of points, neighbours within a radius, statistical outlier scores)
ADDED_WITHIN_ABI_POINT_NEIGHBOURS = ("dvmvs_knn_fwd", "dvmvs_radius_count_fwd", "dvmvs_outlier_statistics_fwd")
# ... and the thirteenth (oriented normals of points from rows of nearest neighbours)
ADDED_WITHIN_ABI_POINT_NORMALS = ("dvmvs_point_normals_fwd",)
# ... and the fourteenth (registering a point cloud to another with normals by point-to-plane ICP)
ADDED_WITHIN_ABI_REGISTRATION_PLANE = ("dvmvs_icp_plane_workspace_bytes", "dvmvs_icp_plane_fwd")
# ... and the fifteenth (the implicit signed distance of an oriented point cloud on a voxel grid, and the trimming of its mesh)
ADDED_WITHIN_ABI_IMPLICIT = ("dvmvs_implicit_band_fwd", "dvmvs_implicit_nodes_fwd", "dvmvs_implicit_values_fwd", "dvmvs_implicit_trim_fwd")
# ... and the sixteenth (simplifying a triangle mesh by vertex clustering with quadric error representatives)
ADDED_WITHIN_ABI_MESH_SIMPLIFY = ("dvmvs_mesh_simplify_workspace_bytes", "dvmvs_voxel_downsample_runs", "dvmvs_mesh_simplify_keys",
                                  "dvmvs_mesh_simplify_pair_keys", "dvmvs_mesh_simplify_count", "dvmvs_mesh_simplify_emit")
# ... and the seventeenth (smoothing a triangle mesh by the Laplacian and Taubin filters; vertex normals from the faces)
ADDED_WITHIN_ABI_MESH_SMOOTH = ("dvmvs_mesh_smooth_workspace_bytes", "dvmvs_mesh_smooth_keys", "dvmvs_mesh_smooth_rows",
                                "dvmvs_mesh_smooth_rows_export", "dvmvs_mesh_smooth_steps", "dvmvs_mesh_smooth_normals")
# ... and the eighteenth (a TSDF volume without bounds: a hash table of bricks over a pool)
ADDED_WITHIN_ABI_SPARSE_VOLUME = ("dvmvs_sparse_mark", "dvmvs_sparse_assign", "dvmvs_sparse_integrate", "dvmvs_sparse_gather")
# ... and the nineteenth (marching cubes straight from the pool of the sparse volume)
ADDED_WITHIN_ABI_SPARSE_EXTRACT = ("dvmvs_sparse_neighbours", "dvmvs_sparse_extract_count", "dvmvs_sparse_extract_scan",
                                   "dvmvs_sparse_extract_emit")
# ... and the twentieth (ray-casting the sparse volume straight from its pool)
ADDED_WITHIN_ABI_SPARSE_RAYCAST = ("dvmvs_sparse_raycast_index", "dvmvs_sparse_raycast_flags", "dvmvs_sparse_raycast_fwd")

_lib = None
_lock = threading.Lock()


def lib():
    """Loads the shared library once; raises RuntimeError (never falls back) when it is missing or stale."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"dvmvs HIP library not found at {LIB_PATH}. Build it with `make -C deep-video-mvs_amd/csrc` "
                f"(or __graft_entry__.build()). The plane-sweep ops have no CPU / eager fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        added = (ADDED_WITHIN_ABI + ADDED_WITHIN_ABI_DEPTH_ERRORS + ADDED_WITHIN_ABI_TSDF_RAYCAST + ADDED_WITHIN_ABI_TSDF_FUSE
                 + ADDED_WITHIN_ABI_NEAREST + ADDED_WITHIN_ABI_CONSISTENCY + ADDED_WITHIN_ABI_SURFACE_SAMPLE + ADDED_WITHIN_ABI_MESH_RASTER
                 + ADDED_WITHIN_ABI_REGISTRATION + ADDED_WITHIN_ABI_DIRECT_CONV_SHAPE + ADDED_WITHIN_ABI_MESH_COMPONENTS
                 + ADDED_WITHIN_ABI_POINT_NEIGHBOURS + ADDED_WITHIN_ABI_POINT_NORMALS + ADDED_WITHIN_ABI_REGISTRATION_PLANE
                 + ADDED_WITHIN_ABI_IMPLICIT + ADDED_WITHIN_ABI_MESH_SIMPLIFY + ADDED_WITHIN_ABI_MESH_SMOOTH + ADDED_WITHIN_ABI_SPARSE_VOLUME
                 + ADDED_WITHIN_ABI_SPARSE_EXTRACT + ADDED_WITHIN_ABI_SPARSE_RAYCAST)
        missing = [name for name in added if not hasattr(handle, name)]
        if missing:
            raise RuntimeError(f"{LIB_PATH} was built before {', '.join(missing)} joined ABI {ABI_VERSION} (the number did not change); "
                               f"rebuild it with `make -C deep-video-mvs_amd/csrc` (or __graft_entry__.build())")
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here = header/library mismatch: let it propagate loudly
            fn.restype = restype
            fn.argtypes = argtypes
        got = handle.dvmvs_abi_version()
        if got != ABI_VERSION:
            raise RuntimeError(f"libdvmvs_hip.so ABI {got} does not match the Python binding ({ABI_VERSION}); rebuild")
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().dvmvs_error_string(code).decode()
        raise RuntimeError(f"{what} failed with code {code}: {msg}")


def float_array(values):
    """Host array of floats (``const float* ..._host`` in the header)."""
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def pointer_array(ptrs):
    """Host array of device pointers (``const float* const*`` in the header)."""
    arr = (ctypes.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr
