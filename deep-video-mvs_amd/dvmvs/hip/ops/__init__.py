"""``torch.library`` custom ops over the C ABI of ``libdvmvs_hip.so``.

Each op is a thin shim: check device/dtype, make inputs contiguous, allocate the output with torch, pass raw device
pointers and the current HIP stream to the ``extern "C"`` launcher.  No op synchronises or touches the host, so a
whole frame can be captured into a hipGraph (``torch.cuda.graph``).  Tensors that are not on the GPU are rejected:
the CPU restatement lives in ``oracle/`` and is test infrastructure only.

The ops live in one module per family (``sweep``, ``frame``, ``baselines``, ``reconstruction``) over the shared plumbing of ``_common``
(checks, pointers, the launch, the registration) and ``_workspace`` (the persistent device buffers).  Importing this package imports
them all, which registers every ``torch.ops.dvmvs`` op, and every public name is available here.
"""
# the names the single-module form of this package exposed next to its own; kept so that ``ops.<name>`` means what it did
import ctypes  # noqa: F401
import os  # noqa: F401
from typing import Optional, Sequence, Tuple  # noqa: F401

import numpy as np  # noqa: F401
import torch  # noqa: F401
from torch import Tensor  # noqa: F401

from dvmvs.hip.ops import baselines, frame, reconstruction, sweep  # noqa: F401
from dvmvs.hip.ops._common import EUNSUPPORTED  # noqa: F401
from dvmvs.hip.ops.baselines import dps_regress, dps_volume, gp_filter_step, rgb_sweep  # noqa: F401
from dvmvs.hip.ops.frame import (ACTIVATION_SIGMOID_TO_DEPTH, ACTIVATIONS, RESIDUAL_NEAREST_UP2, RESIDUAL_NONE, RESIDUAL_SAME, batchable,  # noqa: F401
                                 bias_act_, bias_act_into, bottleneck_conv_into, bottleneck_conv_pack, bottleneck_conv_splits,
                                 conv_bias_act_into, conv_head_into, copy_batch, depth_reproject, depth_reproject_estimate_into,
                                 depth_reproject_lowres, depth_reproject_lowres_into, depthwise_conv, depthwise_conv_bwd, depthwise_conv_train,
                                 direct_conv_into, direct_conv_pack, direct_conv_shape, direct_conv_tile, hidden_warp, hidden_warp_into, lstm_gates, lstm_gates_into,
                                 lstm_gates_partials_into, partial_sums_bias_act_into, pointwise_conv_into, pointwise_conv_pack,
                                 pointwise_conv_supported, upsample2x, upsample2x_bwd, upsample2x_into, upsample2x_pair_into)
from dvmvs.hip.ops.reconstruction import (CONSISTENCY_MAX_SOURCES, TSDF_FUSE_TILE, consistency_matrices, depth_consistency, depth_errors,  # noqa: F401
                                          depth_errors_workspace, distance_metrics, nearest_build, nearest_distance,
                                          nearest_distance_workspace, nearest_grid_header, nearest_query, preprocess_depth, preprocess_rgb,
                                          tsdf_fuse_tile_count, tsdf_integrate_frames, tsdf_integrate_frames_workspace, tsdf_raycast,
                                          tsdf_raycast_mask)
# COST_VOLUME_TWO_PASS here is the value at import; the switch the sweep reads at call time is ``sweep.COST_VOLUME_TWO_PASS``
from dvmvs.hip.ops.sweep import (COST_VOLUME_TWO_PASS, cost_volume, cost_volume_into, drop_sweep_workspace, nchw_to_nhwc_into, relative_pose,  # noqa: F401
                                 sweep_matrices, sweep_plan_host, sweep_work_list_host, sweep_work_list_words, sweep_workspace)

__all__ = ["cost_volume", "sweep_matrices", "hidden_warp", "relative_pose", "lstm_gates", "depth_reproject", "depth_reproject_lowres",
           "bias_act_", "upsample2x", "depthwise_conv", "rgb_sweep", "gp_filter_step", "dps_volume", "dps_regress", "preprocess_rgb",
           "preprocess_depth", "depth_errors", "tsdf_raycast", "tsdf_raycast_mask", "tsdf_integrate_frames", "nearest_distance", "nearest_build",
           "nearest_query", "distance_metrics", "consistency_matrices", "depth_consistency"]


# The listing of this package (``dir``, ``__all__``) is recorded in tests/golden/ops_surface.json and held fixed.  Ops added after that
# record are defined and listed in their family module and are served from here by name, so ``ops.surface_sample(...)`` and
# ``from dvmvs.hip.ops import voxel_downsample`` work like every other op.
_LATER_OPS = {"surface_sample": reconstruction, "voxel_downsample": reconstruction, "mesh_raster": reconstruction,
              "mesh_raster_workspace": reconstruction, "mesh_visibility": reconstruction}


def __getattr__(name):
    if name in _LATER_OPS:
        return getattr(_LATER_OPS[name], name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
