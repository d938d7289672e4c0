"""Multi-view geometric consistency of depth maps: the step between "depth maps" and "fusion" of a multi-view-stereo pipeline.

Each depth map is checked against the depth maps of neighbouring views and only the pixels that several views agree on are kept
(``filter_depths``); the survivors of all views together are the "fused point cloud" of an MVS system (``fused_point_cloud``).  The check
is one HIP launch for all frames (``dvmvs.hip.ops.depth_consistency``, csrc/depth_consistency.hip); its definition, operation by
operation, is in include/dvmvs_hip.h.  GPU only, like the rest of the package.
"""
import numpy as np
import torch


def nearest_sources(n, count, segments=None):
    """Host table int32 [n, count]: for frame i the ``count`` other frames nearest in sequence order (distance 1 first, then 2, ...; at
    equal distance the lower index first), never across a segment boundary, padded with -1.  ``segments``: a sequence of n segment ids
    (frames with the same id belong together, e.g. the stretches between two "TRACKING LOST" lines) or None for one segment."""
    n, count = int(n), int(count)
    if n < 0 or count < 0:
        raise ValueError(f"nearest_sources: n and count must not be negative, got {n} and {count}")
    if segments is not None and len(segments) != n:
        raise ValueError(f"nearest_sources: {len(segments)} segment ids for {n} frames")
    table = np.full((n, count), -1, dtype=np.int32)
    for i in range(n):
        k = 0
        for distance in range(1, n):
            for j in (i - distance, i + distance):
                if k < count and 0 <= j < n and (segments is None or segments[j] == segments[i]):
                    table[i, k] = j
                    k += 1
    return table


def _device_f32(a, device):
    if torch.is_tensor(a):
        return a.to(device, torch.float32).contiguous()
    return torch.as_tensor(np.array(a, dtype=np.float32), device=device)      # (a copy: the caller's array may be read-only)


def filter_depths(depths, K, poses, sources=None, n_sources=4, pixel_threshold=1.0, relative_threshold=0.01, min_views=2, average=True,
                  with_count=True, with_points=False, device="cuda"):
    """``dvmvs.hip.ops.depth_consistency`` with conveniences: ``depths`` [N,H,W], ``K`` [N,3,3] or one [3,3] for all frames and
    camera-to-world ``poses`` [N,4,4] may be numpy arrays or tensors (device tensors of the kernel's types are used in place; ``device``
    is where host data goes); ``sources`` int [N,S] (S <= 16) defaults to ``nearest_sources(N, n_sources)``.  Returns the op's device
    tensors ``(depth, count or None, points or None)``."""
    from dvmvs.hip import ops
    if torch.is_tensor(depths) and depths.device.type != "cpu":
        device = depths.device
    depths = _device_f32(depths, device)
    if depths.dim() != 3:
        raise ValueError(f"filter_depths: depths must be [N,H,W], got {tuple(depths.shape)}")
    n = int(depths.shape[0])
    K, poses = _device_f32(K, depths.device), _device_f32(poses, depths.device)
    if K.dim() == 2:
        K = K.unsqueeze(0).expand(n, 3, 3).contiguous()
    if sources is None:
        sources = nearest_sources(n, n_sources)
    if torch.is_tensor(sources):
        sources = sources.to(depths.device, torch.int32)
    else:
        sources = torch.as_tensor(np.ascontiguousarray(sources, dtype=np.int32), device=depths.device)
    return ops.depth_consistency(depths, K, poses, sources, pixel_threshold=pixel_threshold, relative_threshold=relative_threshold,
                                 min_views=min_views, average=average, with_count=with_count, with_points=with_points)


def fused_point_cloud(depth, points, colours=None):
    """The surviving pixels of ``filter_depths(..., with_points=True)`` as one cloud: ``depth`` [N,H,W] and ``points`` [N,H,W,3] device
    tensors -> float32 [P,3], frame-major then row-major; with ``colours`` ([N,H,W,3], uint8 or float, numpy or tensor) float32 [P,6]
    xyzrgb, ready for ``TSDFFusion.pcwrite``.  One boolean index in torch: P is not known to the host beforehand, so this costs ONE
    synchronisation with the device."""
    if tuple(points.shape) != tuple(depth.shape) + (3,):
        raise ValueError(f"fused_point_cloud: points {tuple(points.shape)} do not belong to depth {tuple(depth.shape)}")
    cloud = points
    if colours is not None:
        colours = colours.to(points.device) if torch.is_tensor(colours) else torch.as_tensor(np.ascontiguousarray(colours), device=points.device)
        if tuple(colours.shape) != tuple(points.shape):
            raise ValueError(f"fused_point_cloud: colours {tuple(colours.shape)} do not belong to points {tuple(points.shape)}")
        cloud = torch.cat([points, colours.to(torch.float32)], dim=-1)
    return cloud[depth > 0]


def fused_point_views(depth):
    """Which frame every point of ``fused_point_cloud(depth, ...)`` came from: ``depth`` [N,H,W] (a tensor on any device) -> int32 [P] on
    its device, the frame index of every kept pixel in that function's order (frame-major, then row-major): what orients a point's normal
    toward the camera that saw it (``dvmvs.normals``).  One boolean index, as there: one synchronisation with the device."""
    if depth.dim() != 3:
        raise ValueError(f"fused_point_views: depth must be [N,H,W], got {tuple(depth.shape)}")
    frames = torch.arange(depth.shape[0], dtype=torch.int32, device=depth.device)[:, None, None].expand(depth.shape)
    return frames[depth > 0]
