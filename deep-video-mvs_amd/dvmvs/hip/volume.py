"""The voxel volume's own entries on the device: per-frame TSDF integration (csrc/tsdf.hip) and marching cubes
(csrc/marching_cubes.hip; definitions in include/dvmvs_hip.h): plain functions over the C ABI and the ops package's launch plumbing.
Inference-time geometry only: nothing here is registered under ``torch.ops.dvmvs`` and nothing needs autograd."""
import numpy as np
import torch

from dvmvs.hip import _capi
from dvmvs.hip.ops._common import launch, opt_ptr, ptr


def tsdf_integrate(tsdf, weight, color, origin, voxel_size, cam_intr, cam_pose, folded, depth, trunc_margin, obs_weight):
    """Fuses one frame into a TSDF volume in place (``dvmvs_tsdf_integrate``, one launch on the current stream): the three contiguous
    float32 [X,Y,Z] device tensors of ``dvmvs.tsdf.TSDFVolume``, ``cam_intr`` [3,3], camera-to-world ``cam_pose`` [4,4], the folded
    colour and the depth [h,w], all contiguous float32 on the volume's device.  ``TSDFVolume.integrate`` prepares them; nothing is
    checked, allocated or read here (the per-frame path)."""
    X, Y, Z = (int(d) for d in tsdf.shape)
    h, w = depth.shape
    launch("dvmvs_tsdf_integrate", tsdf.device, ptr(tsdf), ptr(weight), ptr(color), X, Y, Z, float(origin[0]), float(origin[1]),
           float(origin[2]), voxel_size, ptr(cam_intr), ptr(cam_pose), ptr(folded), ptr(depth), h, w, trunc_margin, float(obs_weight))


def marching_cubes(volume, level=0.0, color=None, origin=(0.0, 0.0, 0.0), voxel_size=1.0):
    """Iso-surface ``value == level`` of a device float32 volume [X,Y,Z] (z fastest) as device tensors
    ``(verts [V,3] float32, faces [F,3] int32, normals [V,3] float32, colors [V,3] uint8 or None)``.

    A corner is inside when ``value < level``; each grid edge with exactly one inside endpoint carries one vertex, shared by the
    faces around it.  Vertices are ordered by (linear index of the voxel that owns the edge, axis x < y < z), faces by cube, so
    two calls give the same bytes.  ``verts = index-space position * voxel_size + origin``; ``normals`` are the interpolated
    ``np.gradient`` of the volume, unit length (zero where it vanishes), pointing toward increasing values; faces are
    counter-clockwise seen from that side.  ``color`` (the folded ``b * 65536 + g * 256 + r`` volume) is read at the rounded
    vertex position and decoded to RGB.  A volume thinner than 2 voxels on an axis, or without a crossing, gives V = F = 0.

    Makes ONE host read (a synchronisation): the vertex and face counts, to size the outputs.  The case table is not the
    Lewiner (MC33) one of scikit-image: in cubes with ambiguous faces its triangles can differ from the reference's."""
    if not torch.is_tensor(volume) or volume.device.type != "cuda":
        raise TypeError("marching_cubes takes a device tensor (the HIP kernel has no CPU path)")
    if volume.dim() != 3 or volume.dtype != torch.float32:
        raise ValueError(f"volume must be float32 [X,Y,Z], got {volume.dtype} {tuple(volume.shape)}")
    dev = volume.device
    vol = volume.contiguous()
    col = None
    if color is not None:
        if not torch.is_tensor(color) or color.shape != volume.shape or color.dtype != torch.float32 or color.device != dev:
            raise ValueError("color must be a float32 device tensor of the volume's shape")
        col = color.contiguous()
    X, Y, Z = (int(d) for d in vol.shape)

    def empty(v, f):
        return (torch.empty((v, 3), dtype=torch.float32, device=dev), torch.empty((f, 3), dtype=torch.int32, device=dev),
                torch.empty((v, 3), dtype=torch.float32, device=dev), None if col is None else torch.empty((v, 3), dtype=torch.uint8, device=dev))

    if vol.numel() == 0:
        return empty(0, 0)
    nbytes = _capi.lib().dvmvs_marching_cubes_workspace_bytes(X, Y, Z)
    if nbytes == 0:
        raise RuntimeError(f"marching_cubes: volume {X}x{Y}x{Z} is too large for the kernel (2^31 voxels at most)")
    origin = [float(o) for o in np.asarray(origin, dtype=np.float32).reshape(3)]
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    launch("dvmvs_marching_cubes_count", dev, ptr(vol), X, Y, Z, float(level), ptr(workspace), nbytes, ptr(counts))
    V, F = (int(c) for c in counts.cpu())                      # the one host read
    verts, faces, normals, colors = empty(V, F)
    if V or F:
        launch("dvmvs_marching_cubes_emit", dev, ptr(vol), opt_ptr(col), X, Y, Z, float(level), origin[0], origin[1], origin[2],
               float(np.float32(voxel_size)), ptr(workspace), ptr(verts), ptr(normals), opt_ptr(colors), ptr(faces), V, F)
    return verts, faces, normals, colors
