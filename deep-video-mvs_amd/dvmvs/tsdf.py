"""Volumetric TSDF fusion of posed RGB-D frames on an MI355X (surface of the ``TSDFVolume`` / ``TSDFFusion`` classes of the
reference's reconstruction script, /root/reference/sample-data/run-tsdf-reconstruction.py:30-330).

``TSDFVolume.integrate`` is the hot function: one HIP launch (``dvmvs_tsdf_integrate``) updates the whole voxel volume in
place in HBM; the volumes never leave the device until ``get_volume()``.  The reference compiles an equivalent CUDA kernel
with pycuda and launches it once per "gpu loop"; its numba CPU fall-back has no counterpart here (GPU only, like the rest of
the package).

``get_mesh`` / ``get_point_cloud`` extract the zero iso-surface on the device with ``marching_cubes`` (csrc/marching_cubes.hip,
four launches), where the reference calls scikit-image's ``marching_cubes_lewiner`` on the host.  Vertices are the same (one on
every grid edge whose sign changes, linearly interpolated); in cubes with an ambiguous face or interior the Lewiner (MC33) cases
of scikit-image may triangulate differently, so face counts can differ slightly from the reference's; normals are the
interpolated ``np.gradient`` of the volume.  ``TSDFFusion`` carries the script's helpers (``meshwrite`` / ``pcwrite`` write the
same bytes, ``integrate``, ``calculate_volume_bounds``) and ``run`` is its main program: ``python -m dvmvs.tsdf --help``.
"""
import glob
import os
import time
from argparse import ArgumentParser

import numpy as np
import torch

from dvmvs.hip import _capi


def fold_color(color_im):
    """[H,W,3] RGB (0..255) -> float32 [H,W] holding b * 65536 + g * 256 + r (run-tsdf-reconstruction.py:236-238)."""
    c = np.asarray(color_im, dtype=np.float32)
    return np.floor(c[..., 2] * np.float32(65536.0) + c[..., 1] * np.float32(256.0) + c[..., 0]).astype(np.float32)


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
    lib = _capi.lib()
    nbytes = lib.dvmvs_marching_cubes_workspace_bytes(X, Y, Z)
    if nbytes == 0:
        raise RuntimeError(f"marching_cubes: volume {X}x{Y}x{Z} is too large for the kernel (2^31 voxels at most)")
    origin = [float(o) for o in np.asarray(origin, dtype=np.float32).reshape(3)]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _capi.check(lib.dvmvs_marching_cubes_count(vol.data_ptr(), X, Y, Z, float(level), workspace.data_ptr(), nbytes,
                                                   counts.data_ptr(), stream), "dvmvs_marching_cubes_count")
        V, F = (int(c) for c in counts.cpu())                      # the one host read
        verts, faces, normals, colors = empty(V, F)
        if V or F:
            _capi.check(lib.dvmvs_marching_cubes_emit(
                vol.data_ptr(), None if col is None else col.data_ptr(), X, Y, Z, float(level), origin[0], origin[1], origin[2],
                float(np.float32(voxel_size)), workspace.data_ptr(), verts.data_ptr(), normals.data_ptr(),
                None if colors is None else colors.data_ptr(), faces.data_ptr(), V, F, stream), "dvmvs_marching_cubes_emit")
    return verts, faces, normals, colors


def _mesh_and_cameras(verts, faces, cam_intr, cam_poses, device=None):
    """Device tensors (verts float32 [V,3], faces int32 [F,3], K float32 [N,3,3], poses float32 [N,4,4]) of a mesh and its views, given as
    arrays or tensors, the cameras as one matrix or a batch.  ``device``: where arrays go (default: where the vertices are, else "cuda")."""
    if device is None:
        device = verts.device if torch.is_tensor(verts) and verts.device.type == "cuda" else torch.device("cuda")

    def as_dev(a, dtype):
        if torch.is_tensor(a):
            return a.to(device, dtype)
        return torch.as_tensor(np.asarray(a, dtype={torch.float32: np.float32, torch.int32: np.int32}[dtype]), device=device)

    def cameras(a, tail):
        t = as_dev(a, torch.float32)
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or tuple(t.shape[1:]) != tail:
            raise ValueError(f"expected [{tail[0]},{tail[1]}] or [N,{tail[0]},{tail[1]}], got {tuple(t.shape)}")
        return t

    verts, faces = as_dev(verts, torch.float32), as_dev(faces, torch.int32)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"expected vertices [V,3] and faces [F,3], got {tuple(verts.shape)} and {tuple(faces.shape)}")
    P, K = cameras(cam_poses, (4, 4)), cameras(cam_intr, (3, 3))
    if K.shape[0] == 1 and P.shape[0] > 1:
        K = K.expand(P.shape[0], 3, 3)
    if K.shape[0] != P.shape[0]:
        raise ValueError(f"{K.shape[0]} intrinsics for {P.shape[0]} poses")
    return verts.contiguous(), faces.contiguous(), K.contiguous(), P.contiguous()


def render_mesh(verts, faces, cam_intr, cam_poses, height, width, near=0.05, far=float("inf"), cull_backfaces=False):
    """Rasterises a triangle mesh from N views in one call (``dvmvs.hip.ops.mesh_raster``, csrc/mesh_raster.hip; definition in
    include/dvmvs_hip.h): ``verts`` [V,3] world space and ``faces`` [F,3], ``cam_poses`` camera-to-world [N,4,4] or one [4,4], ``cam_intr``
    [N,3,3] or one [3,3] for all views; numpy arrays or tensors, as ``TSDFVolume.render`` takes them.  Returns DEVICE tensors ``(depth
    [N,height,width] float32, face [N,height,width] int32)``: the camera depth of the nearest face at every pixel (0 where there is none)
    and its index (-1), at the pixel positions of ``TSDFVolume.render``, so that the depth maps can go to ``compute_errors_device``.
    Reads ONE number per view from the device (a synchronisation): the triangles left out because they project beyond 2^21 pixels, and
    warns when there are any."""
    import warnings
    from dvmvs.hip import ops
    verts, faces, K, P = _mesh_and_cameras(verts, faces, cam_intr, cam_poses)
    depth, face, overflow = ops.mesh_raster(verts, faces, K, P, height, width, near=near, far=far, cull_backfaces=cull_backfaces,
                                            return_overflow=True)
    left_out = int(overflow.sum())                                  # the one host read
    if left_out:
        warnings.warn(f"render_mesh: {left_out} clipped triangles project beyond 2^21 pixels and were left out", RuntimeWarning, stacklevel=2)
    return depth, face


VISIBLE_MESH_CHUNK = 32       # views rasterised per call of visible_mesh: bounds the z-buffer keys (8 bytes per pixel and view)


def visible_mesh(verts, faces, cam_intr, cam_poses, height, width, min_views=1, near=0.05, relative=0.01, absolute=0.0):
    """The part of a mesh that N views observed: the mesh is rasterised from the views (``render_mesh``'s op), every vertex is tested
    against those depth maps (``dvmvs.hip.ops.mesh_visibility``: in front of ``near``, inside the image, not deeper than the rendered
    surface by more than ``relative`` of it plus ``absolute`` metres), and the faces whose three vertices are each seen by at least
    ``min_views`` views are kept.  Arguments as ``render_mesh``.  Returns DEVICE tensors ``(verts, kept_faces)``: the vertices are
    unchanged, so the face indices stay valid.  The views go through in chunks of ``VISIBLE_MESH_CHUNK``, so the memory does not grow
    with the length of the sequence.  No host read but the size of the result (the boolean selection of the kept faces)."""
    from dvmvs.hip import ops
    verts, faces, K, P = _mesh_and_cameras(verts, faces, cam_intr, cam_poses)
    min_views = int(min_views)
    if min_views < 1:
        raise ValueError(f"visible_mesh: min_views must be at least 1, got {min_views}")
    count = torch.zeros(verts.shape[0], dtype=torch.int32, device=verts.device)
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        return verts, faces[:0]
    for first in range(0, P.shape[0], VISIBLE_MESH_CHUNK):
        k, p = K[first:first + VISIBLE_MESH_CHUNK], P[first:first + VISIBLE_MESH_CHUNK]
        depth, _ = ops.mesh_raster(verts, faces, k, p, height, width, near=near)
        count += ops.mesh_visibility(verts, depth, k, p, near=near, relative=relative, absolute=absolute)
    V = verts.shape[0]
    index = faces.long()
    valid = ((index >= 0) & (index < V)).all(dim=1)
    seen = (count[index.clamp(0, V - 1)] >= min_views).all(dim=1) & valid
    return verts, faces[seen]


class TSDFVolume:
    """Voxel volume over ``vol_bnds`` ([[x0, x1], [y0, y1], [z0, z1]] in metres) with ``voxel_size`` edges.  tsdf starts at 1,
    weight and colour at 0; truncation = 5 voxels, as in the reference."""

    def __init__(self, vol_bnds, voxel_size, device="cuda", use_gpu=True):
        if not use_gpu:
            raise RuntimeError("TSDFVolume runs on an MI355X only: there is no CPU integration path in this package")
        vol_bnds = np.array(vol_bnds, dtype=np.float64)
        assert vol_bnds.shape == (3, 2), "[!] `vol_bnds` should be of shape (3, 2)."
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume needs a HIP device")
        self._voxel_size = float(voxel_size)
        self._trunc_margin = 5 * self._voxel_size
        self._color_const = 256 * 256
        self._vol_dim = np.ceil((vol_bnds[:, 1] - vol_bnds[:, 0]) / self._voxel_size).astype(int)
        vol_bnds[:, 1] = vol_bnds[:, 0] + self._vol_dim * self._voxel_size
        self._vol_bnds = vol_bnds
        self._vol_origin = vol_bnds[:, 0].astype(np.float32)
        dims = tuple(int(d) for d in self._vol_dim)
        self._tsdf = torch.ones(dims, dtype=torch.float32, device=self.device)
        self._weight = torch.zeros(dims, dtype=torch.float32, device=self.device)
        self._color = torch.zeros(dims, dtype=torch.float32, device=self.device)
        self._raycast_mask = None     # brick mask of render(): describes the volumes' contents, so integrate() drops it

    @property
    def vol_dim(self):
        return self._vol_dim

    def integrate(self, color_im, depth_im, cam_intr, cam_pose, obs_weight=1.0):
        """Fuses one frame: ``color_im`` [H,W,3] RGB, ``depth_im`` [H,W] metres (0 = invalid), ``cam_intr`` [3,3],
        ``cam_pose`` [4,4] camera-to-world; numpy arrays or tensors (device tensors are used in place)."""
        dev = self.device
        depth = torch.as_tensor(np.asarray(depth_im, dtype=np.float32) if not torch.is_tensor(depth_im) else depth_im,
                                dtype=torch.float32, device=dev).contiguous()
        if torch.is_tensor(color_im) and color_im.dim() == 2:
            color = color_im.to(dev, torch.float32).contiguous()            # already folded
        else:
            # (contiguous: an image that numpy indexing produced, e.g. by resize_nearest, is not row-major, and neither is its fold)
            color = torch.from_numpy(np.ascontiguousarray(fold_color(color_im.cpu().numpy() if torch.is_tensor(color_im) else color_im))).to(dev)
        if color.shape != depth.shape:
            raise ValueError(f"colour {tuple(color.shape)} and depth {tuple(depth.shape)} images differ in size")
        K = torch.as_tensor(np.asarray(cam_intr, dtype=np.float32) if not torch.is_tensor(cam_intr) else cam_intr,
                            dtype=torch.float32, device=dev).reshape(3, 3).contiguous()
        P = torch.as_tensor(np.asarray(cam_pose, dtype=np.float32) if not torch.is_tensor(cam_pose) else cam_pose,
                            dtype=torch.float32, device=dev).reshape(4, 4).contiguous()
        im_h, im_w = depth.shape
        x, y, z = (int(d) for d in self._vol_dim)
        with torch.cuda.device(dev):
            rc = _capi.lib().dvmvs_tsdf_integrate(
                self._tsdf.data_ptr(), self._weight.data_ptr(), self._color.data_ptr(), x, y, z,
                float(self._vol_origin[0]), float(self._vol_origin[1]), float(self._vol_origin[2]), self._voxel_size,
                K.data_ptr(), P.data_ptr(), color.data_ptr(), depth.data_ptr(), im_h, im_w, self._trunc_margin, float(obs_weight),
                torch.cuda.current_stream(dev).cuda_stream)
        self._raycast_mask = None      # (before the check: a failed call may have been enqueued)
        _capi.check(rc, "dvmvs_tsdf_integrate")

    def integrate_frames(self, color_ims, depth_ims, cam_intr, cam_poses, obs_weight=1.0, max_depth=float("inf"), stats=False):
        """Fuses N frames with ONE pass over the volume (``dvmvs.hip.ops.tsdf_integrate_frames``, csrc/tsdf_fuse.hip): the same bits as
        ``integrate`` called for frame 0, 1, ... N-1, after ``depth[depth > max_depth] = 0``.  ``color_ims`` [N,H,W,3] uint8 RGB or
        [N,H,W] folded colour, ``depth_ims`` [N,H,W] metres, ``cam_intr`` [3,3] or [N,3,3], ``cam_poses`` [N,4,4] camera-to-world,
        ``obs_weight`` one number or N; numpy arrays or tensors.  Contiguous device tensors of the kernel's types (float32; uint8 colour)
        are used in place: no copy and no synchronisation.  ``stats`` as in the op (tile counters, for tests and benchmarks)."""
        from dvmvs.hip import ops
        dev = self.device

        def as_dev(a, dtype):
            if torch.is_tensor(a):
                return a.to(dev, dtype).contiguous()     # the same tensor when it is already there in that type
            return torch.as_tensor(np.ascontiguousarray(a, dtype={torch.float32: np.float32, torch.uint8: np.uint8}[dtype]), device=dev)

        depth = as_dev(depth_ims, torch.float32)
        if depth.dim() != 3:
            raise ValueError(f"depth images must be [N,H,W], got {tuple(depth.shape)}")
        n = depth.shape[0]
        colour_dims = color_ims.dim() if torch.is_tensor(color_ims) else np.ndim(color_ims)
        if colour_dims == 4:
            is_u8 = color_ims.dtype == (torch.uint8 if torch.is_tensor(color_ims) else np.uint8)
            if is_u8:
                rgb, folded = as_dev(color_ims, torch.uint8), None
            else:         # float RGB, as ``integrate`` accepts it: folded on the host
                host = color_ims.cpu().numpy() if torch.is_tensor(color_ims) else np.asarray(color_ims)
                rgb, folded = None, torch.from_numpy(np.stack([fold_color(c) for c in host])).to(dev)
        elif colour_dims == 3:
            rgb, folded = None, as_dev(color_ims, torch.float32)
        else:
            raise ValueError("colour images must be [N,H,W,3] RGB or [N,H,W] folded")
        colour = rgb if rgb is not None else folded
        if tuple(colour.shape[:3]) != tuple(depth.shape):
            raise ValueError(f"colour {tuple(colour.shape)} and depth {tuple(depth.shape)} images differ in size")
        K, P = as_dev(cam_intr, torch.float32), as_dev(cam_poses, torch.float32)
        if K.dim() == 2:
            K = K.unsqueeze(0).expand(n, 3, 3).contiguous()
        if tuple(K.shape) != (n, 3, 3) or tuple(P.shape) != (n, 4, 4):
            raise ValueError(f"expected intrinsics [3,3] or [{n},3,3] and poses [{n},4,4], got {tuple(K.shape)} and {tuple(P.shape)}")
        self._raycast_mask = None      # (before the call: a failed call may have been enqueued)
        return ops.tsdf_integrate_frames(self._tsdf, self._weight, self._color, self._vol_origin, self._voxel_size, K, P, depth, rgb_u8=rgb,
                                         folded=folded, trunc_margin=self._trunc_margin, obs_weight=obs_weight, max_depth=max_depth,
                                         stats=stats)

    def render(self, cam_intr, cam_poses, height, width, near=0.0, far=float("inf"), step=1.0, normals=True, colour=True, skip_empty=True):
        """Ray-casts the volume from N views in one launch (csrc/tsdf_raycast.hip; definition in include/dvmvs_hip.h): ``cam_poses``
        camera-to-world [N,4,4] or one [4,4], ``cam_intr`` [N,3,3] or one [3,3] for all views; numpy arrays or tensors.  Returns device
        tensors ``(depth [N,height,width] float32, normals [N,height,width,3] float32 or None, rgb [N,height,width,3] uint8 or None)``:
        the camera depth of the fused surface along each pixel's ray (0 where the ray meets none between ``near`` and ``far``), its
        world-space unit normal (pointing toward increasing distance, i.e. to the observer's side; zero where undefined) and its colour.
        ``step``: sample spacing in voxels, in (0, 5].  ``skip_empty``: jump over bricks that cannot hold a crossing, with a mask
        cached on the volume until the next ``integrate``; the result is bit-identical either way."""
        from dvmvs.hip import ops
        dev = self.device

        def as_dev(a, tail):
            t = torch.as_tensor(np.asarray(a, dtype=np.float32) if not torch.is_tensor(a) else a, dtype=torch.float32, device=dev)
            if t.dim() == 2:
                t = t.unsqueeze(0)
            if t.dim() != 3 or tuple(t.shape[1:]) != tail:
                raise ValueError(f"expected [{tail[0]},{tail[1]}] or [N,{tail[0]},{tail[1]}], got {tuple(t.shape)}")
            return t

        P, K = as_dev(cam_poses, (4, 4)), as_dev(cam_intr, (3, 3))
        if K.shape[0] == 1 and P.shape[0] > 1:
            K = K.expand(P.shape[0], 3, 3)
        if K.shape[0] != P.shape[0]:
            raise ValueError(f"{K.shape[0]} intrinsics for {P.shape[0]} poses")
        mask = None
        if skip_empty:
            if self._raycast_mask is None:
                self._raycast_mask = ops.tsdf_raycast_mask(self._tsdf, self._weight)
            mask = self._raycast_mask
        return ops.tsdf_raycast(self._tsdf, self._weight, self._color if colour else None, self._vol_origin, self._voxel_size, K.contiguous(),
                                P.contiguous(), height, width, near=near, far=far, step=step, mask=mask, normals=normals, colour=colour)

    def get_volume(self):
        """(tsdf, colour) as numpy arrays, like the reference; ``get_weight_volume()`` for the weights."""
        return self._tsdf.cpu().numpy(), self._color.cpu().numpy()

    def get_weight_volume(self):
        return self._weight.cpu().numpy()

    def _extract(self, color, clean):
        """``marching_cubes`` of the volume, with ``clean`` (a ``dvmvs.components.ComponentFilter``) through ``filter_components`` on the
        device: the components of the welded mesh that the filter does not keep (floaters) are gone before anything else sees it."""
        mesh = marching_cubes(self._tsdf, 0.0, self._color if color else None, self._vol_origin, self._voxel_size)
        if clean is not None:
            from dvmvs.components import filter_components_device
            mesh = filter_components_device(mesh[0], mesh[1], clean, mesh[2], mesh[3])
        return mesh

    def get_mesh(self, clean=None):
        """(verts [V,3] float32 in world units, faces [F,3] int32, normals [V,3] float32, colours [V,3] uint8 RGB) of the zero
        iso-surface, as numpy arrays (run-tsdf-reconstruction.py:334-351); extracted on the device by ``marching_cubes``.  ``clean``: a
        ``dvmvs.components.ComponentFilter``; the mesh then goes through ``filter_components`` on the device before it is downloaded."""
        verts, faces, norms, colors = self._extract(True, clean)
        return verts.cpu().numpy(), faces.cpu().numpy(), norms.cpu().numpy(), colors.cpu().numpy()

    def get_point_cloud(self):
        """[N,6] float32: the mesh's vertices (xyz, world units) followed by their colour (rgb) (run-tsdf-reconstruction.py:313-332)."""
        verts, _, _, colors = self.get_mesh()
        return np.hstack([verts, colors])

    def vertices(self, clean=None):
        """The vertices of the zero iso-surface (``get_mesh()[0]``) as a float32 [V,3] DEVICE tensor: nothing but ``marching_cubes``'
        two counts is read by the host (with ``clean``, as ``get_mesh`` takes it, also ``filter_components``' counts)."""
        return self._extract(False, clean)[0]

    def mesh_tensors(self, clean=None):
        """``(verts float32 [V,3], faces int32 [F,3])`` of the zero iso-surface as DEVICE tensors, as ``marching_cubes`` leaves them (with
        ``clean``, as ``get_mesh`` takes it: as ``filter_components`` leaves them)."""
        return self._extract(False, clean)[:2]

    def surface_points(self, sample_density=None, voxel=None, clean=None):
        """The point set the 3-D metrics take from this volume's surface, as a float32 [N,3] DEVICE tensor: the vertices of the zero
        iso-surface; with ``sample_density`` (points per square metre) instead ``dvmvs.hip.ops.surface_sample`` of its faces; with ``voxel``
        (metres) then ``dvmvs.hip.ops.voxel_downsample`` of that (``dvmvs.errors.prepare_points`` is the host definition of both).  The
        vertices and faces stay on the device; each step reads its output's size once.  ``clean``: as ``get_mesh`` takes it; the points are
        then those of the cleaned mesh."""
        from dvmvs.errors import prepare_points_device
        verts, faces = self.mesh_tensors(clean)
        return prepare_points_device(verts, faces, sample_density, voxel)

    def score_against(self, reference, threshold=0.05, return_sizes=False, sample_density=None, voxel=None, visible_from=None, clean=None,
                      align_plane=False, align_normal_neighbours=20, align_normal_distance=np.inf, align_distance=None, align_scale=False,
                      return_transform=False):
        """The 3-D reconstruction metrics of this volume's surface (the prediction) against ``reference`` (the ground truth): a float32 [6]
        DEVICE tensor in the order of ``dvmvs.errors.RECONSTRUCTION_METRICS`` (acc, comp, chamfer, precision, recall, fscore), computed by
        ``dvmvs.errors.compute_reconstruction_errors_device`` without a download.  ``reference``: another ``TSDFVolume``, [M,3] points as a
        tensor or a numpy array (uploaded), or a mesh as a ``(verts [V,3], faces [F,3])`` pair of tensors or arrays.

        With ``sample_density`` and ``voxel`` at None the point sets are the VERTICES of the surfaces (of the zero iso-surface, taken on the
        device from ``marching_cubes``: one per crossed grid edge, about a voxel apart), and a distance is measured to the nearest vertex,
        not to the nearest point of a face.  That compares two volumes of one voxel size soundly; it does not suit a coarse reference mesh
        or two voxel sizes.  For those, ``sample_density`` (points per square metre) replaces the vertices of every side that has faces by
        ``surface_points``-style samples of them, and ``voxel`` (metres) replaces each side by one point per occupied voxel, so that both
        clouds have the same resolution (the usual evaluation protocol; ``dvmvs.errors.prepare_points``).  Each of those steps reads its
        output's size once.  Raises ``ValueError`` when either point set is empty.  ``return_sizes``: also return the sizes of the two
        point sets that were scored ``(prediction, reference)``, numbers the host has anyway (tensor shapes).

        ``visible_from``: a tuple ``(cam_intr, cam_poses, height, width)`` or ``(cam_intr, cam_poses, height, width, min_views)``.  The
        reference, which must then be a mesh (a pair, or a ``TSDFVolume``), is first restricted by ``visible_mesh`` to the faces those views
        observed, so that surface the sequence never faced does not count against completeness and recall.  It needs ``sample_density``:
        the vertices of a culled face set would still include those that no kept face uses.  ``ValueError`` otherwise, and for a bare
        point set.  With ``return_sizes`` a third entry ``(kept faces, all faces)`` of the reference is returned.

        ``clean``: a ``dvmvs.components.ComponentFilter``.  The PREDICTION's mesh, this volume's, goes through
        ``filter_components`` on the device before its vertices are taken or its faces sampled, so that floaters do not count against
        accuracy and precision; the reference is never cleaned (a ``TSDFVolume`` reference included).

        ``align_distance`` (metres): before it is scored, the prediction's point set is registered to the reference's by trimmed ICP
        with that inlier distance and moved by the result (``dvmvs.hip.registration.icp``; ``dvmvs.errors.register_points`` is the host
        definition), so that a residual pose offset does not decide the score; ``align_scale`` lets the registration also find a scale.
        Nothing is read by the host.  ``return_transform``: the transform, a float64 [4,4] DEVICE tensor that takes this volume's
        coordinates into the reference's, comes back as the LAST entry of the returned tuple.

        ``align_plane`` (needs ``align_distance``, excludes ``align_scale``): the registration is point-to-plane on the reference's
        normals (``dvmvs.hip.registration.icp_plane``; ``dvmvs.errors.register_points_plane`` is the host definition), which needs a
        fraction of the iterations on walls and floors.  A ``TSDFVolume`` reference scored on its vertices brings the normals of its
        marching-cubes mesh; in every other mode they are estimated from the reference's prepared points
        (``dvmvs.hip.normals.estimate_normals`` with ``align_normal_neighbours`` nearest points within ``align_normal_distance``)."""
        return self._score_against(reference, threshold, return_sizes, sample_density, voxel, visible_from, align_distance, align_scale,
                                   return_transform, clean=clean, align_plane=align_plane, align_normal_neighbours=align_normal_neighbours,
                                   align_normal_distance=align_normal_distance)[0]

    def _score_against(self, reference, threshold, return_sizes, sample_density, voxel, visible_from, align_distance, align_scale,
                       return_transform, clean=None, align_plane=False, align_normal_neighbours=20, align_normal_distance=np.inf):
        """``score_against``: ``(what it returns, the registration's record or None)``; the record is ``dvmvs.hip.registration.icp``'s
        (with ``align_plane``: ``icp_plane``'s) ``info`` (device tensors)."""
        from dvmvs.errors import _check_alignment, _check_plane, _score_device, prepare_points_device
        _check_alignment("score_against", align_distance, align_scale, None, return_transform)
        _check_plane("score_against", align_plane, align_distance, align_scale, None, False, align_normal_neighbours, align_normal_distance)
        gt_normals = None
        prepare = sample_density is not None or voxel is not None
        if visible_from is not None:
            if sample_density is None:
                raise ValueError("score_against: visible_from needs sample_density (the kept faces are sampled; the vertices are not culled)")
            if len(visible_from) not in (4, 5):
                raise ValueError("score_against: visible_from is (cam_intr, cam_poses, height, width[, min_views])")
        gt_faces = None
        if isinstance(reference, TSDFVolume):
            if prepare:
                gt, gt_faces = reference.mesh_tensors()
            elif align_plane:                            # the gradient normals of the reference's marching-cubes mesh come with its vertices
                gt, _, gt_normals = reference._extract(False, None)[:3]
                gt_normals = gt_normals.to(self.device).contiguous()
            else:
                gt = reference.vertices()
            gt = gt.to(self.device)
        else:
            if isinstance(reference, (tuple, list)) and len(reference) == 2 and all(len(getattr(part, "shape", ())) == 2 for part in reference):
                reference, gt_faces = reference          # a mesh: two arrays or tensors [V,3] and [F,3]
            gt = torch.as_tensor(reference, dtype=torch.float32, device=self.device)
            if gt.dim() != 2 or gt.shape[1] != 3:
                raise ValueError(f"score_against: reference points must be [M,3], got {tuple(gt.shape)}")
        face_counts = None
        if visible_from is not None:
            if gt_faces is None:
                raise ValueError("score_against: visible_from restricts a mesh reference; a bare point set has no faces to cull")
            cam_intr, cam_poses, height, width = visible_from[:4]
            all_faces = int(gt_faces.shape[0])
            gt, gt_faces = visible_mesh(gt.contiguous(), torch.as_tensor(gt_faces, device=self.device).to(torch.int32), cam_intr, cam_poses,
                                        height, width, min_views=visible_from[4] if len(visible_from) == 5 else 1)
            face_counts = (int(gt_faces.shape[0]), all_faces)
        if prepare:
            if gt_faces is not None:
                gt_faces = torch.as_tensor(gt_faces, device=self.device).to(torch.int32)
            pred = self.surface_points(sample_density, voxel, clean=clean)
            gt = prepare_points_device(gt.contiguous(), gt_faces, sample_density, voxel)
        else:
            pred = self.vertices(clean=clean)
        if pred.shape[0] == 0 or gt.shape[0] == 0:
            raise ValueError(f"score_against: a surface without a vertex cannot be scored ({pred.shape[0]} predicted, {gt.shape[0]} reference)")
        row, transform, info = _score_device(pred, gt.contiguous(), threshold, None, None, None, None, None, align_distance, align_scale, None,
                                             align_plane, gt_normals, align_normal_neighbours, align_normal_distance)
        result = (row,)
        if return_sizes:
            result += ((int(pred.shape[0]), int(gt.shape[0])),) + (() if face_counts is None else (face_counts,))
        if return_transform:
            result += (transform,)
        return (result[0] if len(result) == 1 else result), info


class TSDFFusion:
    """Host-side helpers of the reference class of the same name."""

    @staticmethod
    def rigid_transform(xyz, transform):
        xyz_h = np.hstack([xyz, np.ones((len(xyz), 1), dtype=np.float32)])
        return np.dot(transform, xyz_h.T).T[:, :3]

    @staticmethod
    def get_view_frustum(depth_im, cam_intr, cam_pose):
        """[3,5] world-space corners (camera centre + the four far corners) of the frame's view frustum."""
        im_h, im_w = depth_im.shape[0], depth_im.shape[1]
        far = np.max(depth_im)
        xs = (np.array([0, 0, 0, im_w, im_w]) - cam_intr[0, 2]) * np.array([0, far, far, far, far]) / cam_intr[0, 0]
        ys = (np.array([0, 0, im_h, 0, im_h]) - cam_intr[1, 2]) * np.array([0, far, far, far, far]) / cam_intr[1, 1]
        pts = np.array([xs, ys, np.array([0, far, far, far, far])])
        return TSDFFusion.rigid_transform(pts.T, cam_pose).T

    @staticmethod
    def volume_bounds(frames):
        """Axis-aligned bounds [[x0,x1],[y0,y1],[z0,z1]] enclosing the view frusta of ``frames`` = iterable of
        (depth_im, cam_intr, cam_pose), the way the reference's main loop accumulates them."""
        bounds = np.zeros((3, 2))
        bounds[:, 0], bounds[:, 1] = np.inf, -np.inf
        for depth_im, cam_intr, cam_pose in frames:
            frustum = TSDFFusion.get_view_frustum(depth_im, cam_intr, cam_pose)
            bounds[:, 0] = np.minimum(bounds[:, 0], np.amin(frustum, axis=1))
            bounds[:, 1] = np.maximum(bounds[:, 1], np.amax(frustum, axis=1))
        return bounds

    @staticmethod
    def calculate_volume_bounds(depth_maps, poses, K):
        """Bounds of the view frusta of ``depth_maps`` seen from ``poses`` with intrinsics ``K``, the reconstruction script's way:
        the running min / max start at ZERO, so the world origin is always inside (``volume_bounds`` starts at +-inf)."""
        assert len(depth_maps) == len(poses)
        bounds = np.zeros((3, 2))
        for depth_map, pose in zip(depth_maps, poses):
            frustum = TSDFFusion.get_view_frustum(depth_map, K, pose)
            bounds[:, 0] = np.minimum(bounds[:, 0], np.amin(frustum, axis=1))
            bounds[:, 1] = np.maximum(bounds[:, 1], np.amax(frustum, axis=1))
        return bounds

    @staticmethod
    def frustum_bounds(poses, K, height, width, max_depth):
        """``calculate_volume_bounds`` of depth maps that are ``max_depth`` everywhere, without the maps: the bounds of every view's frustum
        cut at ``max_depth`` (and of the world origin, as there).  They contain the bounds of any depth maps <= ``max_depth`` seen from the
        same poses, so a live run can size its volume before a depth exists."""
        constant = np.full((int(height), int(width)), max_depth)
        return TSDFFusion.calculate_volume_bounds([constant] * len(poses), poses, K)

    @staticmethod
    def _columns(formats, columns):
        """Rows of space-separated, %-formatted columns, each ending in a newline: one string, built without a Python loop
        over the rows (np.char formats each column element with the same % operator a per-row write uses)."""
        if len(columns[0]) == 0:
            return ""
        line = np.char.mod(formats[0], columns[0])
        for fmt, col in zip(formats[1:], columns[1:]):
            line = np.char.add(np.char.add(line, " "), np.char.mod(fmt, col))
        return "\n".join(line.tolist()) + "\n"

    @staticmethod
    def meshwrite(filename, verts, faces, norms, colors):
        """ASCII .ply of a coloured mesh with normals, byte for byte the reconstruction script's format (:379-415)."""
        verts, faces, norms, colors = (np.asarray(a) for a in (verts, faces, norms, colors))
        header = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                  "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
                  "property uchar blue\nelement face %d\nproperty list uchar int vertex_index\nend_header\n") % (len(verts), len(faces))
        body = TSDFFusion._columns(["%f"] * 6 + ["%d"] * 3, [verts[:, 0], verts[:, 1], verts[:, 2], norms[:, 0], norms[:, 1], norms[:, 2],
                                                            colors[:, 0], colors[:, 1], colors[:, 2]])
        tris = TSDFFusion._columns(["3 %d", "%d", "%d"], [faces[:, 0], faces[:, 1], faces[:, 2]])
        with open(filename, "w") as f:
            f.write(header + body + tris)

    _PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
                  "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}

    @staticmethod
    def meshread(filename):
        """``(verts float32 [V,3], faces int32 [F,3])`` of a .ply mesh, numpy only: ``format ascii 1.0`` or ``binary_little_endian 1.0``;
        the vertex element needs the scalar properties x, y, z, in any order and of any scalar type, and its other properties are
        skipped; the face element is ``property list uchar|int int|uint vertex_index|vertex_indices`` (other face properties are
        skipped), a polygon of n corners becoming the fan (0, i, i + 1) of n - 2 triangles; other elements are skipped.  Reads what
        ``meshwrite`` writes.  Raises ``ValueError`` for a ``binary_big_endian`` file and for anything else it cannot read."""
        types = TSDFFusion._PLY_TYPES
        with open(filename, "rb") as f:
            data = f.read()
        end = data.find(b"end_header")
        if not data.startswith(b"ply") or end < 0:
            raise ValueError(f"meshread: {filename} is not a PLY file")
        body = data.find(b"\n", end) + 1
        fmt, elements = None, []          # elements: [name, count, [(kind, name, type or (count type, item type)), ...]]
        for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
            words = line.split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            if words[0] == "format":
                fmt = words[1]
            elif words[0] == "element":
                elements.append([words[1], int(words[2]), []])
            elif words[0] == "property" and elements:
                if words[1] == "list":
                    elements[-1][2].append(("list", words[4], (types.get(words[2]), types.get(words[3]))))
                else:
                    elements[-1][2].append(("scalar", words[2], types.get(words[1])))
        if fmt == "binary_big_endian":
            raise ValueError(f"meshread: {filename} is a binary_big_endian PLY file; only ascii and binary_little_endian are read")
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError(f"meshread: {filename} has the unknown format {fmt!r}")
        for name, _, properties in elements:
            for kind, prop, t in properties:
                if (t if kind == "scalar" else t[0] and t[1]) is None:
                    raise ValueError(f"meshread: property {prop} of element {name} has an unknown type")
        verts, faces = None, np.zeros((0, 3), dtype=np.int32)
        tokens, pos = (data[body:].split(), 0) if fmt == "ascii" else (None, body)
        for name, count, properties in elements:
            scalar_only = all(kind == "scalar" for kind, _, _ in properties)
            if fmt == "ascii":
                width = len(properties)
                if scalar_only:
                    rows = np.array(tokens[pos:pos + count * width], dtype=np.float64).reshape(count, width)
                    pos += count * width
                    columns = {prop: rows[:, i] for i, (_, prop, _) in enumerate(properties)}
                    lists = {}
                elif count and len(properties) == 1 and len(tokens) >= pos + count * (int(tokens[pos]) + 1) and np.all(
                        np.array(tokens[pos:pos + count * (int(tokens[pos]) + 1)], dtype=np.float64).reshape(count, -1)[:, 0] == int(tokens[pos])):
                    n = int(tokens[pos])                         # the usual case: every polygon has the corners of the first
                    table = np.array(tokens[pos:pos + count * (n + 1)], dtype=np.float64).reshape(count, n + 1)
                    pos += count * (n + 1)
                    columns, lists = {}, {properties[0][1]: table[:, 1:].astype(np.int64)}
                else:
                    columns, lists = {}, {prop: [] for kind, prop, _ in properties if kind == "list"}
                    for _ in range(count):
                        for kind, prop, _ in properties:
                            if kind == "list":
                                n = int(tokens[pos])
                                lists[prop].append(np.array(tokens[pos + 1:pos + 1 + n], dtype=np.int64))
                                pos += 1 + n
                            else:
                                pos += 1
            else:
                if scalar_only:
                    dtype = np.dtype([(prop, "<" + t) for _, prop, t in properties])
                    table = np.frombuffer(data, dtype=dtype, count=count, offset=pos)
                    pos += count * dtype.itemsize
                    columns, lists = {prop: table[prop] for _, prop, _ in properties}, {}
                else:
                    columns, lists = {}, {prop: [] for kind, prop, _ in properties if kind == "list"}
                    uniform = None
                    if count and len(properties) == 1:          # the usual case: every polygon has the corners of the first
                        ct, it = (np.dtype("<" + t) for t in properties[0][2])
                        n = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0])
                        dtype = np.dtype([("n", ct), ("v", it, (n,))])
                        if pos + count * dtype.itemsize <= len(data):
                            table = np.frombuffer(data, dtype=dtype, count=count, offset=pos)
                            if np.all(table["n"] == n):
                                uniform = table["v"].astype(np.int64).reshape(count, n)
                                pos += count * dtype.itemsize
                    if uniform is not None:
                        lists[properties[0][1]] = uniform
                    else:
                        for _ in range(count):
                            for kind, prop, t in properties:
                                if kind == "list":
                                    ct, it = (np.dtype("<" + x) for x in t)
                                    n = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0])
                                    pos += ct.itemsize
                                    lists[prop].append(np.frombuffer(data, dtype=it, count=n, offset=pos).astype(np.int64))
                                    pos += n * it.itemsize
                                else:
                                    pos += np.dtype(t).itemsize
            if name == "vertex":
                if not all(axis in columns for axis in "xyz"):
                    raise ValueError(f"meshread: the vertex element of {filename} lacks x, y or z")
                verts = np.stack([np.asarray(columns[axis], dtype=np.float32) for axis in "xyz"], axis=1).reshape(-1, 3)
            elif name == "face":
                polygons = lists.get("vertex_index", lists.get("vertex_indices"))
                if polygons is None:
                    raise ValueError(f"meshread: the face element of {filename} has no vertex_index list")
                if isinstance(polygons, np.ndarray):
                    n = polygons.shape[1]
                    fans = [polygons[:, [0, i, i + 1]] for i in range(1, n - 1)]
                    triangles = np.stack(fans, axis=1).reshape(-1, 3) if fans else np.zeros((0, 3), np.int64)
                else:
                    triangles = [(p[0], p[i], p[i + 1]) for p in polygons for i in range(1, len(p) - 1)]
                faces = np.asarray(triangles, dtype=np.int64).reshape(-1, 3).astype(np.int32)
        if verts is None:
            raise ValueError(f"meshread: {filename} has no vertex element")
        return verts, faces

    @staticmethod
    def pcwrite(filename, xyzrgb):
        """ASCII .ply of a coloured point cloud [N,6] (xyz, rgb), byte for byte the reconstruction script's format (:417-439)."""
        xyzrgb = np.asarray(xyzrgb)
        xyz, rgb = xyzrgb[:, :3], xyzrgb[:, 3:].astype(np.uint8)
        header = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n") % len(xyz)
        body = TSDFFusion._columns(["%f"] * 3 + ["%d"] * 3, [xyz[:, 0], xyz[:, 1], xyz[:, 2], rgb[:, 0], rgb[:, 1], rgb[:, 2]])
        with open(filename, "w") as f:
            f.write(header + body)

    @staticmethod
    def pcwrite_normals(filename, xyzrgb, normals):
        """ASCII .ply of a coloured point cloud [N,6] (xyz, rgb) with a normal [N,3] for every point: ``pcwrite``'s format with ``property float
        nx/ny/nz`` between z and red, the vertex layout of ``meshwrite`` (what MeshLab, Open3D and ``meshread`` read)."""
        xyzrgb, normals = np.asarray(xyzrgb), np.asarray(normals)
        if normals.shape != (len(xyzrgb), 3):
            raise ValueError(f"pcwrite_normals: normals {normals.shape} do not belong to {len(xyzrgb)} points")
        xyz, rgb = xyzrgb[:, :3], xyzrgb[:, 3:].astype(np.uint8)
        header = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                  "property float nx\nproperty float ny\nproperty float nz\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n") % len(xyz)
        body = TSDFFusion._columns(["%f"] * 6 + ["%d"] * 3, [xyz[:, 0], xyz[:, 1], xyz[:, 2], normals[:, 0], normals[:, 1], normals[:, 2],
                                                            rgb[:, 0], rgb[:, 1], rgb[:, 2]])
        with open(filename, "w") as f:
            f.write(header + body)

    @staticmethod
    def integrate(tsdf_volume, images, depths, poses, K, mesh_name, save_progressive, clean=None):
        """Fuses every (image, depth, pose) with weight 1 and writes ``<mesh_name>_complete.ply`` (with ``save_progressive``,
        also ``<mesh_name>_frame_<i>.ply`` after each frame), like the reconstruction script (:442-462).  ``clean`` (a
        ``dvmvs.components.ComponentFilter``) is handed to every ``get_mesh`` whose mesh is written, the progressive ones included."""
        n = len(images)
        start = time.time()
        for i in range(n):
            print(f"Fusing frame {i + 1}/{n} for {mesh_name}")
            tsdf_volume.integrate(images[i], depths[i], K, poses[i], obs_weight=1.0)
            if save_progressive:
                print("Saving for progressive visuals...")
                TSDFFusion.meshwrite(f"{mesh_name}_frame_{i:05d}.ply", *tsdf_volume.get_mesh(clean=clean))
        torch.cuda.synchronize(tsdf_volume.device)
        print("Average FPS: {:.2f}".format(n / max(time.time() - start, 1e-9)))
        print("Saving mesh to", mesh_name)
        TSDFFusion.meshwrite(mesh_name + "_complete.ply", *tsdf_volume.get_mesh(clean=clean))


class LiveFusion:
    """Fuses depth maps into a TSDF volume WHILE a scene runs: ``add`` takes the network's depth where it lies on the device and returns
    at once; every ``batch`` frames one ``TSDFVolume.integrate_frames`` launch fuses them (one pass over the volume; the bits of per-frame
    ``integrate`` on depths with ``depth > max_depth`` set to 0).  ``volume`` is the reconstruction at any moment, ready for ``get_mesh()``,
    ``render(...)`` and ``get_point_cloud()``.

    ``add`` enqueues and returns: the depth is copied device-to-device on the current stream into the next slot of a ring [batch,h,w] (the
    engine's output buffer is static and the next frame overwrites it); the intrinsics, the pose and a host colour image go up together
    through one slot of a ring of 8 pinned buffers with one non-blocking copy (``FrameUploader``) and from there into their rings
    [batch,3,3], [batch,4,4], [batch,h,w,3].  It never waits for the device to finish work of the CURRENT frame; the one wait it can
    make is ``FrameUploader``'s, before a pinned slot is written again, for the upload that last read that slot -- the one of 8 ``add``
    calls earlier.  So the host runs at most 8 frames ahead of the device's copy queue, and no further.  (That wait is on an event, which
    torch's synchronisation detector does not see.)
    ASSUMPTION: every call (``add``, ``flush``, ``volume`` and whatever uses the volume) is issued on ONE stream.  Everything is then in
    stream order -- a ring slot is rewritten only by copies enqueued after the launch that read it -- so no event guards the rings.

    ``min_consistent_views`` > 0 filters every batch by multi-view geometric consistency before it is fused (``dvmvs.consistency``, one more
    launch pair per flush): the pending frames are checked against each other, frame i against the ``consistency_sources`` frames nearest
    to it in the batch (``nearest_sources``), and a pixel is fused, with its own depth (``average=False``), only where at least that many of
    them agree within ``pixel_threshold`` pixels and ``relative_threshold`` of the depth.  The source tables of every batch size up to
    ``batch`` go up once, in the constructor, so ``add`` and ``flush`` stay free of blocking copies and host reads.  CONSEQUENCE: a flush of
    a single pending frame (the tail of a scene, or ``batch=1``) has no neighbour to agree with and fuses nothing.  With the default 0
    nothing is allocated or launched for the filter and the volume's bits are those of the unfiltered fusion."""

    def __init__(self, vol_bnds, voxel_size=0.025, max_depth=5.0, batch=8, device="cuda", min_consistent_views=0, consistency_sources=4,
                 pixel_threshold=1.0, relative_threshold=0.01):
        batch = int(batch)
        if batch < 1:
            raise ValueError(f"LiveFusion: batch must be at least 1, got {batch}")
        min_consistent_views, consistency_sources = int(min_consistent_views), int(consistency_sources)
        if min_consistent_views < 0:
            raise ValueError(f"LiveFusion: min_consistent_views must not be negative, got {min_consistent_views}")
        if not 0 <= consistency_sources <= 16:
            raise ValueError(f"LiveFusion: consistency_sources must be between 0 and 16, got {consistency_sources}")
        if float(pixel_threshold) != float(pixel_threshold) or float(relative_threshold) != float(relative_threshold):
            raise ValueError("LiveFusion: a consistency threshold is NaN")
        if not float(voxel_size) > 0.0:
            raise ValueError(f"LiveFusion: voxel_size must be positive, got {voxel_size}")
        if float(max_depth) != float(max_depth):
            raise ValueError("LiveFusion: max_depth is NaN")
        from dvmvs.dataset_loader import FrameUploader
        self.batch, self.max_depth = batch, float(max_depth)
        self._volume = TSDFVolume(vol_bnds, voxel_size, device=device)
        self.device = self._volume._tsdf.device      # with its index ("cuda" -> "cuda:0"): what a tensor's ``.device`` compares equal to
        self._uploader = FrameUploader(self.device, slots=8)
        self._depth = self._rgb = self._K = self._P = None
        self._weights, self._pending, self.frames = [], 0, 0
        self.min_consistent_views, self.pixel_threshold, self.relative_threshold = min_consistent_views, float(pixel_threshold), float(relative_threshold)
        self._filtered = self._source_tables = None
        if min_consistent_views > 0:
            from dvmvs.consistency import nearest_sources
            tables = np.full((batch, batch, consistency_sources), -1, dtype=np.int32)     # [n - 1, :n] = the table of a flush of n frames
            for n in range(1, batch + 1):
                tables[n - 1, :n] = nearest_sources(n, consistency_sources)
            self._source_tables = torch.as_tensor(tables, device=self.device)

    def _rings(self, h, w):
        if self._depth is None:
            dev = self.device
            self._depth = torch.empty((self.batch, h, w), dtype=torch.float32, device=dev)
            self._rgb = torch.empty((self.batch, h, w, 3), dtype=torch.uint8, device=dev)
            self._K = torch.empty((self.batch, 3, 3), dtype=torch.float32, device=dev)
            self._P = torch.empty((self.batch, 4, 4), dtype=torch.float32, device=dev)
            if self.min_consistent_views > 0:
                self._filtered = torch.empty((self.batch, h, w), dtype=torch.float32, device=dev)
        elif tuple(self._depth.shape[1:]) != (h, w):
            raise ValueError(f"LiveFusion: a {h}x{w} frame in a run of {self._depth.shape[1]}x{self._depth.shape[2]} frames")

    def add(self, depth, rgb_u8, K, pose, obs_weight=1.0):
        """``depth``: float32 device tensor with h * w elements in its last two dimensions ([h,w], [1,h,w], [1,1,h,w]); ``rgb_u8``
        [h,w,3] uint8 (numpy, host or device tensor); ``K`` [3,3] and camera-to-world ``pose`` [4,4] (numpy or host tensors)."""
        if not torch.is_tensor(depth) or depth.device != self.device or depth.dtype != torch.float32 or depth.dim() < 2:
            raise ValueError(f"LiveFusion.add: depth must be a float32 tensor on {self.device}")
        h, w = int(depth.shape[-2]), int(depth.shape[-1])
        if depth.numel() != h * w:
            raise ValueError(f"LiveFusion.add: one depth map at a time, got {tuple(depth.shape)}")
        if tuple(rgb_u8.shape) != (h, w, 3) or rgb_u8.dtype != (torch.uint8 if torch.is_tensor(rgb_u8) else np.uint8):
            raise ValueError(f"LiveFusion.add: colour must be uint8 [{h},{w},3] like the depth, got {rgb_u8.dtype} {tuple(rgb_u8.shape)}")
        matrices = np.concatenate([np.asarray(K, dtype=np.float32).reshape(9), np.asarray(pose, dtype=np.float32).reshape(16)])
        self._rings(h, w)
        slot = self._pending
        self._depth[slot].copy_(depth.reshape(h, w), non_blocking=True)
        staged = matrices.view(np.uint8)             # 100 bytes first, so the floats are aligned; a host colour image goes behind them
        if torch.is_tensor(rgb_u8) and rgb_u8.device.type != "cpu":
            self._rgb[slot].copy_(rgb_u8, non_blocking=True)
        else:
            host = rgb_u8.numpy() if torch.is_tensor(rgb_u8) else rgb_u8
            staged = np.concatenate([staged, np.ascontiguousarray(host).reshape(-1)])
        staged = self._uploader.upload(staged)       # ONE pinned slot and one host-to-device copy per frame
        if staged.numel() > 100:
            self._rgb[slot].copy_(staged[100:].view(h, w, 3), non_blocking=True)
        floats = staged[:100].view(torch.float32)
        self._K[slot].copy_(floats[:9].view(3, 3), non_blocking=True)
        self._P[slot].copy_(floats[9:].view(4, 4), non_blocking=True)
        self._weights.append(float(obs_weight))
        self._pending += 1
        self.frames += 1
        if self._pending == self.batch:
            self.flush()

    def flush(self):
        """Fuses the frames that are pending (fewer than ``batch``); nothing happens when there is none."""
        n = self._pending
        if n == 0:
            return
        depth = self._depth[:n]
        if self.min_consistent_views > 0:
            from dvmvs.hip import ops
            depth, _, _ = ops.depth_consistency(depth, self._K[:n], self._P[:n], self._source_tables[n - 1, :n], self.pixel_threshold,
                                                self.relative_threshold, self.min_consistent_views, average=False, with_count=False,
                                                out=self._filtered[:n])
        self._volume.integrate_frames(self._rgb[:n], depth, self._K[:n], self._P[:n], obs_weight=self._weights, max_depth=self.max_depth)
        self._weights, self._pending = [], 0

    @property
    def volume(self):
        self.flush()
        return self._volume


def _mesh_name(reconstruction_folder, voxel_size, max_depth, anchor, system, dataset_name, scene_name):
    return (f"{reconstruction_folder}/reconstruction_voxelsize-{voxel_size}_maxdepth-{max_depth}_anchor-{anchor}_"
            f"{system}_{dataset_name}_{scene_name}")


def run(reconstruction_folder, prediction_folder, data_folder, dataset_name, scene_name, system_name, voxel_size, max_depth,
        use_groundtruth_to_anchor, save_progressive, save_groundtruth, device="cuda", device_preprocess=False, render_keyframes=False,
        evaluate_3d=False, threshold_3d=0.05, filter_consistency=False, consistency_views=2, consistency_sources=4, consistency_pixel=1.0,
        consistency_relative=0.01, save_point_cloud=False, evaluate_3d_density=None, evaluate_3d_voxel=None, groundtruth_mesh=None,
        evaluate_3d_visible=False, evaluate_3d_min_views=1, evaluate_3d_align=None, evaluate_3d_align_scale=False, evaluate_3d_align_plane=False,
        evaluate_3d_align_neighbours=20, evaluate_3d_align_normal_distance=None, point_mesh_voxel=None, point_mesh_radius=None,
        point_mesh_neighbours=32, point_mesh_min_neighbours=3, groundtruth_transform=None, point_normals_neighbours=None,
        point_normals_max_distance=None, clean_points_neighbours=None, clean_points_ratio=2.0, clean_points_max_distance=None,
        clean_points_radius=None, clean_points_min_neighbours=None, clean_mesh_area=None, clean_mesh_faces=None, clean_mesh_largest=False):
    """The reconstruction script's main program (run-tsdf-reconstruction.py:477-636): fuses a scene's saved keyframe depth
    predictions (``keyframe_<dataset>_<system>_predictions_<scene>*.npz`` in ``prediction_folder``) into a TSDF volume and writes
    the mesh; optionally the same from the ground-truth depth maps.  Images and depth PNGs are read with the package's own
    loaders (no OpenCV).  ``device_preprocess`` (the switch the scene runners share): this program resamples its colour images with
    nearest selection only and integrates them as 8-bit, so all the switch does here is keep them 8-bit from the decoder on
    (``load_image_u8``: no float32 round trip); the values, and the meshes, are the same.

    ``render_keyframes``: after fusion, ray-cast the volume from every fused keyframe's own view at the prediction size (one launch,
    ``TSDFVolume.render``) and save the fused depth maps next to the meshes as ``keyframe_<dataset>_<system>+tsdf_predictions_<scene>.npz``,
    the layout of the network's predictions; if the scene has ground-truth depth, also their error metrics (``..._errors_<scene>.npz``),
    evaluated on the device over the pixels where a surface was hit.  Without the flag nothing else is written or changed.

    ``evaluate_3d``: also fuse the ground-truth depth maps (as ``save_groundtruth`` does; its mesh file is written only with that flag),
    keep that surface's vertices on the device, score the system's surface against them (``TSDFVolume.score_against`` with
    ``threshold_3d`` metres), print the six metrics on one line and save them as ``<mesh name of the system>_errors3d.npz``: ``arr_0``
    float32 [6], ``names``, ``counts`` int64 [2] (vertices of the prediction and of the ground truth) and ``threshold``.  Without the flag
    the program writes what it writes without it, byte for byte.

    ``evaluate_3d_density`` (points per square metre), ``evaluate_3d_voxel`` (metres), ``groundtruth_mesh`` (a .ply file), each with
    ``evaluate_3d``: the usual evaluation protocol instead of the vertex-to-vertex one.  With a density both surfaces are sampled on their
    faces, with a voxel both point sets are down-sampled to one point per voxel (``TSDFVolume.score_against``); with a ground-truth mesh
    (``TSDFFusion.meshread``) the system's surface is scored against that mesh, the ground-truth depth maps are not fused for the score
    (and not even loaded unless another flag needs them).  With any of the three, ``_errors3d.npz`` additionally holds ``sample_density``
    and ``voxel`` (NaN where not given) and ``points`` int64 [2], the sizes of the two point sets that were scored; ``counts`` stays the
    vertices of the two surfaces.  Without them the file is what it is without them, byte for byte.

    ``evaluate_3d_visible`` (needs ``evaluate_3d``, ``groundtruth_mesh`` and ``evaluate_3d_density``): the ground-truth mesh is first
    restricted to what the sequence observed, the faces whose three vertices are each seen by at least ``evaluate_3d_min_views`` of the
    fused keyframes' views at the prediction size (``visible_mesh``: the mesh is rasterised from those views on the device), so that the
    parts of a scan that the camera never faced do not count against completeness and recall.  ``_errors3d.npz`` then also holds
    ``visible_faces`` and ``total_faces``.

    ``evaluate_3d_align`` (metres; needs ``evaluate_3d``): the system's point set is registered to the ground truth's by trimmed ICP with
    that inlier distance before it is scored (``TSDFVolume.score_against(align_distance=...)``), ``evaluate_3d_align_scale`` (needs
    ``evaluate_3d_align``) with a scale.  ``_errors3d.npz`` then also holds ``transform`` float64 [4,4] (system -> ground truth),
    ``align_iterations``, ``align_status`` (an index of ``dvmvs.errors.REGISTRATION_STATUS``), ``align_fitness`` and ``align_rmse`` (of the
    last recorded iteration); they come down with the row, in the one download.  ``groundtruth_transform`` (needs
    ``groundtruth_mesh``): a text file of 16 numbers, the 4x4 that takes the mesh's frame into the dataset's world frame, applied to the
    mesh's vertices (in float64, rounded once) when the mesh is read, before visibility culling and sampling.  Without these flags the
    files are what they are without them, byte for byte.

    ``evaluate_3d_align_plane`` (needs ``evaluate_3d_align``, excludes ``evaluate_3d_align_scale``): the registration is point-to-plane
    (``TSDFVolume.score_against(align_plane=True)``) on normals estimated from the ground truth's point set, from
    ``evaluate_3d_align_neighbours`` nearest points within ``evaluate_3d_align_normal_distance`` metres (None: any distance).
    ``align_status`` is then an index of ``dvmvs.errors.REGISTRATION_PLANE_STATUS``, ``align_rmse`` the RMSE of the plane residual, and
    ``_errors3d.npz`` also holds ``align_status_name`` and ``align_rmse_point``.

    ``filter_consistency``: after the masks above, the keyframe predictions go up once and are filtered by multi-view geometric consistency
    in one launch (``dvmvs.consistency.filter_depths``): a pixel is kept, with its own depth, where at least ``consistency_views`` of the
    ``consistency_sources`` keyframes nearest to it in keyframe order (never across a "TRACKING LOST" line) agree within
    ``consistency_pixel`` pixels and ``consistency_relative`` of the depth.  The filtered predictions come down and are fused as before; the
    volume bounds are still those of the UNFILTERED predictions, so the meshes with and without the filter share a grid.  The system's mesh
    and the files of ``evaluate_3d`` and ``render_keyframes`` are written under ``<system_name>+consistent``; the kept share of the valid
    pixels is printed.  ``save_point_cloud`` (needs ``filter_consistency``): also writes ``<mesh name>_pointcloud.ply``, the kept pixels of
    a second call that averages the agreeing depths, as coloured world-space points.  Without these flags the program writes what it
    writes without them, byte for byte.

    ``clean_mesh_area`` (square metres), ``clean_mesh_faces`` (a count), ``clean_mesh_largest``: the system's mesh goes through
    ``dvmvs.components.filter_components`` on the device, which removes the connected components (floaters) with less area or fewer faces
    and, with ``clean_mesh_largest``, all but the largest (``ComponentFilter``).  With any of the three the system's files are written
    under ``<system_name>+clean`` (after ``+consistent`` when both are given), its ``.ply`` files, the progressive ones included, are the
    cleaned meshes, and ``evaluate_3d`` scores the cleaned surface; ``_errors3d.npz`` then also holds ``clean_min_area``,
    ``clean_min_faces``, ``clean_largest`` and ``clean_faces`` int64 [2], the kept and all faces of the system's mesh.  The ground-truth
    side is never cleaned, and ``render_keyframes`` ray-casts the VOLUME, which cleaning a mesh does not touch: its depth maps are what
    they are without these flags (under the ``+clean`` name).  Without these flags every file is what it is without them, byte for byte.

    ``clean_points_neighbours`` (a count, 1 .. 32) with ``clean_points_ratio`` and ``clean_points_max_distance`` (metres),
    ``clean_points_radius`` (metres) with ``clean_points_min_neighbours`` (each needs ``save_point_cloud``): the fused point cloud goes
    through ``dvmvs.outliers.filter_outliers`` on the device before it comes down (``OutlierFilter``).  The first removes the points whose
    mean distance to their ``clean_points_neighbours`` nearest points is more than ``clean_points_ratio`` sample deviations above the
    cloud's mean (statistical outlier removal; ``clean_points_max_distance`` bounds the neighbour search, which otherwise follows a far
    outlier until it has its neighbours, and a point without a neighbour inside it is removed), the second those with fewer than
    ``clean_points_min_neighbours`` points within ``clean_points_radius``; with both, the second runs on what the first keeps.  The
    filtered cloud is written ADDITIONALLY as ``<mesh name>_pointcloud_clean.ply`` and the kept share of the points is printed;
    ``_pointcloud.ply`` and every other file are what they are without these flags, byte for byte.

    ``point_normals_neighbours`` (a count, 3 .. 32) with ``point_normals_max_distance`` (metres; None: unbounded), each needing
    ``save_point_cloud``: the point cloud, the cleaned one where ``clean_points_*`` are given and the fused one otherwise, gets oriented
    normals on the device (``dvmvs.normals.estimate_normals``): the direction of least spread of each point's ``point_normals_neighbours``
    nearest points within ``point_normals_max_distance``, the point itself among them, turned toward the camera centre of the keyframe
    the point came from (``dvmvs.consistency.fused_point_views``).  The cloud with its normals is written ADDITIONALLY as
    ``<mesh name>_pointcloud_normals.ply`` (``TSDFFusion.pcwrite_normals``), without the points that have no valid normal (fewer than
    three neighbours within the distance, or all of them in one place), and the share of valid points is printed; every other file is
    what it is without these flags, byte for byte.

    ``point_mesh_voxel`` (metres) with ``point_mesh_radius`` (metres; None: 2.5 voxels), ``point_mesh_neighbours`` (1 .. 32) and
    ``point_mesh_min_neighbours``, needing ``filter_consistency``, ``save_point_cloud`` and ``point_normals_neighbours``: the cloud that
    ``_pointcloud_normals.ply`` holds is meshed on the device (``dvmvs.implicit.mesh_points_device``: the implicit moving-least-squares
    signed distance of the oriented points on a grid of ``point_mesh_voxel``, with weights that reach zero at ``point_mesh_radius``, then
    marching cubes, without the crossings at the edge of the band around the points) and written ADDITIONALLY as
    ``<mesh name>_pointcloud_mesh.ply`` (``TSDFFusion.meshwrite``; normals and colours are those of the nearest point); with
    ``clean_mesh_*`` that mesh goes through the same component filter.  Every other file is what it is without these flags, byte for
    byte."""
    clean = _clean_filter(clean_mesh_area, clean_mesh_faces, clean_mesh_largest)
    clean_points = _clean_points_filter(save_point_cloud, clean_points_neighbours, clean_points_ratio, clean_points_max_distance,
                                        clean_points_radius, clean_points_min_neighbours)
    point_normals = _point_normals_settings(save_point_cloud, point_normals_neighbours, point_normals_max_distance)
    point_mesh = _point_mesh_settings(filter_consistency, save_point_cloud, point_normals, point_mesh_voxel, point_mesh_radius,
                                      point_mesh_neighbours, point_mesh_min_neighbours)
    if save_point_cloud and not filter_consistency:
        raise ValueError("save_point_cloud needs filter_consistency: the point cloud is made of the pixels the filter keeps")
    protocol_3d = evaluate_3d_density is not None or evaluate_3d_voxel is not None or groundtruth_mesh is not None
    if protocol_3d and not evaluate_3d:
        raise ValueError("evaluate_3d_density, evaluate_3d_voxel and groundtruth_mesh say how evaluate_3d scores: they need evaluate_3d")
    if evaluate_3d_visible and not (evaluate_3d and groundtruth_mesh is not None and evaluate_3d_density is not None):
        raise ValueError("evaluate_3d_visible culls a ground-truth mesh whose kept faces are then sampled: it needs evaluate_3d, "
                         "groundtruth_mesh and evaluate_3d_density")
    if int(evaluate_3d_min_views) != 1 and not evaluate_3d_visible:
        raise ValueError("evaluate_3d_min_views says how evaluate_3d_visible culls: it needs evaluate_3d_visible")
    if int(evaluate_3d_min_views) < 1:
        raise ValueError(f"evaluate_3d_min_views must be at least 1, got {evaluate_3d_min_views}")
    if evaluate_3d_align is not None and not evaluate_3d:
        raise ValueError("evaluate_3d_align registers the surface that evaluate_3d scores: it needs evaluate_3d")
    if evaluate_3d_align_scale and evaluate_3d_align is None:
        raise ValueError("evaluate_3d_align_scale says how evaluate_3d_align registers: it needs evaluate_3d_align")
    if evaluate_3d_align_plane and (evaluate_3d_align is None or evaluate_3d_align_scale):
        raise ValueError("evaluate_3d_align_plane says how evaluate_3d_align registers, a rigid motion: it needs evaluate_3d_align and excludes "
                         "evaluate_3d_align_scale")
    if not evaluate_3d_align_plane and (int(evaluate_3d_align_neighbours) != 20 or evaluate_3d_align_normal_distance is not None):
        raise ValueError("evaluate_3d_align_neighbours and evaluate_3d_align_normal_distance say how evaluate_3d_align_plane estimates normals: "
                         "they need evaluate_3d_align_plane")
    align_plane = None
    if evaluate_3d_align_plane:
        align_plane = {"align_plane": True, "align_normal_neighbours": int(evaluate_3d_align_neighbours),
                       "align_normal_distance": np.inf if evaluate_3d_align_normal_distance is None else float(evaluate_3d_align_normal_distance)}
    if groundtruth_transform is not None and groundtruth_mesh is None:
        raise ValueError("groundtruth_transform moves the mesh of groundtruth_mesh: it needs groundtruth_mesh")
    if evaluate_3d_align is not None and not float(evaluate_3d_align) > 0.0:
        raise ValueError(f"evaluate_3d_align must be a positive distance, got {evaluate_3d_align}")
    fuse_groundtruth_3d = evaluate_3d and groundtruth_mesh is None
    from dvmvs.dataset_loader import PreprocessImage, load_depth_png, load_image, load_image_u8, resize_nearest
    if device_preprocess:
        load_image = load_image_u8       # resize_nearest only selects pixels: the uint8 values are those of the float path's astype
    scene_folder = os.path.join(data_folder, dataset_name, scene_name)
    original_K = np.loadtxt(os.path.join(scene_folder, "K.txt")).astype(np.float32)
    all_poses = np.fromfile(os.path.join(scene_folder, "poses.txt"), dtype=float, sep="\n ").reshape((-1, 4, 4))
    all_image_filenames = sorted(glob.glob(os.path.join(scene_folder, "images", "*.png")))

    pattern = f"keyframe_{dataset_name}_{system_name}_predictions_{scene_name}*"
    prediction_files = glob.glob(os.path.join(prediction_folder, pattern))
    if not prediction_files:
        raise FileNotFoundError(f"no prediction file {pattern} in {prediction_folder}")
    predictions = np.load(prediction_files[0])["arr_0"]
    prediction_height, prediction_width = np.shape(predictions[0])

    nmeas = system_name.split("_")[2]
    with open(os.path.join(data_folder, "indices", f"keyframe+{dataset_name}+{scene_name}+nmeas+{nmeas}")) as f:
        keyframe_lines = [line.rstrip("\n") for line in f if line.strip()]
    keyframe_poses, keyframe_image_filenames, keyframe_segments = [], [], []
    segment = 0
    for line in keyframe_lines:
        if line == "TRACKING LOST":
            segment += 1
            continue
        keyframe_segments.append(segment)
        image_filename = os.path.join(scene_folder, "images", line.split(" ")[0])
        keyframe_poses.append(all_poses[all_image_filenames.index(image_filename)])
        keyframe_image_filenames.append(image_filename)

    first = load_image(all_image_filenames[0])
    preprocessor = PreprocessImage(K=original_K, old_width=first.shape[1], old_height=first.shape[0], new_width=prediction_width,
                                   new_height=prediction_height, distortion_crop=0, perform_crop=False)
    scaled_K = preprocessor.get_updated_intrinsics()

    # ScanNet frames have black, undistorted-away borders: predictions there are masked
    edge = 10
    edge_mask = np.zeros((prediction_height, prediction_width), dtype=bool)
    edge_mask[:edge, :] = edge_mask[-edge:, :] = True
    edge_mask[:, :edge] = edge_mask[:, -edge:] = True
    keyframe_images, keyframe_predictions = [], []
    for index, image_filename in enumerate(keyframe_image_filenames):
        image = resize_nearest(load_image(image_filename), prediction_width, prediction_height)
        prediction = predictions[index]
        if "scannet" in dataset_name:
            prediction[np.logical_and(np.mean(image.astype(float), axis=-1) < 10.0, edge_mask)] = 0.0
        prediction[prediction > max_depth] = 0.0
        keyframe_predictions.append(prediction)
        keyframe_images.append(image.astype(np.uint8))

    groundtruths = None
    if use_groundtruth_to_anchor or save_groundtruth or fuse_groundtruth_3d:
        groundtruths = []
        for filename in sorted(glob.glob(os.path.join(scene_folder, "depth", "*.png"))):
            depth = load_depth_png(filename)
            depth[depth > max_depth] = 0.0
            groundtruths.append(depth)
    if use_groundtruth_to_anchor:
        volume_bounds = TSDFFusion.calculate_volume_bounds(groundtruths, all_poses, original_K)
    else:
        volume_bounds = TSDFFusion.calculate_volume_bounds(keyframe_predictions, keyframe_poses, scaled_K)
    volume_bounds *= 1.05      # margin for errors in the bounds

    point_cloud = clean_point_cloud = normals_point_cloud = point_cloud_mesh = None
    if filter_consistency:
        system_name = f"{system_name}+consistent"
        if keyframe_predictions:
            keyframe_predictions, point_cloud, clean_point_cloud, normals_point_cloud, point_cloud_mesh = _filter_keyframes(
                keyframe_predictions, keyframe_images if save_point_cloud else None, keyframe_poses, scaled_K, keyframe_segments,
                consistency_views, consistency_sources, consistency_pixel, consistency_relative, device, clean_points, point_normals,
                None if point_mesh is None else point_mesh + (clean,))

    if clean is not None:
        system_name = f"{system_name}+clean"
    os.makedirs(reconstruction_folder, exist_ok=True)
    groundtruth_vertices = None
    if save_groundtruth or fuse_groundtruth_3d:
        volume = TSDFVolume(volume_bounds, voxel_size=voxel_size, device=device)
        images = [load_image(f).astype(np.uint8) for f in all_image_filenames]
        if save_groundtruth:
            TSDFFusion.integrate(volume, images, groundtruths, all_poses, original_K,
                                 _mesh_name(reconstruction_folder, voxel_size, max_depth, use_groundtruth_to_anchor, "GROUNDTRUTH",
                                            dataset_name, scene_name), save_progressive=False)
        else:      # the same fusion, without its mesh file
            for image, depth, pose in zip(images, groundtruths, all_poses):
                volume.integrate(image, depth, original_K, pose, obs_weight=1.0)
        if fuse_groundtruth_3d:       # stay on the device when the volume goes
            groundtruth_vertices = volume.mesh_tensors() if protocol_3d else volume.vertices()
        del volume
    if evaluate_3d and groundtruth_mesh is not None:
        mesh_verts, mesh_faces = TSDFFusion.meshread(groundtruth_mesh)
        if groundtruth_transform is not None:
            mesh_verts = apply_transform(mesh_verts, load_transform(groundtruth_transform))
        groundtruth_vertices = tuple(torch.as_tensor(a, device=device) for a in (mesh_verts, mesh_faces))
    volume = TSDFVolume(volume_bounds, voxel_size=voxel_size, device=device)
    system_mesh_name = _mesh_name(reconstruction_folder, voxel_size, max_depth, use_groundtruth_to_anchor, system_name, dataset_name, scene_name)
    TSDFFusion.integrate(volume, keyframe_images, keyframe_predictions, keyframe_poses, scaled_K, system_mesh_name, save_progressive, clean=clean)
    if save_point_cloud:
        print("Saving point cloud to", system_mesh_name + "_pointcloud.ply")
        TSDFFusion.pcwrite(system_mesh_name + "_pointcloud.ply", point_cloud if point_cloud is not None else np.zeros((0, 6), np.float32))
        if clean_points is not None:
            print("Saving cleaned point cloud to", system_mesh_name + "_pointcloud_clean.ply")
            TSDFFusion.pcwrite(system_mesh_name + "_pointcloud_clean.ply",
                               clean_point_cloud if clean_point_cloud is not None else np.zeros((0, 6), np.float32))
        if point_normals is not None:
            print("Saving point cloud with normals to", system_mesh_name + "_pointcloud_normals.ply")
            TSDFFusion.pcwrite_normals(system_mesh_name + "_pointcloud_normals.ply",
                                       *(normals_point_cloud if normals_point_cloud is not None
                                         else (np.zeros((0, 6), np.float32), np.zeros((0, 3), np.float32))))
        if point_mesh is not None:
            print("Saving mesh of the point cloud to", system_mesh_name + "_pointcloud_mesh.ply")
            TSDFFusion.meshwrite(system_mesh_name + "_pointcloud_mesh.ply",
                                 *(point_cloud_mesh if point_cloud_mesh is not None
                                   else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32),
                                         np.zeros((0, 3), np.uint8))))
    if evaluate_3d:
        if protocol_3d:
            visible_from = None
            if evaluate_3d_visible:
                if not keyframe_poses:
                    raise ValueError("evaluate_3d_visible: the scene has no keyframe to take the visibility from")
                visible_from = (scaled_K, np.stack(keyframe_poses), prediction_height, prediction_width, int(evaluate_3d_min_views))
            _evaluate_3d_protocol(volume, groundtruth_vertices, threshold_3d, system_mesh_name, evaluate_3d_density, evaluate_3d_voxel,
                                  visible_from, evaluate_3d_align, evaluate_3d_align_scale, clean=clean, align_plane=align_plane)
        else:
            _evaluate_3d(volume, groundtruth_vertices, threshold_3d, system_mesh_name, evaluate_3d_align, evaluate_3d_align_scale, clean=clean,
                         align_plane=align_plane)
    if render_keyframes:
        _render_keyframes(volume, keyframe_poses, keyframe_image_filenames, scaled_K, preprocessor, prediction_height, prediction_width,
                          scene_folder, f"keyframe_{dataset_name}_{system_name}+tsdf", scene_name, reconstruction_folder)


def _filter_keyframes(predictions, images, poses, K, segments, min_views, n_sources, pixel_threshold, relative_threshold, device,
                      clean_points=None, point_normals=None, point_mesh=None):
    """The keyframe predictions filtered by consistency (a list of host arrays, as they came) and, with ``images``, the fused point cloud
    [P,6] xyzrgb on the host, with ``clean_points`` (an ``OutlierFilter``) also the rows of it that the filter keeps, chosen on the
    device, with ``point_normals`` (``(neighbours, max_distance)``) also ``(xyzrgb [Q,6], normals [Q,3])``: the points of the cleaned
    cloud (of the fused one without ``clean_points``) that have a valid normal, oriented toward the camera centre of their keyframe, and
    with ``point_mesh`` (``(voxel, radius, neighbours, min_neighbours, clean)``) also the mesh of those points and normals
    (``mesh_points_device``) as the four host arrays of ``TSDFFusion.meshwrite``."""
    from dvmvs.consistency import filter_depths, fused_point_cloud, fused_point_views, nearest_sources
    depths = torch.as_tensor(np.stack(predictions).astype(np.float32), device=device)
    cameras = torch.as_tensor(np.stack(poses).astype(np.float32), device=device)
    sources = torch.as_tensor(nearest_sources(len(predictions), n_sources, segments), device=device)
    thresholds = dict(pixel_threshold=pixel_threshold, relative_threshold=relative_threshold, min_views=min_views)
    kept, _, _ = filter_depths(depths, K, cameras, sources, average=False, with_count=False, **thresholds)
    valid = torch.isfinite(depths) & (depths > 0)
    print("Consistency filter: kept {:.1f} % of the valid pixels of {} keyframes".format(
        100.0 * float((kept > 0).sum()) / max(int(valid.sum()), 1), len(predictions)))
    cloud = clean_cloud = normals_cloud = cloud_mesh = None
    if images is not None:
        averaged, _, points = filter_depths(depths, K, cameras, sources, average=True, with_count=False, with_points=True, **thresholds)
        cloud = fused_point_cloud(averaged, points, np.stack(images))
        oriented = cloud                                                  # the cloud that gets the normals, on the device
        if clean_points is not None:
            from dvmvs.outliers import filter_outliers_device
            oriented, keep = filter_outliers_device(cloud, clean_points, return_mask=True)
            clean_cloud = oriented.cpu().numpy()
            print("Outlier filter: kept {:.1f} % of the {} points of the cloud".format(
                100.0 * len(clean_cloud) / max(int(cloud.shape[0]), 1), int(cloud.shape[0])))
        if point_normals is not None:
            from dvmvs.normals import estimate_normals_device
            views = fused_point_views(averaged)
            if clean_points is not None:
                views = views[keep]
            normals, _, valid = estimate_normals_device(oriented[:, :3], point_normals[0], point_normals[1], cameras[:, :3, 3], views)
            normals_cloud = (oriented[valid].cpu().numpy(), normals[valid].cpu().numpy())
            print("Point normals: {:.1f} % of the {} points have a valid normal".format(
                100.0 * len(normals_cloud[0]) / max(int(oriented.shape[0]), 1), int(oriented.shape[0])))
            if point_mesh is not None and len(normals_cloud[0]) > 0:
                from dvmvs.implicit import mesh_points_device
                voxel, radius, neighbours, min_neighbours, clean = point_mesh
                cloud_mesh = tuple(a.cpu().numpy() for a in mesh_points_device(oriented[valid], normals[valid], voxel, radius, neighbours,
                                                                                min_neighbours, clean=clean))
                print("Point mesh: {} vertices and {} faces from {} points".format(len(cloud_mesh[0]), len(cloud_mesh[1]),
                                                                                   len(normals_cloud[0])))
        cloud = cloud.cpu().numpy()
    return list(kept.cpu().numpy()), cloud, clean_cloud, normals_cloud, cloud_mesh


def load_transform(filename):
    """The float64 4x4 of a ``groundtruth_transform`` file: 16 numbers separated by white space, row by row, on any number of lines."""
    with open(filename) as f:
        words = f.read().split()
    try:
        values = np.array([float(w) for w in words], dtype=np.float64)
    except ValueError:
        values = np.zeros(0)
    if values.size != 16 or not np.isfinite(values).all():
        raise ValueError(f"groundtruth_transform: {filename} must hold the 16 finite numbers of a 4x4 matrix")
    return values.reshape(4, 4)


def apply_transform(verts, transform):
    """Mesh vertices [V,3] moved by a float64 4x4 (affine: its last row is not used), evaluated in float64 and rounded to float32 once."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    return (verts @ transform[:3, :3].T + transform[:3, 3]).astype(np.float32)


def _aligned_score(volume, align_distance, align_scale, align_plane=None, **score):
    """``score_against`` with its row on the host; with ``align_distance`` also the entries ``_errors3d.npz`` gains.  Row, transform and
    record come down as ONE float64 tensor (a float32 row is exact in float64).  ``align_plane``: None, or ``score_against``'s
    point-to-plane keywords; the entries then include the point RMSE and the status name."""
    if align_distance is None:
        result = volume.score_against(**score)
        return (result[0].cpu().numpy(),) + tuple(result[1:]) + ({},)
    score = {"return_sizes": False, "sample_density": None, "voxel": None, "visible_from": None, **score}
    plane = align_plane is not None
    result, info = volume._score_against(align_distance=align_distance, align_scale=False if plane else align_scale,
                                         return_transform=True, **(align_plane or {}), **score)
    last = (info["iterations"] - 1).clamp(min=0).reshape(1)      # (selected on the device: indexing with a 0-d tensor would read it)
    record = ("fitness", "rmse", "rmse_point") if plane else ("fitness", "rmse")
    down = torch.cat([result[0].double(), result[-1].reshape(-1), info["iterations"].double().reshape(1), info["status"].double().reshape(1)]
                     + [info[key].index_select(0, last) for key in record]).cpu().numpy()
    extra = {"transform": down[6:22].reshape(4, 4), "align_iterations": np.int64(down[22]), "align_status": np.int64(down[23]),
             "align_fitness": np.float64(down[24]), "align_rmse": np.float64(down[25])}
    from dvmvs.errors import REGISTRATION_PLANE_STATUS, REGISTRATION_STATUS
    name = (REGISTRATION_PLANE_STATUS if plane else REGISTRATION_STATUS)[int(down[23])]
    if plane:                                                    # with the point RMSE and the status name
        extra.update(align_rmse_point=np.float64(down[26]), align_status_name=np.array(name))
        print("Registered the surface to the ground truth within {} m, point to plane: {} after {} iterations, fitness {:.4f}, plane rmse {:.5f} "
              "m, point rmse {:.5f} m".format(align_distance, name, int(down[22]), down[24], down[25], down[26]))
    else:
        print("Registered the surface to the ground truth within {} m{}: {} after {} iterations, fitness {:.4f}, rmse {:.5f} m".format(
            align_distance, " with scale" if align_scale else "", name, int(down[22]), down[24], down[25]))
    return (down[:6].astype(np.float32),) + tuple(result[1:-1]) + (extra,)


def _clean_filter(clean_mesh_area, clean_mesh_faces, clean_mesh_largest):
    """The ``ComponentFilter`` of ``run``'s three settings, None when none is given; each refusal names its flag."""
    if not isinstance(clean_mesh_largest, bool):
        raise ValueError(f"clean_mesh_largest must be a bool, got {clean_mesh_largest!r}")
    if clean_mesh_area is not None and not float(clean_mesh_area) >= 0.0:
        raise ValueError(f"clean_mesh_area must be an area in square metres, not negative or NaN, got {clean_mesh_area}")
    if clean_mesh_faces is not None and not (float(clean_mesh_faces) >= 0.0 and float(clean_mesh_faces).is_integer()):
        raise ValueError(f"clean_mesh_faces must be a whole number of faces, not negative, got {clean_mesh_faces}")
    if clean_mesh_area is None and clean_mesh_faces is None and not clean_mesh_largest:
        return None
    from dvmvs.components import ComponentFilter, filter_settings
    clean = ComponentFilter(0.0 if clean_mesh_area is None else float(clean_mesh_area), 0 if clean_mesh_faces is None else int(clean_mesh_faces),
                            clean_mesh_largest)
    try:
        filter_settings(clean)
    except ValueError as e:
        raise ValueError(f"clean_mesh_area / clean_mesh_faces: {e}") from None
    return clean


def _clean_points_filter(save_point_cloud, neighbours, ratio, max_distance, radius, min_neighbours):
    """The ``OutlierFilter`` of ``run``'s five ``clean_points_*`` settings, None when none is given; each refusal names its flag."""
    def number(value):
        return not isinstance(value, bool) and isinstance(value, (int, float, np.integer, np.floating))
    if not number(ratio) or not 0.0 <= float(ratio) < np.inf:
        raise ValueError(f"clean_points_ratio must be a finite number of deviations, not negative, got {ratio!r}")
    if neighbours is not None and not (number(neighbours) and float(neighbours).is_integer() and 1 <= int(neighbours) <= 32):
        raise ValueError(f"clean_points_neighbours must be a whole number of neighbours in [1, 32], got {neighbours!r}")
    if max_distance is not None and not (number(max_distance) and float(max_distance) > 0.0):
        raise ValueError(f"clean_points_max_distance must be a positive distance in metres, got {max_distance!r}")
    if radius is not None and not (number(radius) and 0.0 <= float(radius) < np.inf):
        raise ValueError(f"clean_points_radius must be a finite distance in metres, not negative, got {radius!r}")
    if min_neighbours is not None and not (number(min_neighbours) and float(min_neighbours).is_integer() and 1 <= int(min_neighbours) < 2 ** 31):
        raise ValueError(f"clean_points_min_neighbours must be a whole number of neighbours, at least 1, got {min_neighbours!r}")
    if float(ratio) != 2.0 and neighbours is None:
        raise ValueError("clean_points_ratio says how clean_points_neighbours filters: it needs clean_points_neighbours")
    if max_distance is not None and neighbours is None:
        raise ValueError("clean_points_max_distance bounds the search of clean_points_neighbours: it needs clean_points_neighbours")
    if radius is not None and min_neighbours is None:
        raise ValueError("clean_points_radius needs clean_points_min_neighbours, the neighbours a point must have within it")
    if min_neighbours is not None and radius is None:
        raise ValueError("clean_points_min_neighbours needs clean_points_radius, the distance its neighbours are counted within")
    if neighbours is None and radius is None:
        return None
    if not save_point_cloud:
        raise ValueError("clean_points_neighbours and clean_points_radius filter the cloud of save_point_cloud: they need save_point_cloud")
    from dvmvs.outliers import OutlierFilter, filter_settings
    clean_points = OutlierFilter(None if neighbours is None else int(neighbours), float(ratio), None if max_distance is None else float(max_distance),
                                 None if radius is None else float(radius), None if min_neighbours is None else int(min_neighbours))
    filter_settings(clean_points)
    return clean_points


def _point_normals_settings(save_point_cloud, neighbours, max_distance):
    """``(neighbours, max_distance)`` of ``run``'s two ``point_normals_*`` settings (``max_distance`` inf when not given), None when neither
    is given; each refusal names its flag."""
    def number(value):
        return not isinstance(value, bool) and isinstance(value, (int, float, np.integer, np.floating))
    if neighbours is not None and not (number(neighbours) and float(neighbours).is_integer() and 3 <= int(neighbours) <= 32):
        raise ValueError(f"point_normals_neighbours must be a whole number of neighbours in [3, 32], got {neighbours!r}")
    if max_distance is not None and not (number(max_distance) and float(max_distance) > 0.0):
        raise ValueError(f"point_normals_max_distance must be a positive distance in metres, got {max_distance!r}")
    if max_distance is not None and neighbours is None:
        raise ValueError("point_normals_max_distance bounds the search of point_normals_neighbours: it needs point_normals_neighbours")
    if neighbours is None:
        return None
    if not save_point_cloud:
        raise ValueError("point_normals_neighbours estimates the normals of the cloud of save_point_cloud: it needs save_point_cloud")
    return int(neighbours), np.inf if max_distance is None else float(max_distance)


def _point_mesh_settings(filter_consistency, save_point_cloud, point_normals, voxel, radius, neighbours, min_neighbours):
    """``(voxel, radius, neighbours, min_neighbours)`` of ``run``'s four ``point_mesh_*`` settings (``radius`` 2.5 voxels when not given), None
    when ``point_mesh_voxel`` is not given; each refusal names its flag."""
    def number(value):
        return not isinstance(value, bool) and isinstance(value, (int, float, np.integer, np.floating))
    if voxel is not None and not (number(voxel) and 0.0 < float(voxel) < np.inf):
        raise ValueError(f"point_mesh_voxel must be a positive voxel size in metres, got {voxel!r}")
    if radius is not None and not (number(radius) and 0.0 < float(radius) < np.inf):
        raise ValueError(f"point_mesh_radius must be a positive distance in metres, got {radius!r}")
    if not (number(neighbours) and float(neighbours).is_integer() and 1 <= int(neighbours) <= 32):
        raise ValueError(f"point_mesh_neighbours must be a whole number of neighbours in [1, 32], got {neighbours!r}")
    if not (number(min_neighbours) and float(min_neighbours).is_integer() and 1 <= int(min_neighbours) < 2 ** 31):
        raise ValueError(f"point_mesh_min_neighbours must be a whole number of neighbours, at least 1, got {min_neighbours!r}")
    if voxel is None:
        if radius is not None or int(neighbours) != 32 or int(min_neighbours) != 3:
            raise ValueError("point_mesh_radius, point_mesh_neighbours and point_mesh_min_neighbours say how point_mesh_voxel meshes: they need "
                             "point_mesh_voxel")
        return None
    if not (filter_consistency and save_point_cloud and point_normals is not None):
        raise ValueError("point_mesh_voxel meshes the cloud with normals of point_normals_neighbours: it needs filter_consistency, "
                         "save_point_cloud and point_normals_neighbours")
    return float(voxel), 2.5 * float(voxel) if radius is None else float(radius), int(neighbours), int(min_neighbours)


def _clean_entries(volume, clean):
    """What ``_errors3d.npz`` gains with a ``ComponentFilter``: its settings and the kept and all faces of the system's mesh (tensor shapes:
    nothing more is read than the extractions read themselves)."""
    if clean is None:
        return {}
    kept, total = int(volume.mesh_tensors(clean=clean)[1].shape[0]), int(volume.mesh_tensors()[1].shape[0])
    print("Mesh cleaned of small components: {} of {} faces kept".format(kept, total))
    return {"clean_min_area": np.float64(clean.min_area), "clean_min_faces": np.int64(clean.min_faces), "clean_largest": np.bool_(clean.keep_largest),
            "clean_faces": np.array([kept, total], dtype=np.int64)}


def _evaluate_3d(volume, groundtruth_vertices, threshold, mesh_name, align_distance=None, align_scale=False, clean=None, align_plane=None):
    """Scores the fused surface against the ground-truth vertices on the device; one row comes down, is printed and saved."""
    from dvmvs.errors import RECONSTRUCTION_METRICS
    cleaning = {} if clean is None else {"clean": clean}
    row, sizes, aligned = _aligned_score(volume, align_distance, align_scale, align_plane, reference=groundtruth_vertices, threshold=threshold,
                                         return_sizes=True, **cleaning)
    print("3-D metrics at {} m over {} predicted and {} ground-truth vertices: {}".format(
        threshold, sizes[0], sizes[1], ", ".join(f"{n} {v:.4f}" for n, v in zip(RECONSTRUCTION_METRICS, row))))
    np.savez_compressed(mesh_name + "_errors3d.npz", arr_0=row, names=np.array(RECONSTRUCTION_METRICS),
                        counts=np.array(sizes, dtype=np.int64), threshold=np.float32(threshold), **aligned, **_clean_entries(volume, clean))


def _evaluate_3d_protocol(volume, groundtruth_mesh, threshold, mesh_name, sample_density, voxel, visible_from=None, align_distance=None,
                          align_scale=False, clean=None, align_plane=None):
    """``_evaluate_3d`` against a ground-truth mesh (device verts and faces), with face sampling and / or voxel down-sampling of both sides;
    with ``visible_from`` (``TSDFVolume.score_against``) against the part of the mesh those views observed."""
    from dvmvs.errors import RECONSTRUCTION_METRICS
    extra = {}
    score = dict(reference=groundtruth_mesh, threshold=threshold, return_sizes=True, sample_density=sample_density, voxel=voxel)
    if clean is not None:
        score["clean"] = clean
    if visible_from is None:
        row, points, aligned = _aligned_score(volume, align_distance, align_scale, align_plane, **score)
    else:
        row, points, kept, aligned = _aligned_score(volume, align_distance, align_scale, align_plane, visible_from=visible_from, **score)
        print("Ground truth restricted to what {} keyframes saw: {} of {} faces".format(len(visible_from[1]), kept[0], kept[1]))
        extra = {"visible_faces": np.int64(kept[0]), "total_faces": np.int64(kept[1])}
    sizes = (int(volume.vertices(clean=clean).shape[0]), int(groundtruth_mesh[0].shape[0]))
    print("3-D metrics at {} m over {} predicted and {} ground-truth points (density {}, voxel {}; {} and {} vertices): {}".format(
        threshold, points[0], points[1], sample_density, voxel, sizes[0], sizes[1],
        ", ".join(f"{n} {v:.4f}" for n, v in zip(RECONSTRUCTION_METRICS, row))))
    np.savez_compressed(mesh_name + "_errors3d.npz", arr_0=row, names=np.array(RECONSTRUCTION_METRICS),
                        counts=np.array(sizes, dtype=np.int64), threshold=np.float32(threshold),
                        sample_density=np.float64(np.nan if sample_density is None else sample_density),
                        voxel=np.float64(np.nan if voxel is None else voxel), points=np.array(points, dtype=np.int64), **extra, **aligned,
                        **_clean_entries(volume, clean))


def _render_keyframes(volume, poses, image_filenames, K, preprocessor, height, width, scene_folder, system_name, scene_name, save_folder):
    """The fused depth of every keyframe: rendered, saved like predictions and, where ground truth exists, scored on the device."""
    from dvmvs.dataset_loader import load_depth_png
    from dvmvs.errors import compute_errors_device
    from dvmvs.utils import save_predictions, save_results
    if not poses:
        print("No keyframe to render")
        return
    depth, _, _ = volume.render(K, np.stack(poses), height, width, normals=False, colour=False)
    hit = depth > 0
    print("Rendered {} keyframes from the fused volume: {:.1f} % of the pixels hit a surface".format(len(poses), 100.0 * float(hit.float().mean())))
    rendered = depth.cpu().numpy()
    depth_files = [os.path.join(scene_folder, "depth", os.path.basename(f)) for f in image_filenames]
    if os.path.isdir(os.path.join(scene_folder, "depth")) and all(os.path.exists(f) for f in depth_files):
        groundtruths = np.stack([preprocessor.apply_depth(load_depth_png(f)) for f in depth_files]).astype(np.float32)
        gt = torch.from_numpy(groundtruths).to(depth.device)
        gt = torch.where(hit, gt, torch.zeros_like(gt))       # a miss takes no part in the metrics
        rows = compute_errors_device(gt, depth).cpu().numpy()
        save_results(rendered, groundtruths, system_name, scene_name, save_folder, errors=rows)
    else:
        save_predictions(rendered, system_name, scene_name, save_folder)


def build_parser():
    parser = ArgumentParser(description="TSDF reconstruction of a scene from saved keyframe depth predictions (writes .ply meshes)")
    parser.add_argument("--reconstruction_folder", default="./reconstructions", type=str)
    parser.add_argument("--prediction_folder", default="./predictions", type=str)
    parser.add_argument("--data_folder", default=".", type=str)
    parser.add_argument("--dataset_name", default="hololens-dataset", type=str)
    parser.add_argument("--scene_name", default="000", type=str)
    parser.add_argument("--system_name", default="320_256_3_dvmvs_fusionnet_online", type=str)
    parser.add_argument("--voxel_size", default=0.025, type=float)
    parser.add_argument("--max_depth", default=5.0, type=float)
    parser.add_argument("--use_groundtruth_to_anchor", action="store_true",
                        help="compute the volume bounds from the ground-truth depth maps (recommended when they are available)")
    parser.add_argument("--save_progressive", action="store_true", help="also write the mesh after every fused keyframe")
    parser.add_argument("--save_groundtruth", action="store_true", help="also write the reconstruction from the ground-truth depth maps")
    parser.add_argument("--device-preprocess", dest="device_preprocess", action="store_true",
                        help="load the colour images as 8-bit (no float32 round trip); same meshes")
    parser.add_argument("--render_keyframes", action="store_true",
                        help="also ray-cast the fused volume from every keyframe's view and save the fused depth maps (<system>+tsdf)")
    parser.add_argument("--evaluate_3d", action="store_true",
                        help="also fuse the ground-truth depth maps and score the system's mesh against that surface in 3-D on the device "
                             "(accuracy, completeness, chamfer, precision, recall, F-score; saved as <mesh name>_errors3d.npz)")
    parser.add_argument("--threshold_3d", default=0.05, type=float, help="distance threshold of precision / recall / F-score, metres")
    parser.add_argument("--evaluate_3d_density", default=None, type=float,
                        help="with --evaluate_3d: sample both surfaces on their faces, this many points per square metre, instead of taking their vertices")
    parser.add_argument("--evaluate_3d_voxel", default=None, type=float,
                        help="with --evaluate_3d: down-sample both point sets to one point per voxel of this edge, metres")
    parser.add_argument("--groundtruth_mesh", default=None, type=str,
                        help="with --evaluate_3d: score against this .ply mesh (ascii or binary little endian) instead of the fused ground-truth depth maps")
    parser.add_argument("--evaluate_3d_visible", action="store_true",
                        help="with --evaluate_3d, --groundtruth_mesh and --evaluate_3d_density: score against the part of the ground-truth "
                             "mesh that the fused keyframes saw (the mesh is rasterised from their views on the device)")
    parser.add_argument("--evaluate_3d_min_views", default=1, type=int,
                        help="with --evaluate_3d_visible: keyframes that must see each vertex of a ground-truth face for it to be kept")
    parser.add_argument("--evaluate_3d_align", default=None, type=float,
                        help="with --evaluate_3d: register the system's point set to the ground truth's by trimmed ICP with this inlier "
                             "distance, metres, before it is scored (on the device)")
    parser.add_argument("--evaluate_3d_align_scale", action="store_true", help="with --evaluate_3d_align: the registration also finds a scale")
    parser.add_argument("--evaluate_3d_align_plane", action="store_true",
                        help="with --evaluate_3d_align: register point to plane, on normals estimated from the ground truth's points (a rigid "
                             "motion; far fewer iterations on walls and floors)")
    parser.add_argument("--evaluate_3d_align_neighbours", default=20, type=int,
                        help="with --evaluate_3d_align_plane: nearest points a ground-truth normal is estimated from (3 .. 32)")
    parser.add_argument("--evaluate_3d_align_normal_distance", default=None, type=float,
                        help="with --evaluate_3d_align_plane: those points are searched within this distance only, metres")
    parser.add_argument("--groundtruth_transform", default=None, type=str,
                        help="with --groundtruth_mesh: a text file of 16 numbers, the 4x4 that takes the mesh's frame into the dataset's world frame")
    parser.add_argument("--filter_consistency", action="store_true",
                        help="fuse only the pixels that neighbouring keyframes agree on (multi-view geometric consistency, on the device); "
                             "files are written under <system>+consistent")
    parser.add_argument("--consistency_views", default=2, type=int, help="neighbouring keyframes that must agree for a pixel to be kept")
    parser.add_argument("--consistency_sources", default=4, type=int, help="neighbouring keyframes each keyframe is checked against (at most 16)")
    parser.add_argument("--consistency_pixel", default=1.0, type=float, help="largest re-projection error of an agreeing view, pixels")
    parser.add_argument("--consistency_relative", default=0.01, type=float, help="largest relative depth difference of an agreeing view")
    parser.add_argument("--save_point_cloud", action="store_true",
                        help="with --filter_consistency: also write the kept pixels as a coloured point cloud (<mesh name>_pointcloud.ply)")
    parser.add_argument("--point_normals_neighbours", default=None, type=int,
                        help="with --save_point_cloud: oriented normals of the point cloud (the cleaned one with --clean_points_*) on the "
                             "device, from this many nearest neighbours (3 .. 32), turned toward the camera that saw each point; the "
                             "cloud with normals is written additionally as <mesh name>_pointcloud_normals.ply")
    parser.add_argument("--point_normals_max_distance", default=None, type=float,
                        help="with --point_normals_neighbours: neighbours are searched within this distance only, metres (bounds the search; "
                             "a point with fewer than three inside it gets no normal and is left out of the file)")
    parser.add_argument("--point_mesh_voxel", default=None, type=float,
                        help="with --filter_consistency --save_point_cloud --point_normals_neighbours: mesh the point cloud with normals on "
                             "the device (implicit moving-least-squares signed distance on a grid of this voxel size, metres, then marching "
                             "cubes); the mesh is written additionally as <mesh name>_pointcloud_mesh.ply")
    parser.add_argument("--point_mesh_radius", default=None, type=float,
                        help="with --point_mesh_voxel: the distance at which a point's weight reaches zero, metres (default: 2.5 voxels)")
    parser.add_argument("--point_mesh_neighbours", default=32, type=int,
                        help="with --point_mesh_voxel: at most this many nearest points within the radius shape a node (1 .. 32)")
    parser.add_argument("--point_mesh_min_neighbours", default=3, type=int,
                        help="with --point_mesh_voxel: a node with fewer points with a normal within the radius carries no surface")
    parser.add_argument("--clean_points_neighbours", default=None, type=int,
                        help="with --save_point_cloud: statistical outlier removal of the fused cloud on the device, over this many nearest "
                             "neighbours (1 .. 32); the result is written additionally as <mesh name>_pointcloud_clean.ply")
    parser.add_argument("--clean_points_ratio", default=2.0, type=float,
                        help="with --clean_points_neighbours: a point goes when its mean neighbour distance is more than this many sample "
                             "deviations above the cloud's mean")
    parser.add_argument("--clean_points_max_distance", default=None, type=float,
                        help="with --clean_points_neighbours: neighbours are searched within this distance only, metres (bounds the search "
                             "of far outliers; a point without a neighbour inside it goes)")
    parser.add_argument("--clean_points_radius", default=None, type=float,
                        help="with --save_point_cloud and --clean_points_min_neighbours: radius outlier removal of the fused cloud on the "
                             "device, metres (after the statistical filter when both are given)")
    parser.add_argument("--clean_points_min_neighbours", default=None, type=int,
                        help="with --clean_points_radius: a point stays when it has at least this many other points within the radius")
    parser.add_argument("--clean_mesh_area", default=None, type=float,
                        help="remove the connected components of the system's mesh with less area than this, square metres (on the device); "
                             "files are written under <system>+clean")
    parser.add_argument("--clean_mesh_faces", default=None, type=int,
                        help="remove the connected components of the system's mesh with fewer faces than this; files are written under <system>+clean")
    parser.add_argument("--clean_mesh_largest", action="store_true",
                        help="keep only the largest connected component of the system's mesh (by area), if it passes the two thresholds")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    run(**vars(args))


if __name__ == "__main__":
    main()
