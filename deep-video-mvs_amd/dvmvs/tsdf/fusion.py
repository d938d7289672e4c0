"""Fusion of depth maps into a ``TSDFVolume``: ``TSDFFusion``, the reconstruction script's host-side helpers (view frusta, volume bounds,
the frame loop that writes the meshes), and ``LiveFusion``, which fuses a scene's depth maps while the scene runs."""
import time

import numpy as np
import torch

from dvmvs.tsdf import ply
from dvmvs.tsdf.volume import TSDFVolume


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
    def _enclose(bounds, frames):
        """``bounds`` [3,2] grown in place to enclose the view frusta of ``frames`` = iterable of (depth_im, cam_intr, cam_pose)."""
        for depth_im, cam_intr, cam_pose in frames:
            frustum = TSDFFusion.get_view_frustum(depth_im, cam_intr, cam_pose)
            bounds[:, 0] = np.minimum(bounds[:, 0], np.amin(frustum, axis=1))
            bounds[:, 1] = np.maximum(bounds[:, 1], np.amax(frustum, axis=1))
        return bounds

    @staticmethod
    def volume_bounds(frames):
        """Axis-aligned bounds [[x0,x1],[y0,y1],[z0,z1]] enclosing the view frusta of ``frames`` = iterable of
        (depth_im, cam_intr, cam_pose), the way the reference's main loop accumulates them."""
        return TSDFFusion._enclose(np.array([[np.inf, -np.inf]] * 3), frames)

    @staticmethod
    def calculate_volume_bounds(depth_maps, poses, K):
        """Bounds of the view frusta of ``depth_maps`` seen from ``poses`` with intrinsics ``K``, the reconstruction script's way:
        the running min / max start at ZERO, so the world origin is always inside (``volume_bounds`` starts at +-inf)."""
        assert len(depth_maps) == len(poses)
        return TSDFFusion._enclose(np.zeros((3, 2)), ((depth_map, K, pose) for depth_map, pose in zip(depth_maps, poses)))

    @staticmethod
    def frustum_bounds(poses, K, height, width, max_depth):
        """``calculate_volume_bounds`` of depth maps that are ``max_depth`` everywhere, without the maps: the bounds of every view's frustum
        cut at ``max_depth`` (and of the world origin, as there).  They contain the bounds of any depth maps <= ``max_depth`` seen from the
        same poses, so a live run can size its volume before a depth exists."""
        constant = np.full((int(height), int(width)), max_depth)
        return TSDFFusion.calculate_volume_bounds([constant] * len(poses), poses, K)

    # the PLY reader and writers (dvmvs.tsdf.ply), under the names the reference class gives them
    _PLY_TYPES = ply._PLY_TYPES
    _columns = staticmethod(ply._columns)
    meshread = staticmethod(ply.meshread)
    meshwrite = staticmethod(ply.meshwrite)
    pcwrite = staticmethod(ply.pcwrite)
    pcwrite_normals = staticmethod(ply.pcwrite_normals)

    @staticmethod
    def integrate(tsdf_volume, images, depths, poses, K, mesh_name, save_progressive, simplify=None, smooth=None, clean=None):
        """Fuses every (image, depth, pose) with weight 1 and writes ``<mesh_name>_complete.ply`` (with ``save_progressive``,
        also ``<mesh_name>_frame_<i>.ply`` after each frame), like the reconstruction script (:442-462).  ``clean`` (a
        ``dvmvs.components.ComponentFilter``) and ``simplify`` (a ``dvmvs.simplify.SimplifySettings``) are handed to every ``get_mesh`` whose mesh is written, the progressive
        ones included; so is ``smooth`` (a ``dvmvs.smooth.SmoothSettings``)."""
        from dvmvs.tsdf.volume import mesh_stages
        simplify, smooth, clean = mesh_stages(simplify, smooth, clean)
        n = len(images)
        start = time.time()
        for i in range(n):
            print(f"Fusing frame {i + 1}/{n} for {mesh_name}")
            tsdf_volume.integrate(images[i], depths[i], K, poses[i], obs_weight=1.0)
            if save_progressive:
                print("Saving for progressive visuals...")
                TSDFFusion.meshwrite(f"{mesh_name}_frame_{i:05d}.ply", *tsdf_volume.get_mesh(clean=clean, smooth=smooth, simplify=simplify))
        torch.cuda.synchronize(tsdf_volume.device)
        print("Average FPS: {:.2f}".format(n / max(time.time() - start, 1e-9)))
        print("Saving mesh to", mesh_name)
        TSDFFusion.meshwrite(mesh_name + "_complete.ply", *tsdf_volume.get_mesh(clean=clean, smooth=smooth, simplify=simplify))


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
    nothing is allocated or launched for the filter and the volume's bits are those of the unfiltered fusion.

    ``vol_bnds=None``: the extent of the scene is not known, and the frames are fused into a ``SparseTSDFVolume`` (``sparse``; a lattice
    from ``sparse_origin`` and a pool of ``max_bricks`` bricks of 8 x 8 x 8 voxels) instead, which allocates what the frames touch; frames
    before a brick's birth are not applied to it -- the one stated difference from the dense volume, inherent to every hashed volume.
    ``volume`` is then ``sparse.dense()``, a ``TSDFVolume`` over the allocated bricks, made when it is asked for (one host read) and kept
    until the next ``add``; ``get_mesh`` / ``mesh_tensors`` / ``render`` take the surface straight from the sparse volume's pool, without ``dense()``
    (with bounds given: from the dense volume).  The consistency filter works on the depth maps before fusion and is the same in both modes.  With bounds
    given nothing differs from what it was: ``sparse`` is None."""

    def __init__(self, vol_bnds, voxel_size=0.025, max_depth=5.0, batch=8, device="cuda", min_consistent_views=0, consistency_sources=4,
                 pixel_threshold=1.0, relative_threshold=0.01, max_bricks=65536, sparse_origin=(0.0, 0.0, 0.0)):
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
        if vol_bnds is None:
            from dvmvs.tsdf.sparse_volume import SparseTSDFVolume
            self.sparse = SparseTSDFVolume(voxel_size, origin=sparse_origin, max_bricks=max_bricks, device=device)
            self._volume = None                      # sparse.dense(), made by ``volume`` and dropped by ``add``
            self.device = self.sparse.device
        else:
            self.sparse = None
            self._volume = TSDFVolume(vol_bnds, voxel_size, device=device)
            self.device = self._volume._tsdf.device  # with its index ("cuda" -> "cuda:0"): what a tensor's ``.device`` compares equal to
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
        if self.sparse is not None:
            self._volume = None
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
        target = self.sparse if self.sparse is not None else self._volume
        target.integrate_frames(self._rgb[:n], depth, self._K[:n], self._P[:n], obs_weight=self._weights, max_depth=self.max_depth)
        self._weights, self._pending = [], 0

    @property
    def volume(self):
        self.flush()
        if self._volume is None:
            self._volume = self.sparse.dense()
        return self._volume

    def _surface_source(self):
        """What the mesh is extracted from, after a flush: the sparse volume itself where there is one (from its pool, no ``dense()``),
        else the dense volume."""
        self.flush()
        return self.sparse if self.sparse is not None else self._volume

    def get_mesh(self, **stages):
        """``get_mesh`` of the reconstruction so far (``clean=`` / ``smooth=`` / ``simplify=`` as ``TSDFVolume.get_mesh`` takes them), as
        numpy arrays.  Without bounds the surface comes straight from the sparse volume's pool (``SparseTSDFVolume.get_mesh``): ``volume``
        is not made."""
        return self._surface_source().get_mesh(**stages)

    def mesh_tensors(self, **stages):
        """``(verts, faces)`` device tensors of the reconstruction so far; as ``get_mesh``."""
        return self._surface_source().mesh_tensors(**stages)

    def render(self, cam_intr, cam_poses, height, width, **settings):
        """``render`` of the reconstruction so far (``near`` / ``far`` / ``step`` / ``normals`` / ``colour`` / ``skip_empty`` as
        ``TSDFVolume.render`` takes them): pending frames are fused first.  Without bounds the views are ray-cast straight from the sparse
        volume's pool (``SparseTSDFVolume.render``, which also takes ``bounds=``): ``volume`` is not made, so looking at the reconstruction
        while it grows costs no dense copy.  With bounds given: ``TSDFVolume.render`` of the dense volume."""
        return self._surface_source().render(cam_intr, cam_poses, height, width, **settings)
