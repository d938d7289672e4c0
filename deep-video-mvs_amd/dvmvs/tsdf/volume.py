"""The voxel volume on the device: ``TSDFVolume`` (integration, ray-casting, surface extraction) and ``fold_color``."""
import numpy as np
import torch

from dvmvs.hip.volume import marching_cubes, tsdf_integrate
from dvmvs.tsdf.mesh_views import camera_tensors


def fold_color(color_im):
    """[H,W,3] RGB (0..255) -> float32 [H,W] holding b * 65536 + g * 256 + r (run-tsdf-reconstruction.py:236-238)."""
    c = np.asarray(color_im, dtype=np.float32)
    return np.floor(c[..., 2] * np.float32(65536.0) + c[..., 1] * np.float32(256.0) + c[..., 0]).astype(np.float32)


def mesh_stages(*stages):
    """``(simplify, clean)`` of a method's two arguments, or ``(simplify, smooth, clean)`` of its three, as they stand in the signatures.
    ``simplify`` stands before ``clean``, where ``clean`` alone stood before, and ``smooth`` now stands between them, so a settings object
    given by position may arrive in another stage's slot: a ``ComponentFilter`` is the ``clean`` it always was, a ``SimplifySettings`` the
    ``simplify`` and a ``SmoothSettings`` the ``smooth``, wherever they arrive.  Anything else stays in its slot, for the stage's own
    check to refuse; two values for one stage are a ``ValueError``."""
    from dvmvs.components import ComponentFilter
    from dvmvs.simplify import SimplifySettings
    from dvmvs.smooth import SmoothSettings
    names = {2: ("simplify", "clean"), 3: ("simplify", "smooth", "clean")}[len(stages)]
    types = {"simplify": SimplifySettings, "smooth": SmoothSettings, "clean": ComponentFilter}
    placed = {}
    for slot, value in zip(names, stages):
        if value is None:
            continue
        stage = next((name for name in names if isinstance(value, types[name])), slot)
        if stage in placed:
            raise ValueError(f"two values for the stage {stage}: {placed[stage]!r} and {value!r}")
        placed[stage] = value
    return tuple(placed.get(name) for name in names)


def finish_mesh(mesh, simplify, smooth, clean):
    """What follows the extraction, on ``mesh`` = ``(verts, faces, normals, colours or None)`` device tensors, whichever volume they come
    from (``TSDFVolume``, ``SparseTSDFVolume``): with ``clean`` (a ``dvmvs.components.ComponentFilter``) through ``filter_components``,
    then with ``smooth`` (a ``dvmvs.smooth.SmoothSettings``) through ``smooth_mesh``, then with ``simplify`` (a
    ``dvmvs.simplify.SimplifySettings``) through ``simplify_mesh``, all on the device.  The stages are taken as given (``mesh_stages``
    sorts a method's arguments first); a stage that is None is left out."""
    if clean is not None:
        from dvmvs.components import filter_components_device
        mesh = filter_components_device(mesh[0], mesh[1], clean, mesh[2], mesh[3])
    if smooth is not None:
        from dvmvs.smooth import smooth_mesh_device, smooth_settings
        smooth_settings(smooth)
        mesh = smooth_mesh_device(mesh[0], mesh[1], smooth, mesh[2], mesh[3])
    if simplify is not None:
        from dvmvs.simplify import simplify_mesh_device, simplify_settings
        simplify_settings(simplify)
        mesh = simplify_mesh_device(mesh[0], mesh[1], simplify, mesh[2], mesh[3])
    return mesh


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
        self._raycast_mask = None      # (before the call: a failed call may have been enqueued)
        tsdf_integrate(self._tsdf, self._weight, self._color, self._vol_origin, self._voxel_size, K, P, color, depth, self._trunc_margin,
                       obs_weight)

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
        K, P = camera_tensors(cam_intr, cam_poses, dev, frames=n)
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
        K, P = camera_tensors(cam_intr, cam_poses, self.device)
        mask = None
        if skip_empty:
            if self._raycast_mask is None:
                self._raycast_mask = ops.tsdf_raycast_mask(self._tsdf, self._weight)
            mask = self._raycast_mask
        return ops.tsdf_raycast(self._tsdf, self._weight, self._color if colour else None, self._vol_origin, self._voxel_size, K, P, height, width, near=near, far=far, step=step, mask=mask, normals=normals, colour=colour)

    def get_volume(self):
        """(tsdf, colour) as numpy arrays, like the reference; ``get_weight_volume()`` for the weights."""
        return self._tsdf.cpu().numpy(), self._color.cpu().numpy()

    def get_weight_volume(self):
        return self._weight.cpu().numpy()

    def _extract(self, color, clean):
        """``marching_cubes`` of the volume, with ``clean`` (a ``dvmvs.components.ComponentFilter``) through ``filter_components`` on the
        device: the components of the welded mesh that the filter does not keep (floaters) are gone before anything else sees it."""
        mesh = marching_cubes(self._tsdf, 0.0, self._color if color else None, self._vol_origin, self._voxel_size)
        return finish_mesh(mesh, None, None, clean)

    def _surface(self, color, simplify, smooth, clean):
        """``_extract``; with ``smooth`` (a ``dvmvs.smooth.SmoothSettings``) what it leaves through ``smooth_mesh`` on the device; with
        ``simplify`` (a ``dvmvs.simplify.SimplifySettings``) what that leaves through ``simplify_mesh`` on the device: extract -> clean ->
        smooth -> simplify (``finish_mesh``).  Without the two, ``_extract`` and nothing else."""
        simplify, smooth, clean = mesh_stages(simplify, smooth, clean)
        return finish_mesh(self._extract(color, clean), simplify, smooth, None)

    def get_mesh(self, simplify=None, smooth=None, clean=None):
        """(verts [V,3] float32 in world units, faces [F,3] int32, normals [V,3] float32, colours [V,3] uint8 RGB) of the zero
        iso-surface, as numpy arrays (run-tsdf-reconstruction.py:334-351); extracted on the device by ``marching_cubes``.  ``clean``: a
        ``dvmvs.components.ComponentFilter``; the mesh then goes through ``filter_components`` on the device before it is downloaded.
        ``simplify``: a ``dvmvs.simplify.SimplifySettings``; the mesh, cleaned first where ``clean`` is given, then goes through
        ``simplify_mesh`` on the device: one vertex per occupied cell of ``simplify.voxel`` metres, normals and colours merged alongside.
        ``smooth``: a ``dvmvs.smooth.SmoothSettings``; the mesh, after ``clean`` and before ``simplify``, goes through ``smooth_mesh`` on
        the device: the Laplacian or Taubin filter moves the vertices, the normals are recomputed from the smoothed faces, faces and
        colours stay."""
        verts, faces, norms, colors = self._surface(True, simplify, smooth, clean)
        return verts.cpu().numpy(), faces.cpu().numpy(), norms.cpu().numpy(), colors.cpu().numpy()

    def get_point_cloud(self):
        """[N,6] float32: the mesh's vertices (xyz, world units) followed by their colour (rgb) (run-tsdf-reconstruction.py:313-332)."""
        verts, _, _, colors = self.get_mesh()
        return np.hstack([verts, colors])

    def vertices(self, simplify=None, smooth=None, clean=None):
        """The vertices of the zero iso-surface (``get_mesh()[0]``) as a float32 [V,3] DEVICE tensor: nothing but ``marching_cubes``'
        two counts is read by the host (with ``clean``, as ``get_mesh`` takes it, also ``filter_components``' counts; with ``simplify``, as
        ``get_mesh`` takes it, also ``simplify_mesh``'s; ``smooth``, as ``get_mesh`` takes it, reads nothing)."""
        return self._surface(False, simplify, smooth, clean)[0]

    def mesh_tensors(self, simplify=None, smooth=None, clean=None):
        """``(verts float32 [V,3], faces int32 [F,3])`` of the zero iso-surface as DEVICE tensors, as ``marching_cubes`` leaves them (with
        ``clean``, as ``get_mesh`` takes it: as ``filter_components`` leaves them; with ``simplify``, as ``get_mesh`` takes it: as
        ``simplify_mesh`` leaves them; with ``smooth``, as ``get_mesh`` takes it: smoothed between the two)."""
        return self._surface(False, simplify, smooth, clean)[:2]

    def surface_points(self, sample_density=None, voxel=None, simplify=None, smooth=None, clean=None):
        """The point set the 3-D metrics take from this volume's surface, as a float32 [N,3] DEVICE tensor: the vertices of the zero
        iso-surface; with ``sample_density`` (points per square metre) instead ``dvmvs.hip.ops.surface_sample`` of its faces; with ``voxel``
        (metres) then ``dvmvs.hip.ops.voxel_downsample`` of that (``dvmvs.errors.prepare_points`` is the host definition of both).  The
        vertices and faces stay on the device; each step reads its output's size once.  ``clean``: as ``get_mesh`` takes it; the points are
        then those of the cleaned mesh; ``simplify``: as ``get_mesh`` takes it; the points are then those of the simplified mesh;
        ``smooth``: as ``get_mesh`` takes it; the points are then those of the smoothed mesh."""
        from dvmvs.errors import prepare_points_device
        verts, faces = self.mesh_tensors(simplify=simplify, smooth=smooth, clean=clean)
        return prepare_points_device(verts, faces, sample_density, voxel)

    def score_against(self, reference, threshold=0.05, return_sizes=False, sample_density=None, voxel=None, visible_from=None, clean=None,
                      simplify=None, smooth=None, align_plane=False, align_normal_neighbours=20, align_normal_distance=np.inf, align_distance=None,
                      align_scale=False, return_transform=False):
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

        ``simplify``: a ``dvmvs.simplify.SimplifySettings``.  The PREDICTION's mesh, after ``clean``, goes through ``simplify_mesh`` on the
        device before its vertices are taken or its faces sampled: the score is that of the simplified surface.  The reference is never
        simplified.

        ``smooth``: a ``dvmvs.smooth.SmoothSettings``.  The PREDICTION's mesh, after ``clean`` and before ``simplify``, goes through
        ``smooth_mesh`` on the device: the score is that of the smoothed surface.  The reference is never smoothed.

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
        from dvmvs.tsdf.scoring import score_volume      # (scoring sits above this module: it needs TSDFVolume to tell a volume reference)
        return score_volume(self, reference, threshold, return_sizes, sample_density, voxel, visible_from, align_distance, align_scale,
                            return_transform, clean=clean, align_plane=align_plane, align_normal_neighbours=align_normal_neighbours,
                            align_normal_distance=align_normal_distance, simplify=simplify, smooth=smooth)[0]
