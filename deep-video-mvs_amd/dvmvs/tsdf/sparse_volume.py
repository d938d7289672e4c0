"""``SparseTSDFVolume``: a TSDF volume that needs no bounds.  Space is an unbounded lattice of 8 x 8 x 8-voxel
bricks, a hash table on the device maps brick coordinates to existence, a pool of fixed capacity holds the voxels of the bricks that the
frames' truncation bands touched, and only those are updated.  ``dense()`` hands the result to everything that takes a ``TSDFVolume``;
``mesh_tensors`` / ``get_mesh`` and what builds on them extract the surface straight from the pool, and
``render`` ray-casts it from the pool."""
import numpy as np
import torch

from dvmvs.hip import sparse as hip_sparse
from dvmvs.sparse import BRICK, unpack_keys
from dvmvs.tsdf.mesh_views import camera_tensors
from dvmvs.tsdf.volume import TSDFVolume, finish_mesh, fold_color, mesh_stages


class SparseTSDFVolume:
    """Voxel ``v`` (a signed integer triple) lies at ``origin + float(v) * voxel_size``, in float32 as the dense kernel evaluates it, so
    voxel ``v`` here and voxel ``v`` of a dense volume with the same origin see the same floats.  Brick ``b = floor(v / 8)``, ``|b| < 2^20``.
    tsdf starts at 1, weight and colour at 0; truncation = 5 voxels, as in ``TSDFVolume``.

    A frame ALLOCATES the bricks that ``dvmvs.sparse.mark_bricks`` gives for it (a superset of the bricks in which it leaves a tsdf < 1).
    The volume counts the frames it is given, g = 0, 1, ...; a brick's BIRTH is the smallest g of a frame that marks it, and frame g is
    applied to a brick iff g >= birth, with the dense kernel's per-voxel statements, free-space updates included.  FRAMES BEFORE A BRICK'S
    BIRTH ARE NOT APPLIED: that is the one stated difference from the dense volume, inherent to every hashed volume.  The result does not
    depend on how frames are batched into calls, and new bricks get pool slots in ascending key order behind the existing ones, so the
    pool's layout is deterministic.

    The capacity (``max_bricks`` bricks of 6 KiB, ``table_slots`` table entries, default the power of two >= 2 * max_bricks) is fixed at
    construction: ``integrate_frames`` never reallocates and never reads the device.  Bricks beyond the capacity, and marks that find no
    table slot, are dropped and counted; ``overflow`` reads the count, and ``dense()`` raises when it is non-zero unless told otherwise.  In
    the overflowed state which bricks exist is unspecified."""

    def __init__(self, voxel_size, origin=(0.0, 0.0, 0.0), max_bricks=65536, table_slots=None, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SparseTSDFVolume needs a HIP device: there is no CPU integration path in this package")
        if not float(voxel_size) > 0.0 or not np.isfinite(float(voxel_size)):
            raise ValueError(f"SparseTSDFVolume: voxel_size must be positive and finite, got {voxel_size}")
        origin = np.asarray(origin, dtype=np.float32).reshape(-1)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError("SparseTSDFVolume: origin must be three finite numbers")
        self._voxel_size = float(voxel_size)
        self._trunc_margin = 5 * self._voxel_size
        self._origin = origin
        self._state = hip_sparse.SparseState(max_bricks, table_slots, self.device)
        self.device = self._state.tsdf.device
        self.frames = 0                   # frames given so far: the number of the next frame
        self._neighbour = None            # neighbour table of the extraction: describes which bricks exist, so integrate_frames drops it
        self._render_tables = None        # (index, flags) of render(): describe the pool's keys and contents; dropped likewise
        self._render_read = None          # (status, extent) of render(): its one host read per state of the volume; dropped likewise

    voxel_size = property(lambda self: self._voxel_size)
    origin = property(lambda self: self._origin.copy())
    trunc_margin = property(lambda self: self._trunc_margin)
    max_bricks = property(lambda self: self._state.max_bricks)
    table_slots = property(lambda self: self._state.table_slots)

    def integrate_frames(self, color_ims, depth_ims, cam_intr, cam_poses, obs_weight=1.0, max_depth=float("inf")):
        """Fuses N frames (one flush: mark, sort, assign, integrate; five launches and a device sort, nothing read by the host).  Arguments as
        on ``TSDFVolume.integrate_frames``: ``color_ims`` [N,H,W,3] uint8 RGB or [N,H,W] folded colour, ``depth_ims`` [N,H,W] metres,
        ``cam_intr`` [3,3] or [N,3,3], ``cam_poses`` [N,4,4] camera-to-world, ``obs_weight`` one number or N; a depth above ``max_depth``
        counts as invalid.  Contiguous device tensors of the kernel's types are used in place."""
        dev = self.device

        def as_dev(a, dtype):
            if torch.is_tensor(a):
                return a.to(dev, dtype).contiguous()
            return torch.as_tensor(np.ascontiguousarray(a, dtype={torch.float32: np.float32, torch.uint8: np.uint8}[dtype]), device=dev)

        depth = as_dev(depth_ims, torch.float32)
        if depth.dim() != 3:
            raise ValueError(f"depth images must be [N,H,W], got {tuple(depth.shape)}")
        n = depth.shape[0]
        colour_dims = color_ims.dim() if torch.is_tensor(color_ims) else np.ndim(color_ims)
        if colour_dims == 4:
            if color_ims.dtype == (torch.uint8 if torch.is_tensor(color_ims) else np.uint8):
                rgb, folded = as_dev(color_ims, torch.uint8), None
            else:
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
        if hasattr(obs_weight, "tolist"):
            obs_weight = obs_weight.tolist()
        weights = [float(x) for x in obs_weight] if isinstance(obs_weight, (list, tuple)) else [float(obs_weight)] * n
        if len(weights) != n:
            raise ValueError(f"{len(weights)} observation weights for {n} frames")
        max_depth = float(max_depth)
        if max_depth != max_depth:
            raise ValueError("max_depth is NaN")
        first, state = self.frames, self._state
        self.frames += n                  # (before the calls: a failed call may have been enqueued)
        self._neighbour = self._render_tables = self._render_read = None
        hip_sparse.sparse_mark(state, depth, K, P, self._origin, self._voxel_size, self._trunc_margin, max_depth, first)
        hip_sparse.sparse_assign(state)
        hip_sparse.sparse_integrate(state, depth, K, P, rgb, folded, self._origin, self._voxel_size, self._trunc_margin, weights, max_depth,
                                    first)

    def integrate(self, color_im, depth_im, cam_intr, cam_pose, obs_weight=1.0, max_depth=float("inf")):
        """One frame: ``color_im`` [H,W,3] RGB or [H,W] folded, ``depth_im`` [H,W], ``cam_intr`` [3,3], ``cam_pose`` [4,4]."""
        def one(a):
            return a.unsqueeze(0) if torch.is_tensor(a) else np.asarray(a)[None]
        self.integrate_frames(one(color_im), one(depth_im), cam_intr, one(cam_pose), obs_weight=obs_weight, max_depth=max_depth)

    def _status(self):
        return [int(x) for x in self._state.status.cpu()]

    @property
    def n_bricks(self):
        """Bricks allocated (a host read)."""
        return self._status()[hip_sparse.STATUS_BRICKS]

    @property
    def overflow(self):
        """Bricks dropped because the pool was full plus marks dropped because the table was full (a host read); 0 = nothing was lost."""
        status = self._status()
        return status[hip_sparse.STATUS_DROPPED_POOL] + status[hip_sparse.STATUS_DROPPED_TABLE]

    @property
    def rejected_pixels(self):
        """Pixels that marked nothing because a sample left the coordinate range or spanned more than 4 bricks (a host read)."""
        return self._status()[hip_sparse.STATUS_REJECTED_PIXELS]

    def bricks(self):
        """``(coords [n,3] int32, birth [n] int32)`` of the allocated bricks in pool order (host arrays; a host read)."""
        n = self.n_bricks
        return unpack_keys(self._state.pool_key[:n].cpu().numpy()).astype(np.int32), self._state.pool_birth[:n].cpu().numpy()

    def pool(self):
        """The pool's device tensors ``(tsdf, weight, colour)`` [max_bricks, 512], local index x * 64 + y * 8 + z; slots >= n_bricks are
        (1, 0, 0)."""
        return self._state.tsdf, self._state.weight, self._state.color

    def brick_bounds(self, first_brick, last_brick):
        """[[x0,x1],[y0,y1],[z0,z1]] in metres of the box of bricks ``first_brick`` .. ``last_brick`` (inclusive), for ``dense(bounds)``."""
        first, last = np.asarray(first_brick, dtype=np.float64), np.asarray(last_brick, dtype=np.float64)
        size = BRICK * np.float64(np.float32(self._voxel_size))
        o = self._origin.astype(np.float64)
        return np.stack([o + first * size, o + (last + 1) * size], axis=1)

    def _refuse_overflow(self, what, status, allow_overflow):
        lost = status[hip_sparse.STATUS_DROPPED_POOL] + status[hip_sparse.STATUS_DROPPED_TABLE]
        if lost and not allow_overflow:
            raise RuntimeError(f"SparseTSDFVolume.{what}: {status[hip_sparse.STATUS_DROPPED_POOL]} bricks did not fit the pool of "
                               f"{self._state.max_bricks} and {status[hip_sparse.STATUS_DROPPED_TABLE]} marks found no table slot: the volume is "
                               f"incomplete (a larger max_bricks / table_slots, or allow_overflow=True)")

    def _box(self, what, bounds, extent):
        """The brick-aligned box of ``dense()`` and ``render()``, so the two cannot drift: ``(first [3] int64, count [3] int64, low [3]
        float64)`` -- ``bounds`` grown outwards to whole bricks, or without ``bounds`` the box of ``extent`` = (first, last) allocated brick
        per axis (None: no brick).  ``low = origin + first * 8 * voxel``; the box's float32 origin is ``low.astype(float32)`` and its
        dimensions are ``8 * count`` voxels."""
        size = BRICK * np.float64(np.float32(self._voxel_size))
        o = self._origin.astype(np.float64)
        if bounds is None:
            if extent is None:
                raise ValueError(f"SparseTSDFVolume.{what}: no brick is allocated and no bounds were given")
            first, last = (np.asarray(e, dtype=np.int64) for e in extent)
        else:
            bounds = np.asarray(bounds, dtype=np.float64)
            if bounds.shape != (3, 2) or not np.isfinite(bounds).all() or not (bounds[:, 1] > bounds[:, 0]).all():
                raise ValueError(f"SparseTSDFVolume.{what}: bounds must be a finite [[x0,x1],[y0,y1],[z0,z1]] with x1 > x0 ...")
            first = np.floor((bounds[:, 0] - o) / size).astype(np.int64)
            last = np.ceil((bounds[:, 1] - o) / size).astype(np.int64) - 1
        count = (last - first + 1).astype(np.int64)
        if (np.abs(first) > (1 << 20)).any() or (np.abs(last) > (1 << 20)).any():
            raise ValueError(f"SparseTSDFVolume.{what}: the box leaves the lattice's coordinate range")
        return first, count, o + first * size

    def dense(self, bounds=None, allow_overflow=False):
        """A ``TSDFVolume`` over the brick-aligned box of the allocated bricks, or over ``bounds`` ([[x0,x1],[y0,y1],[z0,z1]] in metres,
        grown outwards to whole bricks), holding the allocated bricks' voxels and (1, 0, 0) elsewhere.  This is the one host read of the
        sparse volume's use: the status and the bricks' keys, to size the result.  Everything downstream -- ``get_mesh``, ``render``,
        ``clean=`` / ``smooth=`` / ``simplify=``, ``score_against`` -- is reached through it unchanged.  Raises ``RuntimeError`` when bricks
        were dropped (``overflow``), unless ``allow_overflow``; ``ValueError`` when there is no brick and no ``bounds``.

        The result's origin is ``float32(origin + first_brick * 8 * voxel_size)``, and its voxel ``w`` lies at that origin +
        ``float(w) * voxel_size``.  The VALUES are the pool's, bit for bit.  The POSITIONS are those of the sparse voxels
        (``origin + float(v) * voxel_size``) bit for bit only where the brick offset and the products are exact in float32, e.g. a dyadic
        voxel size and origin; on any other lattice they can differ in the last bits, so a frame integrated into the result afterwards
        may round a voxel at a pixel or truncation boundary the other way than the sparse volume would."""
        state = self._state
        status = self._status()
        n = status[hip_sparse.STATUS_BRICKS]
        self._refuse_overflow("dense", status, allow_overflow)
        extent = None
        if bounds is None and n > 0:
            coords = unpack_keys(state.pool_key[:n].cpu().numpy())
            extent = coords.min(axis=0), coords.max(axis=0)
        first, count, low = self._box("dense", bounds, extent)
        # (the upper bound half a voxel short: TSDFVolume takes ceil((x1 - x0) / voxel) voxels, which is then the brick count times 8)
        volume = TSDFVolume(np.stack([low, low + (count * BRICK - 0.5) * self._voxel_size], axis=1), self._voxel_size, device=self.device)
        if tuple(int(d) for d in volume.vol_dim) != tuple(int(c) * BRICK for c in count):
            raise RuntimeError(f"SparseTSDFVolume.dense: a box of {tuple(int(c) for c in count)} bricks became a volume of {tuple(volume.vol_dim)} voxels")
        hip_sparse.sparse_gather(state, n, volume._tsdf, volume._weight, volume._color, first)
        return volume

    def _render_state(self):
        """``(status, extent)``: the status words and the (first, last) allocated brick per axis (None without a brick), the minimum and
        maximum of the key fields of the slots < n_bricks computed on the device.  ONE host read, kept until the next ``integrate_frames``."""
        if self._render_read is None:
            state = self._state
            with torch.cuda.device(self.device):
                live = torch.arange(state.max_bricks, dtype=torch.int64, device=self.device) < state.status[hip_sparse.STATUS_BRICKS]
                fields = torch.stack([(state.pool_key >> shift) & 0x1FFFFF for shift in (42, 21, 0)], dim=1) - ((1 << 20) - 1)
                low = torch.where(live[:, None], fields, torch.full_like(fields, 1 << 40)).amin(dim=0)
                high = torch.where(live[:, None], fields, torch.full_like(fields, -(1 << 40))).amax(dim=0)
                words = [int(x) for x in torch.cat([state.status, low, high]).cpu()]      # the one host read
            status, low, high = words[:hip_sparse.STATUS_WORDS], words[-6:-3], words[-3:]
            extent = (np.array(low, dtype=np.int64), np.array(high, dtype=np.int64)) if status[hip_sparse.STATUS_BRICKS] > 0 else None
            self._render_read = status, extent
        return self._render_read

    @property
    def brick_extent(self):
        """``(first [3], last [3])`` brick coordinates of the box of the allocated bricks, or None when there is no brick: the box that
        ``render`` takes without ``bounds`` (its one host read, kept until the next ``integrate_frames``)."""
        extent = self._render_state()[1]
        return None if extent is None else (extent[0].copy(), extent[1].copy())

    def render(self, cam_intr, cam_poses, height, width, near=0.0, far=float("inf"), step=1.0, normals=True, colour=True, skip_empty=True,
               bounds=None, allow_overflow=False):
        """``TSDFVolume.render`` of this volume, without a dense copy (csrc/sparse_raycast.hip): for the box that
        ``dense(bounds)`` computes -- ``bounds`` grown outwards to whole bricks, or without ``bounds`` the box of the allocated bricks --
        ``(depth [N,height,width] float32, normals [N,height,width,3] float32 or None, rgb [N,height,width,3] uint8 or None)`` equal BIT FOR
        BIT to ``self.dense(bounds).render(...)`` with the same ``near``, ``far``, ``step``, ``normals``, ``colour`` and ``skip_empty``.
        ``skip_empty`` jumps over unallocated bricks and bricks without a crossing; the result is the same bits either way.

        The host is read at most once per state of the volume (the status words and the box of the allocated bricks, computed on the
        device), and that read, the render index, the bricks' crossing flags and the neighbour table are built on first use and kept until
        the next ``integrate_frames``.  ``RuntimeError`` when bricks were dropped (``overflow``), unless ``allow_overflow``; ``ValueError``
        when there is no brick and no ``bounds``, and when the box is too long to march (pass ``bounds=``).

        Coordinates are BOX-RELATIVE float32: a point of a ray is ``g = (p - box origin) / voxel``.  A caller whose volume has parts far
        apart should pass ``bounds`` around what is looked at: without them the box spans everything, and where ``g`` reaches 2^18 voxels
        the trilinear weights ``g - floor(g)`` have only 2^-5 voxel of resolution left."""
        state = self._state
        status, extent = self._render_state()
        self._refuse_overflow("render", status, allow_overflow)
        first, count, low = self._box("render", bounds, extent)
        step = float(step)
        if not 0.0 < step <= 5.0:
            raise ValueError(f"SparseTSDFVolume.render: step must be in (0, 5] voxels (the truncation), got {step}")
        if (count > 1 << 21).any() or hip_sparse.raycast_steps(count, step) >= hip_sparse.RAYCAST_MAX_STEPS:
            raise ValueError(f"SparseTSDFVolume.render: a box of {tuple(int(c) for c in count)} bricks is too long to march at step {step}: "
                             f"pass bounds= around what is looked at")
        K, P = camera_tensors(cam_intr, cam_poses, self.device)
        if self._render_tables is None:
            index = hip_sparse.sparse_raycast_index(state)
            self._render_tables = index, hip_sparse.sparse_raycast_flags(state, self.neighbours(), index)
        index, flags = self._render_tables
        return hip_sparse.sparse_raycast(state, index, flags, self.neighbours(), first, count, low.astype(np.float32), self._voxel_size, K, P,
                                         height, width, near=near, far=far, step=step, normals=normals, colour=colour, skip_empty=skip_empty)

    def neighbours(self):
        """The neighbour table of the allocated bricks (``dvmvs.hip.sparse.sparse_neighbours``; int32 [max_bricks, 27] on the device),
        built on first use and kept until the next ``integrate_frames``.  No host read."""
        if self._neighbour is None:
            self._neighbour = hip_sparse.sparse_neighbours(self._state)
        return self._neighbour

    def _extract(self, color, clean, allow_overflow=False):
        """Marching cubes over the allocated bricks, reading only the pool (``dvmvs.hip.sparse.sparse_extract``), then ``clean`` as
        ``TSDFVolume._extract`` applies it."""
        mesh = hip_sparse.sparse_extract(self._state, self._origin, self._voxel_size, colour=color, neighbour=self.neighbours(),
                                         allow_overflow=allow_overflow)
        return finish_mesh(mesh, None, None, clean)

    def _surface(self, color, simplify, smooth, clean, allow_overflow=False):
        """extract -> clean -> smooth -> simplify on device tensors, the stages of ``TSDFVolume._surface`` (``finish_mesh``)."""
        simplify, smooth, clean = mesh_stages(simplify, smooth, clean)
        return finish_mesh(self._extract(color, clean, allow_overflow), simplify, smooth, None)

    def get_mesh(self, simplify=None, smooth=None, clean=None, allow_overflow=False):
        """``TSDFVolume.get_mesh`` of this volume, without a dense copy: (verts [V,3] float32 in world units, faces [F,3] int32, normals
        [V,3] float32, colours [V,3] uint8 RGB) as numpy arrays.  The surface is that of the unbounded volume whose voxels are the
        allocated bricks' and (1, 0, 0) elsewhere -- the mesh of ``dense(box).get_mesh()`` for any box that holds the allocated bricks
        with a brick of margin, as a set of welded triangles; the normals' gradient is the central difference everywhere; the order is by
        handling brick.  ``clean`` / ``smooth`` / ``simplify`` as there.  One host read (brick, overflow, vertex
        and face counts together) plus those of the stages.  ``RuntimeError`` when bricks were dropped (``overflow``), unless
        ``allow_overflow``; no brick gives V = F = 0."""
        verts, faces, norms, colors = self._surface(True, simplify, smooth, clean, allow_overflow)
        return verts.cpu().numpy(), faces.cpu().numpy(), norms.cpu().numpy(), colors.cpu().numpy()

    def get_point_cloud(self):
        """[N,6] float32: the mesh's vertices (xyz, world units) followed by their colour (rgb), as ``TSDFVolume.get_point_cloud``."""
        verts, _, _, colors = self.get_mesh()
        return np.hstack([verts, colors])

    def vertices(self, simplify=None, smooth=None, clean=None, allow_overflow=False):
        """The vertices of the zero iso-surface as a float32 [V,3] DEVICE tensor (``TSDFVolume.vertices``)."""
        return self._surface(False, simplify, smooth, clean, allow_overflow)[0]

    def mesh_tensors(self, simplify=None, smooth=None, clean=None, allow_overflow=False):
        """``(verts float32 [V,3], faces int32 [F,3])`` of the zero iso-surface as DEVICE tensors (``TSDFVolume.mesh_tensors``), extracted
        from the pool."""
        return self._surface(False, simplify, smooth, clean, allow_overflow)[:2]

    def surface_points(self, sample_density=None, voxel=None, simplify=None, smooth=None, clean=None):
        """The point set the 3-D metrics take from this volume's surface, a float32 [N,3] DEVICE tensor (``TSDFVolume.surface_points``)."""
        from dvmvs.errors import prepare_points_device
        verts, faces = self.mesh_tensors(simplify=simplify, smooth=smooth, clean=clean)
        return prepare_points_device(verts, faces, sample_density, voxel)

    def score_against(self, reference, threshold=0.05, return_sizes=False, sample_density=None, voxel=None, visible_from=None, clean=None,
                      simplify=None, smooth=None, align_plane=False, align_normal_neighbours=20, align_normal_distance=np.inf, align_distance=None,
                      align_scale=False, return_transform=False):
        """``TSDFVolume.score_against`` with this volume's surface, extracted from the pool, as the prediction; ``reference`` and every
        keyword as there.  (As the REFERENCE of another volume's ``score_against``, pass ``mesh_tensors()``.)"""
        from dvmvs.tsdf.scoring import score_volume
        return score_volume(self, reference, threshold, return_sizes, sample_density, voxel, visible_from, align_distance, align_scale,
                            return_transform, clean=clean, align_plane=align_plane, align_normal_neighbours=align_normal_neighbours,
                            align_normal_distance=align_normal_distance, simplify=simplify, smooth=smooth)[0]
