"""The sparse TSDF volume's entries on the device (csrc/sparse_volume.hip; contract in include/dvmvs_hip.h): the
state of a brick-hashed volume and the four steps of a flush -- mark, sort, assign, integrate -- plus the gather of ``dense()``.  Plain
functions over the C ABI and the ops package's launch plumbing; ``dvmvs.tsdf.SparseTSDFVolume`` is the class that users see.  Below them,
marching cubes straight from the pool (csrc/sparse_extract.hip): ``sparse_neighbours`` and ``sparse_extract`` with
the steps it is made of; and ray-casting straight from the pool (csrc/sparse_raycast.hip): ``sparse_raycast_index``,
``sparse_raycast_flags`` and ``sparse_raycast``."""
import math

import torch

from dvmvs.hip import _capi
from dvmvs.hip.ops._common import check_tensors, launch, opt_ptr, ptr

BRICK = 8
BRICK_VOXELS = 512
EMPTY_KEY = (1 << 63) - 1
UNBORN = (1 << 31) - 1
STATUS_WORDS = 8
STATUS_BRICKS, STATUS_DROPPED_POOL, STATUS_DROPPED_TABLE, STATUS_REJECTED_PIXELS, STATUS_FRESH = range(5)


class SparseState:
    """Every device buffer of one sparse volume, allocated once: the capacity is fixed, so a flush never allocates pool or table memory
    and never reads the device."""

    def __init__(self, max_bricks, table_slots, device):
        max_bricks = int(max_bricks)
        if max_bricks < 1 or max_bricks >= 1 << 31:
            raise ValueError(f"sparse volume: max_bricks must be in [1, 2^31), got {max_bricks}")
        if table_slots is None:
            table_slots = 1 << max(4, (2 * max_bricks - 1).bit_length())      # a power of two >= 2 * max_bricks: at most half full
        table_slots = int(table_slots)
        if table_slots < 1 or table_slots & (table_slots - 1) or table_slots > 1 << 30:
            raise ValueError(f"sparse volume: table_slots must be a power of two up to 2^30, got {table_slots}")
        self.max_bricks, self.table_slots, self.device = max_bricks, table_slots, torch.device(device)
        dev = self.device
        self.table_keys = torch.full((table_slots,), EMPTY_KEY, dtype=torch.int64, device=dev)
        self.table_birth = torch.full((table_slots,), UNBORN, dtype=torch.int32, device=dev)
        self.fresh = torch.full((table_slots,), EMPTY_KEY, dtype=torch.int64, device=dev)
        self.sorted = torch.empty((table_slots,), dtype=torch.int64, device=dev)
        self.sort_index = torch.empty((table_slots,), dtype=torch.int64, device=dev)
        self.status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
        self.pool_key = torch.full((max_bricks,), EMPTY_KEY, dtype=torch.int64, device=dev)
        self.pool_birth = torch.full((max_bricks,), UNBORN, dtype=torch.int32, device=dev)
        self.tsdf = torch.ones((max_bricks, BRICK_VOXELS), dtype=torch.float32, device=dev)
        self.weight = torch.zeros((max_bricks, BRICK_VOXELS), dtype=torch.float32, device=dev)
        self.color = torch.zeros((max_bricks, BRICK_VOXELS), dtype=torch.float32, device=dev)
        self.device = self.tsdf.device      # with its index ("cuda" -> "cuda:0"): what a tensor's ``.device`` compares equal to


def sparse_mark(state, depth, cam_intr, cam_pose, origin, voxel_size, trunc_margin, max_depth, first_frame):
    """Step 1 of a flush (``dvmvs_sparse_mark``): the bricks that the N frames ``depth`` [N,h,w] mark enter the table, with their births."""
    name = "sparse_mark"
    check_tensors(name, depth, label="depth", shape=(None, None, None), device=state.device, contiguous=True)
    N, h, w = (int(d) for d in depth.shape)
    if N < 1 or h < 1 or w < 1:
        raise ValueError(f"dvmvs::{name}: expected at least one non-empty frame, got depth {tuple(depth.shape)}")
    check_tensors(name, cam_intr, label="cam_intr", shape=(N, 3, 3), device=state.device, contiguous=True)
    check_tensors(name, cam_pose, label="cam_pose", shape=(N, 4, 4), device=state.device, contiguous=True)
    launch("dvmvs_sparse_mark", state.device, ptr(state.table_keys), ptr(state.table_birth), state.table_slots, ptr(state.fresh),
           ptr(state.status), ptr(depth), ptr(cam_intr), ptr(cam_pose), N, h, w, float(origin[0]), float(origin[1]), float(origin[2]),
           float(voxel_size), float(trunc_margin), float(max_depth), int(first_frame))


def sparse_assign(state):
    """Steps 2 and 3: the keys this flush inserted, sorted on the device into the state's scratch (no host read), get pool slots in
    ascending key order behind the existing bricks (``dvmvs_sparse_assign``)."""
    with torch.cuda.device(state.device):
        torch.sort(state.fresh, out=(state.sorted, state.sort_index))
    launch("dvmvs_sparse_assign", state.device, ptr(state.table_keys), ptr(state.table_birth), state.table_slots, ptr(state.sorted),
           ptr(state.fresh), ptr(state.status), ptr(state.pool_key), ptr(state.pool_birth), state.max_bricks)


def sparse_integrate(state, depth, cam_intr, cam_pose, rgb_u8, folded, origin, voxel_size, trunc_margin, weights, max_depth, first_frame):
    """Step 4 (``dvmvs_sparse_integrate``): every allocated brick receives the frames at or after its birth, in index order, with the
    dense kernel's statements.  Exactly one of ``rgb_u8`` [N,h,w,3] uint8 and ``folded`` [N,h,w] float32; ``weights``: N host floats."""
    name = "sparse_integrate"
    if (rgb_u8 is None) == (folded is None):
        raise ValueError(f"dvmvs::{name}: exactly one of rgb_u8 and folded must be given")
    N, h, w = (int(d) for d in depth.shape)
    if rgb_u8 is not None:
        check_tensors(name, rgb_u8, dtype=torch.uint8, label="rgb_u8", shape=(N, h, w, 3), device=state.device, contiguous=True)
    else:
        check_tensors(name, folded, label="folded", shape=(N, h, w), device=state.device, contiguous=True)
    if len(weights) != N:
        raise ValueError(f"dvmvs::{name}: {len(weights)} observation weights for {N} frames")
    launch("dvmvs_sparse_integrate", state.device, ptr(state.tsdf), ptr(state.weight), ptr(state.color), ptr(state.pool_key),
           ptr(state.pool_birth), ptr(state.status), state.max_bricks, float(origin[0]), float(origin[1]), float(origin[2]),
           float(voxel_size), ptr(cam_intr), ptr(cam_pose), opt_ptr(rgb_u8), opt_ptr(folded), ptr(depth), N, h, w, float(trunc_margin),
           _capi.float_array(weights), float(max_depth), int(first_frame))


def sparse_gather(state, n_bricks, tsdf, weight, color, first_brick):
    """Copies the allocated bricks (``n_bricks``: a host number) that lie in the dense [X,Y,Z] tensors, whose voxel (0,0,0) is the first
    voxel of brick ``first_brick`` and whose sizes are multiples of 8, to their place there (``dvmvs_sparse_gather``)."""
    name = "sparse_gather"
    check_tensors(name, tsdf, label="tsdf", shape=(None, None, None), device=state.device, contiguous=True)
    X, Y, Z = (int(d) for d in tsdf.shape)
    if X < BRICK or Y < BRICK or Z < BRICK or X % BRICK or Y % BRICK or Z % BRICK:
        raise ValueError(f"dvmvs::{name}: the dense volume must be whole bricks, got {(X, Y, Z)}")
    check_tensors(name, weight, label="weight", shape=(X, Y, Z), device=state.device, contiguous=True)
    check_tensors(name, color, label="color", shape=(X, Y, Z), device=state.device, contiguous=True)
    n_bricks = int(n_bricks)
    if not 0 <= n_bricks <= state.max_bricks:
        raise ValueError(f"dvmvs::{name}: {n_bricks} bricks in a pool of {state.max_bricks}")
    launch("dvmvs_sparse_gather", state.device, ptr(state.tsdf), ptr(state.weight), ptr(state.color), ptr(state.pool_key), n_bricks, ptr(tsdf),
           ptr(weight), ptr(color), X // BRICK, Y // BRICK, Z // BRICK, int(first_brick[0]), int(first_brick[1]), int(first_brick[2]))


EXTRACT_ROW = 27          # neighbour entries per brick: (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)
EXTRACT_CELLS = 729       # voxels a brick can handle: local coordinates -1 .. 7 per axis


def sparse_neighbours(state):
    """The neighbour table of the allocated bricks (``dvmvs_sparse_neighbours``): int32 [max_bricks, 27] on the
    device, row ``slot`` defined for slots < n_bricks, entry ``(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)`` = the pool slot of brick b + d or
    -1.  Reads ``status`` and ``pool_key`` only -- not the hash table: the keys of the slots < n_bricks (compared on the device) are sorted
    with ``torch.sort``, every other slot counting as the empty key, and each neighbour is found by a bounded binary search.  No host
    read.  The table holds until the next flush; ``SparseTSDFVolume`` caches it."""
    dev = state.device
    with torch.cuda.device(dev):
        slots = torch.arange(state.max_bricks, dtype=torch.int64, device=dev)
        keys = torch.where(slots < state.status[STATUS_BRICKS], state.pool_key, torch.full_like(state.pool_key, EMPTY_KEY))
        ordered, index = torch.sort(keys)
    neighbour = torch.empty((state.max_bricks, EXTRACT_ROW), dtype=torch.int32, device=dev)
    launch("dvmvs_sparse_neighbours", dev, ptr(state.pool_key), ptr(ordered), ptr(index), ptr(state.status), state.max_bricks, ptr(neighbour))
    return neighbour


def sparse_extract_count(state, neighbour, counts=None):
    """Step 2 of an extraction (``dvmvs_sparse_extract_count``): int32 [max_bricks, 2], the owned crossing edges and the triangles of
    the voxels each brick handles (rows of slots >= n_bricks are not written)."""
    name = "sparse_extract_count"
    check_tensors(name, neighbour, dtype=torch.int32, label="neighbour", shape=(state.max_bricks, EXTRACT_ROW), device=state.device, contiguous=True)
    if counts is None:
        counts = torch.empty((state.max_bricks, 2), dtype=torch.int32, device=state.device)
    check_tensors(name, counts, dtype=torch.int32, label="counts", shape=(state.max_bricks, 2), device=state.device, contiguous=True)
    launch("dvmvs_sparse_extract_count", state.device, ptr(state.tsdf), ptr(neighbour), ptr(state.status), state.max_bricks, ptr(counts))
    return counts


def sparse_extract_scan(state, counts):
    """Step 3 (``dvmvs_sparse_extract_scan``): ``(offsets int64 [max_bricks, 2], summary int64 [5])`` on the device; summary =
    (n_bricks, bricks dropped by the pool, marks dropped by the table, V, F)."""
    check_tensors("sparse_extract_scan", counts, dtype=torch.int32, label="counts", shape=(state.max_bricks, 2), device=state.device, contiguous=True)
    offsets = torch.empty((state.max_bricks, 2), dtype=torch.int64, device=state.device)
    summary = torch.empty(5, dtype=torch.int64, device=state.device)
    launch("dvmvs_sparse_extract_scan", state.device, ptr(counts), ptr(state.status), state.max_bricks, ptr(offsets), ptr(summary))
    return offsets, summary


def sparse_extract_emit(state, neighbour, offsets, n_bricks, V, F, origin, voxel_size, colour=True):
    """Step 4 (``dvmvs_sparse_extract_emit``) with the numbers of the summary: ``(verts [V,3] float32, faces [F,3] int32, normals [V,3]
    float32, colours [V,3] uint8 or None)``.  The workspace is 729 int32 per ALLOCATED brick."""
    name = "sparse_extract_emit"
    dev = state.device
    n_bricks, V, F = int(n_bricks), int(V), int(F)
    if not 0 <= n_bricks <= state.max_bricks:
        raise ValueError(f"dvmvs::{name}: {n_bricks} bricks in a pool of {state.max_bricks}")
    if V >= 1 << 31 or F >= 1 << 31:
        raise RuntimeError(f"dvmvs::{name}: {V} vertices and {F} faces do not fit int32 indices")
    check_tensors(name, neighbour, dtype=torch.int32, label="neighbour", shape=(state.max_bricks, EXTRACT_ROW), device=dev, contiguous=True)
    check_tensors(name, offsets, dtype=torch.int64, label="offsets", shape=(state.max_bricks, 2), device=dev, contiguous=True)
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    colours = torch.empty((V, 3), dtype=torch.uint8, device=dev) if colour else None
    if n_bricks and (V or F):
        origin = [float(o) for o in origin]
        vertex_base = torch.empty((n_bricks, EXTRACT_CELLS), dtype=torch.int32, device=dev)
        launch("dvmvs_sparse_extract_emit", dev, ptr(state.tsdf), ptr(state.color) if colour else None, ptr(state.pool_key), ptr(neighbour),
               ptr(offsets), n_bricks, origin[0], origin[1], origin[2], float(voxel_size), ptr(vertex_base), ptr(verts), ptr(normals),
               opt_ptr(colours), ptr(faces), V, F)
    return verts, faces, normals, colours


def sparse_extract(state, origin, voxel_size, colour=True, neighbour=None, allow_overflow=False):
    """Marching cubes over the allocated bricks, reading only the pool (csrc/sparse_extract.hip; definition in include/dvmvs_hip.h and
    DESIGN.md section 4.8s): ``(verts [V,3] float32, faces [F,3] int32, normals [V,3] float32, colours [V,3] uint8 or None)`` device
    tensors, the mesh that ``marching_cubes`` gives at level 0 on the unbounded volume whose voxels are the allocated bricks' and
    (1, 0, 0) elsewhere.  ``neighbour``: the table of ``sparse_neighbours`` for the state as it is (built when None).  ONE host read: the
    summary (n_bricks, dropped counts, V, F).  ``RuntimeError`` when bricks or marks were dropped, unless ``allow_overflow``.  No brick:
    V = F = 0 with typed empty tensors."""
    if neighbour is None:
        neighbour = sparse_neighbours(state)
    counts = sparse_extract_count(state, neighbour)
    offsets, summary = sparse_extract_scan(state, counts)
    n_bricks, dropped_pool, dropped_table, V, F = (int(x) for x in summary.cpu())      # the one host read
    if (dropped_pool or dropped_table) and not allow_overflow:
        raise RuntimeError(f"sparse_extract: {dropped_pool} bricks did not fit the pool of {state.max_bricks} and {dropped_table} marks found "
                           f"no table slot: the volume is incomplete (a larger max_bricks / table_slots, or allow_overflow=True)")
    return sparse_extract_emit(state, neighbour, offsets, n_bricks, V, F, origin, voxel_size, colour=colour)


# ---- ray-casting straight from the pool (csrc/sparse_raycast.hip) -------------------------------------------------
RAYCAST_MAX_STEPS = 1 << 20      # kSrMaxSteps: the box diagonal in steps, floor(|8 count - 1| / step) + 2, must stay below


def raycast_index_slots(max_bricks):
    """Entries of the render index of a pool of ``max_bricks`` bricks: the power of two >= 2 * max_bricks (at most half full)."""
    return 1 << max(4, (2 * int(max_bricks) - 1).bit_length())


def sparse_raycast_index(state):
    """The render index of the allocated bricks (``dvmvs_sparse_raycast_index``): int64 [slots, 2] on the device, an open-addressing table
    of (key, value) entries filled from ``pool_key[:n_bricks]`` with ``n_bricks`` read on the device; value = pool slot (the crossing flag
    joins it in ``sparse_raycast_flags``).  Reads ``status`` and ``pool_key`` only -- not the volume's hash table.  No host read."""
    slots = raycast_index_slots(state.max_bricks)
    index = torch.empty((slots, 2), dtype=torch.int64, device=state.device)
    launch("dvmvs_sparse_raycast_index", state.device, ptr(state.pool_key), ptr(state.status), state.max_bricks, ptr(index), slots)
    return index


def sparse_raycast_flags(state, neighbour, index):
    """Per-slot crossing flags (``dvmvs_sparse_raycast_flags``): uint8 [max_bricks], 1 where one of the 9^3 corners of the brick's cells has
    ``weight > 0 and tsdf <= 0``; the same bit enters the brick's value in ``index``, in place.  ``neighbour``: the table of
    ``sparse_neighbours``; ``index``: that of ``sparse_raycast_index``, both for the state as it is.  No host read."""
    name = "sparse_raycast_flags"
    check_tensors(name, neighbour, dtype=torch.int32, label="neighbour", shape=(state.max_bricks, EXTRACT_ROW), device=state.device, contiguous=True)
    check_tensors(name, index, dtype=torch.int64, label="index", shape=(raycast_index_slots(state.max_bricks), 2), device=state.device,
                  contiguous=True)
    flags = torch.zeros((state.max_bricks,), dtype=torch.uint8, device=state.device)
    launch("dvmvs_sparse_raycast_flags", state.device, ptr(state.tsdf), ptr(state.weight), ptr(state.pool_key), ptr(neighbour), ptr(state.status),
           state.max_bricks, ptr(index), int(index.shape[0]), ptr(flags))
    return flags


def raycast_steps(count, step):
    """The longest march through a box of ``count`` bricks per axis, as the C entry computes it: floor(diagonal / step) + 2."""
    d = [8.0 * int(c) - 1.0 for c in count]
    return math.floor(math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / float(step)) + 2.0


def sparse_raycast(state, index, flags, neighbour, first_brick, count, origin, voxel_size, cam_intr, cam_pose, height, width, near=0.0,
                   far=float("inf"), step=1.0, normals=True, colour=True, skip_empty=True):
    """Renders the sparse volume from N views in one launch, reading only the pool (``dvmvs_sparse_raycast_fwd``): the outputs of
    ``dvmvs.hip.ops.tsdf_raycast`` on the dense volume over the box of ``count`` bricks per axis from brick ``first_brick``, whose voxel
    (0, 0, 0) lies at ``origin`` (float32), bit for bit.  ``index``, ``flags``, ``neighbour``: the tables of ``sparse_raycast_index``,
    ``sparse_raycast_flags`` and ``sparse_neighbours`` for the state as it is.  ``cam_intr`` [N,3,3] and camera-to-world ``cam_pose``
    [N,4,4], float32 on the state's device.  Returns ``(depth [N,height,width] float32, normals [N,height,width,3] float32 or None, rgb
    [N,height,width,3] uint8 or None)``.  Runs on the current stream without touching the host."""
    name = "sparse_raycast"
    dev = state.device
    check_tensors(name, index, dtype=torch.int64, label="index", shape=(raycast_index_slots(state.max_bricks), 2), device=dev, contiguous=True)
    check_tensors(name, flags, dtype=torch.uint8, label="flags", shape=(state.max_bricks,), device=dev, contiguous=True)
    check_tensors(name, neighbour, dtype=torch.int32, label="neighbour", shape=(state.max_bricks, EXTRACT_ROW), device=dev, contiguous=True)
    check_tensors(name, cam_intr, label="cam_intr", shape=(None, 3, 3), device=dev)
    check_tensors(name, cam_pose, label="cam_pose", shape=(None, 4, 4), device=dev)
    N = int(cam_pose.shape[0])
    height, width = int(height), int(width)
    if N < 1 or cam_intr.shape[0] != N or height < 1 or width < 1:
        raise ValueError(f"dvmvs::{name}: expected N >= 1 poses and as many intrinsics and a positive image size, got "
                         f"{tuple(cam_pose.shape)}, {tuple(cam_intr.shape)}, {height}x{width}")
    near, far, step, voxel_size = float(near), float(far), float(step), float(voxel_size)
    if not (0.0 < step <= 5.0):
        raise ValueError(f"dvmvs::{name}: step must be in (0, 5] voxels (the truncation), got {step}")
    if not (0.0 <= near < float("inf")) or far != far:
        raise ValueError(f"dvmvs::{name}: near must be finite and >= 0 and far not NaN, got {near}, {far}")
    if not voxel_size > 0.0:
        raise ValueError(f"dvmvs::{name}: voxel_size must be positive, got {voxel_size}")
    origin = [float(o) for o in origin]
    first, count = [int(f) for f in first_brick], [int(c) for c in count]
    if len(origin) != 3 or len(first) != 3 or len(count) != 3:
        raise ValueError(f"dvmvs::{name}: origin, first_brick and count must have three components")
    if min(count) < 1 or max(count) > 1 << 21 or min(first) < -(1 << 20) or max(f + c - 1 for f, c in zip(first, count)) > 1 << 20:
        raise ValueError(f"dvmvs::{name}: the box of {count} bricks from {first} is empty or leaves the lattice's coordinate range")
    if raycast_steps(count, step) >= RAYCAST_MAX_STEPS:
        raise ValueError(f"dvmvs::{name}: the box of {count} bricks is too long to march at step {step}")
    cam_intr, cam_pose = cam_intr.contiguous(), cam_pose.contiguous()
    depth = torch.empty((N, height, width), dtype=torch.float32, device=dev)
    normal = torch.empty((N, height, width, 3), dtype=torch.float32, device=dev) if normals else None
    rgb = torch.empty((N, height, width, 3), dtype=torch.uint8, device=dev) if colour else None
    launch("dvmvs_sparse_raycast_fwd", dev, ptr(state.tsdf), ptr(state.weight), ptr(state.color) if colour else None, ptr(state.status),
           state.max_bricks, ptr(index), int(index.shape[0]), ptr(neighbour), ptr(flags), first[0], first[1], first[2], count[0], count[1],
           count[2], origin[0], origin[1], origin[2], voxel_size, 1 if skip_empty else 0, ptr(cam_intr), ptr(cam_pose), N, height, width,
           near, far, step, ptr(depth), opt_ptr(normal), opt_ptr(rgb))
    return depth, normal, rgb
