"""The sparse TSDF volume's entries on the device (csrc/sparse_volume.hip; contract in include/dvmvs_hip.h): the
state of a brick-hashed volume and the four steps of a flush -- mark, sort, assign, integrate -- plus the gather of ``dense()``.  Plain
functions over the C ABI and the ops package's launch plumbing; ``dvmvs.tsdf.SparseTSDFVolume`` is the class that users see."""
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
