"""Registration of a point cloud to another by trimmed ICP on the device (csrc/registration.hip; definition in include/dvmvs_hip.h):
plain functions over the C ABI and the ops package's workspace and launch plumbing.  Inference-time geometry only: nothing here is
registered under ``torch.ops.dvmvs`` and nothing needs autograd."""
import ctypes
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from dvmvs.hip import _capi
from dvmvs.hip.ops import _workspace
from dvmvs.hip.ops._common import check_tensors, launch, out_or_new, ptr

STATUS_NAMES = ("running", "converged", "too few correspondences", "iteration limit")
STATUS_RUNNING, STATUS_CONVERGED, STATUS_TOO_FEW, STATUS_LIMIT = range(4)
PLANE_STATUS_NAMES = STATUS_NAMES + ("degenerate geometry",)
STATUS_DEGENERATE = 4
MAX_ITERATIONS = 1024
# the head of the state block in 8-byte words (include/dvmvs_hip.h): T | iterations | status | moments up to the variant's head words
_WORD_ITERATIONS, _WORD_STATUS, _WORD_MOMENTS = 16, 17, 18
# a variant of the loop: the op's name (its symbols are dvmvs_<name>_workspace_bytes and dvmvs_<name>_fwd), the head words of its state
# block (18 + its 18 or 30 moments) and the arrays of max_iterations entries that follow the head
_POINT = ("icp", 36, ("inliers", "fitness", "rmse"))
_PLANE = ("icp_plane", 48, ("inliers", "fitness", "rmse", "rmse_point"))


def _state(variant, device, N, max_iterations):
    name = variant[0]
    N, max_iterations = int(N), int(max_iterations)
    nbytes = getattr(_capi.lib(), f"dvmvs_{name}_workspace_bytes")(N, max_iterations)
    if nbytes == 0:
        raise ValueError(f"dvmvs::{name}: {N} points over {max_iterations} iterations are outside what the kernels take (1 .. 2^28 points, "
                         f"1 .. {MAX_ITERATIONS} iterations)")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def icp_workspace(device, N, max_iterations):
    """A state block for one registration of ``N`` source points over at most ``max_iterations`` iterations: a float64 device tensor of
    ``dvmvs_icp_workspace_bytes(N, max_iterations)`` bytes, uninitialised (the call writes what it reads).  It is a FRESH block, not a
    per-device one: the transform and the record that ``icp`` returns are views of it."""
    return _state(_POINT, device, N, max_iterations)


def icp_plane_workspace(device, N, max_iterations):
    """``icp_workspace`` for ``icp_plane``: ``dvmvs_icp_plane_workspace_bytes(N, max_iterations)`` bytes, a fresh float64 device tensor."""
    return _state(_PLANE, device, N, max_iterations)


def _cloud(name, label, t, device=None):
    check_tensors(name, t, label=label, shape=(None, 3), device=device)
    if t.shape[0] < 1:
        raise ValueError(f"dvmvs::{name}: {label} is empty")
    return t.contiguous()


def _host_matrix(name, init):
    if init is None:
        return None
    if torch.is_tensor(init):
        if init.device.type != "cpu":
            raise ValueError(f"dvmvs::{name}: init is a HOST 4x4 (it is read before the call returns), got a tensor on {init.device}")
        init = init.detach().numpy()
    init = np.ascontiguousarray(init, dtype=np.float64)
    if init.shape != (4, 4) or not np.isfinite(init).all():
        raise ValueError(f"dvmvs::{name}: init must be a finite 4x4 matrix, got shape {init.shape}")
    return init


def _settings(name, max_distance, tolerance, max_iterations):
    max_distance, tolerance, max_iterations = float(max_distance), float(tolerance), int(max_iterations)
    if not max_distance > 0.0 or not tolerance >= 0.0:
        raise ValueError(f"dvmvs::{name}: max_distance must be positive and tolerance not negative (neither NaN), got {max_distance}, {tolerance}")
    if not 1 <= max_iterations <= MAX_ITERATIONS:
        raise ValueError(f"dvmvs::{name}: max_iterations must be in 1 .. {MAX_ITERATIONS}, got {max_iterations}")
    return max_distance, tolerance, max_iterations


def _grid(name, grid, target):
    """The target's grid: built here, or the caller's after a check of its size."""
    from dvmvs.hip.ops import reconstruction
    if grid is None:
        return reconstruction.nearest_build(target)
    M = int(target.shape[0])
    check_tensors(name, grid, dtype=torch.uint8, label="grid", device=target.device, contiguous=True)
    if grid.numel() < _capi.lib().dvmvs_nearest_workspace_bytes(M):
        raise ValueError(f"dvmvs::{name}: grid is smaller than the workspace of a {M}-point target")
    return grid


def _register(variant, source, target, normals, max_distance, options, max_iterations, tolerance, init, grid):
    """Enqueues the loop of ``variant`` on clouds and settings that have been checked: ``normals`` and ``options`` are the arguments of its
    launcher after ``target`` and after ``max_distance``.  Returns ``(T, info)``, views of a fresh state block."""
    name, head_words, records = variant
    dev, N, M = source.device, int(source.shape[0]), int(target.shape[0])
    init = _host_matrix(name, init)
    grid = _grid(name, grid, target)
    scratch = _workspace.grown("nearest_query", dev, _capi.lib().dvmvs_nearest_query_workspace_bytes(N, M), torch.uint8)
    state = _state(variant, dev, N, max_iterations)
    init_ptr = None if init is None else init.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    launch(f"dvmvs_{name}_fwd", dev, ptr(source), N, ptr(target), *normals, M, ptr(grid), ptr(scratch), scratch.numel(), max_distance, *options,
           max_iterations, tolerance, init_ptr, ptr(state), state.numel() * 8)
    words = state.view(torch.int64)
    info = {"iterations": words[_WORD_ITERATIONS], "status": words[_WORD_STATUS]}
    for r, key in enumerate(records):                            # inliers are int64, the others float64
        first = head_words + r * max_iterations
        info[key] = (words if key == "inliers" else state)[first:first + max_iterations]
    info["moments"] = state[_WORD_MOMENTS:head_words]
    return state[:16].view(4, 4), info


def icp(source: Tensor, target: Tensor, max_distance: float, init=None, max_iterations: int = 30, with_scale: bool = False,
        tolerance: float = 1e-6, grid: Optional[Tensor] = None):
    """Registers ``source`` (float32 [N,3]) to ``target`` (float32 [M,3], both on one GPU, finite) by trimmed ICP: returns ``(T, info)``,
    ``T`` a float64 [4,4] DEVICE tensor that takes source coordinates into the target's frame (rigid; with ``with_scale`` a similarity),
    ``info`` a dict of DEVICE tensors: ``iterations`` and ``status`` (int64 scalars; ``STATUS_NAMES``), ``inliers`` (int64), ``fitness``
    and ``rmse`` (float64), each [max_iterations] with the entries below ``iterations`` written, and ``moments`` (float64 [18]: the
    sums of the last recorded iteration).  Nothing is read by the call: ``max_iterations`` iterations are enqueued on the current stream,
    and those after the loop has stopped find the status on the device and do nothing.  A pair is an inlier when its distance is at most
    ``max_distance`` (``inf`` keeps all); the loop stops when RMSE and fitness both change by less than ``tolerance``, with fewer than 3
    inliers, or at the limit.  ``init``: a HOST 4x4 (array, nested list or CPU tensor) to start from instead of the identity.  ``grid``:
    the workspace of ``ops.nearest_build(target)`` when the caller has it (it is not changed).  The arithmetic, including the order of
    every sum, is fixed (include/dvmvs_hip.h): ``dvmvs.errors.register_points`` gives the same bits."""
    source = _cloud("icp", "source", source)
    target = _cloud("icp", "target", target, source.device)
    max_distance, tolerance, max_iterations = _settings("icp", max_distance, tolerance, max_iterations)
    return _register(_POINT, source, target, (), max_distance, (int(bool(with_scale)),), max_iterations, tolerance, init, grid)


def icp_plane(source: Tensor, target: Tensor, target_normals: Tensor, max_distance: float, init=None, max_iterations: int = 30,
              tolerance: float = 1e-6, grid: Optional[Tensor] = None):
    """Registers ``source`` (float32 [N,3]) to ``target`` (float32 [M,3]) with normals ``target_normals`` (float32 [M,3], all on one GPU)
    by trimmed point-to-plane ICP: ``(T, info)`` as ``icp`` returns them, rigid only.  A normal that is all zero or not finite is "no
    normal": such a target pairs with nothing; a normal's sign does not matter.  ``info`` holds ``iterations``, ``status``
    (``PLANE_STATUS_NAMES``), ``inliers``, ``fitness``, ``rmse`` (of the plane residual), ``rmse_point`` (of the point distance), each
    [max_iterations], and ``moments`` (float64 [30]).  The loop stops when RMSE and fitness both change by less than ``tolerance``, with
    fewer than 6 inliers, at the limit, or with status 4 where the paired geometry (a single plane, two planes) leaves a freedom open, in
    which case T is left as it was.  Nothing is read by the call.  ``init`` and ``grid`` as in ``icp``.  The arithmetic is fixed
    (include/dvmvs_hip.h): ``dvmvs.errors.register_points_plane`` gives the same bits."""
    source = _cloud("icp_plane", "source", source)
    target = _cloud("icp_plane", "target", target, source.device)
    check_tensors("icp_plane", target_normals, label="target_normals", shape=(int(target.shape[0]), 3), device=source.device)
    target_normals = target_normals.contiguous()
    max_distance, tolerance, max_iterations = _settings("icp_plane", max_distance, tolerance, max_iterations)
    return _register(_PLANE, source, target, (ptr(target_normals),), max_distance, (), max_iterations, tolerance, init, grid)


def transform_points(points: Tensor, T: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """``points`` float32 [N,3] moved by ``T`` (float64 [4,4] on the same GPU, e.g. ``icp``'s): every entry of ``T[:3,:4]`` is rounded to
    float32 and ``p' = ((A00 x + A01 y) + A02 z) + A03`` (and so on) is evaluated in float32 without FMA, as the registration itself
    moves its points.  ``out``: a contiguous float32 [N,3] tensor, which may be ``points``; it is returned.  One launch, no host read."""
    check_tensors("transform_points", points, label="points", shape=(None, 3))
    dev = points.device
    check_tensors("transform_points", T, dtype=torch.float64, label="T", shape=(4, 4), device=dev)
    if out is not None and out is not points:
        check_tensors("transform_points", out)
    if out is points and not points.is_contiguous():
        raise ValueError("dvmvs::transform_points: in place needs a contiguous tensor")
    src = points.contiguous()
    N = int(src.shape[0])
    out = out_or_new("transform_points", out, (N, 3), torch.float32, dev)
    if N > 0:
        launch("dvmvs_transform_points_fwd", dev, ptr(src), N, ptr(T.contiguous()), ptr(out))
    return out
