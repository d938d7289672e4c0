"""Batched TSDF fusion (csrc/tsdf_fuse.hip, dvmvs.tsdf.LiveFusion), the part that needs no GPU: the volume bounds of a live run, argument
errors that are raised before the library is touched, the C ABI's bookkeeping, and the small scene the GPU tests share (checked here
against the CPU oracle, so that those tests compare volumes that the frames really touch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsdf_fuse_scene as scene
import tsdf_oracle as tso

NEW_NAMES = ("dvmvs_tsdf_integrate_frames_workspace_bytes", "dvmvs_tsdf_integrate_frames")


def test_small_scene_touches_what_the_oracle_says():
    """Voxels the CPU oracle updates per pose: front, inside and tilt observe thousands, away and far none, graze a corner."""
    depth, _ = scene.frames()
    touched = []
    for d, pose in zip(depth, scene.poses()):
        vols = [np.ones(scene.DIMS, np.float32), np.zeros(scene.DIMS, np.float32), np.zeros(scene.DIMS, np.float32)]
        ok = tso.integrate(*vols, scene.BOUNDS[:, 0].astype(np.float32), scene.VOXEL, scene.K, pose, np.zeros_like(d), d, 5 * scene.VOXEL)
        touched.append(int(ok.sum()))
    assert touched[0] == 7954 and touched[1] == 4710 and touched[4] == 6548
    assert touched[2] == 0 and touched[5] == 0 and 0 < touched[3] < 1000


def test_frustum_bounds_equal_the_bounds_of_constant_depth_maps():
    from dvmvs.tsdf import TSDFFusion
    poses = [p.astype(np.float64) for p in scene.poses()]
    K = scene.K.astype(np.float64)
    got = TSDFFusion.frustum_bounds(poses, K, scene.HEIGHT, scene.WIDTH, 5.0)
    want = TSDFFusion.calculate_volume_bounds([np.full((scene.HEIGHT, scene.WIDTH), 5.0)] * len(poses), poses, K)
    assert got.shape == (3, 2) and np.array_equal(got, want)
    # any depth maps <= max_depth seen from the same poses lie inside
    rng = np.random.RandomState(3)
    maps = [rng.uniform(0.0, 5.0, (scene.HEIGHT, scene.WIDTH)) for _ in poses]
    inner = TSDFFusion.calculate_volume_bounds(maps, poses, K)
    assert (got[:, 0] <= inner[:, 0]).all() and (got[:, 1] >= inner[:, 1]).all()
    depth, _ = scene.frames()
    inner = TSDFFusion.calculate_volume_bounds(list(depth), poses, K)
    assert (got[:, 0] <= inner[:, 0]).all() and (got[:, 1] >= inner[:, 1]).all()


def test_live_fusion_rejects_bad_arguments_before_anything_is_built():
    from dvmvs.tsdf import LiveFusion
    for batch in (0, -3):
        with pytest.raises(ValueError, match="batch"):
            LiveFusion(scene.BOUNDS, batch=batch)
    with pytest.raises(ValueError, match="voxel_size"):
        LiveFusion(scene.BOUNDS, voxel_size=0.0)
    with pytest.raises(ValueError, match="max_depth"):
        LiveFusion(scene.BOUNDS, max_depth=float("nan"))


def test_integrate_frames_op_rejects_bad_arguments_before_the_library_is_touched(monkeypatch):
    from dvmvs.hip import _capi, ops

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_capi, "lib", no_library)
    vol = [torch.ones(4, 5, 6), torch.zeros(4, 5, 6), torch.zeros(4, 5, 6)]
    N, h, w = 2, 3, 4
    K, P, depth = torch.zeros(N, 3, 3), torch.zeros(N, 4, 4), torch.ones(N, h, w)
    rgb, folded = torch.zeros(N, h, w, 3, dtype=torch.uint8), torch.zeros(N, h, w)

    def call(*, K=K, P=P, depth=depth, vol=vol, **kw):
        return ops.tsdf_integrate_frames(*vol, (0.0, 0.0, 0.0), 0.1, K, P, depth, **kw)

    with pytest.raises(ValueError, match="exactly one"):
        call()
    with pytest.raises(ValueError, match="exactly one"):
        call(rgb_u8=rgb, folded=folded)
    with pytest.raises(ValueError, match="rgb_u8"):
        call(rgb_u8=rgb[:, :, :3])                       # size mismatch with the depth
    with pytest.raises(ValueError, match="folded"):
        call(folded=folded[:1])
    with pytest.raises(ValueError, match="rgb_u8"):
        call(rgb_u8=rgb.float())
    with pytest.raises(ValueError, match="cam_pose"):
        call(P=P[:1], folded=folded)
    with pytest.raises(ValueError, match="cam_intr"):
        call(K=K[0], folded=folded)
    with pytest.raises(ValueError, match="depth"):
        call(depth=depth[0], folded=folded)
    with pytest.raises(ValueError, match="weight"):
        call(vol=[vol[0], vol[1][:3], vol[2]], folded=folded)
    with pytest.raises(ValueError, match="observation weights"):
        call(folded=folded, obs_weight=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="max_depth"):
        call(folded=folded, max_depth=float("nan"))
    with pytest.raises(RuntimeError, match="MI355X"):     # well-formed, but on the host: there is no CPU path
        call(folded=folded)
    # observation weights: a 0-d array or tensor is one number for all frames, a 1-d one is a weight per frame
    for one_number in (np.float32(2.0), np.array(2.0), torch.tensor(2.0)):
        with pytest.raises(RuntimeError, match="MI355X"):
            call(folded=folded, obs_weight=one_number)
    for per_frame in (np.array([1.0, 2.0]), torch.tensor([1.0, 2.0]), (1.0, 2.0)):
        with pytest.raises(RuntimeError, match="MI355X"):
            call(folded=folded, obs_weight=per_frame)
    for wrong_length in (np.ones(3), torch.ones(1)):
        with pytest.raises(ValueError, match="observation weights"):
            call(folded=folded, obs_weight=wrong_length)


def test_python_states_the_tile_the_kernel_is_built_with():
    """``ops.TSDF_FUSE_TILE`` (the tile counts of tests and tools) against the constants of csrc/tsdf_fuse.hip; the product library carries
    that one shape and its entry point reads no environment variable."""
    from dvmvs.hip import _capi, ops
    repo_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo_root, "deep-video-mvs_amd", "csrc", "tsdf_fuse.hip")) as f:
        source = f.read()
    found = re.search(r"constexpr int kFuseTX = (\d+), kFuseTY = (\d+), kFuseTZ = (\d+);", source)
    assert found and tuple(int(g) for g in found.groups()) == tuple(ops.TSDF_FUSE_TILE)
    assert ops.TSDF_FUSE_TILE[0] * ops.TSDF_FUSE_TILE[1] * ops.TSDF_FUSE_TILE[2] % 256 == 0       # whole voxels per thread
    assert ops.tsdf_fuse_tile_count((37, 30, 43)) == 10 * 8 * 2 and ops.tsdf_fuse_tile_count((8, 8, 64), (8, 8, 8)) == 8
    # the shapes of the tuning build and their environment switch are compiled out of the product
    product, tuning = source.split("#ifdef DVMVS_TSDF_FUSE_TUNING", 1)[0], source.split("#ifdef DVMVS_TSDF_FUSE_TUNING", 1)[1]
    assert "getenv" not in product and "getenv" in tuning
    assert not hasattr(ctypes.CDLL(_capi.LIB_PATH), "dvmvs_tsdf_fuse_tuning_tiles")


def test_header_signatures_and_exports_agree_on_the_new_names():
    from dvmvs.hip import _capi
    repo_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo_root, "include", "dvmvs_hip.h")) as f:
        header = f.read()
    assert "#define DVMVS_ABI_VERSION 11" in header and _capi.ABI_VERSION == 11
    assert tuple(_capi.ADDED_WITHIN_ABI_TSDF_FUSE) == NEW_NAMES
    for name in NEW_NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _capi.SIGNATURES
    # the declaration's parameter count is the binding's
    declaration = re.search(r"int dvmvs_tsdf_integrate_frames\((.*?)\);", header, re.S).group(1)
    assert len(declaration.split(",")) == len(_capi.SIGNATURES["dvmvs_tsdf_integrate_frames"][1]) == 24
    library = _capi.lib()                                  # raises if a name of ADDED_WITHIN_ABI_TSDF_FUSE is not exported
    assert library.dvmvs_abi_version() == 11
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW_NAMES:
        assert hasattr(raw, name), name


def test_a_library_without_the_new_names_is_reported(monkeypatch):
    from dvmvs.hip import _capi
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "ADDED_WITHIN_ABI_TSDF_FUSE", _capi.ADDED_WITHIN_ABI_TSDF_FUSE + ("dvmvs_symbol_of_a_later_build",))
    with pytest.raises(RuntimeError, match="dvmvs_symbol_of_a_later_build"):
        _capi.lib()


def test_workspace_bytes_are_monotone_and_zero_for_no_frames():
    from dvmvs.hip import _capi
    size = _capi.lib().dvmvs_tsdf_integrate_frames_workspace_bytes
    assert size(0) == 0 and size(-1) == 0 and size(-2 ** 31) == 0
    sizes = [size(n) for n in range(1, 200)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))


def test_entry_point_refuses_bad_arguments_without_a_launch():
    """EINVAL paths return before any HIP call, so they run without a device (pointers are only compared with NULL)."""
    from dvmvs.hip import _capi
    lib = _capi.lib()
    one = _capi.float_array([1.0])

    def call(tsdf=8, rgb=8, folded=None, n=1, voxel=0.1, trunc=0.5, max_depth=float("inf"), weights=one, workspace=8):
        return lib.dvmvs_tsdf_integrate_frames(tsdf, 8, 8, 4, 4, 4, 0.0, 0.0, 0.0, voxel, 8, 8, rgb, folded, 8, n, 4, 4, trunc, weights,
                                               max_depth, workspace, None, None)

    EINVAL = call(tsdf=None)
    assert EINVAL != 0
    assert call(rgb=8, folded=8) == EINVAL and call(rgb=None, folded=None) == EINVAL      # both, neither
    assert call(n=0) == EINVAL and call(voxel=0.0) == EINVAL and call(trunc=0.0) == EINVAL
    assert call(max_depth=float("nan")) == EINVAL and call(workspace=None) == EINVAL and call(weights=None) == EINVAL
