"""CPU: the ray-caster's definition (tests/raycast_reference.py) against a closed form, the conditions the GPU tests' inputs must meet,
float32 against float64 within the reference, and the C ABI's argument validation (nothing is enqueued: no device is needed)."""
import numpy as np
import pytest

import raycast_reference as rr

ALL_CASES = sorted(rr.CASES)


def every_case():
    return [rr.case(name) for name in ALL_CASES] + [rr.oracle_case(2), rr.oracle_case(1)]


def test_float64_reference_equals_the_closed_form_plane_depth():
    """Trilinear interpolation of a linear function is linear, and with step < truncation both bracket samples lie in the band where
    tsdf = sd / trunc is not clipped: the interpolated crossing IS the ray-plane intersection.  A hit needs both samples valid, i.e. all
    sixteen corners observed, so no hit pixel's bracket touches the unobserved box.  The volume is kept in float64 here."""
    for dims, image, step in ((rr.DIMS_ODD, rr.IMAGE_A, 1.0), (rr.DIMS_SMALL, rr.IMAGE_B, 2.0), (rr.DIMS_SMALL, rr.IMAGE_A, 0.5)):
        vol = rr.plane_volume(dims)
        K = rr.intrinsics(image)
        poses = np.stack([rr.view(v) for v in rr.THREE_VIEWS])
        ref = rr.raycast(vol.tsdf64, vol.weight, vol.color, vol.origin, vol.voxel_size, K, poses, image[0], image[1], step=step)
        for i, pose in enumerate(poses):
            closed = rr.plane_depth(vol, K, pose, *image)
            hit = ref.hit[i]
            err = np.abs(ref.depth[i] - closed)[hit].max()
            print(f"plane {dims} step {step} view {i}: {hit.sum()} hits of {hit.size}, max |depth - closed form| = {err:.2e} m")
            assert hit.mean() >= rr.HIT_FLOOR and err <= 1e-9
            # the normal of a linear field is the plane's normal (towards the observer), wherever it is defined and the six
            # gradient samples are not clamped to the box
            g = rr.voxel_points(vol, K, pose, ref.depth[i])
            defined = hit & (np.abs(ref.normal[i]).sum(-1) > 0) & ((g >= 1) & (g <= np.array(dims) - 2)).all(-1)
            assert defined.sum() > 0.5 * hit.sum()
            assert np.abs(ref.normal[i][defined] - vol.plane_normal).max() <= 1e-9


@pytest.mark.parametrize("name", ALL_CASES + ["oracle_2", "oracle_1"])
def test_caps_hold_for_every_input_of_the_gpu_tests(name):
    c = rr.oracle_case(int(name[-1])) if name.startswith("oracle") else rr.case(name)
    for i, (amb, hit, n_ex, c_ex) in enumerate(rr.check_caps(c.ref64)):
        print(f"{name} view {i}: {100 * amb:.2f} % ambiguous, {100 * hit:.1f} % hits, {100 * n_ex:.2f} % / {100 * c_ex:.2f} % of the hits "
              f"excluded for normals / colours")


def test_float32_and_float64_agree_on_unambiguous_pixels():
    for c in every_case():
        clear = ~c.ref64.ambiguous
        assert np.array_equal(c.ref32.hit[clear], c.ref64.hit[clear]), c.name
        both = clear & c.ref64.hit
        assert np.abs(c.ref32.depth - c.ref64.depth)[both].max() <= 2e-6, c.name
        colours = both & ~c.ref64.colour_excluded
        assert np.array_equal(c.ref32.rgb[colours], c.ref64.rgb[colours]), c.name
        assert np.array_equal(c.ref32.n_samples[clear], c.ref64.n_samples[clear]), c.name


def test_cases_cover_what_they_are_meant_to():
    """The inputs exercise the paths they were chosen for (a check of the test design, from the reference alone)."""
    c = rr.case("plane_small_parallel")
    assert c.K[0, 2] == 16 and c.K[1, 2] == 12 and np.array_equal(c.poses[0][:3, :3], np.eye(3))      # exact zeros in d_g at u = 16 / v = 12
    c = rr.case("plane_small_near_far")
    full = rr.case("plane_small_n3")
    assert 0 < c.ref64.hit[0].sum() < full.ref64.hit[0].sum()        # near / far cut through the surface
    d = c.ref64.depth[0][c.ref64.hit[0]]
    assert d.min() >= np.float32(0.74) and d.max() <= np.float32(0.83)
    inside = rr.view("yaw-inside")[:3, 3]
    assert inside[2] > 0.8                                            # that camera is inside the volume
    for c in every_case():
        mask = rr.brick_mask(c.vol.tsdf, c.vol.weight)
        assert mask.any() and not mask.all(), c.name                 # something to march through and something to skip
    for c in every_case()[:len(ALL_CASES)]:
        assert c.vol.hole is not None and (c.vol.weight[c.vol.hole] == 0).all()
        assert len(np.unique(c.ref64.rgb[c.ref64.hit], axis=0)) > 20      # the colour pattern varies over the surface


def test_each_integrated_frame_needs_a_new_mask():
    """The input of the GPU test of mask invalidation: the mask of the still empty volume has no flagged brick, so every brick the
    first frame flags is new, and the reference's hits have their crossing in such bricks -- a render with the older mask would jump
    over them."""
    before = rr.brick_mask(rr.oracle_volume(0).tsdf, rr.oracle_volume(0).weight)
    c = rr.oracle_case(1)
    after = rr.brick_mask(c.vol.tsdf, c.vol.weight)
    new = (after > 0) & ~(before > 0)
    assert not before.any() and new.any()
    dims = np.array(c.vol.dims)
    for i, pose in enumerate(c.poses):
        hit = c.ref64.hit[i]
        g = rr.voxel_points(c.vol, c.K[i], pose, c.ref64.depth[i])[hit]
        brick = np.minimum(np.floor(g).astype(int), dims - 2) >> 3
        in_new = new[brick[:, 0], brick[:, 1], brick[:, 2]]
        print(f"view {i}: {hit.sum()} hits, {in_new.sum()} of them cross in bricks the older mask leaves unflagged")
        assert hit.sum() > 0 and in_new.all()


def test_degenerate_inputs_render_nothing():
    K = rr.intrinsics(rr.IMAGE_B)
    empty = rr.empty_volume(rr.DIMS_SMALL)
    plane = rr.plane_volume(rr.DIMS_SMALL)
    for vol, kind in ((empty, "frontal"), (plane, "away")):
        for dtype in (np.float32, np.float64):
            ref = rr.raycast(vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size, K, rr.view(kind), *rr.IMAGE_B, dtype=dtype)
            assert not ref.hit.any() and not ref.depth.any() and not ref.normal.any() and not ref.rgb.any()
    bad = rr.view("frontal").copy()
    bad[0, 3] = np.nan
    ref = rr.raycast(plane.tsdf, plane.weight, plane.color, plane.origin, plane.voxel_size, K, bad, *rr.IMAGE_B, dtype=np.float32)
    assert not ref.depth.any()


# ---- C ABI ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    import os
    from dvmvs.hip import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


def test_symbols_are_declared_bound_and_exported(library):
    import ctypes
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dvmvs_hip.h")).read()
    handle = ctypes.CDLL(library.LIB_PATH)
    for name in ("dvmvs_tsdf_raycast_mask_bytes", "dvmvs_tsdf_raycast_mask", "dvmvs_tsdf_raycast_fwd"):
        assert name + "(" in header and name in library.SIGNATURES and hasattr(handle, name)
        assert name in library.ADDED_WITHIN_ABI_TSDF_RAYCAST
    assert library.lib().dvmvs_abi_version() == 11          # a later addition: the number does not move


def test_mask_bytes_is_one_byte_per_brick_of_cells(library):
    lib = library.lib()
    for dims in ((2, 2, 2), (9, 9, 9), (10, 9, 2), rr.DIMS_SMALL, rr.DIMS_ODD, (256, 256, 256), (257, 300, 17)):
        expect = int(np.prod([-(-(d - 1) // 8) for d in dims]))
        assert lib.dvmvs_tsdf_raycast_mask_bytes(*dims) == expect, dims
    assert lib.dvmvs_tsdf_raycast_mask_bytes(1, 8, 8) == 0 and lib.dvmvs_tsdf_raycast_mask_bytes(8, 0, 8) == 0
    assert lib.dvmvs_tsdf_raycast_mask_bytes(4, 1 << 16, 1 << 15) == 0      # dim_y * dim_z >= 2^31


def test_argument_validation_without_gpu(library):
    """Every rejection happens before anything is enqueued.  The pointers are never dereferenced: any non-null value will do."""
    lib = library.lib()
    p = 4096
    inf = float("inf")
    good = dict(tsdf=p, weight=p, color=p, dims=(24, 20, 16), origin=(0.0, 0.0, 0.0), voxel=0.05, mask=None, K=p, pose=p, n=1, h=24, w=32,
                near=0.0, far=inf, step=1.0, depth=p, normal=None, rgb=None)

    def fwd(**change):
        a = dict(good, **change)
        return lib.dvmvs_tsdf_raycast_fwd(a["tsdf"], a["weight"], a["color"], *a["dims"], *a["origin"], a["voxel"], a["mask"], a["K"], a["pose"],
                                          a["n"], a["h"], a["w"], a["near"], a["far"], a["step"], a["depth"], a["normal"], a["rgb"], None)

    EINVAL, EUNSUPPORTED = -1, -2
    for change in (dict(tsdf=None), dict(weight=None), dict(K=None), dict(pose=None), dict(depth=None), dict(color=None, rgb=p),
                   dict(n=0), dict(h=0), dict(w=-1), dict(voxel=0.0), dict(voxel=float("nan")),
                   dict(step=0.0), dict(step=-1.0), dict(step=5.5), dict(step=float("nan")), dict(near=-0.1), dict(near=inf),
                   dict(near=float("nan")), dict(far=float("nan")),
                   dict(dims=(1, 20, 16)), dict(dims=(24, 1, 16)), dict(dims=(24, 20, 1)), dict(dims=(24, 0, 16))):
        assert fwd(**change) == EINVAL, change
    for change in (dict(dims=(4, 1 << 16, 1 << 15)), dict(n=65536), dict(n=65535, h=4096, w=4096), dict(n=256, h=4096, w=4096), dict(h=1 << 16, w=1 << 15), dict(h=16 * 65535 + 1, w=1),
                   dict(dims=(2000, 2000, 500), step=0.002)):
        assert fwd(**change) == EUNSUPPORTED, change
    assert lib.dvmvs_tsdf_raycast_mask(None, p, 24, 20, 16, p, None) == EINVAL
    assert lib.dvmvs_tsdf_raycast_mask(p, None, 24, 20, 16, p, None) == EINVAL
    assert lib.dvmvs_tsdf_raycast_mask(p, p, 24, 20, 16, None, None) == EINVAL
    assert lib.dvmvs_tsdf_raycast_mask(p, p, 24, 1, 16, p, None) == EINVAL
    assert lib.dvmvs_tsdf_raycast_mask(p, p, 4, 1 << 16, 1 << 15, p, None) == EUNSUPPORTED


def test_python_surface_rejects_bad_arguments_without_a_device():
    """The op's checks raise before the library is asked for anything a device would be needed for."""
    import torch
    from dvmvs.hip import ops
    vol = torch.ones(4, 4, 4)
    with pytest.raises(RuntimeError):          # no CPU path
        ops.tsdf_raycast(vol, vol, vol, (0, 0, 0), 0.05, torch.eye(3)[None], torch.eye(4)[None], 4, 4)
    with pytest.raises(RuntimeError):
        ops.tsdf_raycast_mask(vol, vol)
    from dvmvs import tsdf
    import inspect
    assert "render_keyframes" in inspect.signature(tsdf.run).parameters and hasattr(tsdf.TSDFVolume, "render")
