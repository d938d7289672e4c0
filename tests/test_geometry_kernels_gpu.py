"""The two forward kernels that move geometry, against float64 references (tests/splat_reference.py) at the shapes and inputs
where rounding a projected coordinate to a pixel goes wrong quietly.

Depth re-projection (csrc/depth_reproject.hip, all three entry points): every case of the shared table -- per-item transformations and
intrinsics at B = 3, odd sizes, the smallest sizes, rotations, points behind the camera, zero / negative / non-finite depths,
occlusion -- under one comparison rule that says which cells may differ and why (no count of tolerated pixels).  The low-resolution
and estimate forms must equal the nearest decimation of the full splat bit for bit at factors that do not divide the size, inside
canary borders.  test_splat_reference.py shows on the CPU that the float32 oracle passes the same rule on the same cases.

TSDF integration (csrc/tsdf.hip): two non-cubic volumes, one of 4.8 M voxels (beyond the 16 384 x 256 threads of one launch: the
grid-stride loop and the 64-bit index split run), six frames from rotated poses, against oracle/tsdf_oracle.py after every frame."""
import numpy as np
import pytest
import torch

import splat_reference as sr
import tsdf_oracle as tso

pytestmark = pytest.mark.gpu

EINVAL = -1
CANARY = -123.0
PAD = 1031              # elements of canary on either side of a carved buffer


@pytest.fixture(scope="module")
def ops():
    from dvmvs.hip import ops
    return ops


_memo = {}


def prepared(name, dev):
    """Case -> (the case, its inputs on the device, the float64 reference, the float32 oracle's map); computed once per module run."""
    if name not in _memo:
        case = sr.splat_case(name)
        args = [case[k] for k in ("T", "depth", "full_K", "half_K")]
        _memo[name] = (case, [a.to(dev) for a in args], sr.splat_reference(*args), sr.oracle_splat(*args))
    return _memo[name]


def carved(shape, dev, fill):
    """A contiguous tensor of ``shape`` inside a larger canary-filled one -> (view, check that the border is untouched)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), CANARY, device=dev)
    view = whole[PAD:PAD + n].view(shape)
    view.fill_(fill)

    def border_intact():
        return bool((whole[:PAD] == CANARY).all()) and bool((whole[PAD + n:] == CANARY).all())
    return view, border_intact


# ---- the full splat ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sr.SPLAT_CASES))
def test_depth_reproject_against_the_float64_reference(hip_device, ops, name):
    case, dargs, ref, oracle = prepared(name, hip_device)
    sr.assert_caps(ref, name, sr.min_landing(name))
    got = ops.depth_reproject(*dargs)
    B, _, H, W = case["depth"].shape
    assert tuple(got.shape) == (B, 1, H // 2, W // 2)
    ambiguous, bracketed = sr.check_splat(got, oracle, ref)
    assert ambiguous <= sr.MAX_AMBIGUOUS_POINTS and bracketed <= sr.MAX_BRACKETED_CELLS
    # non-finite and non-positive depths leave every other cell alone: the same inputs with those pixels set to 0 give the same map
    bad = ~torch.isfinite(case["depth"]) | (case["depth"] < 0)
    if bool(bad.any()):
        cleaned = torch.where(bad, torch.zeros_like(case["depth"]), case["depth"])
        ref_cleaned = sr.splat_reference(case["T"], cleaned, case["full_K"], case["half_K"])
        same = ~ref.bracketed & ~ref_cleaned.bracketed
        assert torch.equal(got.cpu()[:, 0][torch.from_numpy(same)],
                           ops.depth_reproject(dargs[0], cleaned.to(hip_device), *dargs[2:]).cpu()[:, 0][torch.from_numpy(same)])


@pytest.mark.parametrize("name", sorted(sr.EXACT_CASES))
def test_exact_ties_round_half_to_even_in_every_form(hip_device, ops, name):
    """Inputs whose arithmetic is exact in float32: coordinates ON n + 0.5 and on the border -0.5 (rintf gives -0.0, which is inside).
    Nothing is ambiguous here, so the map equals the float64 splat bit for bit, and so does every low-resolution form."""
    case = sr.exact_case(name)
    args = [case[k] for k in ("T", "depth", "full_K", "half_K")]
    ref = sr.splat_reference(*args)
    dargs = [a.to(hip_device) for a in args]
    full = ops.depth_reproject(*dargs)
    differ = full.cpu().double().numpy()[:, 0] != ref.exact
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} cells differ from the exact splat, first at {tuple(int(a[0]) for a in np.nonzero(differ))}"
    B, hh, hw = ref.shape
    for f in sr.valid_factors(name):
        want = sr.decimated(torch.from_numpy(ref.exact).float()[:, None], f).to(hip_device)
        assert torch.equal(ops.depth_reproject_lowres(*dargs, f)[1], want), (name, f)
        est, intact = carved(tuple(want.shape), hip_device, 0.0)
        assert torch.equal(ops.depth_reproject_estimate_into(*dargs, est, None, f), want) and intact(), (name, f)
        zbuffer = torch.zeros(B, hh, hw, device=hip_device)
        assert torch.equal(ops.depth_reproject_lowres_into(*dargs, zbuffer, torch.empty_like(want), f), want), (name, f)
        assert float(zbuffer.abs().max()) == 0.0


@pytest.mark.parametrize("name", sr.TWO_LAYER_CASES)
def test_the_far_surface_wins_an_occluded_cell(hip_device, ops, name):
    case, dargs, ref, oracle = prepared(name, hip_device)
    got = ops.depth_reproject(*dargs).cpu().double().numpy()[:, 0]
    both, far_z, near_z = sr.layer_cells(ref, case["near"])
    print(f"{name}: {int(both.sum())} cells receive certain points of both layers")
    assert both.sum() >= 40
    tol = 3.0 * float(np.abs(oracle.double().numpy()[:, 0][both] - far_z[both]).max()) + 2e-6
    assert (np.abs(got[both] - far_z[both]) <= tol).all(), f"{int((np.abs(got[both] - far_z[both]) > tol).sum())} cells do not hold the far layer's z"
    assert (got[both] > near_z[both] + 1.0).all()          # the layers are metres apart: this is not a rounding matter


# ---- the low-resolution forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sr.SPLAT_CASES))
def test_lowres_forms_equal_the_decimated_full_splat(hip_device, ops, name):
    case, dargs, ref, oracle = prepared(name, hip_device)
    dev = hip_device
    B, _, H, W = case["depth"].shape
    hh, hw = H // 2, W // 2
    full = ops.depth_reproject(*dargs)
    for f in sr.valid_factors(name):
        want = sr.decimated(full, f)
        assert tuple(want.shape) == (B, 1, hh // f, hw // f)
        both, low = ops.depth_reproject_lowres(*dargs, f)
        assert torch.equal(both, full) and torch.equal(low, want), (name, f)
        zbuffer, z_intact = carved((B, hh, hw), dev, 0.0)
        out, out_intact = carved((B, 1, hh // f, hw // f), dev, -1.0)
        for n in range(3):          # the same buffers again: the z-buffer comes back all-zero every time
            ops.depth_reproject_lowres_into(*dargs, zbuffer, out, f)
            assert torch.equal(out, want), (name, f, n)
            assert float(zbuffer.abs().max()) == 0.0, (name, f, n)
        assert z_intact() and out_intact(), (name, f)


@pytest.mark.parametrize("name", sorted(sr.SPLAT_CASES))
def test_estimate_form_equals_the_decimated_full_splat(hip_device, ops, name):
    case, dargs, ref, oracle = prepared(name, hip_device)
    dev = hip_device
    B, _, H, W = case["depth"].shape
    hh, hw = H // 2, W // 2
    full = ops.depth_reproject(*dargs)
    for f in sr.valid_factors(name):
        want = sr.decimated(full, f)
        shape = (B, 1, hh // f, hw // f)
        (a, a_intact), (b, b_intact) = carved(shape, dev, 0.0), carved(shape, dev, 7.0)
        est = [a, b]
        for n in range(4):          # two buffers alternating: each launch splats into one and zero-fills the other
            cur, other = est[n % 2], est[1 - n % 2]
            ops.depth_reproject_estimate_into(*dargs, cur, other, f)
            assert torch.equal(cur, want), (name, f, n)
            assert float(other.abs().max()) == 0.0, (name, f, n)
            assert a_intact() and b_intact(), (name, f, n)
        # without a buffer to clear
        alone, alone_intact = carved(shape, dev, 0.0)
        ops.depth_reproject_estimate_into(*dargs, alone, None, f)
        assert torch.equal(alone, want) and alone_intact(), (name, f)


@pytest.mark.parametrize("name", sr.TWO_LAYER_CASES)
def test_every_form_is_bit_equal_run_to_run(hip_device, ops, name):
    """The atomic max on the bits of relu(z) does not depend on the order of arrival: two runs are equal exactly."""
    case, dargs, ref, oracle = prepared(name, hip_device)
    B, _, H, W = case["depth"].shape
    f = 3
    shape = (B, 1, H // 2 // f, W // 2 // f)

    def run():
        full = ops.depth_reproject(*dargs)
        _, low = ops.depth_reproject_lowres(*dargs, f)
        into = ops.depth_reproject_lowres_into(*dargs, torch.zeros(B, H // 2, W // 2, device=hip_device), torch.empty(shape, device=hip_device), f)
        est = ops.depth_reproject_estimate_into(*dargs, torch.zeros(shape, device=hip_device), None, f)
        return [t.clone() for t in (full, low, into, est)]
    first = run()
    for _ in range(3):
        for x, y in zip(first, run()):
            assert torch.equal(x, y)
    assert torch.equal(first[1], first[2]) and torch.equal(first[1], first[3])


def test_lowres_and_estimate_entry_points_reject_invalid_arguments_without_a_launch(hip_device):
    from dvmvs.hip import _capi
    lib = _capi.lib()
    x = torch.full((4096,), 7.0, device=hip_device)
    p, s = x.data_ptr(), torch.cuda.current_stream(hip_device).cuda_stream
    q = p + 2048 * 4
    for entry in (lib.dvmvs_depth_reproject_lowres_fwd, lib.dvmvs_depth_reproject_estimate_fwd):
        assert entry(p, p, p, p, p, q, 4, 1, 6, 10, s) == EINVAL            # 3x5 at half resolution: factor 4 leaves no row
        assert entry(p, p, p, p, p, q, 6, 1, 12, 10, s) == EINVAL           # 6x5: factor 6 leaves no column
        assert entry(p, p, p, p, p, q, 2, 1, 2, 2, s) == EINVAL             # 1x1: any factor above 1
        assert entry(p, p, p, p, p, q, 0, 1, 8, 8, s) == EINVAL and entry(p, p, p, p, p, q, -3, 1, 8, 8, s) == EINVAL
        assert entry(p, p, p, p, p, q, 1, 0, 8, 8, s) == EINVAL and entry(p, p, p, p, p, q, 1, -1, 8, 8, s) == EINVAL
        assert entry(p, p, p, p, p, q, 1, 1, 1, 8, s) == EINVAL and entry(p, p, p, p, p, q, 1, 1, 8, 1, s) == EINVAL
        for hole in range(5):
            args = [p, p, p, p, p]
            args[hole] = None
            assert entry(*args, q, 1, 1, 8, 8, s) == EINVAL, hole
    assert lib.dvmvs_depth_reproject_lowres_fwd(p, p, p, p, p, None, 1, 1, 8, 8, s) == EINVAL
    assert lib.dvmvs_depth_reproject_estimate_fwd(p, p, p, p, p, p, 1, 1, 8, 8, s) == EINVAL      # estimate == the buffer to clear
    torch.cuda.synchronize(hip_device)
    assert bool((x == 7.0).all())


# ---- TSDF integration ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sr.TSDF_VOLUMES))
def test_tsdf_integrate_matches_the_oracle_on_non_cubic_volumes(hip_device, name):
    from dvmvs.tsdf import TSDFVolume
    bounds, voxel, frames = sr.tsdf_case(name)
    dims = sr.TSDF_VOLUMES[name][0]
    vol = TSDFVolume(bounds.copy(), voxel, device=hip_device)
    assert tuple(int(d) for d in vol.vol_dim) == dims
    if name.startswith("grid_stride"):
        assert dims[0] * dims[1] * dims[2] > 16384 * 256 and len(set(dims)) == 3
    o_tsdf, o_weight, o_color = np.ones(dims, np.float32), np.zeros(dims, np.float32), np.zeros(dims, np.float32)
    trunc = 5 * voxel
    for n, (rgb, depth, K, pose, w) in enumerate(frames):
        vol.integrate(rgb, depth, K, pose, obs_weight=w)
        updated = tso.integrate(o_tsdf, o_weight, o_color, bounds[:, 0], voxel, K, pose, tso.fold_color(rgb), depth, trunc, obs_weight=w)
        assert updated.mean() > 0.02, "the frame does not reach the volume"
        tsdf, color = vol.get_volume()
        weight = vol.get_weight_volume()
        differs = (weight != o_weight) | (color != o_color) | (np.abs(tsdf - o_tsdf) > 1e-6)
        if differs.any():           # say whose fault it is before the assertion fires
            first = tuple(int(a[0]) for a in np.nonzero(differs))
            print(f"{name}, frame {n}: {sr.tsdf_explain(differs, dims, bounds[:, 0], voxel, frames[n], trunc)}; first at voxel {first}: "
                  f"weight {weight[first]} / {o_weight[first]}, colour {color[first]} / {o_color[first]}, tsdf {tsdf[first]} / {o_tsdf[first]}")
        assert np.array_equal(weight, o_weight) and np.array_equal(color, o_color), (name, n)   # same pixels, same integer colour mix
        np.testing.assert_allclose(tsdf, o_tsdf, atol=1e-6, rtol=0)
    # what the six frames were meant to exercise did happen
    b, g, r = np.floor(o_color / 65536), np.floor(o_color / 256) % 256, o_color % 256
    seen = o_weight > 0
    for channel in (b, g, r):
        assert channel[seen].min() == 0 and channel[seen].max() == 255
    assert len(np.unique(o_weight)) > 6 and (~seen).any() and (o_tsdf[seen] < 1).any()
