"""Pins tests/splat_reference.py on the CPU: the float64 splat reference reproduces the hand-checked scalar evaluator and the
reference-generated golden, the float32 oracle passes the comparison rule on every case of tests/test_geometry_kernels_gpu.py (so a
failure there is the kernel's), and every case respects the caps on its share of ambiguous points and bracketed cells.  The same
for the float64 restatement of the TSDF oracle: in float32 it is the oracle, bit for bit.

(The scalar evaluator and its three cases are imported from test_kornia_kats.py rather than copied: the point is to be held to the
very transcription that is checked by hand there.)"""
import os

import numpy as np
import pytest
import torch

import splat_reference as sr
import synthetic as syn
import tsdf_oracle as tso
from test_kornia_kats import by_the_book_splat, splat_cases, t32


@pytest.mark.parametrize("name", sorted(splat_cases().keys()))
def test_reference_reproduces_the_scalar_evaluator(name):
    depth, T, fK, hK = splat_cases()[name]
    ref = sr.splat_reference(t32(T)[None], t32(depth)[None, None], t32(fK)[None], t32(hK)[None])
    np.testing.assert_allclose(ref.exact[0], by_the_book_splat(depth, T, fK, hK), rtol=0, atol=1e-12)
    # these inputs sit on ties on purpose (x / 2 for odd x): the reference must say so, and must bracket what it cannot decide
    assert (ref.lo <= ref.exact).all() and (ref.exact <= ref.hi).all()
    if name == "parity":
        assert ref.ambiguous[0][:, 1::2].all() and not ref.ambiguous[0][::2, ::2].any()
    oracle = sr.oracle_splat(t32(T)[None], t32(depth)[None, None], t32(fK)[None], t32(hK)[None])
    sr.check_splat(oracle, oracle, ref)


def test_reference_reproduces_the_reference_generated_golden(golden_dir, fixture_host_algebra):
    z = np.load(os.path.join(golden_dir, "reproject.npz"))
    fullK = syn.full_K()
    halfK = syn.scaled_K(fullK, 2.0)
    T = fixture_host_algebra.relative_pose_host(syn.pose(10), syn.pose(9))
    ref = sr.splat_reference(T, syn.analytic_depth(), fullK, halfK)
    golden = torch.from_numpy(z["kat"])
    sr.assert_caps(ref, "golden kat")
    sr.check_splat(golden, golden, ref)
    clean = ~ref.bracketed[0]
    np.testing.assert_allclose(z["kat"][0, 0][clean], ref.lo[0][clean], rtol=0, atol=2e-6)
    assert ((z["kat"][0, 0] != 0) == (ref.exact[0] != 0))[clean].all()


@pytest.mark.parametrize("name", sorted(sr.SPLAT_CASES))
def test_oracle_passes_the_rule_and_the_case_respects_the_caps(name):
    case = sr.splat_case(name)
    H, W, B = sr.SPLAT_CASES[name][:3]
    assert tuple(case["depth"].shape) == (B, 1, H, W)
    if B > 1:       # every batch item is its own problem
        assert not torch.equal(case["T"][0], case["T"][1]) and not torch.equal(case["half_K"][0], case["half_K"][1])
    ref = sr.splat_reference(case["T"], case["depth"], case["full_K"], case["half_K"])
    sr.assert_caps(ref, name, sr.min_landing(name))
    oracle = sr.oracle_splat(case["T"], case["depth"], case["full_K"], case["half_K"])
    shares = sr.check_splat(oracle, oracle, ref)
    assert shares == (ref.ambiguous_share, ref.bracketed_share)
    motion, kind = sr.SPLAT_CASES[name][3:5]
    if motion == "behind":
        assert (ref.z == 0).mean() >= 1.0 / 3.0
    if motion == "outside":
        assert ref.landing_share < 0.5
    if kind == "two_layer":
        both, far_z, near_z = sr.layer_cells(ref, case["near"])
        assert both.sum() >= 40 and (far_z[both] > near_z[both]).all()
        np.testing.assert_array_equal(ref.lo[both], far_z[both])


@pytest.mark.parametrize("name", sorted(sr.EXACT_CASES))
def test_exact_tie_cases_are_exact_and_sit_on_ties(name):
    """Exact arithmetic in both precisions: the float32 oracle equals the float64 splat bit for bit, a good share of the landing
    points sits exactly on n + 0.5, some on the border -0.5 (which half-to-even keeps, as -0.0), and rounding half away from zero
    would give another map."""
    case = sr.exact_case(name)
    args = [case[k] for k in ("T", "depth", "full_K", "half_K")]
    ref = sr.splat_reference(*args)
    assert np.array_equal(sr.oracle_splat(*args).double().numpy()[:, 0], ref.exact)
    B, hh, hw = ref.shape
    on_tie = ((ref.u - np.floor(ref.u) == 0.5) | (ref.v - np.floor(ref.v) == 0.5)) & ref.lands
    assert on_tie.mean() > 0.15 and (((ref.u == -0.5) | (ref.v == -0.5)) & ref.lands).sum() >= 2
    away = lambda c: np.where(c >= 0, np.floor(c + 0.5), np.ceil(c - 0.5))
    j, i = away(ref.u), away(ref.v)
    ok = (j >= 0) & (j < hw) & (i >= 0) & (i < hh) & (ref.z > 0)
    other = np.zeros(ref.shape)
    b = np.broadcast_to(np.arange(B)[:, None, None], ok.shape)
    np.maximum.at(other, (b[ok], i[ok].astype(int), j[ok].astype(int)), ref.z[ok])
    print(f"{name}: {100 * on_tie.mean():.1f} % of the points land from an exact tie; half away from zero would change {int((other != ref.exact).sum())} "
          f"of {other.size} cells")
    assert (other != ref.exact).mean() > 0.1


def test_the_rule_rejects_what_it_must():
    """One moved point, a near surface winning, a value that is nobody's z, a filled empty cell: each is refused."""
    name = "lateral_130x98_two_layer_b3"
    case = sr.splat_case(name)
    ref = sr.splat_reference(case["T"], case["depth"], case["full_K"], case["half_K"])
    oracle = sr.oracle_splat(case["T"], case["depth"], case["full_K"], case["half_K"])
    both, far_z, near_z = sr.layer_cells(ref, case["near"])
    b, i, j = (int(a[0]) for a in np.nonzero(both))
    wrong = oracle.clone()
    wrong[b, 0, i, j] = float(near_z[b, i, j])                      # the near layer wins one cell
    with pytest.raises(AssertionError):
        sr.check_splat(wrong, oracle, ref)
    br = np.nonzero(ref.bracketed & (ref.lo > 0))
    b, i, j = (int(a[0]) for a in br)
    wrong = oracle.clone()
    wrong[b, 0, i, j] = 0.0                                         # a bracketed cell emptied although a certain point lands there
    with pytest.raises(AssertionError):
        sr.check_splat(wrong, oracle, ref)
    wrong = oracle.clone()
    wrong[b, 0, i, j] = float(ref.hi[b, i, j]) + 0.01               # above every candidate
    with pytest.raises(AssertionError):
        sr.check_splat(wrong, oracle, ref)
    wide = np.nonzero(ref.bracketed & (ref.hi - ref.lo > 0.05))
    if len(wide[0]):
        b, i, j = (int(a[0]) for a in wide)
        wrong = oracle.clone()
        wrong[b, 0, i, j] = float(0.5 * (ref.lo[b, i, j] + ref.hi[b, i, j]))    # inside the bracket, but nobody's z
        with pytest.raises(AssertionError):
            sr.check_splat(wrong, oracle, ref)
    empty = np.nonzero(~ref.bracketed & (ref.lo == 0))
    b, i, j = (int(a[0]) for a in empty)
    wrong = oracle.clone()
    wrong[b, 0, i, j] = 1e-3
    with pytest.raises(AssertionError):
        sr.check_splat(wrong, oracle, ref)
    shifted = torch.roll(oracle, 1, dims=-1)                        # every point one cell to the right
    with pytest.raises(AssertionError):
        sr.check_splat(shifted, oracle, ref)


def test_decimation_helper():
    x = torch.arange(2 * 18 * 26, dtype=torch.float32).reshape(2, 1, 18, 26)
    for f in sr.FACTORS:
        d = sr.decimated(x, f)
        assert tuple(d.shape) == (2, 1, 18 // f, 26 // f)
        for (i, j) in ((0, 0), (18 // f - 1, 26 // f - 1), (18 // f - 1, 0)):
            assert float(d[1, 0, i, j]) == float(x[1, 0, i * f, j * f])
    assert sr.valid_factors("tiny_2x2") == [1] and sr.valid_factors("tiny_3x5") == [1] and sr.valid_factors("scene_37x53_two_layer_b3") == [1, 2, 3, 5, 16]


def test_tsdf_restatement_is_the_oracle_in_float32_and_close_in_float64():
    name = "odd_37x53x29"
    bounds, voxel, frames = sr.tsdf_case(name)
    dims = tuple(int(d) for d in np.ceil((bounds[:, 1] - bounds[:, 0]) / voxel))
    assert dims == sr.TSDF_VOLUMES[name][0]
    fresh = lambda t: [np.ones(dims, t), np.zeros(dims, t), np.zeros(dims, t)]
    a, b, c = fresh(np.float32), fresh(np.float32), fresh(np.float64)
    behind = 0
    for n, (rgb, depth, K, pose, w) in enumerate(frames):
        folded = tso.fold_color(rgb)
        assert folded.min() == 0 and folded.max() == 255 * 65536 + 255 * 256 + 255 and (depth == 0).any()
        ok = tso.integrate(*a, bounds[:, 0], voxel, K, pose, folded, depth, 5 * voxel, obs_weight=w)
        ok32 = sr.tsdf_integrate(*b, bounds[:, 0], voxel, K, pose, folded, depth, 5 * voxel, w)[0]
        ok64, _, _, _ = sr.tsdf_integrate(*c, bounds[:, 0], voxel, K, pose, folded, depth, 5 * voxel, w, np.float64)
        assert np.array_equal(ok, ok32) and all(np.array_equal(x, y) for x, y in zip(a, b))
        assert ok.sum() > 2000 and (ok != ok64).mean() < 1e-3
        differs = ok != ok64
        print(f"frame {n}: {int(ok.sum())} voxels updated; float32 vs float64: {sr.tsdf_explain(differs, dims, bounds[:, 0], voxel, frames[n], 5 * voxel)}")
        world = np.stack(np.meshgrid(*[bounds[k, 0] + voxel * np.arange(dims[k]) for k in range(3)], indexing="ij"), -1)
        behind = max(behind, int((((world - pose[:3, 3]) @ pose[:3, 2]) < 0).sum()) if n == 3 else 0)
    assert behind > 1000, "the camera of frame 3 is inside the volume: there are voxels behind it"
    assert len(np.unique(a[1])) > 6 and (a[0] < 1).sum() > 10000
