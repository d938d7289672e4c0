"""CPU: the numpy restatement of the depth-map consistency filter (tests/consistency_reference.py) -- the caps on the shared scenes, the
float32 form against the float64 form, known answers, and ``dvmvs.consistency.nearest_sources``."""
import numpy as np
import pytest

import consistency_reference as cr

# Largest relative deviation of the float32 restatement's fused depth from the float64 form on the shipped scenes, over the pixels that are
# valid, unambiguous and have equal counts: measured 5.4e-7 (24x32), 4.7e-7 (23x37), 9.2e-7 (64x80).  The bound is 4 x the largest; the
# margin covers a scene changed later.
FUSED_MEASURED, FUSED_BOUND = 9.2e-7, 4 * 9.2e-7


@pytest.mark.parametrize("name", list(cr.SIZES))
def test_caps_hold(name):
    figures = cr.check_caps(name)
    print(f"{name}: ambiguous share per frame {figures['ambiguous'].round(4)}, count >= 2 on {figures['kept']:.3f} of the valid pixels, "
          f"{figures['patch_kept']} pixels of the scaled patch kept")


@pytest.mark.parametrize("name", list(cr.SIZES))
def test_float32_form_against_float64_form(name):
    depths = cr.scene(name)[0]
    r32, r64 = cr.scene_result(name, "float32"), cr.scene_result(name, "float64")
    unambiguous = ~r64["ambiguous"]
    differ = r32["count"] != r64["count"]
    print(f"{name}: counts differ at {int(differ.sum())} pixels, {int((differ & unambiguous).sum())} of them unambiguous")
    assert not (differ & unambiguous).any()
    m = cr._valid(depths) & unambiguous & ~differ
    assert m.sum() > 0.9 * cr._valid(depths).sum()
    deviation = np.abs(r32["fused"][m].astype(np.float64) - r64["fused"][m]) / r64["fused"][m]
    print(f"{name}: fused depth, float32 from float64, relative: max {deviation.max():.3e} (bound {FUSED_BOUND:.3e})")
    assert deviation.max() <= FUSED_BOUND
    # an invalid pixel gives 0 / 0 / zeros in both forms
    for r in (r32, r64):
        bad = ~cr._valid(depths)
        assert bad.sum() >= 3 and not r["depth"][bad].any() and not r["count"][bad].any() and not r["points"][bad].any()


# ---- known answers ----------------------------------------------------------------------------------------------------------------
H, W, FOCAL = 12, 16, 30.0


def _flat(n, value=1.5):
    """n views from ONE pose of a constant map.  1.5 u and 1.5 v are exact in float32 and so is (1.5 u) / 1.5; k * 1.5 is exact for the
    sums, so everything below is exact by construction."""
    K = np.stack([cr.intrinsics(H, W, FOCAL)] * n)
    poses = np.stack([np.eye(4, dtype=np.float32)] * n)
    return np.full((n, H, W), value, np.float32), K, poses


def test_identical_views_agree_everywhere():
    depths, K, poses = _flat(5)
    depths[2, 3, 4] = 0.0
    sources = np.array([[1, 3, 4, 1], [0, 3, 4, 0], [0, 1, 3, 4], [0, 1, 4, 4], [0, 1, 3, 3]], np.int32)     # (a frame named twice counts twice)
    r = cr.depth_consistency(depths, K, poses, sources, min_views=4)
    interior = np.zeros((5, H, W), bool)
    interior[:, 1:-1, 1:-1] = True
    interior &= cr._valid(depths)
    # K K^-1 leaves a residue of ~1e-16 in A's last column, which only matters on the image border: hence "interior"
    assert (r["count"][interior] == 4).all() and np.array_equal(r["depth"][interior], depths[interior])
    assert np.array_equal(r["fused"][interior], depths[interior])
    assert r["count"][2, 3, 4] == 0 and r["depth"][2, 3, 4] == 0
    # frame 2 is nobody's source here, so its hole costs no other view a pixel; as a source it costs the taps around it
    r2 = cr.depth_consistency(depths, K, poses, np.array([[2], [2], [0], [2], [2]], np.int32), min_views=1)
    assert r2["count"][0, 3, 4] == 0 and r2["count"][0, 3, 3] == 0 and r2["count"][0, 6, 6] == 1 and r2["count"][2, 6, 6] == 1


def test_source_behind_the_camera_and_source_that_looks_elsewhere():
    depths, K, poses = _flat(3)
    poses[1, :3, :3] = np.diag([-1.0, 1.0, -1.0])        # turned by 180 degrees about y: the points lie behind it
    poses[2, 0, 3] = 100.0                                # 100 m to the side: the points leave its image
    sources = np.array([[1], [0], [0]], np.int32)
    r = cr.depth_consistency(depths, K, poses, sources, min_views=1)
    assert not r["count"].any() and not r["depth"].any() and not r["points"].any()
    sources = np.array([[2], [0], [0]], np.int32)
    r = cr.depth_consistency(depths, K, poses, sources, min_views=1)
    assert not r["count"][0].any() and not r["depth"][0].any()


@pytest.mark.parametrize("average", [False, True])
def test_min_views_zero_keeps_every_valid_pixel(average):
    depths, K, poses, sources = cr.scene("24x32")
    r = cr.depth_consistency(depths, K, poses, sources, min_views=0, average=average)
    valid = cr._valid(depths)
    assert ((r["depth"] > 0) == valid).all()
    assert np.array_equal(r["depth"][valid], (r["fused"] if average else depths)[valid])
    assert (np.abs(r["points"][valid]).sum(-1) > 0).all() and not r["points"][~valid].any()


def test_a_skipped_slot_changes_nothing():
    depths, K, poses, sources = cr.scene("24x32")
    want = cr.scene_result("24x32", "float32")
    own = np.arange(6, dtype=np.int32)[:, None]
    wide = np.concatenate([np.full((6, 1), -1, np.int32), sources[:, :2], own, sources[:, 2:], np.full((6, 1), 6, np.int32)], axis=1)
    got = cr.depth_consistency(depths, K, poses, wide)
    for key in ("depth", "count", "points"):
        assert np.array_equal(got[key], want[key], equal_nan=True)
    assert not cr.consistency_matrices(K, poses, wide)[:, [0, 3, 6]].any()        # skipped slots are zeros


def test_a_map_without_a_tap_cell_has_no_consistent_slot():
    depths, K, poses = _flat(2)
    r = cr.depth_consistency(depths[:, :1], K, poses, np.array([[1], [0]], np.int32), min_views=0)
    assert not r["count"].any() and np.array_equal(r["depth"], depths[:, :1])


# ---- nearest_sources --------------------------------------------------------------------------------------------------------------
def test_nearest_sources():
    from dvmvs.consistency import nearest_sources
    assert nearest_sources(1, 4).tolist() == [[-1, -1, -1, -1]]
    assert nearest_sources(2, 4).tolist() == [[1, -1, -1, -1], [0, -1, -1, -1]]
    # ties go to the lower index first
    assert nearest_sources(5, 4).tolist() == [[1, 2, 3, 4], [0, 2, 3, 4], [1, 3, 0, 4], [2, 4, 1, 0], [3, 2, 1, 0]]
    assert nearest_sources(5, 2).tolist() == [[1, 2], [0, 2], [1, 3], [2, 4], [3, 2]]
    # choices never cross a segment boundary
    assert nearest_sources(5, 4, [0, 0, 1, 1, 1]).tolist() == [[1, -1, -1, -1], [0, -1, -1, -1], [3, 4, -1, -1], [2, 4, -1, -1], [3, 2, -1, -1]]
    table = nearest_sources(5, 4)
    assert table.dtype == np.int32 and table.shape == (5, 4) and nearest_sources(3, 0).shape == (3, 0)
    with pytest.raises(ValueError):
        nearest_sources(3, 2, [0, 0])
