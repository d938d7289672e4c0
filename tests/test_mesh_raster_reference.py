"""CPU: the numpy definitions of the mesh rasteriser and of the vertex visibility (tests/mesh_raster_reference.py) against answers worked
out by hand, and the float32 restatement against the float64 reference within the bounds derived in that module's docstring."""
import numpy as np
import pytest

import mesh_raster_reference as R


def raster(case, **kwargs):
    verts, faces, K, P, H, W = case
    return R.raster_fp32(verts, faces, K, R.world_to_camera(P), H, W, **kwargs)


@pytest.fixture(scope="module")
def hand():
    return R.hand_cases()


def pixels_of(face_map, f):
    vs, us = np.nonzero(face_map == f)
    return sorted(zip(us.tolist(), vs.tolist()))


def test_top_left_rule_on_all_eight_edge_directions(hand):
    depth, face, overflow = raster(hand["fan"])
    for f, expected in R.FAN_PIXELS.items():
        assert pixels_of(face[0], f) == sorted(expected), f"face {f}"
    assert (face[0] >= 0).sum() == 16 and np.all(face[0, 2:6, 2:6] >= 0)         # the square [2,6)^2, once each, nothing else
    assert np.all(depth[0][face[0] >= 0] == np.float32(2.0)) and np.all(depth[0][face[0] < 0] == 0)
    assert overflow.tolist() == [0]


def test_quad_of_two_triangles_covers_every_sample_once(hand):
    verts, faces, K, P, H, W = hand["quad"]
    _, face, _ = raster(hand["quad"])
    assert len(pixels_of(face[0], 0)) == 10 and len(pixels_of(face[0], 1)) == 6
    assert np.all(face[0, 2:6, 2:6] >= 0) and (face[0] >= 0).sum() == 16
    # each triangle alone covers what it covers in the pair: no sample of the shared edge belongs to both or to neither
    alone = [R.raster_fp32(verts, faces[i:i + 1], K, R.world_to_camera(P), H, W)[1][0] >= 0 for i in range(2)]
    assert not np.any(alone[0] & alone[1]) and np.array_equal(alone[0] | alone[1], face[0] >= 0)
    assert pixels_of(face[0], 0) == sorted((u, v) for v in range(2, 6) for u in range(2, 6) if u + v < 8)


def test_triangles_that_cross_the_near_plane(hand):
    """The floor: face 0 has two corners behind the camera, face 1 one; rows 35.. are covered entirely, at z = 32 / (v - 24)."""
    depth, face, overflow = raster(hand["floor"])
    assert overflow.tolist() == [0]
    assert np.all(face[0, :35] == -1) and np.all(depth[0, :35] == 0)
    assert np.all(face[0, 35:] >= 0)
    v = np.arange(35, 48, dtype=np.float64)
    expected = 32.0 / (v - 24.0)
    assert np.allclose(depth[0, 35:], expected[:, None], rtol=1e-5, atol=0)
    # the diagonal from (-2, -1) to (2, 3) in (x, z): face 0 on the side x > z - 1
    u = np.arange(64, dtype=np.float64)
    x = (u[None, :] - 32.0) / 64.0 * expected[:, None]
    side = x - (expected[:, None] - 1.0)
    clear = np.abs(side) > 1e-3
    assert np.array_equal(face[0, 35:][clear], np.where(side > 0, 0, 1)[clear])
    # each face alone: one piece for face 0, two for face 1, and together exactly the pair's coverage
    verts, faces, K, P, H, W = hand["floor"]
    alone = [R.raster_fp32(verts, faces[i:i + 1], K, R.world_to_camera(P), H, W)[1][0] >= 0 for i in range(2)]
    assert alone[0].any() and alone[1].any() and not np.any(alone[0] & alone[1])
    assert np.array_equal(alone[0] | alone[1], face[0] >= 0)


def test_triangle_behind_the_camera_leaves_nothing(hand):
    depth, face, overflow = raster(hand["behind"])
    assert np.all(depth == 0) and np.all(face == -1) and overflow.tolist() == [0]


def test_equal_depths_go_to_the_lowest_face_index(hand):
    depth, face, _ = raster(hand["duplicates"])
    assert set(np.unique(face)) == {-1, 0}
    verts, faces, K, P, H, W = hand["duplicates"]
    single = R.raster_fp32(verts, faces[:1], K, R.world_to_camera(P), H, W)
    assert np.array_equal(single[0], depth) and np.array_equal(single[1], face)


def test_overflowing_triangle_is_counted_and_left_out(hand):
    depth, face, overflow = raster(hand["overflow"])
    assert overflow.tolist() == [1]
    assert set(np.unique(face)) == {-1, 1}


def test_far_and_backface_culling(hand):
    depth, face, _ = raster(hand["fan"], far=1.5)
    assert np.all(face == -1) and np.all(depth == 0)
    verts, faces, K, P, H, W = hand["fan"]
    front = raster(hand["fan"], cull_backfaces=True)[1]
    back = R.raster_fp32(verts, faces[:, ::-1], K, R.world_to_camera(P), H, W, cull_backfaces=True)[1]
    assert ((front >= 0).sum(), (back >= 0).sum()) in ((16, 0), (0, 16))


def test_faces_with_bad_indices_are_skipped(hand):
    verts, faces, K, P, H, W = hand["fan"]
    bad = np.concatenate([np.array([[0, 1, 99], [-1, 2, 3]], dtype=np.int32), faces])
    _, face, _ = R.raster_fp32(verts, bad, K, R.world_to_camera(P), H, W)
    assert np.array_equal(np.where(face >= 0, face - 2, -1), raster(hand["fan"])[1])


@pytest.mark.parametrize("name", ["grid", "soup"])
def test_restatement_against_float64(name):
    verts, faces, K, P, H, W = R.random_case(name)
    assert len(faces) == (384 if name == "grid" else 300)
    depth, face, overflow = R.raster_fp32(verts, faces, K, R.world_to_camera(P), H, W)
    excluded = R.compare_with_f64(depth[0:1], face[0:1], R.random_reference(name))
    print(f"{name}: {100 * excluded:.2f} % of the pixels excluded")
    assert excluded <= R.MAX_EXCLUDED
    assert overflow.tolist() == [0] and (face >= 0).mean() > (0.9 if name == "grid" else 0.2)


def test_restatement_does_not_depend_on_the_order_of_the_faces():
    verts, faces, K, P, H, W = R.random_case("soup")
    order = np.random.default_rng(5).permutation(len(faces))
    a = R.raster_fp32(verts, faces, K, R.world_to_camera(P), H, W)
    b = R.raster_fp32(verts, faces[order], K, R.world_to_camera(P), H, W)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], np.where(b[1] >= 0, order[np.maximum(b[1], 0)], -1))


# ---- visibility -------------------------------------------------------------------------------------------------------
def one_view_depth(value=2.0, H=48, W=64):
    return np.full((1, H, W), value, dtype=np.float32)


def count(points, depth, **kwargs):
    K, P = R.exact_camera()
    return R.visibility_fp32(np.asarray(points, dtype=np.float32), depth, K, R.world_to_camera(P), **kwargs).tolist()


def test_visibility_clauses():
    d = one_view_depth(2.0)
    on_axis = lambda z: [0.0, 0.0, z]                                            # noqa: E731  projects to (32, 24)
    assert count([on_axis(2.0), on_axis(2.019), on_axis(2.021), on_axis(1.0)], d) == [1, 1, 0, 1]      # z <= D (1 + 0.01)
    assert count([on_axis(2.05)], d, relative=0.0, absolute=0.05) == [1] and count([on_axis(2.06)], d, relative=0.0, absolute=0.05) == [0]
    assert count([on_axis(0.04), on_axis(-1.0)], d) == [0, 0]                    # z >= near
    assert count([on_axis(0.04)], d, near=0.03) == [1]
    # inside the image: x_p in [0, 63], y_p in [0, 47] for the exact camera (f = 64, centre (32, 24)) at z = 2
    assert count([[-1.0, 0.0, 2.0], [-1.01, 0.0, 2.0], [31.0 / 32.0, 0.0, 2.0], [31.5 / 32.0, 0.0, 2.0]], d) == [1, 0, 1, 0]
    assert count([[0.0, -0.75, 2.0], [0.0, -0.76, 2.0], [0.0, 23.0 / 32.0, 2.0], [0.0, 23.5 / 32.0, 2.0]], d) == [1, 0, 1, 0]


def test_visibility_takes_the_largest_positive_depth_of_the_2x2_pixels():
    d = np.zeros((1, 48, 64), dtype=np.float32)
    p = [[0.5 / 32.0, 0.5 / 32.0, 2.0]]                                          # projects to (32.5, 24.5)
    assert count(p, d) == [0]                                                    # nothing rendered there
    for y, x in ((24, 32), (24, 33), (25, 32), (25, 33)):
        d[:] = 0
        d[0, y, x] = 2.0
        assert count(p, d) == [1]
    d[:] = 1.0
    assert count(p, d) == [0]
    d[0, 25, 33] = 2.0
    assert count(p, d) == [1]                                                    # the maximum, not the nearest sample
    d[0, 25, 33] = np.nan
    assert count(p, d) == [0]
    # at the last column / row only the pixels inside the image are looked at
    d[:] = 2.0
    assert count([[31.0 / 32.0, 23.0 / 32.0, 2.0]], d) == [1]


def test_visibility_counts_views():
    K, P = R.views(3)
    verts = np.array([[0.0, 0.0, 3.0], [0.0, 0.0, -3.0]], dtype=np.float32)
    depth = np.full((3, 48, 64), 10.0, dtype=np.float32)
    depth[1] = 0.5
    assert R.visibility_fp32(verts, depth, K, R.world_to_camera(P)).tolist() == [2, 0]


def test_two_walls_hidden_vertices_are_not_seen():
    verts, faces, K, P, H, W, n_near = R.two_walls()
    w2c = R.world_to_camera(P)
    depth, face, _ = R.raster_fp32(verts, faces, K, w2c, H, W)
    seen = R.visibility_fp32(verts, depth, K, w2c)
    assert np.all(seen[:n_near] == 1)                                            # the near wall, its rim included (the 2x2 maximum)
    far = verts[n_near:]
    inside = (np.abs(far[:, 0]) <= 2.0) & (np.abs(far[:, 1]) <= 1.5)              # projects inside the image (|x| <= 2.1, |y| <= 1.56 at 4 m)
    hidden = (np.abs(far[:, 0]) < 1.1) & (np.abs(far[:, 1]) < 1.1)                # behind the near wall (|x| < 1.2 at 4 m), clear of its rim
    clear = (np.abs(far[:, 0]) > 1.3) | (np.abs(far[:, 1]) > 1.3)
    assert hidden.sum() >= 9 and np.all(seen[n_near:][hidden] == 0)
    assert (inside & clear).sum() > 0 and np.all(seen[n_near:][inside & clear] == 1)
    kept = R.kept_faces(faces, seen)
    assert 0 < len(kept) < len(faces)
    assert np.all(seen[kept] >= 1)
