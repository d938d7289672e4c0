"""CPU: the host definition of the point-to-plane registration (dvmvs.errors.register_points_plane): the vectorised moments against the
per-point loop, the LDL^T solve against numpy, and the loop on the corner scene, on degenerate scenes and at its stop conditions."""
import numpy as np
import pytest

import registration_plane_reference as pr
import registration_reference as rr
from dvmvs import errors


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same_record(a_T, a, b_T, b):
    assert bits(a_T) == bits(b_T)
    assert a["iterations"] == b["iterations"] and a["status"] == b["status"]
    for key in ("inliers", "fitness", "rmse", "rmse_point", "moments"):
        assert bits(a[key]) == bits(b[key]), key


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_moments_equal_the_per_point_loop(N):
    rng = np.random.default_rng(6000 + N)
    moved, matched = rng.normal(size=(N, 3)).astype(np.float32), rng.normal(size=(N, 3)).astype(np.float32)
    normals = rng.normal(size=(N, 3)).astype(np.float32)
    dist = np.abs(rng.normal(size=N)).astype(np.float32)
    inlier = rng.uniform(size=N) < 0.7
    normals[~inlier] = np.nan                                  # what a trimmed pair holds must not reach a sum
    fast = errors.registration_plane_moments(moved, matched, normals, dist, inlier)
    slow = errors._registration_plane_moments_loop(moved, matched, normals, dist, inlier)
    assert fast.dtype == np.float64 and fast.shape == (30,) and fast[0] == inlier.sum() and np.isfinite(fast).all()
    assert bits(fast) == bits(slow), np.abs(fast - slow).max()
    everything = np.ones(N, bool)
    normals = np.nan_to_num(normals)
    assert bits(errors.registration_plane_moments(moved, matched, normals, dist, everything)) == \
        bits(errors._registration_plane_moments_loop(moved, matched, normals, dist, everything))


def moments_of_system(A, b):
    v = np.zeros(30)
    v[0] = 100.0
    v[1:22] = [A[a, c] for a in range(6) for c in range(a, 6)]
    v[22:28] = b
    return v


@pytest.mark.parametrize("cond", [1.0, 1e2, 1e4, 1e6])
def test_solve_against_numpy(cond):
    """x = (small rotation, translation) of random symmetric positive-definite systems with the given condition number: the LDL^T step
    against numpy.linalg.solve within 64 cond 2^-53, relative (the backward-error bound of a 6x6 Cholesky with slack), read off the
    translation and the first-order rotation of the returned update."""
    rng = np.random.default_rng(int(np.log10(cond)) + 70)
    for _ in range(20):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        A = (Q * np.geomspace(1.0, 1.0 / cond, 6)) @ Q.T
        A = (A + A.T) / 2.0
        b = rng.normal(size=6) * 1e-3
        want = np.linalg.solve(A, -b)
        got = errors._ldlt_solve([[float(e) for e in row] for row in A], [float(e) for e in b])
        assert got is not None
        bound = 64.0 * np.linalg.cond(A) * 2.0 ** -53
        assert np.linalg.norm(np.array(got) - want) <= bound * np.linalg.norm(want), (np.linalg.norm(np.array(got) - want), bound)
        # the update built from it: o = 0 makes the translation column x[3:6]; the rotation is that of the quaternion (1, x[:3] / 2)
        T = errors.registration_plane_solve(moments_of_system(A, b), np.eye(4), np.zeros(3, np.float32))
        assert np.array_equal(T[:3, 3], np.array(got[3:]) + 0.0) and np.array_equal(T[3], [0, 0, 0, 1])
        R = T[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14
        half = np.array(got[:3]) / 2.0
        angle = 2.0 * np.arctan(np.linalg.norm(half))
        assert abs(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)) - angle) < 1e-7


def test_corner_scene():
    """Independent samples of the corner, displaced by 1 degree and 2 cm: point-to-plane converges within 10 iterations, point-to-point is
    still sliding at the limit of 30."""
    source, target, normals = pr.corner_case(3600, 4500)
    T, info = pr.corner_result(3600, 4500)
    _, point = errors.register_points(source, target, 0.1)
    print(f"plane: status {info['status']} after {info['iterations']} iterations, |T - truth| {np.abs(T - pr.MOTION).max():.2e}, rmse {info['rmse']}; "
          f"point: status {point['status']} after {point['iterations']}")
    assert info["status"] == pr.CONVERGED and info["iterations"] <= 10
    assert np.abs(T - pr.MOTION).max() < 2e-3                                    # (independent samples: the answer is the samples' own)
    assert errors.REGISTRATION_PLANE_STATUS[info["status"]] == "converged" and len(errors.REGISTRATION_PLANE_STATUS) == 5
    assert info["moments"].shape == (30,) and info["inliers"].dtype == np.int64 and info["inliers"][-1] == info["moments"][0]
    assert np.all(info["rmse"] <= info["rmse_point"])                            # |(p - q) . n| <= |p - q| for unit normals
    assert point["status"] == rr.LIMIT and point["iterations"] == 30


def test_exact_correspondences():
    _, target, normals = pr.corner_case(3600, 4500)
    source = pr.displaced(np.array(target[::2]))
    T, info = errors.register_points_plane(source, target, normals, 0.1)
    point_T, point = errors.register_points(source, target, 0.1)
    print(f"plane {info['iterations']} iterations, |T - truth| {np.abs(T - pr.MOTION).max():.2e}; point {point['iterations']}")
    assert info["status"] == pr.CONVERGED and point["status"] == rr.CONVERGED
    assert np.abs(T - pr.MOTION).max() < 1e-6
    assert info["iterations"] < point["iterations"]


@pytest.mark.parametrize("name,kw", [("one plane", dict(which=(2,))), ("two planes", dict(which=(0, 1), second_tilt=25.0))])
def test_degenerate_geometry(name, kw):
    target, normals = pr.squares(1500, 21, **kw)
    source = pr.displaced(pr.squares(1200, 22, **kw)[0])
    T, info = errors.register_points_plane(source, target, normals, 0.1, init=pr.START)
    assert info["status"] == pr.DEGENERATE and info["iterations"] == 1 and errors.REGISTRATION_PLANE_STATUS[4] == "degenerate geometry"
    assert info["inliers"][0] > 1000 and bits(T) == bits(pr.START)


def test_stop_conditions_and_inputs():
    source, target, normals = pr.corner_case(1200, 1500)
    # five inliers: too few for six unknowns
    T, info = errors.register_points_plane(source[:5], target, normals, 0.1)
    assert info["status"] == pr.TOO_FEW and info["inliers"].tolist() == [5] and bits(T) == bits(np.eye(4))
    assert errors.register_points_plane(source[:6], target, normals, 0.1)[1]["status"] in (pr.CONVERGED, pr.LIMIT, pr.DEGENERATE)
    # the iteration limit
    T3, info3 = errors.register_points_plane(source, target, normals, 0.1, max_iterations=2)
    assert info3["status"] == pr.LIMIT and info3["iterations"] == 2
    # init is honoured: the loop continued from where two iterations left it is the loop itself
    full_T, full = pr.corner_result(1200, 1500)
    rest_T, rest = errors.register_points_plane(source, target, normals, 0.1, init=T3)
    assert bits(rest_T) == bits(full_T) and rest["iterations"] == full["iterations"] - 2
    assert bits(rest["rmse"]) == bits(full["rmse"][2:])
    # the sign of the normals, and their length's irrelevance to which pairs count
    flipped_T, flipped = errors.register_points_plane(source, target, -np.array(normals), 0.1)
    same_record(flipped_T, flipped, full_T, full)
    # targets without a normal are not inliers: one square's normals zeroed (or not finite) decides like the other two squares alone
    face = np.arange(1500) % 3
    for blank in (0.0, np.nan, np.inf):
        partly = np.array(normals)
        partly[face == 2] = blank
        got_T, got = errors.register_points_plane(source, target, partly, 0.1, max_iterations=1)
        assert 0 < got["inliers"][0] < full["inliers"][0]
        moved = errors.transform_points(source, np.eye(4))
        dist, index = errors.nearest_distances(moved, target, return_index=True)
        keep = (dist <= np.float32(0.1)) & (face[index] != 2)
        want = errors.registration_plane_moments(moved, target[index], np.array(normals)[index], dist, keep)
        assert got["inliers"][0] == keep.sum() and bits(got["moments"]) == bits(want)
        assert got["status"] == pr.DEGENERATE and bits(got_T) == bits(np.eye(4))       # two planes are left


def test_argument_checks():
    source, target, normals = pr.corner_case(1200, 1500)
    for bad in (dict(max_distance=0.0), dict(max_distance=float("nan")), dict(tolerance=-1.0), dict(max_iterations=0),
                dict(max_iterations=1025), dict(init=np.eye(3)), dict(init=np.full((4, 4), np.nan))):
        with pytest.raises(ValueError):
            errors.register_points_plane(source, target, normals, **{"max_distance": 0.1, **bad})
    for s, t, n in ((source[:0], target, normals), (source, target[:0], normals[:0]), (source, target, normals[:-1])):
        with pytest.raises(ValueError):
            errors.register_points_plane(s, t, n, 0.1)
