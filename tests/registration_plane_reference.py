"""Shared cases of the point-to-plane registration tests (dvmvs.errors.register_points_plane, csrc/registration.hip): the corner scene of
three mutually orthogonal unit squares in general position, single-plane and two-plane scenes, and the host definition's answers on them,
each computed once and read-only."""
import functools

import numpy as np

import registration_reference as rr

RUNNING, CONVERGED, TOO_FEW, LIMIT, DEGENERATE = range(5)
POSE = rr.rigid([0.6, -0.3, 1.0], 33.0, [0.4, -0.2, 0.3])                        # takes the axis-aligned corner into general position
MOTION = rr.rigid([0.4, 1.0, -0.3], 1.0, np.array([0.012, -0.01, 0.0125]))       # 1 degree and 2 cm: what a registration has to find
START = rr.rigid([0.3, -1.0, 0.5], 0.4, [0.004, 0.002, -0.006])                  # a T_0 that is not the identity


def squares(count, seed, which=(0, 1, 2), second_tilt=None):
    """``(points float32 [count,3], normals float32 [count,3])``: uniform samples of the unit squares x = 0, y = 0, z = 0 named by ``which``
    (dealt in turn), moved by ``POSE``.  ``second_tilt`` (degrees): the second listed square is turned about the shared edge direction so
    that two planes meet at that angle off the right one."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0.0, 1.0, (count, 2))
    face = np.asarray(which)[np.arange(count) % len(which)]
    points, normals = np.zeros((count, 3)), np.zeros((count, 3))
    for axis in range(3):
        rows = face == axis
        others = [a for a in range(3) if a != axis]
        points[np.ix_(rows, others)] = uv[rows]
        normals[rows, axis] = 1.0
    if second_tilt is not None:
        rows = face == which[1]
        shared, = [a for a in range(3) if a not in which[:2]]
        turn = rr.rotation(np.eye(3)[shared], second_tilt)
        points[rows], normals[rows] = points[rows] @ turn.T, normals[rows] @ turn.T
    R, t = POSE[:3, :3], POSE[:3, 3]
    return (points @ R.T + t).astype(np.float32), (normals @ R.T).astype(np.float32)


def displaced(points):
    """``points`` moved by the inverse of ``MOTION`` (float32), so that registering them back finds ``MOTION``."""
    return rr.transform32(points, np.linalg.inv(MOTION))


CORNER_SEED = 19


@functools.lru_cache(maxsize=None)
def corner_case(n_source, n_target):
    """``(source, target, normals)``: independent samples of the corner, the source displaced.  Read-only.  How many iterations the
    point-to-point loop needs on 3 600 against 4 500 points depends on the samples: over the seeds 1, 3, .., 39 it converged after 17 to 26
    iterations on nineteen of them and ran into the limit of 30 on one, ``CORNER_SEED``, which is the sample set kept here because the
    comparison test wants a scene on which 30 iterations do not suffice; point-to-plane took 3 to 5 on every seed tried."""
    target, normals = squares(n_target, CORNER_SEED)
    source = displaced(squares(n_source, CORNER_SEED + 1)[0])
    for a in (source, target, normals):
        a.setflags(write=False)
    return source, target, normals


@functools.lru_cache(maxsize=None)
def corner_result(n_source, n_target, max_iterations=30):
    """The host definition's answer on ``corner_case``, computed once."""
    from dvmvs import errors
    source, target, normals = corner_case(n_source, n_target)
    return errors.register_points_plane(source, target, normals, 0.1, max_iterations=max_iterations)


def one_iteration_case(N, M=500):
    """``(source, target, normals, max_distance)`` of the one-iteration tests: Gaussian clouds, every fifth normal zero, one not finite,
    and a distance that trims about half of the pairs after ``START``."""
    import nearest_reference as nr
    rng = np.random.default_rng(7000 + N)
    target = rng.normal(size=(M, 3)).astype(np.float32)
    normals = rng.normal(size=(M, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    normals[::5] = 0.0
    normals[7, 1] = np.nan
    source = rng.normal(size=(N, 3)).astype(np.float32)
    dist = nr.nearest32(rr.transform32(source, START), target)[0]
    return source, target, normals, float(np.sort(dist)[N // 2])
