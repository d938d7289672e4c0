"""CPU: the registration's contract (tests/registration_reference.py) against independent mathematics -- Kabsch / Umeyama by SVD, a known
motion, degenerate inputs --, ``dvmvs.errors.register_points`` against it bit for bit, and the surface the feature adds: header, library,
binding, argument checks (which return before anything is enqueued), refusals and program flags.  No compute call reaches a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import nearest_reference as nr
import registration_reference as rr

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SYMBOLS = ("dvmvs_icp_workspace_bytes", "dvmvs_icp_fwd", "dvmvs_transform_points_fwd")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the solve against Kabsch and Umeyama -----------------------------------------------------------------------------------------------
def kabsch(p, q, with_scale):
    """(s R, t) minimising sum |q - s R p - t|^2 by SVD (Umeyama 1991)."""
    pc, qc = p - p.mean(axis=0), q - q.mean(axis=0)
    U, D, Vt = np.linalg.svd(qc.T @ pc)
    sign = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ sign @ Vt
    s = float((D * np.diag(sign)).sum() / (pc ** 2).sum()) if with_scale else 1.0
    return s * R, q.mean(axis=0) - s * R @ p.mean(axis=0)


def exact_moments(p, q):
    """The 18 moments of float64 pairs, summed plainly (the solve does not care how they were added)."""
    m = np.zeros(18)
    m[0] = len(p)
    m[1:4], m[4:7] = p.sum(axis=0), q.sum(axis=0)
    m[7:16] = (p[:, :, None] * q[:, None, :]).sum(axis=0).reshape(9)
    m[16], m[17] = (p ** 2).sum(), ((p - q) ** 2).sum()
    return m


@pytest.mark.parametrize("with_scale", [False, True])
def test_solve_against_svd(with_scale):
    rng = np.random.default_rng(100 + with_scale)
    for case in range(50):
        n = int(rng.integers(4, 200))
        p = rng.normal(size=(n, 3)) * rng.uniform(0.2, 3.0) + rng.normal(size=3) * 2.0
        scale = float(rng.uniform(0.5, 2.0)) if with_scale else 1.0
        motion = rr.rigid(rng.normal(size=3), rng.uniform(-170.0, 170.0), rng.normal(size=3) * 2.0, scale)
        q = p @ motion[:3, :3].T + motion[:3, 3]
        if case % 2:                                                   # half of the sets are noisy: the optimum is no longer the motion
            q = q + rng.normal(size=q.shape) * 0.05
        M, t, T = rr.solve(exact_moments(p, q), np.eye(4), with_scale)
        want_M, want_t = kabsch(p, q, with_scale)
        assert np.abs(M - want_M).max() < 1e-10, case
        assert np.abs(t - want_t).max() < 1e-10 * np.linalg.norm(want_t), case
        assert same_bits(T[:3, :3], M) and same_bits(T[:3, 3], t) and T[3].tolist() == [0, 0, 0, 1]
        assert np.linalg.det(M) > 0                                    # never a reflection
        if with_scale and case % 2 == 0:
            assert abs(np.cbrt(np.linalg.det(M)) - scale) < 1e-10


def test_solve_composes_with_the_current_transform():
    rng = np.random.default_rng(7)
    p = rng.normal(size=(40, 3))
    q = p @ rr.rotation([0.3, -1.0, 0.2], 20.0).T + [0.1, 0.2, -0.3]
    current = rr.rigid([1.0, 1.0, 0.0], 33.0, [1.0, -2.0, 0.5])
    M, t, T = rr.solve(exact_moments(p, q), current, False)
    step = np.eye(4)
    step[:3, :3], step[:3, 3] = M, t
    assert np.abs(T - step @ current).max() < 1e-14


# ---- the loop -------------------------------------------------------------------------------------------------------------------------
def test_noise_free_recovery():
    """The box moved by 5 degrees about a skew axis and 3 cm comes back within 30 iterations, to 1e-5 in R and 1e-5 m in t."""
    source, target, motion = rr.box_case()
    assert abs(np.linalg.norm(motion[:3, 3]) - 0.03) < 1e-4
    _, _, (T, info) = rr.box_result()
    print(f"iterations {info['iterations']}, status {info['status']}, rmse {info['rmse']}, |dR| {np.abs(T[:3, :3] - motion[:3, :3]).max():.2e}, "
          f"|dt| {np.abs(T[:3, 3] - motion[:3, 3]).max():.2e}")
    assert info["status"] == rr.CONVERGED and info["iterations"] <= 30
    assert np.abs(T[:3, :3] - motion[:3, :3]).max() < 1e-5 and np.abs(T[:3, 3] - motion[:3, 3]).max() < 1e-5
    assert (info["fitness"] == 1.0).all() and (info["inliers"] == 2000).all()
    assert info["rmse"][0] > 0.01 and info["rmse"][-1] < 1e-6 and (np.diff(info["rmse"]) <= 1e-7).all()
    # a longer limit cannot change a converged result; a shorter one stops at the limit
    again, info60 = rr.icp(source, target, 0.5, max_iterations=60)
    assert same_bits(again, T) and info60["iterations"] == info["iterations"]
    early, info3 = rr.icp(source, target, 0.5, max_iterations=3)
    assert info3["status"] == rr.LIMIT and info3["iterations"] == 3 and same_bits(info3["rmse"], info["rmse"][:3])


def test_scaled_copy_is_recovered():
    _, _, (T, info) = rr.box_result(with_scale=True)
    motion = rr.MOTION
    assert info["status"] == rr.CONVERGED
    assert abs(np.cbrt(np.linalg.det(T[:3, :3])) - 1.1) < 1e-5
    assert np.abs(T[:3, :3] - 1.1 * motion[:3, :3]).max() < 1e-5 and np.abs(T[:3, 3] - motion[:3, 3]).max() < 1e-5


def test_trimming_keeps_the_overlap():
    """Half of the source lies far from the target: with a trimming distance it takes no part, and the answer is still the motion."""
    source, target, motion = rr.box_case()
    outliers = (np.random.default_rng(9).uniform(-1.0, 1.0, size=(500, 3)) + [20.0, 0.0, 0.0]).astype(np.float32)
    T, info = rr.icp(np.concatenate([source[:1000], outliers]), target, 0.3)
    assert info["status"] == rr.CONVERGED and (info["inliers"] == 1000).all() and (info["fitness"] == 1000 / 1500).all()
    assert np.abs(T - motion).max() < 1e-5                          # (the inliers are exact copies, as in the full case: the same bound)


@pytest.mark.parametrize("case", rr.degenerate_cases(), ids=lambda c: c[0])
def test_degenerate_inputs(case):
    name, source, target, max_distance, status = case
    T, info = rr.icp(source, target, max_distance)
    assert np.isfinite(T).all() and np.isfinite(info["rmse"]).all() and np.isfinite(info["fitness"]).all() and np.isfinite(info["moments"]).all()
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-9 and T[3].tolist() == [0, 0, 0, 1]
    if status is not None:
        assert info["status"] == status
    else:
        assert info["status"] in (rr.CONVERGED, rr.LIMIT)
    if name == "two":
        assert info["iterations"] == 1 and info["inliers"].tolist() == [2] and same_bits(T, np.eye(4))
    if name == "all_trimmed":
        assert info["iterations"] == 1 and info["inliers"].tolist() == [0] and info["rmse"].tolist() == [0.0] and same_bits(T, np.eye(4))
    if name == "same":
        assert info["iterations"] == 2 and same_bits(T, np.eye(4)) and info["rmse"].tolist() == [0.0, 0.0]
    if name == "three":
        assert (info["inliers"] == 3).all()
    if name in ("coplanar", "collinear"):                           # the residual can only go down
        assert info["rmse"][-1] <= info["rmse"][0]
    # a scale without extent: three coincident points
    if name == "same":
        point = np.array([[1.0, 2.0, 0.5]] * 3, dtype=np.float32)                  # (exact sums: the denominator is exactly 0)
        T, info = rr.icp(point, target, float("inf"), with_scale=True)
        assert info["status"] == rr.TOO_FEW and same_bits(T, np.eye(4))


def test_moments_order_is_the_stated_one():
    """The restatement's lane-by-lane sums against a plain vectorised rendering of the same order (dvmvs.errors), and against fsum."""
    import math
    from dvmvs import errors
    rng = np.random.default_rng(11)
    for n in (1, 63, 65, 257, 1024, 1025, 4099):
        moved, matched = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
        dist = rng.uniform(0.0, 1.0, n).astype(np.float32)
        inlier = dist <= np.float32(0.5)
        got = rr.moments(moved, matched, dist, inlier)
        assert same_bits(got, errors.registration_moments(moved, matched, dist, inlier)), n
        t = rr.terms(moved, matched, dist)[inlier]
        exact = np.array([math.fsum(t[:, k]) for k in range(18)])
        assert np.abs(got - exact).max() <= 1e-12 * max(n, 1)
        assert got[0] == inlier.sum()


# ---- dvmvs.errors -----------------------------------------------------------------------------------------------------------------------
def assert_same_result(got, want):
    (T, info), (want_T, want_info) = got, want
    assert same_bits(T, want_T)
    assert info["iterations"] == want_info["iterations"] and info["status"] == want_info["status"]
    for key in ("inliers", "fitness", "rmse", "moments"):
        assert same_bits(info[key], want_info[key]), key


def test_host_definition_equals_the_restatement():
    from dvmvs import errors
    for with_scale in (False, True):
        source, target, want = rr.box_result(with_scale=with_scale)
        assert_same_result(errors.register_points(source, target, 0.5, with_scale=with_scale), want)
    source, target, _ = rr.box_case()
    start = rr.rigid([0.0, 1.0, 0.2], 2.0, [0.01, 0.0, -0.01])
    assert_same_result(errors.register_points(source, target, 0.05, init=start, max_iterations=4, tolerance=0.0),
                       rr.icp(source, target, 0.05, init=start, max_iterations=4, tolerance=0.0))
    for name, src, tgt, max_distance, _ in rr.degenerate_cases():
        assert_same_result(errors.register_points(src, tgt, max_distance), rr.icp(src, tgt, max_distance))
    assert same_bits(errors.transform_points(source, start), rr.transform32(source, start))
    assert errors.REGISTRATION_STATUS == ("running", "converged", "too few correspondences", "iteration limit")
    for bad in (dict(max_distance=0.0), dict(max_distance=float("nan")), dict(tolerance=-1.0), dict(max_iterations=0), dict(max_iterations=1025),
                dict(init=np.full((4, 4), np.nan)), dict(init=np.eye(3))):
        with pytest.raises(ValueError):
            errors.register_points(source, target, **{"max_distance": 0.5, **bad})


def test_metrics_without_alignment_are_unchanged():
    from dvmvs import errors
    for name, pred, gt, threshold, expected in nr.hand_cases():
        want = nr.reconstruction_errors(pred, gt, threshold)[0]
        for row in (errors.compute_reconstruction_errors(pred, gt, threshold),
                    errors.compute_reconstruction_errors(pred, gt, threshold, align_distance=None, align_scale=False, align_init=None,
                                                         return_transform=False)):
            assert same_bits(row, want) and same_bits(row, np.array(expected, dtype=np.float32)), name
    for fn in (errors.compute_reconstruction_errors, errors.compute_reconstruction_errors_device):
        names = list(inspect.signature(fn).parameters)
        assert names[-4:] == ["align_distance", "align_scale", "align_init", "return_transform"]
        defaults = [inspect.signature(fn).parameters[n].default for n in names[-4:]]
        assert defaults == [None, False, None, False]
        for orphan in (dict(align_scale=True), dict(align_init=np.eye(4)), dict(return_transform=True)):
            with pytest.raises(ValueError, match="align_distance"):
                fn(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), **orphan)


def test_aligned_metrics_on_the_host():
    from dvmvs import errors
    source, target, motion = rr.box_case()
    plain = errors.compute_reconstruction_errors(source, target, 0.01)
    row, T = errors.compute_reconstruction_errors(source, target, 0.01, align_distance=0.5, return_transform=True)
    assert plain[3] < 0.5 and row[3] == 1.0 and row[0] < 1e-5 and np.abs(T - motion).max() < 1e-5
    assert same_bits(T, rr.box_result()[2][0])
    moved = rr.transform32(source, T)
    assert same_bits(row, nr.reconstruction_errors(moved, target, 0.01)[0])


# ---- header, library, binding -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dvmvs.hip import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_header_library_and_binding_carry_the_new_entries(lib):
    from dvmvs.hip import _capi
    header = open(os.path.join(ROOT, "include", "dvmvs_hip.h")).read()
    assert re.search(r"#define DVMVS_ABI_VERSION 11\b", header) and _capi.ABI_VERSION == 11 and lib.dvmvs_abi_version() == 11
    handle = ctypes.CDLL(_capi.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _capi.SIGNATURES and hasattr(handle, name)
    assert tuple(_capi.ADDED_WITHIN_ABI_REGISTRATION) == SYMBOLS
    assert "ADDED_WITHIN_ABI_REGISTRATION" in inspect.getsource(_capi.lib)         # part of the stale-library check
    assert "registration.hip" in open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "Makefile")).read()


def test_workspace_sizes(lib):
    size = lib.dvmvs_icp_workspace_bytes
    assert size(0, 30) == 0 and size(-1, 30) == 0 and size(2 ** 28 + 1, 30) == 0 and size(10, 0) == 0 and size(10, 1025) == 0

    def up(nbytes):
        return (nbytes + 255) // 256 * 256

    def want(n, iterations):      # head and record | p' | d | j | partial rows of 18 doubles per 1024 points
        return up(8 * (36 + 3 * iterations)) + up(12 * n) + 2 * up(4 * n) + up(8 * 18 * ((n + 1023) // 1024))
    for n, iterations in ((1, 1), (1000, 30), (1024, 30), (1025, 30), (250000, 60), (2 ** 28, 1024)):
        assert size(n, iterations) == want(n, iterations), (n, iterations)
    sizes = [size(n, 30) for n in (1, 2, 100, 1024, 1025, 10 ** 5, 10 ** 7, 2 ** 28)]
    assert sizes == sorted(sizes) and sizes[0] > 0


def test_argument_validation_without_a_device(lib):
    """Negative return codes come before anything is enqueued, so these calls are safe without a GPU."""
    one = ctypes.c_void_p(4096)                                                    # a non-null, aligned address; never dereferenced
    odd = ctypes.c_void_p(4098)
    off8 = ctypes.c_void_p(4104)
    eye = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))

    def icp(source=one, N=100, target=one, M=50, grid=one, query=one, query_bytes=1 << 30, max_distance=0.1, with_scale=0, iterations=30,
            tolerance=1e-6, init=eye, state=one, state_bytes=1 << 30):
        return lib.dvmvs_icp_fwd(source, N, target, M, grid, query, query_bytes, max_distance, with_scale, iterations, tolerance, init, state,
                                 state_bytes, None)

    for null in ("source", "target", "grid", "query", "state"):
        assert icp(**{null: None}) == -1, null
    for name in ("source", "target", "grid", "query", "state"):
        assert icp(**{name: odd}) == -1, name
    for name in ("grid", "query", "state"):
        assert icp(**{name: off8}) == -1, name
    bad_init = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    bad_init[7] = float("inf")
    nan_init = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    nan_init[0] = float("nan")
    for bad in ({"N": 0}, {"M": 0}, {"N": -5}, {"iterations": 0}, {"iterations": -1}, {"max_distance": 0.0}, {"max_distance": -1.0},
                {"max_distance": float("nan")}, {"tolerance": float("nan")}, {"tolerance": -1e-9}, {"init": bad_init}, {"init": nan_init},
                {"with_scale": 2}, {"state_bytes": lib.dvmvs_icp_workspace_bytes(100, 30) - 1},
                {"query_bytes": lib.dvmvs_nearest_query_workspace_bytes(100, 50) - 1}):
        assert icp(**bad) == -1, bad
    for unsupported in ({"N": 2 ** 28 + 1}, {"M": 2 ** 28 + 1}, {"iterations": 1025}):
        assert icp(**unsupported) == -2, unsupported

    def transform(points=one, N=10, T=one, out=one):
        return lib.dvmvs_transform_points_fwd(points, N, T, out, None)

    for bad in ({"points": None}, {"T": None}, {"out": None}, {"N": 0}, {"points": odd}, {"out": odd}, {"T": ctypes.c_void_p(4100)}):
        assert transform(**bad) == -1, bad
    assert transform(N=2 ** 28 + 1) == -2


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
def test_binding_module_refuses_host_tensors_and_bad_arguments():
    import torch
    from dvmvs import errors
    from dvmvs.hip import registration
    assert str(inspect.signature(registration.icp)).startswith(
        "(source: torch.Tensor, target: torch.Tensor, max_distance: float, init=None, max_iterations: int = 30, with_scale: bool = False, "
        "tolerance: float = 1e-06, grid: Optional[torch.Tensor] = None)")
    assert registration.STATUS_NAMES == errors.REGISTRATION_STATUS
    cloud = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        registration.icp(cloud, cloud, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        registration.transform_points(cloud, torch.eye(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        errors.register_points_device(cloud, cloud, 0.1)
    with pytest.raises(ValueError):
        registration.icp(torch.zeros(5, 2), cloud, 0.1)
    with pytest.raises(ValueError):
        registration.icp_workspace("cuda", 0, 30)
    with pytest.raises(ValueError):
        registration.icp_workspace("cuda", 10, 1025)
    # not an op of the ops package, and nothing registered under torch.ops.dvmvs
    from dvmvs.hip import ops
    assert not hasattr(ops, "icp") and not hasattr(ops, "registration")
    source = inspect.getsource(registration)
    assert "custom_op" not in source and "torch.library" not in source


def test_score_against_keywords():
    from dvmvs.tsdf import TSDFVolume
    parameters = inspect.signature(TSDFVolume.score_against).parameters
    assert list(parameters)[-3:] == ["align_distance", "align_scale", "return_transform"]
    assert [parameters[n].default for n in list(parameters)[-3:]] == [None, False, False]
    volume = TSDFVolume.__new__(TSDFVolume)                                        # the refusals come before the volume is touched
    for orphan in (dict(align_scale=True), dict(return_transform=True)):
        with pytest.raises(ValueError, match="align_distance"):
            TSDFVolume.score_against(volume, np.zeros((3, 3), np.float32), **orphan)


def test_program_flags(tmp_path):
    from dvmvs.tsdf import build_parser, main, run
    defaults = vars(build_parser().parse_args([]))
    parameters = inspect.signature(run).parameters
    for name, value in (("evaluate_3d_align", None), ("evaluate_3d_align_scale", False), ("groundtruth_transform", None)):
        assert defaults[name] == parameters[name].default and (defaults[name] is value or defaults[name] == value), name
    args = build_parser().parse_args(["--evaluate_3d", "--evaluate_3d_align", "0.1", "--evaluate_3d_align_scale", "--groundtruth_mesh", "gt.ply",
                                      "--groundtruth_transform", "t.txt"])
    assert args.evaluate_3d_align == 0.1 and args.evaluate_3d_align_scale is True and args.groundtruth_transform == "t.txt"
    # each refusal names its flag and comes before any file is read (the folders do not exist)
    with pytest.raises(ValueError, match="evaluate_3d_align"):
        run(**{**defaults, "evaluate_3d_align": 0.1})
    with pytest.raises(ValueError, match="evaluate_3d_align_scale"):
        run(**{**defaults, "evaluate_3d": True, "evaluate_3d_align_scale": True})
    with pytest.raises(ValueError, match="groundtruth_transform"):
        run(**{**defaults, "evaluate_3d": True, "groundtruth_transform": "t.txt"})
    with pytest.raises(ValueError, match="evaluate_3d_align"):
        run(**{**defaults, "evaluate_3d": True, "evaluate_3d_align": 0.0})
    with pytest.raises(ValueError, match="evaluate_3d_align"):
        main(["--reconstruction_folder", str(tmp_path / "out"), "--evaluate_3d_align", "0.1"])
    assert not list(tmp_path.iterdir())


def test_groundtruth_transform_file(tmp_path):
    from dvmvs.tsdf import load_transform
    motion = rr.rigid([0.0, 0.0, 1.0], 30.0, [1.0, 2.0, 3.0])
    np.savetxt(tmp_path / "t.txt", motion)
    assert np.array_equal(load_transform(str(tmp_path / "t.txt")), motion)
    (tmp_path / "flat.txt").write_text(" ".join(repr(float(v)) for v in motion.reshape(-1)))
    assert np.array_equal(load_transform(str(tmp_path / "flat.txt")), motion)
    (tmp_path / "short.txt").write_text("1 0 0 0 1 0 0 0 1")
    with pytest.raises(ValueError, match="groundtruth_transform"):
        load_transform(str(tmp_path / "short.txt"))
    (tmp_path / "nan.txt").write_text(" ".join(["nan"] * 16))
    with pytest.raises(ValueError, match="groundtruth_transform"):
        load_transform(str(tmp_path / "nan.txt"))
