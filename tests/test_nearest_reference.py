"""CPU: the nearest-point contract and the 3-D reconstruction metrics without a GPU -- the float32 formula against float64 (and against
scipy's k-d tree where scipy is installed), dvmvs.errors' host functions against the test reference and against hand-computed clouds, and
the new C-ABI symbols (declared, exported, registered; argument validation and workspace sizes, which make no HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest

import nearest_reference as nr
from dvmvs import errors

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "include", "dvmvs_hip.h")
SYMBOLS = ("dvmvs_nearest_workspace_bytes", "dvmvs_nearest_query_workspace_bytes", "dvmvs_nearest_build", "dvmvs_nearest_distance_fwd",
           "dvmvs_distance_metrics_fwd")


def clouds(scale, seed, n=300, m=400):
    """Queries: random, 1e-4 * scale away from a target, and equal to a target; targets: random."""
    rng = np.random.default_rng(seed)
    target = (rng.normal(size=(m, 3)) * scale).astype(np.float32)
    near = target[:50] + (rng.normal(size=(50, 3)) * 1e-4 * scale).astype(np.float32)
    query = np.concatenate([(rng.normal(size=(n, 3)) * scale).astype(np.float32), near.astype(np.float32), target[50:100]])
    return query, target


@pytest.mark.parametrize("scale", [0.01, 1.0, 100.0])
def test_float32_formula_against_float64(scale):
    query, target = clouds(scale, seed=int(scale * 100))
    d32, i32 = nr.nearest32(query, target)
    d64, i64 = nr.nearest64(query, target)
    assert d32.dtype == np.float32 and i32.dtype == np.int32
    err = np.abs(d32.astype(np.float64) - d64)
    worst = (err[d64 > 0] / d64[d64 > 0]).max() / 2.0 ** -24
    print(f"scale {scale}: max |d32 - d64| / d64 = {worst:.3f} * 2^-24")
    assert (err <= nr.ERROR_BOUND * d64).all()
    assert (d32[-50:] == 0).all() and (d64[-50:] == 0).all()          # a query equal to a target: exactly 0
    assert (i32[-50:] == np.arange(50, 100)).all()


def test_float64_brute_force_against_kdtree():
    spatial = pytest.importorskip("scipy.spatial")
    query, target = clouds(1.0, seed=7)
    d64, _ = nr.nearest64(query, target)
    tree, _ = spatial.cKDTree(target.astype(np.float64)).query(query.astype(np.float64))
    assert np.allclose(d64, tree, rtol=1e-12, atol=0)


@pytest.mark.parametrize("threshold", [0.05, 0.3])
def test_host_function_equals_the_reference(threshold):
    rng = np.random.default_rng(3)
    pred = rng.normal(size=(700, 3)).astype(np.float32)
    gt = np.concatenate([pred[:200] + np.float32(0.01), rng.normal(size=(450, 3)).astype(np.float32)])
    want, want_counts = nr.reconstruction_errors(pred, gt, threshold)
    got = errors.compute_reconstruction_errors(pred, gt, threshold)
    assert got.dtype == np.float32 and got.shape == (6,) and np.array_equal(got, want)
    dist, index = errors.nearest_distances(pred, gt, return_index=True, pairs_per_chunk=1000)       # several chunks
    ref_dist, ref_index = nr.nearest32(pred, gt)
    assert np.array_equal(dist.view(np.int32), ref_dist.view(np.int32)) and np.array_equal(index, ref_index) and index.dtype == np.int32
    row, counts = errors.reconstruction_metrics_from_distances(dist, nr.nearest32(gt, pred)[0], threshold)
    assert np.array_equal(row, want) and np.array_equal(counts, want_counts) and counts.dtype == np.int64
    assert errors.RECONSTRUCTION_METRICS == nr.NAMES


@pytest.mark.parametrize("case", nr.hand_cases(), ids=lambda c: c[0])
def test_hand_computed_clouds(case):
    _, pred, gt, threshold, expected = case
    got = errors.compute_reconstruction_errors(pred, gt, threshold)
    assert np.array_equal(got, np.array(expected, dtype=np.float32)), got


def test_asymmetric_case_has_precision_unlike_recall():
    _, pred, gt, threshold, _ = nr.hand_cases()[-1]
    row = errors.compute_reconstruction_errors(pred, gt, threshold)
    assert row[3] == 1.0 and row[4] == 0.5 and row[0] != row[1]


def test_empty_clouds_raise():
    some, none = np.zeros((3, 3), np.float32), np.zeros((0, 3), np.float32)
    for pred, gt in ((none, some), (some, none), (none, none)):
        with pytest.raises(ValueError):
            errors.compute_reconstruction_errors(pred, gt)
    with pytest.raises(ValueError):
        errors.nearest_distances(some, none)


def test_duplicate_targets_give_the_smallest_index():
    rng = np.random.default_rng(5)
    base = rng.normal(size=(40, 3)).astype(np.float32)
    target = np.repeat(base, 3, axis=0)[rng.permutation(120)]
    dist, index = errors.nearest_distances(target, target, return_index=True)
    first = np.array([np.flatnonzero((target == t).all(axis=1))[0] for t in target])
    assert (dist == 0).all() and np.array_equal(index, first)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    from dvmvs.hip import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


def test_symbols_declared_exported_and_registered(library):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dvmvs_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(library.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared and hasattr(handle, name) and name in library.SIGNATURES
    assert tuple(sorted(library.ADDED_WITHIN_ABI_NEAREST)) == tuple(sorted(SYMBOLS))
    assert {n for n in declared if "nearest" in n or "distance_metrics" in n} == set(SYMBOLS)
    assert library.ABI_VERSION == 11 and library.lib().dvmvs_abi_version() == 11
    assert re.search(r"#define\s+DVMVS_ABI_VERSION\s+11\b", text)


def test_argument_validation_without_gpu(library):
    """Negative return codes are produced before anything is enqueued, so this is safe without a device."""
    lib = library.lib()
    null = None
    buf = (ctypes.c_float * 64)()           # host memory standing in for a pointer: the calls below return before any use of it
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.dvmvs_nearest_build(null, 5, ptr, 1 << 30, null) == -1
    assert lib.dvmvs_nearest_build(ptr, 5, null, 1 << 30, null) == -1
    assert lib.dvmvs_nearest_build(ptr, 0, ptr, 1 << 30, null) == -1
    assert lib.dvmvs_nearest_build(ptr, 5, ptr, 16, null) == -1                                  # workspace too small
    assert lib.dvmvs_nearest_build(ptr, (1 << 28) + 1, ptr, 1 << 62, null) == -2
    assert lib.dvmvs_nearest_distance_fwd(ptr, 4, ptr, 0, ptr, ptr, 1 << 30, ptr, null, null) == -1      # M = 0
    assert lib.dvmvs_nearest_distance_fwd(ptr, 4, null, 5, ptr, ptr, 1 << 30, ptr, null, null) == -1
    assert lib.dvmvs_nearest_distance_fwd(ptr, 4, ptr, 5, null, ptr, 1 << 30, ptr, null, null) == -1
    assert lib.dvmvs_nearest_distance_fwd(null, 4, ptr, 5, ptr, ptr, 1 << 30, ptr, null, null) == -1
    assert lib.dvmvs_nearest_distance_fwd(ptr, 4, ptr, 5, ptr, null, 1 << 30, ptr, null, null) == -1
    assert lib.dvmvs_nearest_distance_fwd(ptr, 4, ptr, 5, ptr, ptr, 1 << 30, null, null, null) == -1
    assert lib.dvmvs_nearest_distance_fwd(ptr, -1, ptr, 5, ptr, ptr, 1 << 30, ptr, null, null) == -1
    assert lib.dvmvs_nearest_distance_fwd(ptr, 4, ptr, 5, ptr, ptr, 16, ptr, null, null) == -1        # query scratch too small
    assert lib.dvmvs_distance_metrics_fwd(null, 4, ptr, 4, 0.05, ptr, null, null) == -1
    assert lib.dvmvs_distance_metrics_fwd(ptr, 4, null, 4, 0.05, ptr, null, null) == -1
    assert lib.dvmvs_distance_metrics_fwd(ptr, 4, ptr, 4, 0.05, null, null, null) == -1
    assert lib.dvmvs_distance_metrics_fwd(ptr, 0, ptr, 4, 0.05, ptr, null, null) == -1
    assert lib.dvmvs_distance_metrics_fwd(ptr, 4, ptr, 0, 0.05, ptr, null, null) == -1
    assert lib.dvmvs_distance_metrics_fwd(ptr, 4, ptr, 4, float("nan"), ptr, null, null) == -1


def test_workspace_sizes(library):
    lib = library.lib()
    assert lib.dvmvs_nearest_workspace_bytes(0) == 0 and lib.dvmvs_nearest_workspace_bytes(-3) == 0
    assert lib.dvmvs_nearest_workspace_bytes((1 << 28) + 1) == 0
    sizes = [lib.dvmvs_nearest_workspace_bytes(m) for m in (1, 2, 15, 16, 17, 1000, 100003, 300000, 1 << 20, 1 << 22, 1 << 24, 1 << 28)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes[6] >= 100003 * 16                                # the sorted copy: x, y, z and the original index
    assert lib.dvmvs_nearest_query_workspace_bytes(0, 5) == 0 and lib.dvmvs_nearest_query_workspace_bytes(5, 0) == 0
    query = [lib.dvmvs_nearest_query_workspace_bytes(n, 1000) for n in (1, 64, 65, 4096, 1 << 20)]
    assert query[0] > 0 and all(b >= a for a, b in zip(query, query[1:]))
    assert lib.dvmvs_nearest_query_workspace_bytes(64, 100003) >= lib.dvmvs_nearest_query_workspace_bytes(64, 1000)


# ---- the grid search, emulated (tests/nearest_grid_emulation.py): the kernel's statements against the brute force without a GPU -----------
def emulated_equals_brute_force(query, target):
    import nearest_grid_emulation as emu
    query, target = np.asarray(query, dtype=np.float32), np.asarray(target, dtype=np.float32)
    dist, index, rings = emu.search(query, target)
    want_dist, want_index = nr.nearest32(query, target)
    assert np.array_equal(dist.view(np.int32), want_dist.view(np.int32)) and np.array_equal(index, want_index)
    return rings


def test_emulated_search_with_targets_on_cell_faces():
    import nearest_grid_emulation as emu
    h = emu.header(emu.provisional_cloud())
    query, target, ks = emu.face_case(h)
    again = emu.header(target)                                    # the same box and M: the same grid
    assert all(np.array_equal(h[key], again[key]) for key in h) and (h["dim"] >= 3).all()
    emu.assert_on_faces(h, target[8:], ks)
    integral = sum(int((emu.scaled(h, target[8:, a], a) == ks[:, a]).sum()) for a in range(3))
    print(f"grid {h['dim']}, {len(target) - 8} targets on faces, {integral} coordinates with an integral s")
    assert integral > 0                                           # some scaled coordinates are whole numbers: exactly on a face
    emulated_equals_brute_force(query[::3], target)


@pytest.mark.parametrize("name", ["gaussian", "coincident", "coplanar", "collinear", "clusters", "outside", "duplicates", "tiny_scale"])
def test_emulated_search_edge_cases(name):
    rng = np.random.default_rng(41)
    query = rng.normal(size=(40, 3))
    if name == "gaussian":
        target = rng.normal(size=(300, 3))
    elif name == "coincident":
        target = np.repeat(rng.normal(size=(1, 3)), 30, axis=0)
    elif name == "coplanar":
        target = rng.normal(size=(200, 3))
        target[:, 2] = 0.5
    elif name == "collinear":
        target = np.zeros((60, 3))
        target[:, 0] = rng.normal(size=60)
    elif name == "clusters":
        a = rng.normal(size=(40, 3)) * 0.01
        target = np.concatenate([a, a + [50.0, 0.0, 0.0]])
        query = np.zeros((21, 3))
        query[:, 0] = np.linspace(0.0, 50.0, 21)
    elif name == "outside":
        target = rng.uniform(-1, 1, size=(300, 3))
        query = np.array([[20.0, 0, 0], [-20.0, 0.1, 0], [0, 20.0, 0], [0, -20.0, 0], [0, 0, 20.0], [0, 0, -20.0], [20.0, 20.0, 20.0]])
    elif name == "duplicates":
        target = np.repeat(rng.normal(size=(50, 3)), 3, axis=0)[rng.permutation(150)]
        query = target.copy()
    else:       # a difference that underflows to d2 = 0 between two distinct points: the smaller index wins for both
        target = np.concatenate([rng.uniform(0, 1e-12, size=(100, 3)), [[0.0, 0.0, 0.0], [1e-23, 0.0, 0.0]]])
        query = target[-2:].copy()
    rings = emulated_equals_brute_force(query, target)
    if name == "clusters":
        assert rings.max() > 20                                   # the search crossed many empty cells
