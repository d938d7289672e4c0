"""CPU: the host definition of the implicit surface of an oriented cloud (dvmvs/implicit.py): the vectorised form against the per-node loop
bit for bit on every case of tests/implicit_cases.py, the derived properties on a plane and a sphere, ``trim_mesh`` and ``grid_for`` on
hand-made input, the argument checks, and the C ABI's new entries (declared, exported, bound, -1 on null pointers without a device)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import implicit_cases as ic
from dvmvs import implicit as im
from dvmvs.outliers import nearest_neighbours

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "include", "dvmvs_hip.h")
SYMBOLS = ("dvmvs_implicit_band_fwd", "dvmvs_implicit_nodes_fwd", "dvmvs_implicit_values_fwd", "dvmvs_implicit_trim_fwd")
CASES = ic.cases()


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def scalar_volume(c, stride=1):
    """The per-node loop over every ``stride``-th node: ``(linear indices, value, valid)``."""
    nodes = im.node_positions(c["origin"], c["voxel"], c["dims"])
    chosen = np.arange(0, len(nodes), stride)
    index = nearest_neighbours(nodes[chosen], c["points"], c["neighbours"], np.float32(c["radius"]), False)[1]
    value, valid = np.zeros(len(chosen), np.float32), np.zeros(len(chosen), bool)
    for a, row in enumerate(index):
        value[a], valid[a] = im._implicit_value_scalar(nodes[chosen[a]], c["points"], c["normals"], row, c["radius"], c["min_neighbours"])
    return chosen, value, valid


@pytest.mark.parametrize("name", list(CASES))
def test_vectorised_equals_the_scalar_loop(name):
    """Bit for bit; on the two large grids every 5th (sheet) and 29th (sphere) node, which keeps the Python loop to a second."""
    c = CASES[name]
    volume, valid = ic.host_volume(name)
    assert volume.dtype == np.float32 and valid.dtype == bool and volume.shape == valid.shape == c["dims"]
    stride = 29 if name == "sphere" else 5 if name.startswith("sheet") else 1
    chosen, value, ok = scalar_volume(c, stride)
    assert value.tobytes() == volume.reshape(-1)[chosen].tobytes()
    assert ok.tobytes() == valid.reshape(-1)[chosen].tobytes()
    assert (volume[~valid] == np.float32(c["radius"])).all() and not (volume[~valid] < 0).any()
    assert valid[volume < 0].all()                                        # a node with a negative value is valid: what trim_mesh relies on


def test_node_positions_are_two_rounded_float32_steps():
    origin, voxel, dims = np.array([0.1, -0.3, 1e-3], np.float32), np.float32(0.035), (33, 17, 12)
    nodes = im.node_positions(origin, voxel, dims).reshape(dims + (3,))
    for (i, j, k) in ((0, 0, 0), (32, 16, 11), (7, 3, 5), (31, 1, 10)):
        want = [np.float32(np.float32(np.float32(n) * voxel) + origin[c]) for c, n in enumerate((i, j, k))]
        assert nodes[i, j, k].tolist() == want
    # not the float64 product rounded once: the two differ somewhere on this grid
    once = (np.arange(33) * np.float64(voxel) + np.float64(origin[0])).astype(np.float32)
    assert (once != nodes[:, 0, 0, 0]).any()


def test_case_tables_cover_what_they_say():
    sizes = {name: int(ic.host_volume(name)[1].sum()) for name in CASES}
    assert sizes["sheet-k8-33x17x12"] > 256 and 64 < sizes["plane"]       # several workgroups, several waves
    assert sizes["normals-all-zero"] == 0 and sizes["tiny-radius"] == 0 and 0 < sizes["small-radius"] < 64
    assert sizes["five-used-min5"] > 0 and sizes["five-used-min6"] == 0   # five used slots: valid at 5, not at 6
    assert 0 < sizes["normals-mixed-zero"] < sizes["cloud-n1000-9x7x5"]
    c = CASES["points-outside"]
    low, high = c["origin"], c["origin"] + np.float32(c["voxel"]) * (np.array(c["dims"], np.float32) - 1)
    for axis in range(3):
        assert (c["points"][:, axis] < low[axis]).any() and (c["points"][:, axis] > high[axis]).any()
    assert any(d < 2 for d in CASES["thin-x-1x9x7"]["dims"]) and any(d < 2 for d in CASES["thin-z-9x7x1"]["dims"])


def test_exact_boundary_is_a_candidate_of_weight_zero():
    """Node (4,3,2) has six points at d2 == radius^2 exactly and no other within the radius: six candidates of the float32 test, six used
    slots, t = 0 in all of them, den = 0: invalid, the fill."""
    c = CASES["exact-boundary"]
    volume, valid = ic.host_volume("exact-boundary")
    node = im.node_positions(c["origin"], c["voxel"], c["dims"]).reshape(c["dims"] + (3,))[4, 3, 2]
    dist, index = nearest_neighbours(node[None], c["points"], 32, np.float32(c["radius"]), False)
    assert (index[0] >= 0).sum() == 6 and (dist[0, :6] == np.float32(0.5)).all()
    assert not valid[4, 3, 2] and volume[4, 3, 2] == np.float32(0.5)
    assert im._implicit_value_scalar(node, c["points"], c["normals"], index[0], c["radius"], 1) == (np.float32(0.5), False)
    assert valid.any()


def test_plane_values_are_the_height():
    """Every term of a node is s = (0 e_x + 0 e_y) + 1 e_z = z - c exactly (a difference of two float32 numbers in float64).  num is a sum of
    w s and den the sum of the same w, so num / den = (z - c)(1 + d) with |d| <= (2 k + 2) 2^-53 < 1e-14 for k <= 32 slots (a product, a
    sum per slot on either side, a division), and the float32 rounding adds 2^-24 = 6e-8 relative (values this close to the plane are
    far above the denormals).  2e-7 relative bounds both with room; max(1, .) only widens it."""
    c = CASES["plane"]
    volume, valid = ic.host_volume("plane")
    z = im.node_positions(c["origin"], c["voxel"], c["dims"])[:, 2].astype(np.float64).reshape(c["dims"])
    height = z - np.float64(ic.PLANE_C)
    assert valid.sum() > 500
    error = np.abs(volume.astype(np.float64) - height)[valid]
    print("plane: max |value - (z - c)| =", error.max())
    assert (error <= 2e-7 * np.maximum(1.0, np.abs(height[valid]))).all()


def test_sphere_values_have_the_sign_of_the_side():
    """For a point p = R n on the sphere and a node x at distance r from the centre, n . (x - p) = (r^2 - R^2 - d^2) / (2 R) with
    d = |x - p| <= radius for every slot with a positive weight.  So the terms of a node with r^2 < R^2 are all negative and those of a
    node with r^2 > R^2 + radius^2 all positive, and so is the weighted mean.  1e-5 on r^2 covers the float32 rounding of p and n."""
    c = CASES["sphere"]
    volume, valid = ic.host_volume("sphere")
    nodes = im.node_positions(c["origin"], c["voxel"], c["dims"]).astype(np.float64)
    r2 = (nodes * nodes).sum(axis=1).reshape(c["dims"])
    R2, h2 = ic.SPHERE_R ** 2, float(np.float32(ic.SPHERE_RADIUS)) ** 2
    inner, outer = valid & (r2 < R2 - 1e-5), valid & (r2 > R2 + h2 + 1e-5)
    assert inner.sum() > 1000 and outer.sum() > 100
    assert (volume[inner] < 0).all() and (volume[outer] > 0).all()


# ---- trim_mesh and grid_for --------------------------------------------------------------------------------------------------------------
def test_trim_mesh_on_hand_made_input():
    valid = np.ones((4, 3, 3), bool)
    valid[3, :, :] = False                                                # the last x layer is the fill
    verts = np.array([[0.5, 1.0, 1.0],      # 0: between valid nodes: kept
                      [2.25, 1.0, 2.0],     # 1: on the edge from (2,1,2) to the invalid (3,1,2): goes
                      [2.0, 1.0, 1.0],      # 2: exactly on a valid node: kept
                      [1.0, 1.75, 0.0],     # 3: kept
                      [3.0, 2.0, 2.0],      # 4: exactly on an invalid node: goes
                      [1.0, 0.0, 0.5]], np.float32)                       # 5: kept
    faces = np.array([[0, 2, 3], [0, 1, 2], [3, 5, 0], [4, 5, 3], [5, 3, 2]], np.int32)
    new_verts, new_faces, kept = im.trim_mesh(verts, faces, valid)
    assert kept.dtype == np.int64 and kept.tolist() == [0, 2, 3, 5]
    assert new_verts.tobytes() == verts[[0, 2, 3, 5]].tobytes()
    assert new_faces.dtype == np.int32 and new_faces.tolist() == [[0, 1, 2], [2, 3, 0], [3, 2, 1]]     # in order, re-indexed
    # an empty mesh, and a mesh that goes entirely
    v, f, k = im.trim_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), valid)
    assert v.shape == (0, 3) and f.shape == (0, 3) and k.shape == (0,)
    v, f, k = im.trim_mesh(verts, faces, np.zeros((4, 3, 3), bool))
    assert v.shape == (0, 3) and f.shape == (0, 3) and k.shape == (0,)
    # a position outside the grid is not kept and never becomes an index
    v, f, k = im.trim_mesh(np.array([[-0.5, 0, 0], [3.5, 0, 0], [0, 0, 7]], np.float32), np.array([[0, 1, 2]], np.int32), np.ones((4, 3, 3), bool))
    assert len(v) == 0 and len(f) == 0
    with pytest.raises(ValueError, match="faces"):
        im.trim_mesh(verts, np.array([[0, 1, 6]], np.int32), valid)
    with pytest.raises(ValueError, match="valid"):
        im.trim_mesh(verts, faces, valid.astype(np.uint8))
    with pytest.raises(ValueError, match="verts_index"):
        im.trim_mesh(verts[:, :2], faces, valid)


def test_grid_for():
    rng = np.random.default_rng(0)
    for voxel, radius, offset in ((0.05, 0.15, 0.0), (0.02, 0.05, 3.7), (0.3, 0.31, -12.0)):
        points = (rng.uniform(-1, 1, size=(200, 3)) * (1.0, 0.5, 0.25) + offset).astype(np.float32)
        origin, dims = im.grid_for(points, voxel, radius)
        assert origin.dtype == np.float32 and origin.shape == (3,) and all(isinstance(d, int) for d in dims)
        v, r = np.float64(np.float32(voxel)), np.float64(np.float32(radius))
        lo, hi = np.floor((points.min(0).astype(np.float64) - r) / v), np.ceil((points.max(0).astype(np.float64) + r) / v)
        assert origin.tolist() == (lo * v).astype(np.float32).tolist() and dims == tuple(int(d) for d in hi - lo + 1)
        nodes = im.node_positions(origin, voxel, dims).reshape(dims + (3,)).astype(np.float64)
        slack = 1e-6 * (abs(offset) + 2.0)                                # the float32 rounding of the origin and the node positions
        assert (nodes[0, 0, 0] <= points.min(0) - r + slack).all() and (nodes[-1, -1, -1] >= points.max(0) + r - slack).all()
    assert im.grid_for(np.zeros((1, 3), np.float32), 0.5, 1.0)[1] == (5, 5, 5)
    with pytest.raises(ValueError, match="2\\^31"):
        im.grid_for(np.array([[0, 0, 0], [100, 100, 100]], np.float32), 0.05, 0.1)       # 2005^3 nodes
    with pytest.raises(ValueError, match="2\\^31"):
        im.grid_for(np.array([[0, 0, 0], [1e9, 0, 0]], np.float32), 0.05, 0.1)
    with pytest.raises(ValueError, match="empty"):
        im.grid_for(np.zeros((0, 3), np.float32), 0.05, 0.1)
    with pytest.raises(ValueError, match="points"):
        im.grid_for(np.zeros((4, 2), np.float32), 0.05, 0.1)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="voxel"):
            im.grid_for(np.zeros((1, 3), np.float32), bad, 0.1)
        with pytest.raises(ValueError, match="radius"):
            im.grid_for(np.zeros((1, 3), np.float32), 0.05, bad)


def test_argument_errors():
    c = CASES["cloud-n64-9x7x5"]
    good = dict(zip(("points", "normals", "origin", "voxel", "dims", "radius", "neighbours", "min_neighbours"), ic.arguments(c)))
    for bad, named in (({"neighbours": 0}, "neighbours"), ({"neighbours": 33}, "neighbours"), ({"neighbours": 8.0}, "neighbours"),
                       ({"neighbours": True}, "neighbours"), ({"min_neighbours": 0}, "min_neighbours"), ({"radius": 0.0}, "radius"),
                       ({"radius": -0.1}, "radius"), ({"radius": np.inf}, "radius"), ({"radius": np.nan}, "radius"), ({"voxel": 0.0}, "voxel"),
                       ({"voxel": np.nan}, "voxel"), ({"points": c["points"][:, :2]}, "points"), ({"normals": c["normals"][:5]}, "normals"),
                       ({"points": np.zeros((0, 3), np.float32), "normals": np.zeros((0, 3), np.float32)}, "empty"),
                       ({"origin": np.zeros(2, np.float32)}, "origin"), ({"origin": [0.0, np.nan, 0.0]}, "origin"), ({"dims": (9, 7)}, "dims"),
                       ({"dims": (9, 7, -1)}, "dims"), ({"dims": (9, 7.5, 5)}, "dims"), ({"dims": (2048, 2048, 1024)}, "2\\^31")):
        with pytest.raises(ValueError, match=named):
            im.implicit_volume(**{**good, **bad})
    volume, valid = im.implicit_volume(**{**good, "dims": (9, 0, 5)})
    assert volume.shape == valid.shape == (9, 0, 5)
    # float64 input is rounded to float32 once, as the device sees it
    as64 = im.implicit_volume(**{**good, "points": c["points"].astype(np.float64), "normals": c["normals"].astype(np.float64)})
    assert as64[0].tobytes() == ic.host_volume("cloud-n64-9x7x5")[0].tobytes()


def test_device_forms_have_the_host_signatures():
    for host, device in ((im.implicit_volume, im.implicit_volume_device), (im.trim_mesh, im.trim_mesh_device)):
        assert list(inspect.signature(host).parameters) == list(inspect.signature(device).parameters)
        assert [p.default for p in inspect.signature(host).parameters.values()] == [p.default for p in inspect.signature(device).parameters.values()]
    assert list(inspect.signature(im.mesh_points_device).parameters) == ["cloud", "normals", "voxel", "radius", "neighbours", "min_neighbours",
                                                                         "bounds", "clean"]
    from dvmvs.hip import implicit as binding
    assert list(inspect.signature(binding.implicit_volume).parameters) == ["points", "normals", "origin", "voxel", "dims", "radius", "neighbours",
                                                                           "min_neighbours", "grid", "nodes_per_chunk"]
    assert inspect.signature(binding.implicit_volume).parameters["nodes_per_chunk"].default == 1 << 20
    assert list(inspect.signature(binding.mesh_points).parameters) == list(inspect.signature(im.mesh_points_device).parameters)
    import torch
    cloud = torch.zeros((5, 3))
    for call in (lambda: binding.implicit_volume(cloud, cloud, (0, 0, 0), 0.1, (4, 4, 4), 0.2),
                 lambda: im.mesh_points_device(cloud, cloud, 0.1, 0.2),
                 lambda: binding.trim_flags(cloud, torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 2, 2), dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    source = inspect.getsource(binding)
    assert "custom_op" not in source and "torch.library" not in source


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
    for symbol in SYMBOLS:
        assert symbol in declared and hasattr(handle, symbol) and symbol in library.SIGNATURES, symbol
    assert library.ADDED_WITHIN_ABI_IMPLICIT == SYMBOLS
    assert library.ABI_VERSION == 11 and library.lib().dvmvs_abi_version() == 11
    assert re.search(r"#define\s+DVMVS_ABI_VERSION\s+11\b", text)
    assert "ADDED_WITHIN_ABI_IMPLICIT" in inspect.getsource(library.lib)
    makefile = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "Makefile")).read()
    sources = [line for line in makefile.splitlines() if line.startswith("SRCS :=")][0].split()
    assert "implicit_surface.hip" in sources
    kernel = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "implicit_surface.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel


def test_argument_validation_without_gpu(library):
    """Negative return codes are produced before anything is enqueued, so this is safe without a device."""
    lib = library.lib()
    buf = (ctypes.c_double * 64)()           # host memory standing in for a pointer: the calls below return before any use of it
    one = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(one.value + 2)
    half = ctypes.c_void_p(one.value + 4)    # 4-byte aligned, not 8
    nan, inf = float("nan"), float("inf")

    def band(points=one, M=4, ox=0.0, oy=0.0, oz=0.0, voxel=0.1, X=4, Y=4, Z=4, radius=0.2, mask=one):
        return lib.dvmvs_implicit_band_fwd(points, M, ox, oy, oz, voxel, X, Y, Z, radius, mask, None)

    def nodes(linear=one, A=4, ox=0.0, oy=0.0, oz=0.0, voxel=0.1, X=4, Y=4, Z=4, out=one):
        return lib.dvmvs_implicit_nodes_fwd(linear, A, ox, oy, oz, voxel, X, Y, Z, out, None)

    def values(nodes=one, A=4, points=one, normals=one, M=5, index=one, k=8, radius=0.2, min_neighbours=3, linear=one, total=64, volume=one,
               valid=one):
        return lib.dvmvs_implicit_values_fwd(nodes, A, points, normals, M, index, k, radius, min_neighbours, linear, total, volume, valid, None)

    def trim(verts=one, V=4, faces=one, F=2, valid=one, X=4, Y=4, Z=4, keep_vertex=one, keep_face=one):
        return lib.dvmvs_implicit_trim_fwd(verts, V, faces, F, valid, X, Y, Z, keep_vertex, keep_face, None)

    for call, nulls, odds in ((band, ("points", "mask"), ("points",)), (nodes, ("linear", "out"), ("linear", "out")),
                              (values, ("nodes", "points", "normals", "index", "linear", "volume", "valid"),
                               ("nodes", "points", "normals", "index", "linear", "volume")),
                              (trim, ("verts", "faces", "valid", "keep_vertex", "keep_face"), ("verts", "faces"))):
        for null in nulls:
            assert call(**{null: None}) == -1, (call.__name__, null)
        for name in odds:
            assert call(**{name: odd}) == -1, (call.__name__, name)
    assert nodes(linear=half) == -1 and values(linear=half) == -1        # int64 indices are 8-byte aligned
    for bad in ({"M": -1}, {"radius": 0.0}, {"radius": -1.0}, {"radius": nan}, {"radius": inf}, {"voxel": 0.0}, {"voxel": nan}, {"voxel": inf},
                {"ox": nan}, {"oy": inf}, {"oz": -inf}, {"X": 0}, {"Y": -1}, {"Z": 0}):
        assert band(**bad) == -1, bad
    for bad in ({"A": -1}, {"voxel": -0.1}, {"ox": nan}, {"X": 0}):
        assert nodes(**bad) == -1, bad
    for bad in ({"A": -1}, {"M": 0}, {"M": -2}, {"k": 0}, {"k": 33}, {"k": -1}, {"radius": 0.0}, {"radius": nan}, {"radius": inf},
                {"min_neighbours": 0}, {"total": 0}):
        assert values(**bad) == -1, bad
    for bad in ({"V": -1}, {"F": -1}, {"X": 0}, {"Y": 0}, {"Z": -4}):
        assert trim(**bad) == -1, bad
    assert band(X=2048, Y=2048, Z=1024) == -2 and band(M=2 ** 28 + 1) == -2
    assert nodes(A=2 ** 28 + 1) == -2 and values(A=2 ** 28 + 1) == -2 and values(M=2 ** 28 + 1) == -2 and values(total=2 ** 31 + 1) == -2
    assert trim(V=2 ** 31) == -2 and trim(F=2 ** 31) == -2
    # nothing to do, nothing enqueued
    assert band(M=0, points=None) == 0 and nodes(A=0, linear=None, out=None) == 0
    assert values(A=0, nodes=None, index=None, linear=None) == 0
    assert trim(V=0, F=0, verts=None, faces=None, keep_vertex=None, keep_face=None) == 0


def test_program_flags(tmp_path):
    from dvmvs.tsdf import build_parser, main, run
    defaults = vars(build_parser().parse_args([]))
    parameters = inspect.signature(run).parameters
    names = ["point_mesh_voxel", "point_mesh_radius", "point_mesh_neighbours", "point_mesh_min_neighbours"]
    assert set(defaults) == set(parameters) - {"device"}
    for name, value in zip(names, (None, None, 32, 3)):
        assert defaults[name] == parameters[name].default and (defaults[name] is value or defaults[name] == value), name
    args = build_parser().parse_args(["--point_mesh_voxel", "0.02", "--point_mesh_radius", "0.05", "--point_mesh_neighbours", "16",
                                      "--point_mesh_min_neighbours", "4"])
    assert [getattr(args, n) for n in names] == [0.02, 0.05, 16, 4]
    # each refusal names its flag and comes before any file is read (the folders do not exist)
    on = {**defaults, "filter_consistency": True, "save_point_cloud": True, "point_normals_neighbours": 10}
    for flags, named in (({"point_mesh_voxel": 0.0}, "point_mesh_voxel"), ({"point_mesh_voxel": -0.1}, "point_mesh_voxel"),
                         ({"point_mesh_voxel": float("nan")}, "point_mesh_voxel"), ({"point_mesh_voxel": float("inf")}, "point_mesh_voxel"),
                         ({"point_mesh_voxel": 0.05, "point_mesh_radius": 0.0}, "point_mesh_radius"),
                         ({"point_mesh_voxel": 0.05, "point_mesh_radius": float("nan")}, "point_mesh_radius"),
                         ({"point_mesh_voxel": 0.05, "point_mesh_neighbours": 0}, "point_mesh_neighbours"),
                         ({"point_mesh_voxel": 0.05, "point_mesh_neighbours": 33}, "point_mesh_neighbours"),
                         ({"point_mesh_voxel": 0.05, "point_mesh_neighbours": 8.5}, "point_mesh_neighbours"),
                         ({"point_mesh_voxel": 0.05, "point_mesh_min_neighbours": 0}, "point_mesh_min_neighbours"),
                         ({"point_mesh_radius": 0.1}, "point_mesh_voxel"), ({"point_mesh_neighbours": 16}, "point_mesh_voxel"),
                         ({"point_mesh_min_neighbours": 4}, "point_mesh_voxel")):
        with pytest.raises(ValueError, match=named):
            run(**{**on, **flags})
    for missing in ("filter_consistency", "save_point_cloud", "point_normals_neighbours"):
        flags = {**on, "point_mesh_voxel": 0.05, missing: defaults[missing]}
        with pytest.raises(ValueError):
            run(**flags)
    with pytest.raises(ValueError, match="point_mesh_voxel.*point_normals_neighbours"):
        run(**{**defaults, "filter_consistency": True, "save_point_cloud": True, "point_mesh_voxel": 0.05})
    with pytest.raises(ValueError, match="point_mesh_voxel"):
        main(["--reconstruction_folder", str(tmp_path / "out"), "--filter_consistency", "--save_point_cloud", "--point_mesh_voxel", "0.05"])
    assert not list(tmp_path.iterdir())
    for phrase in ("point_mesh_voxel", "point_mesh_radius", "_pointcloud_mesh.ply"):
        assert phrase in run.__doc__
