"""CPU: the host definition of point-cloud normals (dvmvs/normals.py): the vectorised form against the scalar loop bit for bit, against
numpy's eigh of a two-pass covariance by angle, hand-worked cases and the edge rules; and the surface the feature adds: the binding table,
the C entry point's refusals (made before anything is enqueued, so safe without a GPU), the binding module, ``fused_point_views``,
``pcwrite_normals`` and the program's flags."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import normals_cases as cases
from dvmvs import normals as nm
from dvmvs.outliers import MAX_NEIGHBOURS, nearest_neighbours

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "include", "dvmvs_hip.h")
SYMBOL = "dvmvs_point_normals_fwd"


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == len(b)


# ---- the two host forms -----------------------------------------------------------------------------------------------------------------
def test_vectorised_form_equals_the_scalar_loop_bit_for_bit():
    valid_seen = invalid_seen = 0
    for name, (points, k, limit, viewpoints, view) in cases.search_cases().items():
        index = nearest_neighbours(points, points, k, limit)[1]
        fast = nm.point_normals(points, points, index, viewpoints, view)
        assert same_bits(fast, nm._point_normals_scalar(points, points, index, viewpoints, view)), name
        assert same_bits(fast, nm.estimate_normals(points, k, limit, viewpoints, view)), name
        assert fast[0].dtype == np.float32 and fast[1].dtype == np.float32 and fast[2].dtype == bool
        valid_seen, invalid_seen = valid_seen + int(fast[2].sum()), invalid_seen + int((~fast[2]).sum())
    for name, arguments in cases.row_cases().items():
        assert same_bits(nm.point_normals(*arguments), nm._point_normals_scalar(*arguments)), name
    assert valid_seen > 20000 and invalid_seen > 100
    # the larger cloud of the GPU test, with rows made from the pixel order (a brute-force search of it is not for the CPU); the scalar
    # loop on every 37th row
    points = cases.sheet()
    n = len(points)
    offsets = np.array([0, 1, -1, 301, -301, 302, -300, 2])
    index = ((np.arange(n)[:, None] + offsets[None, :]) % n).astype(np.int32)
    fast = nm.point_normals(points, points, index, np.array([[1.5, 1.0, 4.0]], np.float32))
    rows = np.arange(0, n, 37)
    slow = nm._point_normals_scalar(points[rows], points, index[rows], np.array([[1.5, 1.0, 4.0]], np.float32))
    assert same_bits([a[rows] for a in fast], slow) and fast[2].all()


def two_pass_normals(points, index):
    """float64 [N,3]: the eigenvector of the smallest eigenvalue of the two-pass covariance of every (full) row, by numpy.linalg.eigh, and
    the relative gap between the two smallest eigenvalues."""
    nb = points.astype(np.float64)[index]
    centred = nb - nb.mean(axis=1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nkc,nkd->ncd", centred, centred) / index.shape[1])
    return v[:, :, 0], (w[:, 1] - w[:, 0]) / w[:, 2]


@pytest.mark.parametrize("cloud", ["sphere", "far_plane"])
@pytest.mark.parametrize("k", [8, 20])
def test_against_eigh_of_a_two_pass_covariance(cloud, k):
    points = cases.sphere(1000, seed=21)[0] if cloud == "sphere" else cases.far_plane(1000, seed=22)[0]
    index = nearest_neighbours(points, points, k)[1]
    normals, curvature, valid = nm.point_normals(points, points, index)
    assert valid.all()
    reference, gap = two_pass_normals(points, index)
    sine = np.linalg.norm(np.cross(normals.astype(np.float64), reference), axis=1)
    separated = gap > 1e-6
    assert np.count_nonzero(~separated) <= 0.01 * len(points)
    # the float32 rounding of the output is the error that is left: 2^-24 a component
    assert sine[separated].max() <= 1e-6, sine[separated].max()
    assert (curvature >= 0).all() and (curvature <= np.float32(1 / 3 + 1e-6)).all()


def test_sphere_normals_follow_the_viewpoint():
    points, directions = cases.sphere(1000, seed=23)
    outside = (directions * 50.0).astype(np.float32)
    normals, _, valid = nm.estimate_normals(points, 12, np.inf, outside, np.arange(len(points), dtype=np.int32))
    assert valid.all() and ((normals * directions).sum(axis=1) > 0.8).all()
    normals, _, valid = nm.estimate_normals(points, 12, np.inf, np.zeros((1, 3), np.float32))
    assert valid.all() and ((normals * directions).sum(axis=1) < -0.8).all()
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 1e-6


def test_planar_lattice_is_exact():
    points = cases.planar_lattice()
    normals, curvature, valid = nm.estimate_normals(points, 9)
    assert valid.all() and (curvature == 0).all()
    assert (normals == np.array([0, 0, 1], np.float32)).all()                      # the canonical sign: z > 0
    below = nm.estimate_normals(points, 9, np.inf, np.array([[3.0, 3.0, -5.0]], np.float32))[0]
    assert (below == np.array([0, 0, -1], np.float32)).all()


# ---- the edge rules ---------------------------------------------------------------------------------------------------------------------
def test_short_rows_coincident_points_and_skipped_slots():
    target = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 2, 2]], np.float32)
    points = np.zeros((6, 3), np.float32)
    M = len(target)
    index = np.array([[0, 1, -1, -1],              # two valid slots
                      [0, 1, 2, 3],                # the full row
                      [0, -1, 1, 2],               # -1 in the middle
                      [M, 0, 1, 2],                # M, 2^31 - 1 and -7 are skipped like -1
                      [0, 2 ** 31 - 1, 1, 2],
                      [4, 4, -7, 4]], np.int32)    # three valid slots, one place
    normals, curvature, valid = nm.point_normals(points, target, index)
    assert valid.tolist() == [False, True, True, True, True, False]
    assert (normals[[0, 5]] == 0).all() and (curvature[[0, 5]] == 0).all()
    three = nm.point_normals(points[:1], target, np.array([[0, 1, 2]], np.int32))
    for row in (2, 3, 4):
        assert same_bits([a[row:row + 1] for a in (normals, curvature, valid)], three)
    assert (three[0] == np.array([0, 0, 1], np.float32)).all()
    # a row of slots that are all outside
    nothing = nm.point_normals(points[:1], target, np.array([[-1, M, -7]], np.int32))
    assert not nothing[2][0] and (nothing[0] == 0).all()
    for bad in (np.zeros((6, 2), np.int32), np.zeros((6, MAX_NEIGHBOURS + 1), np.int32), np.zeros((5, 4), np.int32), np.zeros((6, 4), np.float32)):
        with pytest.raises(ValueError, match="index"):
            nm.point_normals(points, target, bad)
    with pytest.raises(ValueError, match="neighbours"):
        nm.estimate_normals(points, 2)
    with pytest.raises(ValueError, match="neighbours"):
        nm.estimate_normals(points, 33)
    assert nm.MIN_NEIGHBOURS == 3 and nm.MAX_NEIGHBOURS is MAX_NEIGHBOURS
    empty = nm.estimate_normals(np.zeros((0, 3), np.float32))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,) and empty[2].shape == (0,)


def test_orientation_rules():
    target = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)                 # the plane z = 0: canonical normal (0,0,1)
    points = np.array([[0.5, 0.5, 0.0]] * 5, np.float32)
    index = np.tile(np.arange(4, dtype=np.int32), (5, 1))
    viewpoints = np.array([[0, 0, -3], [0, 0, 3], [7, 7, 0]], np.float32)                       # below, above, IN the plane (d = 0)
    view = np.array([0, 1, 2, -1, 3], np.int32)                                                 # -1 and V = 3 are unknown
    normals, _, valid = nm.point_normals(points, target, index, viewpoints, view)
    assert valid.all() and normals[:, 2].tolist() == [-1, 1, 1, 1, 1] and (normals[:, :2] == 0).all()
    with pytest.raises(ValueError, match="view"):
        nm.point_normals(points, target, index, viewpoints)                                     # three viewpoints need view
    with pytest.raises(ValueError, match="viewpoints"):
        nm.point_normals(points, target, index, None, view)


def test_canonical_sign_and_eigenvalue_ties():
    # normals with z = 0: the plane x + y = 1 (normal (1,1,0)/sqrt 2, y > 0), and with z = y = 0: the plane x = 2
    # 4 x 4 grids of small integers: 16 points, so every sum, product and division by n is exact and the z column of the covariance is
    # exactly zero; the (0,1) rotation has theta = 0, t = 1
    a, b = (g.ravel().astype(np.float64) for g in np.meshgrid(np.arange(4), np.arange(4), indexing="ij"))
    root = 1.0 / np.sqrt(2.0)
    for target, expected in ((np.stack([a, 1.0 - a, b], axis=1), [root, root, 0.0]),        # x + y = 1: (1,1,0) / sqrt 2 has y > 0
                             (np.stack([a, a, b], axis=1), [-root, root, 0.0]),             # x = y: (1,-1,0) / sqrt 2 is turned round
                             (np.stack([np.full(16, 2.0), a, b], axis=1), [1.0, 0.0, 0.0])):
        target = target.astype(np.float32)
        normal, curvature, valid = nm.point_normals(target[:1], target, np.arange(16, dtype=np.int32)[None, :])
        assert valid[0] and normal[0, 2] == 0 and np.abs(normal[0] - np.array(expected)).max() < 1e-7 and curvature[0] < 1e-12, target[1]
    assert normal[0].tolist() == [1, 0, 0]
    # the 5^3 lattice: the centre's six nearest neighbours and itself have the covariance (2/7) I, three equal eigenvalues: index 0, x
    points = cases.cubic_lattice()
    normals, curvature, valid = nm.estimate_normals(points, 7)
    centre = (2 * 5 + 2) * 5 + 2
    assert valid.all() and normals[centre].tolist() == [1, 0, 0] and curvature[centre] == np.float32(1 / 3)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    from dvmvs.hip import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


def test_symbol_declared_exported_and_registered(library):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dvmvs_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(library.LIB_PATH)
    assert SYMBOL in declared and hasattr(handle, SYMBOL) and SYMBOL in library.SIGNATURES
    assert library.ADDED_WITHIN_ABI_POINT_NORMALS == (SYMBOL,)
    assert library.ABI_VERSION == 11 and library.lib().dvmvs_abi_version() == 11
    assert re.search(r"#define\s+DVMVS_ABI_VERSION\s+11\b", text)
    assert "ADDED_WITHIN_ABI_POINT_NORMALS" in inspect.getsource(library.lib)
    makefile = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "Makefile")).read()
    sources = [line for line in makefile.splitlines() if line.startswith("SRCS :=")][0].split()
    assert "point_normals.hip" in sources
    kernel = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "point_normals.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel and "nearest_grid.h" not in kernel


def test_argument_validation_without_gpu(library):
    """Negative return codes are produced before anything is enqueued, so this is safe without a device."""
    lib = library.lib()
    buf = (ctypes.c_double * 64)()           # host memory standing in for a pointer: the calls below return before any use of it
    one = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(one.value + 2)
    byte = ctypes.c_void_p(one.value + 1)

    def call(points=one, N=4, target=one, M=5, index=one, k=8, viewpoints=one, V=2, view=one, normals=one, curvature=one, valid=one):
        return lib.dvmvs_point_normals_fwd(points, N, target, M, index, k, viewpoints, V, view, normals, curvature, valid, None)

    for null in ("points", "target", "index", "normals", "curvature", "valid"):
        assert call(**{null: None}) == -1, null
    for name in ("points", "target", "index", "viewpoints", "view", "normals", "curvature"):
        assert call(**{name: odd}) == -1, name
    for bad in ({"N": -1}, {"M": 0}, {"M": -3}, {"k": 2}, {"k": 33}, {"k": 0}, {"k": -1}, {"V": -1},
                {"viewpoints": None},                              # V > 0 without viewpoints
                {"V": 0},                                          # viewpoints with V = 0
                {"viewpoints": None, "V": 0},                      # view without viewpoints
                {"view": None},                                    # V > 1 without view
                {"view": None, "V": 3}):
        assert call(**bad) == -1, bad
    assert call(N=2 ** 28 + 1) == -2 and call(M=2 ** 28 + 1) == -2
    # nothing to do, nothing enqueued: with every legal combination of the optional arguments (valid needs no alignment)
    assert call(N=0) == 0 and call(N=0, valid=byte) == 0
    assert call(N=0, view=None, V=1) == 0 and call(N=0, viewpoints=None, V=0, view=None) == 0
    assert call(N=0, points=None, index=None, normals=None, curvature=None, valid=None) == 0


def test_binding_module_refuses_host_tensors_and_registers_nothing():
    import torch
    from dvmvs.hip import normals as binding
    cloud = torch.zeros((5, 3))
    index = torch.zeros((5, 4), dtype=torch.int32)
    for call in (lambda: binding.point_normals(cloud, cloud, index), lambda: binding.estimate_normals(cloud, 3),
                 lambda: nm.point_normals_device(cloud, cloud, index), lambda: nm.estimate_normals_device(cloud, 8, 0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for k in (2, 33):
        with pytest.raises(ValueError, match="neighbours"):
            binding.estimate_normals(cloud, k)
        with pytest.raises(ValueError, match="index"):
            binding.point_normals(cloud, cloud, torch.zeros((5, k), dtype=torch.int32))
    with pytest.raises(ValueError):
        binding.point_normals(torch.zeros((5, 2)), cloud, index)
    assert list(inspect.signature(binding.point_normals).parameters) == ["points", "target", "index", "viewpoints", "view"]
    assert list(inspect.signature(binding.estimate_normals).parameters) == ["points", "neighbours", "max_distance", "viewpoints", "view", "grid"]
    assert list(inspect.signature(nm.estimate_normals).parameters) == ["points", "neighbours", "max_distance", "viewpoints", "view"]
    for host, device in ((nm.point_normals, nm.point_normals_device), (nm.estimate_normals, nm.estimate_normals_device)):
        assert list(inspect.signature(host).parameters) == list(inspect.signature(device).parameters)
        assert [p.default for p in inspect.signature(host).parameters.values()] == [p.default for p in inspect.signature(device).parameters.values()]
    # not an op of the ops package, and nothing registered under torch.ops.dvmvs
    from dvmvs.hip import ops
    for name in ("point_normals", "estimate_normals", "normals"):
        assert not hasattr(ops, name) and name not in ops.__all__
    source = inspect.getsource(binding)
    assert "custom_op" not in source and "torch.library" not in source


# ---- views, file format, program ----------------------------------------------------------------------------------------------------------
def test_fused_point_views():
    import torch
    from dvmvs.consistency import fused_point_cloud, fused_point_views
    depth = torch.zeros((3, 2, 4))
    depth[0, 0, 1] = depth[0, 1, 3] = 1.5
    depth[2, 0, 0] = depth[2, 0, 2] = depth[2, 1, 1] = 2.0                            # frame 1 keeps nothing
    views = fused_point_views(depth)
    assert views.dtype == torch.int32 and views.tolist() == [0, 0, 2, 2, 2]
    points = torch.arange(3 * 2 * 4 * 3, dtype=torch.float32).reshape(3, 2, 4, 3)
    cloud = fused_point_cloud(depth, points)
    assert cloud.shape[0] == views.shape[0]
    assert (cloud[:, 0] // 24).to(torch.int32).tolist() == views.tolist()              # 24 numbers a frame: the frame of every point
    assert fused_point_views(torch.zeros((2, 3, 3))).shape == (0,)
    with pytest.raises(ValueError, match="N,H,W"):
        fused_point_views(torch.zeros((3, 3)))


def test_pcwrite_normals(tmp_path):
    from dvmvs.tsdf import TSDFFusion
    xyzrgb = np.array([[0.5, -1.25, 2.0, 255, 0, 17], [1e-7, 3.0, -4.5, 1, 2, 3]], np.float32)
    normals = np.array([[0.0, 0.0, 1.0], [-0.6, 0.8, 0.0]], np.float32)
    path = str(tmp_path / "cloud.ply")
    TSDFFusion.pcwrite_normals(path, xyzrgb, normals)
    lines = open(path).read().split("\n")
    assert lines[:13] == ["ply", "format ascii 1.0", "element vertex 2", "property float x", "property float y", "property float z",
                          "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
                          "property uchar blue", "end_header"]
    assert lines[13:] == ["0.500000 -1.250000 2.000000 0.000000 0.000000 1.000000 255 0 17",
                          "0.000000 3.000000 -4.500000 -0.600000 0.800000 0.000000 1 2 3", ""]
    # pcwrite's columns, with the three normal columns between them
    plain = str(tmp_path / "plain.ply")
    TSDFFusion.pcwrite(plain, xyzrgb)
    rows = open(plain).read().split("\n")[10:12]
    assert [" ".join(line.split(" ")[:3] + line.split(" ")[6:]) for line in lines[13:15]] == rows
    TSDFFusion.pcwrite_normals(path, np.zeros((0, 6), np.float32), np.zeros((0, 3), np.float32))
    assert open(path).read().endswith("element vertex 0\n" + "".join(lines[i] + "\n" for i in range(3, 13)))
    with pytest.raises(ValueError, match="normals"):
        TSDFFusion.pcwrite_normals(path, xyzrgb, normals[:1])


def test_program_flags(tmp_path):
    from dvmvs.tsdf import build_parser, main, run
    defaults = vars(build_parser().parse_args([]))
    parameters = inspect.signature(run).parameters
    names = ["point_normals_neighbours", "point_normals_max_distance"]
    order = list(parameters)
    assert order[order.index("groundtruth_transform") + 1:order.index("clean_points_neighbours")] == names
    assert set(defaults) == set(order) - {"device"}
    for name in names:
        assert defaults[name] is None and parameters[name].default is None
    args = build_parser().parse_args(["--point_normals_neighbours", "20", "--point_normals_max_distance", "0.05"])
    assert [getattr(args, n) for n in names] == [20, 0.05]
    # each refusal names its flag and comes before any file is read (the folders do not exist)
    on = {**defaults, "filter_consistency": True, "save_point_cloud": True}
    for flags, named in (({"point_normals_neighbours": 2}, "point_normals_neighbours"), ({"point_normals_neighbours": 33}, "point_normals_neighbours"),
                         ({"point_normals_neighbours": 8.5}, "point_normals_neighbours"),
                         ({"point_normals_neighbours": 8, "point_normals_max_distance": 0.0}, "point_normals_max_distance"),
                         ({"point_normals_neighbours": 8, "point_normals_max_distance": -1.0}, "point_normals_max_distance"),
                         ({"point_normals_neighbours": 8, "point_normals_max_distance": float("nan")}, "point_normals_max_distance"),
                         ({"point_normals_max_distance": 0.5}, "point_normals_max_distance")):
        with pytest.raises(ValueError, match=named):
            run(**{**on, **flags})
    for flags in ({"point_normals_neighbours": 8}, {"point_normals_neighbours": 8, "point_normals_max_distance": 0.1}):
        with pytest.raises(ValueError, match="point_normals_neighbours.*save_point_cloud"):
            run(**{**defaults, **flags})
        with pytest.raises(ValueError, match="save_point_cloud"):
            run(**{**defaults, "filter_consistency": True, **flags})
    with pytest.raises(ValueError, match="point_normals_neighbours"):
        main(["--reconstruction_folder", str(tmp_path / "out"), "--filter_consistency", "--save_point_cloud", "--point_normals_neighbours", "40"])
    with pytest.raises(ValueError, match="save_point_cloud"):
        main(["--reconstruction_folder", str(tmp_path / "out"), "--point_normals_neighbours", "8"])
    assert not list(tmp_path.iterdir())
    for phrase in ("point_normals_neighbours", "point_normals_max_distance", "_pointcloud_normals.ply", "_pointcloud_clean.ply", "render_keyframes"):
        assert phrase in run.__doc__
