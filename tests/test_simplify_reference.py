"""CPU: the host definition of mesh simplification (dvmvs/simplify.py) on the cases of tests/simplify_reference.py: the numpy form against
the scalar loop bit for bit, what the quadric buys over the cell mean on a cube and a plane, the face rules, the errors, and the binding's
table against the header.  No GPU."""
import inspect

import numpy as np
import pytest

import simplify_reference as sr
from dvmvs.simplify import CONTRACTIONS, SimplifySettings, _simplify_scalar, quadric_ranks, simplify_mesh, simplify_settings

NAMES = ("verts", "faces", "normals", "colors", "vertex_cluster", "face_index")
DTYPES = (np.float32, np.int32, np.float32, np.uint8, np.int32, np.int32)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_same(got, want, label):
    for name, g, w in zip(NAMES, got, want):
        assert (g is None) == (w is None), (label, name)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and bits(g) == bits(w), (label, name, g.shape, w.shape)


@pytest.mark.parametrize("contraction", CONTRACTIONS)
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_numpy_definition_equals_the_scalar_loop(name, contraction):
    c = sr.case(name)
    want = _simplify_scalar(c["verts"], c["faces"], c["voxel"], c["normals"], c["colors"], contraction, return_index=True)
    got = sr.host(name, contraction)
    assert_same(got, want[:4] + want[4], (name, contraction))
    for g, dtype in zip(got, DTYPES):
        assert g.dtype == dtype
    V, F = len(c["verts"]), len(c["faces"])
    assert got[0].shape == got[2].shape == got[3].shape and got[0].shape[1:] == (3,) and got[1].shape[1:] == (3,)
    assert got[4].shape == (V,) and got[5].shape == (len(got[1]),) and len(got[1]) <= F and len(got[0]) <= V
    # without the optional arrays: the same mesh
    bare = sr.host(name, contraction, attributes=False)
    assert bare[2] is None and bare[3] is None
    assert bits(bare[0]) == bits(got[0]) and bits(bare[1]) == bits(got[1]) and bits(bare[4]) == bits(got[4]) and bits(bare[5]) == bits(got[5])
    plain = simplify_mesh(c["verts"], c["faces"], c["voxel"], contraction=contraction)
    assert len(plain) == 4 and bits(plain[0]) == bits(got[0]) and bits(plain[1]) == bits(got[1])


def test_cube_quadric_keeps_faces_edges_and_corners():
    c = sr.case("cube")
    ranks = quadric_ranks(c["verts"], c["faces"], c["voxel"])
    assert np.bincount(ranks, minlength=4).tolist() == [0, 24, 24, 8]
    verts = sr.host("cube", "quadric")[0]
    assert len(verts) == 56
    surface, corner = sr.cube_distances(verts)
    print(f"quadric: furthest from the surface {surface:.3g}, a true corner from its nearest vertex {corner:.3g}")
    assert surface <= 1e-5 and corner <= 1e-5


def test_cube_average_rounds_them_off():
    surface, corner = sr.cube_distances(sr.host("cube", "average")[0])
    print(f"average: furthest from the surface {surface:.3g}, a true corner from its nearest vertex {corner:.3g}")
    assert surface > 0.05 and corner > 0.1
    assert bits(sr.host("cube", "average")[1]) == bits(sr.host("cube", "quadric")[1])          # the contraction moves vertices, nothing else


def test_plane_stays_a_plane():
    c = sr.case("plane")
    assert set(quadric_ranks(c["verts"], c["faces"], c["voxel"]).tolist()) == {1}
    for contraction in CONTRACTIONS:
        verts = sr.host("plane", contraction)[0].astype(np.float64)
        off = np.abs((verts - sr.PLANE_POINT) @ sr.PLANE_NORMAL).max()
        print(f"{contraction}: furthest from the plane {off:.3g}")
        assert off <= 1e-5
    # rank 1 moves a vertex along the normal only: it stays at the cell mean in the plane
    moved = sr.host("plane", "quadric")[0].astype(np.float64) - sr.host("plane", "average")[0].astype(np.float64)
    tangential = moved - np.outer(moved @ sr.PLANE_NORMAL, sr.PLANE_NORMAL)
    assert np.abs(tangential).max() <= 1e-6


def test_far_has_the_ranks_of_cube():
    near, far = sr.case("cube"), sr.case("far")
    want = np.bincount(quadric_ranks(near["verts"], near["faces"], near["voxel"]), minlength=4)
    got = np.bincount(quadric_ranks(far["verts"], far["faces"], far["voxel"]), minlength=4)
    assert got.tolist() == want.tolist() == [0, 24, 24, 8]
    assert sr.host("far")[0].shape == sr.host("cube")[0].shape and sr.host("far")[1].shape == sr.host("cube")[1].shape


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_faces_and_index_arrays(name):
    c = sr.case(name)
    verts, faces, normals, colors, vertex_cluster, face_index = sr.host(name)
    V, F = len(c["verts"]), len(c["faces"])
    if len(faces):
        assert faces.min() >= 0 and faces.max() < len(verts)
        assert sorted(np.unique(faces).tolist()) == list(range(len(verts)))                   # no vertex without a face
        assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
        smallest = faces.argmin(axis=1)
        canonical = np.stack([np.roll(f, -s) for f, s in zip(faces, smallest)])
        assert len(np.unique(canonical, axis=0)) == len(faces)                                # none repeats up to rotation
    assert (np.diff(face_index) > 0).all() and (len(face_index) == 0 or (0 <= face_index[0] and face_index[-1] < F))
    assert vertex_cluster.min(initial=0) >= -1 and vertex_cluster.max(initial=-1) < len(verts)
    # the index arrays reproduce the outputs: faces from the old faces, the averaged vertices and colours from the members
    assert bits(vertex_cluster[c["faces"][face_index]].reshape(-1, 3)) == bits(faces)
    average = sr.host(name, "average")
    for v in range(len(verts)):
        members = np.flatnonzero(vertex_cluster == v)
        assert len(members)
        mean = (c["verts"][members].astype(np.float64).sum(axis=0) / len(members)).astype(np.float32)
        assert np.allclose(average[0][v], mean, rtol=0, atol=1e-6)
        assert bits(colors[v]) == bits(np.rint(c["colors"][members].astype(np.float64).mean(axis=0)).astype(np.uint8))
    assert len(average[0]) == len(verts) and bits(average[4]) == bits(vertex_cluster) and bits(average[5]) == bits(face_index)


def test_named_cases():
    assert [len(a) for a in sr.host("empty_both")] == [0, 0, 0, 0, 0, 0]
    out = sr.host("empty_faces")
    assert [len(a) for a in out] == [0, 0, 0, 0, 70, 0] and (out[4] == -1).all()
    out = sr.host("single_cell")
    assert [len(a) for a in out] == [0, 0, 0, 0, 3, 0] and (out[4] == -1).all()
    verts, faces, _, _, vertex_cluster, face_index = sr.host("duplicates")
    assert face_index.tolist() == [0, 2, 8] and vertex_cluster.tolist() == [0, 2, 1, -1, 3]
    assert faces.tolist() == [[0, 2, 1], [0, 1, 2], [2, 1, 3]]
    for name, n in (("sized_1024", 1024), ("sized_1025", 1025)):
        out = sr.host(name)
        assert len(out[0]) == n and len(out[1]) == n and len(sr.case(name)["faces"]) == 2 * n
    c = sr.case("long_run")
    keys_in_hub_cell = (sr.host("long_run")[4][:3002] == sr.host("long_run")[4][0]).all()
    assert keys_in_hub_cell and len(c["faces"]) > 3000
    verts, _, normals, colors, vertex_cluster, _ = sr.host("attributes")
    first, second = vertex_cluster[0], vertex_cluster[2]
    assert vertex_cluster[1] == first and vertex_cluster[3] == second
    assert normals[first].tolist() == [0.0, 0.0, 0.0] and colors[first].tolist() == [128, 0, 254]      # halves go to even
    assert normals[second].tolist() == [0.0, 0.0, 0.0]                                                 # a length that is not finite


def test_errors_and_settings():
    for name in sorted(sr.ERROR_CASES):
        c = sr.case(name)
        for contraction in CONTRACTIONS:
            with pytest.raises(ValueError, match="2\\^21 voxels"):
                simplify_mesh(c["verts"], c["faces"], c["voxel"], contraction=contraction)
            with pytest.raises(ValueError, match="2\\^21 voxels"):
                _simplify_scalar(c["verts"], c["faces"], c["voxel"], contraction=contraction)
    c = sr.case("duplicates")
    for bad in (0.0, -0.1, float("nan"), float("inf"), None, "0.1", True):
        with pytest.raises(ValueError, match="voxel"):
            simplify_mesh(c["verts"], c["faces"], bad)
    with pytest.raises(ValueError, match="voxel"):
        simplify_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0.0)          # judged before the mesh
    with pytest.raises(ValueError, match="contraction"):
        simplify_mesh(c["verts"], c["faces"], 0.5, contraction="median")
    with pytest.raises(ValueError):
        simplify_mesh(c["verts"][:, :2], c["faces"], 0.5)
    with pytest.raises(ValueError):
        simplify_mesh(c["verts"], c["faces"], 0.5, normals=c["normals"][:-1])
    with pytest.raises(ValueError):
        simplify_mesh(c["verts"], c["faces"], 0.5, colors=c["colors"][:-1])
    settings = SimplifySettings(0.5)
    assert settings == (0.5, "quadric") and simplify_settings(SimplifySettings(1, "average")) == (1.0, "average")
    with pytest.raises(ValueError):
        simplify_settings((0.5, "quadric"))
    with pytest.raises(ValueError):
        simplify_settings(SimplifySettings(0.5, "mean"))
    with pytest.raises(AttributeError):
        settings.voxel = 1.0                                                                   # frozen
    by_settings = simplify_mesh(c["verts"], c["faces"], SimplifySettings(c["voxel"], "average"), c["normals"], c["colors"], return_index=True)
    assert_same(by_settings[:4] + by_settings[4], sr.host("duplicates", "average"), "settings")


def test_binding_table_header_and_workspace():
    import os
    import re
    from dvmvs.hip import _capi
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dvmvs_hip.h")).read(), flags=re.S)
    added = _capi.ADDED_WITHIN_ABI_MESH_SIMPLIFY
    assert sorted(added) == sorted(n for n in _capi.SIGNATURES if n.startswith("dvmvs_mesh_simplify") or n == "dvmvs_voxel_downsample_runs")
    for name in added:
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert _capi.ABI_VERSION == 11 and "#define DVMVS_ABI_VERSION 11" in header
    assert "ADDED_WITHIN_ABI_MESH_SIMPLIFY" in inspect.getsource(_capi.lib)
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _capi.lib()
    assert all(hasattr(lib, name) for name in added)
    assert lib.dvmvs_mesh_simplify_workspace_bytes(1 << 29, 1) == 0 and lib.dvmvs_mesh_simplify_workspace_bytes(1, (1 << 28) + 1) == 0
    assert lib.dvmvs_mesh_simplify_workspace_bytes(-1, 1) == 0
    small, large = lib.dvmvs_mesh_simplify_workspace_bytes(10, 20), lib.dvmvs_mesh_simplify_workspace_bytes(1 << 28, 1 << 28)
    assert 0 < small < large
    # refusals come before anything is enqueued: safe without a device
    assert lib.dvmvs_mesh_simplify_keys(None, 4, 2, None, None, None, None, 0, None, None, None, None) == -1
    assert lib.dvmvs_mesh_simplify_pair_keys(None, None, 2, None, None) == -1
    assert lib.dvmvs_mesh_simplify_emit(0, 0, None, 0, 0, 0, None, None, None, None, None, None, None) == -1
    assert lib.dvmvs_voxel_downsample_runs(0, None, None, None) == -1


def test_surface_of_the_package():
    import torch
    from dvmvs import simplify
    from dvmvs.hip import simplify as binding
    from dvmvs.tsdf import TSDFFusion, TSDFVolume, build_parser, run
    names = ["verts", "faces", "voxel", "normals", "colors", "contraction", "return_index"]
    for fn in (simplify.simplify_mesh, simplify._simplify_scalar, simplify.simplify_mesh_device, binding.simplify_mesh):
        assert list(inspect.signature(fn).parameters) == names
        assert [p.default for p in inspect.signature(fn).parameters.values()][3:] == [None, None, "quadric", False]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        simplify.simplify_mesh_device(torch.zeros(5, 3), torch.zeros((4, 3), dtype=torch.int32), 0.1)
    with pytest.raises(ValueError, match="voxel"):
        binding.simplify_mesh(torch.zeros(5, 3), torch.zeros((4, 3), dtype=torch.int32), -1.0)      # the settings are judged first
    source = inspect.getsource(binding)
    assert "custom_op" not in source and "torch.library" not in source
    for method in (TSDFVolume.get_mesh, TSDFVolume.mesh_tensors, TSDFVolume.vertices, TSDFVolume.surface_points, TSDFVolume.score_against,
                   TSDFFusion.integrate):
        assert inspect.signature(method).parameters["simplify"].default is None, method
    defaults = vars(build_parser().parse_args([]))
    parameters = inspect.signature(run).parameters
    assert defaults["simplify_mesh_voxel"] is None and parameters["simplify_mesh_voxel"].default is None
    assert defaults["simplify_mesh_average"] is False and parameters["simplify_mesh_average"].default is False
    args = build_parser().parse_args(["--simplify_mesh_voxel", "0.04", "--simplify_mesh_average"])
    assert args.simplify_mesh_voxel == 0.04 and args.simplify_mesh_average is True
    for bad in (0.0, -1.0, float("nan"), float("inf")):                                         # refused before any file is read
        with pytest.raises(ValueError, match="simplify_mesh_voxel"):
            run(**{**defaults, "simplify_mesh_voxel": bad})
    with pytest.raises(ValueError, match="simplify_mesh_voxel"):
        run(**{**defaults, "simplify_mesh_average": True})
    with pytest.raises(ValueError, match="simplify_mesh_average"):
        run(**{**defaults, "simplify_mesh_voxel": 0.1, "simplify_mesh_average": 1})
    assert "+simple" in run.__doc__
    # a filter given by position where ``clean`` alone stood is still the filter
    from dvmvs.components import ComponentFilter
    from dvmvs.tsdf.volume import mesh_stages
    rule, settings = ComponentFilter(min_faces=3), SimplifySettings(0.1)
    assert mesh_stages(rule, None) == (None, rule) and mesh_stages(settings, rule) == (settings, rule) and mesh_stages(None, None) == (None, None)
