"""CPU: the host definition of mesh cleaning (dvmvs/components.py) against scipy's connected components and hand-computed expectations, and
the surface the feature adds: the binding table, the C entry points' refusals (made before anything is enqueued, so safe without a GPU),
the ``clean`` keywords and the program's flags."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import components_reference as cr
from dvmvs.components import ComponentFilter, filter_components, filter_settings, kept_components, mesh_components

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SYMBOLS = ("dvmvs_mesh_components_workspace_bytes", "dvmvs_mesh_components_fwd", "dvmvs_mesh_filter_count", "dvmvs_mesh_filter_emit")


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cr.CASES))
def test_labels_are_scipys_components_with_smallest_index_labels(name):
    case, parts = cr.case(name), cr.host(name)
    V, F = len(case["verts"]), len(case["faces"])
    labels = parts["labels"]
    assert labels.dtype == np.int32 and labels.shape == (V,)
    assert np.array_equal(labels, cr.scipy_labels(case["faces"], V))
    valid = np.all((case["faces"] >= 0) & (case["faces"] < V), axis=1)
    want_face = np.where(valid, labels[np.where(valid, case["faces"][:, 0], 0)] if V else -1, -1)
    assert parts["face_labels"].dtype == np.int32 and np.array_equal(parts["face_labels"], want_face)
    assert parts["face_count"].dtype == np.int32 and parts["face_count"].shape == (V,)
    assert np.array_equal(parts["face_count"], np.bincount(want_face[valid], minlength=V)[:V] if V else np.zeros(0))
    assert parts["n_components"] == len(np.unique(want_face[valid]))
    from dvmvs.errors import quantised_face_areas
    areas, _ = quantised_face_areas(case["verts"], case["faces"])
    want_area = np.zeros(V, dtype=np.int64)
    for f in np.flatnonzero(valid):
        want_area[want_face[f]] += areas[f]
    assert parts["area"].dtype == np.int64 and np.array_equal(parts["area"], want_area)
    assert parts["face_count"].sum() == valid.sum() and F == len(parts["face_labels"])
    without = mesh_components(case["faces"], V)
    assert "area" not in without and np.array_equal(without["labels"], labels)


def test_tetrahedra_by_hand():
    case, parts = cr.case("tetrahedra"), cr.host("tetrahedra")
    assert parts["labels"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8]
    assert parts["face_labels"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, -1, -1]
    assert parts["face_count"].tolist() == [4, 0, 0, 0, 4, 0, 0, 0, 0] and parts["n_components"] == 2
    # three legs' faces of 1/2 and the slanted face of sqrt(3)/2; the second is half the size: a quarter of the area (each A_f is rounded)
    large, small = parts["area"][0], parts["area"][4]
    assert abs(large - (1.5 + np.sqrt(3.0) / 2.0) * 2.0 ** 32) <= 2 and abs(small - large / 4.0) <= 2
    assert not parts["area"][[1, 2, 3, 5, 6, 7, 8]].any()
    verts, faces, normals, colors, (vertex_index, face_index) = filter_components(
        case["verts"], case["faces"], ComponentFilter(min_area=1.0), case["normals"], case["colors"], return_index=True)
    assert vertex_index.tolist() == [0, 1, 2, 3] and face_index.tolist() == [0, 1, 2, 3] and faces.tolist() == cr.TET.tolist()
    assert np.array_equal(verts, case["verts"][:4]) and np.array_equal(normals, case["normals"][:4]) and np.array_equal(colors, case["colors"][:4])
    assert vertex_index.dtype == face_index.dtype == faces.dtype == np.int32 and colors.dtype == np.uint8
    verts, faces, normals, colors = filter_components(case["verts"], case["faces"], ComponentFilter(min_faces=1))
    assert normals is None and colors is None and len(verts) == 8 and faces.tolist() == np.concatenate([cr.TET, cr.TET + 4]).tolist()
    verts, faces, _, _ = filter_components(case["verts"], case["faces"], ComponentFilter(min_faces=5))
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and verts.dtype == np.float32 and faces.dtype == np.int32


@pytest.mark.parametrize("name", ["tetrahedra", "strip", "soup", "ties"])
def test_face_order_does_not_matter_and_kept_order_is_the_original(name):
    case, parts = cr.case(name), cr.host(name)
    order = np.random.default_rng(11).permutation(len(case["faces"]))
    shuffled = mesh_components(case["faces"][order], len(case["verts"]), case["verts"])
    for key in ("labels", "face_count", "area"):
        assert np.array_equal(shuffled[key], parts[key]), key
    assert np.array_equal(shuffled["face_labels"], parts["face_labels"][order])
    for rule in cr.filters(name):
        verts, faces, normals, colors, vertex_index, face_index = cr.host_filtered(name, rule)
        assert np.all(np.diff(vertex_index) > 0) and np.all(np.diff(face_index) > 0)            # the original order
        assert np.array_equal(verts, case["verts"][vertex_index]) and np.array_equal(colors, case["colors"][vertex_index])
        assert np.array_equal(vertex_index[faces], case["faces"][face_index])                     # re-indexed, the same triangles
        assert set(np.unique(faces)) == set(range(len(verts)))                                    # exactly the vertices that kept faces use
        again = filter_components(case["verts"], case["faces"][order], rule, return_index=True)
        assert set(order[again[4][1]].tolist()) == set(face_index.tolist())                      # the same faces, as a set
        assert np.array_equal(again[4][0], vertex_index)


def test_tie_rules():
    case, parts = cr.case("ties"), cr.host("ties")
    assert parts["labels"].tolist() == [0] * 3 + [3] * 4 + [7] * 4 + [11] * 3 + [14] * 3
    assert parts["area"][[0, 3, 7, 11, 14]].tolist() == [2 ** 32, 2 ** 32, 2 ** 32, 2 ** 31, 2 ** 31]
    assert parts["face_count"][[0, 3, 7, 11, 14]].tolist() == [1, 2, 2, 1, 1]
    keep = kept_components(parts["face_count"], parts["area"], ComponentFilter(keep_largest=True))
    assert np.flatnonzero(keep).tolist() == [3]                     # area ties: the greater count; then the smaller label
    _, _, _, _, (vertex_index, face_index) = filter_components(case["verts"], case["faces"], ComponentFilter(keep_largest=True), return_index=True)
    assert vertex_index.tolist() == [3, 4, 5, 6] and face_index.tolist() == [1, 2]
    # the largest fails a threshold: nothing is kept, although other components pass it
    keep = kept_components(parts["face_count"], parts["area"], ComponentFilter(min_area=1.0 + 2.0 ** -20, keep_largest=True))
    assert not keep.any()
    # the threshold is compared as area >= ceil(min_area 2^32): exactly 1 m^2 passes, the next representable value above does not
    assert np.flatnonzero(kept_components(parts["face_count"], parts["area"], ComponentFilter(min_area=1.0))).tolist() == [0, 3, 7]
    assert not kept_components(parts["face_count"], parts["area"], ComponentFilter(min_area=np.nextafter(1.0, 2.0))).any()
    assert np.flatnonzero(kept_components(parts["face_count"], parts["area"], ComponentFilter(min_faces=2))).tolist() == [3, 7]


def test_refusals():
    case = cr.nan_face()
    with pytest.raises(ValueError, match="not finite"):
        mesh_components(case["faces"], len(case["verts"]), case["verts"])
    with pytest.raises(ValueError, match="not finite"):
        filter_components(case["verts"], case["faces"], ComponentFilter())
    assert mesh_components(case["faces"], len(case["verts"]))["n_components"] == 2           # without areas nothing is read from the vertices
    huge = np.array([[0, 0, 0], [4e4, 0, 0], [0, 4e4, 0], [0, 0, 4e4]], dtype=np.float32)   # each face below 2^31 m^2, the four together above
    with pytest.raises(ValueError, match="2\\^31 square metres"):
        mesh_components(cr.TET, 4, huge)
    assert mesh_components(cr.TET[:2], 4, huge)["area"][0] == 2 * int(8e8 * 2 ** 32)
    for bad in (ComponentFilter(min_area=-1.0), ComponentFilter(min_area=float("nan")), ComponentFilter(min_area=2.0 ** 31),
                ComponentFilter(min_faces=-1), ComponentFilter(min_faces=2.5), ComponentFilter(min_faces=float("nan")),
                ComponentFilter(keep_largest=1), ComponentFilter(min_area="1"), (0.0, 0, False)):
        with pytest.raises(ValueError):
            filter_settings(bad)
        with pytest.raises(ValueError):
            filter_components(case["verts"], case["faces"], bad)
    assert filter_settings(ComponentFilter()) == (0, 0, False)
    assert filter_settings(ComponentFilter(0.5, 3.0, True)) == (2 ** 31, 3, True)
    assert filter_settings(ComponentFilter(min_area=2.0 ** -33)) == (1, 0, False)              # rounded up
    assert ComponentFilter._fields == ("min_area", "min_faces", "keep_largest")


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
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
    assert tuple(_capi.ADDED_WITHIN_ABI_MESH_COMPONENTS) == SYMBOLS
    assert "ADDED_WITHIN_ABI_MESH_COMPONENTS" in inspect.getsource(_capi.lib)        # part of the stale-library check
    assert "mesh_components.hip" in open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "Makefile")).read()


def test_workspace_sizes(lib):
    size = lib.dvmvs_mesh_components_workspace_bytes
    assert size(-1, 10) == 0 and size(10, -1) == 0 and size(2 ** 28 + 1, 10) == 0 and size(10, 2 ** 28 + 1) == 0
    assert size(0, 0) > 0 and size(2 ** 28, 2 ** 28) > 0

    def up(nbytes):
        return (nbytes + 255) // 256 * 256

    def want(V, F):      # header | area halves | parent | new index | block totals of the faces and of the vertices
        return up(256) + 2 * up(8 * V) + 2 * up(4 * V) + up(4 * ((F + 1023) // 1024)) + up(4 * ((V + 1023) // 1024))
    for V, F in ((0, 0), (1, 1), (1000, 2000), (1024, 1025), (2 ** 20, 2 ** 21), (2 ** 28, 2 ** 28)):
        assert size(V, F) == want(V, F), (V, F)


def test_argument_validation_without_a_device(lib):
    """Negative return codes come before anything is enqueued, so these calls are safe without a GPU."""
    one = ctypes.c_void_p(4096)                                                      # a non-null, aligned address; never dereferenced
    odd = ctypes.c_void_p(4098)
    big = 1 << 40

    def fwd(verts=one, V=10, faces=one, F=20, workspace=one, nbytes=big, labels=one, face_labels=one, face_count=one, area=one, result=one):
        return lib.dvmvs_mesh_components_fwd(verts, V, faces, F, workspace, nbytes, labels, face_labels, face_count, area, result, None)

    for null in ("faces", "workspace", "labels", "face_labels", "face_count", "result", "verts", "area"):      # (verts and area go together)
        assert fwd(**{null: None}) == -1, null
    for name in ("verts", "faces", "workspace", "labels", "face_labels", "face_count", "area", "result"):
        assert fwd(**{name: odd}) == -1, name
    for bad in ({"V": -1}, {"F": -1}, {"nbytes": lib.dvmvs_mesh_components_workspace_bytes(10, 20) - 1}, {"area": ctypes.c_void_p(4100)}):
        assert fwd(**bad) == -1, bad
    assert fwd(V=2 ** 28 + 1) == -2 and fwd(F=2 ** 28 + 1) == -2

    def count(labels=one, face_labels=one, face_count=one, area=one, result=one, V=10, F=20, min_area=0, min_faces=0, largest=0, workspace=one,
              nbytes=big, counts=one):
        return lib.dvmvs_mesh_filter_count(labels, face_labels, face_count, area, result, V, F, min_area, min_faces, largest, workspace, nbytes,
                                           counts, None)

    for null in ("labels", "face_labels", "face_count", "area", "result", "workspace", "counts"):
        assert count(**{null: None}) == -1, null
        assert count(**{null: odd}) == -1, null
    for bad in ({"V": -1}, {"F": -1}, {"min_area": -1}, {"min_faces": -1}, {"largest": 2}, {"largest": -1},
                {"nbytes": lib.dvmvs_mesh_components_workspace_bytes(10, 20) - 1}):
        assert count(**bad) == -1, bad
    assert count(V=2 ** 28 + 1) == -2

    def emit(verts=one, faces=one, normals=one, colors=one, labels=one, face_labels=one, face_count=one, area=one, V=10, F=20, min_area=0,
             min_faces=0, largest=0, workspace=one, nbytes=big, V_out=5, F_out=6, verts_out=one, faces_out=one, normals_out=one, colors_out=one,
             vertex_index=one, face_index=one):
        return lib.dvmvs_mesh_filter_emit(verts, faces, normals, colors, labels, face_labels, face_count, area, V, F, min_area, min_faces, largest,
                                          workspace, nbytes, V_out, F_out, verts_out, faces_out, normals_out, colors_out, vertex_index, face_index,
                                          None)

    for null in ("verts", "faces", "labels", "face_labels", "face_count", "area", "workspace", "verts_out", "faces_out", "normals", "normals_out",
                 "colors", "colors_out"):                                         # (an attribute and its output go together)
        assert emit(**{null: None}) == -1, null
    for name in ("verts", "faces", "normals", "labels", "face_labels", "face_count", "area", "workspace", "verts_out", "faces_out", "normals_out",
                 "vertex_index", "face_index"):
        assert emit(**{name: odd}) == -1, name
    for bad in ({"V": 0}, {"F": 0}, {"V_out": -1}, {"F_out": -1}, {"V_out": 11}, {"F_out": 21}, {"min_area": -1}, {"min_faces": -1}, {"largest": 2},
                {"nbytes": lib.dvmvs_mesh_components_workspace_bytes(10, 20) - 1}):
        assert emit(**bad) == -1, bad
    assert emit(V=2 ** 28 + 1) == -2


def test_binding_module_refuses_host_tensors_and_registers_nothing():
    import torch
    from dvmvs import components
    from dvmvs.hip import components as binding
    faces = torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        binding.mesh_components(faces, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        components.mesh_components_device(faces, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        components.filter_components_device(torch.zeros(5, 3), faces, ComponentFilter())
    with pytest.raises(ValueError):
        binding.filter_components(torch.zeros(5, 3), faces, ComponentFilter(min_area=-1.0))      # the settings are judged first
    with pytest.raises(ValueError):
        binding.mesh_components(torch.zeros((4, 2), dtype=torch.int32), 5)
    assert str(inspect.signature(binding.mesh_components)) == "(faces: torch.Tensor, n_verts: int, verts: Optional[torch.Tensor] = None)"
    assert list(inspect.signature(binding.filter_components).parameters) == ["verts", "faces", "filter", "normals", "colors", "return_index"]
    assert list(inspect.signature(components.filter_components).parameters) == ["verts", "faces", "filter", "normals", "colors", "return_index"]
    # not an op of the ops package, and nothing registered under torch.ops.dvmvs
    from dvmvs.hip import ops
    assert not hasattr(ops, "mesh_components") and not hasattr(ops, "filter_components") and not hasattr(ops, "components")
    source = inspect.getsource(binding)
    assert "custom_op" not in source and "torch.library" not in source


def test_clean_keywords():
    from dvmvs.tsdf import TSDFFusion, TSDFVolume
    parameters = inspect.signature(TSDFVolume.score_against).parameters
    names = list(parameters)
    assert names[names.index("visible_from") + 1] == "clean" and parameters["clean"].default is None
    assert names[-3:] == ["align_distance", "align_scale", "return_transform"]
    for method in (TSDFVolume.get_mesh, TSDFVolume.mesh_tensors, TSDFVolume.vertices, TSDFVolume.surface_points, TSDFFusion.integrate):
        parameters = inspect.signature(method).parameters
        assert list(parameters)[-1] == "clean" and parameters["clean"].default is None, method


def test_program_flags(tmp_path):
    from dvmvs.tsdf import build_parser, main, run
    defaults = vars(build_parser().parse_args([]))
    parameters = inspect.signature(run).parameters
    assert list(parameters)[-3:] == ["clean_mesh_area", "clean_mesh_faces", "clean_mesh_largest"]
    for name, value in (("clean_mesh_area", None), ("clean_mesh_faces", None), ("clean_mesh_largest", False)):
        assert defaults[name] == parameters[name].default and defaults[name] is value, name
    args = build_parser().parse_args(["--clean_mesh_area", "0.01", "--clean_mesh_faces", "50", "--clean_mesh_largest"])
    assert args.clean_mesh_area == 0.01 and args.clean_mesh_faces == 50 and args.clean_mesh_largest is True
    # each refusal names its flag and comes before any file is read (the folders do not exist)
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="clean_mesh_area"):
            run(**{**defaults, "clean_mesh_area": bad})
    with pytest.raises(ValueError, match="clean_mesh_faces"):
        run(**{**defaults, "clean_mesh_faces": -1})
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="clean_mesh_largest"):
            run(**{**defaults, "clean_mesh_largest": bad})
    with pytest.raises(ValueError, match="clean_mesh_area"):
        main(["--reconstruction_folder", str(tmp_path / "out"), "--clean_mesh_area", "-1"])
    assert not list(tmp_path.iterdir())
    assert "render_keyframes" in run.__doc__ and "+clean" in run.__doc__
