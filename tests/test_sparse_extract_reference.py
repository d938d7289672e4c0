"""CPU: what the mesh extraction from the sparse TSDF volume (csrc/sparse_extract.hip) can show without a GPU --
the stand-alone check of csrc/sparse_extract_grid.h (binary search, neighbour rows, handling rule) under the sanitizers, the C ABI's new
entries, the parser's ``--sparse_volume_extract`` and the signatures of the new methods."""
import inspect
import os

import pytest

import sparse_extract_program

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ENTRIES = ("dvmvs_sparse_neighbours", "dvmvs_sparse_extract_count", "dvmvs_sparse_extract_scan", "dvmvs_sparse_extract_emit")


def test_sparse_extract_program_builds_and_passes():
    status, output = sparse_extract_program.run(sanitize=True)
    if status is None:
        pytest.skip("no host compiler")
    assert status == 0 and "sparse_extract_check: ok" in output, output
    for pool in ("empty pool", "one brick", "corners of the coordinate range", "slot order that is not key order"):
        assert pool in output
    assert "one brick   " in output and " 217 of their voxels handled" in output      # 9^3 - 8^3: the apron of a brick that stands alone


def test_c_abi_declares_the_extraction_entries():
    from dvmvs.hip import _capi
    assert tuple(_capi.ADDED_WITHIN_ABI_SPARSE_EXTRACT) == ENTRIES and _capi.ABI_VERSION == 11
    assert "ADDED_WITHIN_ABI_SPARSE_EXTRACT" in inspect.getsource(_capi.lib)
    header = open(os.path.join(ROOT, "include", "dvmvs_hip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header and name in _capi.SIGNATURES
    assert "section 4.8s" in header and "ALWAYS the central difference" in header and "SMALLEST KEY" in header and "ORDER:" in header
    lib = _capi.lib()
    # refusals are made before anything is enqueued: safe without a device
    assert lib.dvmvs_sparse_neighbours(None, None, None, None, 16, None, None) == -1
    assert lib.dvmvs_sparse_extract_count(None, None, None, 16, None, None) == -1
    assert lib.dvmvs_sparse_extract_scan(None, None, 16, None, None, None) == -1
    assert lib.dvmvs_sparse_extract_emit(None, None, None, None, None, 1, 0.0, 0.0, 0.0, 0.1, None, None, None, None, None, 0, 0, None) == -1


def test_the_grid_header_is_host_code_and_the_makefile_builds_the_kernels():
    grid = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "sparse_extract_grid.h")).read()
    assert "hip_runtime" not in grid and "__global__" not in grid and '#include "sparse_grid.h"' in grid
    assert "kExtractSearchSteps = 32" in grid
    makefile = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "Makefile")).read()
    assert " sparse_extract.hip" in makefile and makefile.count("sparse_extract_grid.h") == 2
    kernels = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "sparse_extract.hip")).read()
    assert "atomic" not in kernels.split('#include "dvmvs_device.h"')[1].replace("no atomics", "")


def test_tsdf_program_parses_sparse_volume_extract():
    from dvmvs.tsdf import program
    defaults = vars(program.build_parser().parse_args([]))
    assert defaults["sparse_volume_extract"] is False
    order = list(inspect.signature(program.run).parameters)      # behind the two settings it belongs to: the places after them are pinned
    assert order[order.index("sparse_volume"):order.index("sparse_volume") + 3] == ["sparse_volume", "sparse_volume_bricks", "sparse_volume_extract"]
    assert order[-3:] == ["clean_mesh_area", "clean_mesh_faces", "clean_mesh_largest"]
    assert [f for f in program.Settings.__dataclass_fields__][-1] == "sparse_volume_extract"
    args = vars(program.build_parser().parse_args(["--sparse_volume", "--sparse_volume_extract", "--clean_mesh_faces", "10"]))
    settings = program._settings(dict(args, device="cuda"))
    assert settings.sparse_volume and settings.sparse_volume_extract
    assert settings.output_name == args["system_name"] + "+sparse+clean"
    assert not program._settings(dict(defaults, device="cuda", sparse_volume=True)).sparse_volume_extract
    with pytest.raises(ValueError, match="sparse_volume_extract"):
        program._settings(dict(vars(program.build_parser().parse_args(["--sparse_volume_extract"])), device="cuda"))


@pytest.mark.parametrize("method", ["mesh_tensors", "vertices", "get_mesh", "get_point_cloud", "surface_points", "score_against"])
def test_sparse_volume_methods_take_the_dense_volumes_parameters(method):
    from dvmvs.tsdf import SparseTSDFVolume, TSDFVolume
    dense = inspect.signature(getattr(TSDFVolume, method)).parameters
    mine = inspect.signature(getattr(SparseTSDFVolume, method)).parameters
    assert list(mine)[:len(dense)] == list(dense)
    for name, parameter in dense.items():
        default = mine[name].default
        assert default is parameter.default or default == parameter.default
    assert set(mine) - set(dense) <= {"allow_overflow"}


def test_live_fusion_has_the_mesh_methods():
    from dvmvs.tsdf import LiveFusion
    for method in ("get_mesh", "mesh_tensors"):
        parameters = inspect.signature(getattr(LiveFusion, method)).parameters
        assert list(parameters) == ["self", "stages"] and parameters["stages"].kind is inspect.Parameter.VAR_KEYWORD
    assert isinstance(LiveFusion.volume, property)
