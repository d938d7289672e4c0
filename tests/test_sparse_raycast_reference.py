"""CPU: what the ray-caster of the sparse TSDF volume (csrc/sparse_raycast.hip) can show without a GPU -- the
stand-alone check of csrc/sparse_raycast_grid.h (render index, corner arithmetic, flag rule) under the sanitizers, the C ABI's new
entries and their refusals, the parser's ``--sparse_volume_render`` and the signatures of the new methods."""
import inspect
import os

import pytest

import sparse_raycast_program

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ENTRIES = ("dvmvs_sparse_raycast_index", "dvmvs_sparse_raycast_flags", "dvmvs_sparse_raycast_fwd")


def test_sparse_raycast_program_builds_and_passes():
    status, output = sparse_raycast_program.run(sanitize=True)
    if status is None:
        pytest.skip("no host compiler")
    assert status == 0 and "sparse_raycast_check: ok" in output, output
    for case in ("empty pool", "one brick", "corners of the coordinate range", "slot order that is not key order", "an index filled to half",
                 "3x3x3 minus its centre: corners and flags"):
        assert case in output
    assert "4096 bricks in   8192 entries" in output


def test_c_abi_declares_the_raycast_entries():
    from dvmvs.hip import _capi
    assert tuple(_capi.ADDED_WITHIN_ABI_SPARSE_RAYCAST) == ENTRIES and _capi.ABI_VERSION == 11
    assert "ADDED_WITHIN_ABI_SPARSE_RAYCAST" in inspect.getsource(_capi.lib)
    header = open(os.path.join(ROOT, "include", "dvmvs_hip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header and name in _capi.SIGNATURES
    assert "section 4.8t" in header and "BIT FOR BIT" in header and "#define DVMVS_ABI_VERSION 11" in header
    lib = _capi.lib()
    # refusals are made before anything is enqueued: safe without a device
    assert lib.dvmvs_sparse_raycast_index(None, None, 16, None, 32, None) == -1
    assert lib.dvmvs_sparse_raycast_flags(None, None, None, None, None, 16, None, 32, None, None) == -1
    assert lib.dvmvs_sparse_raycast_fwd(None, None, None, None, 16, None, 32, None, None, 0, 0, 0, 1, 1, 1, 0.0, 0.0, 0.0, 0.1, 1, None, None, 1, 8,
                                        8, 0.0, 1.0, 1.0, None, None, None, None) == -1


def test_the_grid_header_is_host_code_and_the_makefile_builds_the_kernels():
    grid = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "sparse_raycast_grid.h")).read()
    assert "hip_runtime" not in grid and "__global__" not in grid and '#include "sparse_grid.h"' in grid
    assert "sg_hash" in grid and "sg_probe" in grid
    makefile = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "Makefile")).read()
    assert " sparse_raycast.hip" in makefile and makefile.count("sparse_raycast_grid.h") == 2 and makefile.count("sparse_extract_grid.h") == 2
    kernels = open(os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "sparse_raycast.hip")).read()
    assert "atomicAdd" not in kernels and "__shared__" not in kernels and "fp contract(off)" in kernels
    assert '#include "sparse_raycast_grid.h"' in kernels


def test_tsdf_program_parses_sparse_volume_render():
    from dvmvs.tsdf import program
    defaults = vars(program.build_parser().parse_args([]))
    assert defaults["sparse_volume_render"] is False
    order = list(inspect.signature(program.run).parameters)
    assert order[order.index("sparse_volume_extract") + 1] == "sparse_volume_render"
    fields = [f for f in program.Settings.__dataclass_fields__]
    assert fields[-2:] == ["sparse_volume_render", "sparse_volume_extract"]
    args = vars(program.build_parser().parse_args(["--sparse_volume", "--render_keyframes", "--sparse_volume_render"]))
    settings = program._settings(dict(args, device="cuda"))
    assert settings.sparse_volume and settings.sparse_volume_render and not settings.sparse_volume_extract
    assert settings.output_name == args["system_name"] + "+sparse"
    assert not program._settings(dict(defaults, device="cuda", sparse_volume=True)).sparse_volume_render
    with pytest.raises(ValueError, match="sparse_volume_render"):
        program._settings(dict(vars(program.build_parser().parse_args(["--sparse_volume_render"])), device="cuda"))


def test_sparse_volume_render_takes_the_dense_volumes_parameters():
    from dvmvs.tsdf import SparseTSDFVolume, TSDFVolume
    dense = inspect.signature(TSDFVolume.render).parameters
    mine = inspect.signature(SparseTSDFVolume.render).parameters
    assert list(mine)[:len(dense)] == list(dense)
    for name, parameter in dense.items():
        default = mine[name].default
        assert default is parameter.default or default == parameter.default
    assert list(mine)[len(dense):] == ["bounds", "allow_overflow"]
    assert mine["bounds"].default is None and mine["allow_overflow"].default is False
    # one helper computes the box for dense() and render(): the two cannot drift
    assert "self._box(" in inspect.getsource(SparseTSDFVolume.dense) and "self._box(" in inspect.getsource(SparseTSDFVolume.render)


def test_live_fusion_has_render():
    from dvmvs.tsdf import LiveFusion
    parameters = inspect.signature(LiveFusion.render).parameters
    assert list(parameters)[:5] == ["self", "cam_intr", "cam_poses", "height", "width"]


def test_the_bindings_stay_out_of_the_ops_surface():
    from dvmvs.hip import ops, sparse
    for name in ("sparse_raycast_index", "sparse_raycast_flags", "sparse_raycast"):
        assert callable(getattr(sparse, name)) and not hasattr(ops, name)
    assert sparse.raycast_index_slots(1) == 16 and sparse.raycast_index_slots(1024) == 2048 and sparse.raycast_index_slots(1025) == 4096
    assert sparse.raycast_steps((17, 17, 25), 1.0) == 277.0
