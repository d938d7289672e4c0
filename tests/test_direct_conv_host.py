"""CPU checks of the host side of csrc/direct_conv.hip (no GPU: the shape choice and the packed-weight sizes are host functions of
libdvmvs_hip.so): which problems of a 320x256 frame the kernel takes and with which output tiling, that it fills exactly 256 workgroups
on them, the size formula of the packed weights, and which of the 16 compiled kernels a problem runs (dvmvs_direct_conv_shape): every
one has a pinning case in tests/direct_conv_cases.py, and every layer of a frame at batches 1..8 runs a kernel that has one."""
import math

import pytest

import direct_conv_cases as dc
from dvmvs.hip import _capi


def lib():
    return _capi.lib()


# (C_in, H, W, C_out, k, stride) -> output-channel tiles per wave; the layers of fusionnet/model.py:167-305 at 320x256
FRAME_LAYERS = {
    (36, 256, 320, 32, 5, 1): 2, (32, 256, 320, 32, 5, 1): 2, (3, 256, 320, 32, 3, 2): 2,
    (96, 128, 160, 32, 5, 1): 2, (64, 128, 160, 32, 5, 1): 2, (65, 128, 160, 32, 5, 1): 2, (32, 128, 160, 32, 5, 1): 2, (32, 128, 160, 32, 3, 1): 2,
    (32, 128, 160, 64, 5, 2): 1, (64, 64, 80, 64, 5, 1): 1, (96, 64, 80, 64, 3, 1): 1, (128, 64, 80, 64, 3, 1): 1, (129, 64, 80, 64, 3, 1): 1,
    (64, 64, 80, 128, 3, 2): 1, (128, 32, 40, 128, 3, 1): 1, (160, 32, 40, 128, 3, 1): 1, (256, 32, 40, 128, 3, 1): 1, (257, 32, 40, 128, 3, 1): 1,
}


@pytest.mark.parametrize("layer", sorted(FRAME_LAYERS))
def test_frame_layers_are_taken_with_the_expected_tile(layer):
    C_in, H, W, C_out, k, s = layer
    assert lib().dvmvs_direct_conv_tile(1, C_in, H, W, C_out, k, s) == FRAME_LAYERS[layer]


def test_workgroup_counts_on_the_frames_maps():
    """The point of the four shapes: 256 workgroups (one per CU) on the full, 1/2 and 1/4 resolution maps, 128 on the 1/8 maps."""
    # (output H, W, C_out, tile) -> workgroups = column tiles x row tiles x channel tiles
    shapes = {2: [(4, 80, 32), (2, 40, 32)], 1: [(1, 80, 16), (2, 40, 16)]}      # tile -> candidate (rows, columns, channels) per workgroup

    def groups(OH, OW, C_out, tile):
        best = 0.0, 0
        for rows, cols, ch in shapes[tile]:
            if OW % cols or C_out % ch:
                continue
            n = (OW // cols) * math.ceil(OH / rows) * (C_out // ch)
            fill = n / (256 * math.ceil(n / 256))
            if fill > best[0] + 1e-9:
                best = fill, n
        return best[1]

    assert groups(256, 320, 32, 2) == 256 and groups(128, 160, 32, 2) == 256 and groups(64, 80, 64, 1) == 256 and groups(32, 40, 128, 1) == 128


REFUSED = [(1, 512, 16, 20, 256, 3, 1), (1, 512, 8, 10, 512, 3, 1), (1, 32, 64, 80, 1, 3, 1), (1, 32, 64, 80, 32, 7, 1),
           (1, 32, 64, 80, 32, 3, 3), (1, 32, 63, 80, 32, 3, 2), (1, 32, 64, 81, 32, 3, 1), (0, 32, 64, 80, 32, 3, 1),
           (1, 32, 64, 80, 24, 3, 1)]


@pytest.mark.parametrize("problem", REFUSED)
def test_problems_left_to_the_library_convolution(problem):
    assert lib().dvmvs_direct_conv_tile(*problem) == 0


def test_batches_keep_the_tile_of_the_single_frame():
    for layer, tile in FRAME_LAYERS.items():
        C_in, H, W, C_out, k, s = layer
        assert lib().dvmvs_direct_conv_tile(8, C_in, H, W, C_out, k, s) in (1, 2)


def test_packed_weight_sizes():
    """[output tile][input-channel groups padded to 16][k rows][ceil(n_tile k / 4) quads][64 lanes] float4."""
    for C_out, C_in, k, tile in [(32, 36, 5, 2), (32, 3, 3, 2), (128, 257, 3, 1), (64, 64, 5, 1), (16, 5, 5, 1), (48, 7, 3, 1)]:
        groups = math.ceil(math.ceil(C_in / 4) / 16) * 16
        want = 4 * (C_out // (16 * tile)) * groups * k * math.ceil(tile * k / 4) * 256
        assert lib().dvmvs_direct_conv_packed_bytes(C_out, C_in, k, tile) == want
    assert lib().dvmvs_direct_conv_packed_bytes(48, 8, 3, 2) == 0       # 48 channels are not a multiple of the 32-channel tile
    assert lib().dvmvs_direct_conv_packed_bytes(32, 8, 4, 2) == 0
    assert lib().dvmvs_direct_conv_packed_bytes(32, 8, 3, 3) == 0


# ---- which of the 16 compiled kernels a problem runs: dvmvs_direct_conv_shape (workgroup shape id) x kernel size x stride ----
def _frame_problems():
    return [(B,) + layer for layer in sorted(FRAME_LAYERS) for B in range(1, 9)]


def _variant(problem):
    return lib().dvmvs_direct_conv_shape(*problem), problem[5], problem[6]


def test_the_shape_query_joined_abi_11_without_a_new_number():
    import inspect
    assert _capi.ABI_VERSION == 11 and lib().dvmvs_abi_version() == 11
    assert tuple(_capi.ADDED_WITHIN_ABI_DIRECT_CONV_SHAPE) == ("dvmvs_direct_conv_shape",) and "dvmvs_direct_conv_shape" in _capi.SIGNATURES
    assert "ADDED_WITHIN_ABI_DIRECT_CONV_SHAPE" in inspect.getsource(_capi.lib)         # part of the stale-library check
    from dvmvs.hip import ops
    assert [ops.direct_conv_shape(*problem) for problem in dc.CASES] == [variant[0] for variant in dc.CASES.values()]


def test_the_tile_is_the_tile_of_the_chosen_shape():
    """dvmvs_direct_conv_tile is a function of dvmvs_direct_conv_shape -- ids 1 and 2 pack two 16-channel tiles per wave, 3 and 4 one --
    and both are 0 together: over the frame's layers at batches 1..8, the refused problems and the kernel-pinning cases."""
    problems = _frame_problems() + REFUSED + list(dc.CASES)
    assert len(problems) == 18 * 8 + 9 + 48
    for problem in problems:
        shape, tile = lib().dvmvs_direct_conv_shape(*problem), lib().dvmvs_direct_conv_tile(*problem)
        assert shape in (0, 1, 2, 3, 4) and tile == dc.TILE_OF_SHAPE[shape], (problem, shape, tile)
    assert all(lib().dvmvs_direct_conv_shape(*problem) == 0 for problem in REFUSED)
    assert all(lib().dvmvs_direct_conv_shape(*problem) != 0 for problem in _frame_problems())


@pytest.mark.parametrize("case", sorted(dc.CASES), ids=dc.case_id)
def test_every_pinning_case_runs_the_kernel_it_is_there_for(case):
    assert _variant(case) == dc.CASES[case]


def test_the_batch_stride_cases_run_one_problem_per_kernel():
    assert sorted(dc.STRIDE_CASES.values()) == dc.ALL_VARIANTS and all(case[0] >= 2 and case[1] == 37 for case in dc.STRIDE_CASES)
    for case, variant in dc.STRIDE_CASES.items():
        assert _variant(case) == variant, case


def test_the_pinning_cases_cover_all_sixteen_kernels():
    """Coverage gate of tests/test_direct_conv_variants_gpu.py: its cases reach every (shape, kernel size, stride) that is compiled."""
    assert len(dc.ALL_VARIANTS) == 16
    assert sorted({_variant(case) for case in dc.CASES}) == dc.ALL_VARIANTS
    for variant in dc.ALL_VARIANTS:      # ... each with a ragged group, a ragged last chunk and whole chunks only
        assert sorted(case[1] for case in dc.CASES if _variant(case) == variant) == sorted(dc.INPUT_CHANNELS)


def test_every_frame_layer_runs_a_pinned_kernel_at_batches_1_to_8():
    """Workload gate: whatever kernel a layer of a 320x256 frame is sent to at batch 1..8 (bench.py's default is 8) is one that a pinning
    case compares with fp64.  A change of the chooser or of the shape table that moves a layer elsewhere fails here, without a GPU."""
    pinned = {_variant(case) for case in dc.CASES}
    for problem in _frame_problems():
        assert _variant(problem) in pinned, problem
