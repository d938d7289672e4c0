"""The problems that pin each of the 16 kernels csrc/direct_conv.hip compiles -- workgroup shape id (1..4, the comment above kDcShapes)
x kernel size (3, 5) x stride (1, 2) -- to an fp64 convolution.  Shared by tests/test_direct_conv_host.py (CPU: the chooser sends
every case to the kernel it is meant for, and every layer of a frame at batches 1..8 to a kernel that has a case) and
tests/test_direct_conv_variants_gpu.py (the kernels themselves).  No GPU and no library needed to import it.

The geometry is the smallest per kernel that still has every edge: more than one workgroup along y with a ragged last row tile where the
tile has more than one row (5 output rows of 4, 5 of 2, 3 of 2), one tile along x (80 or 40 output columns), 512 output channels at
batch 8 / 3 where the chooser needs that many workgroups to prefer the shape, and three input-channel counts:
3 = one ragged group of four; 37 = several chunks with a ragged last group (a chunk is 16 channels for shape 1, 32 for the others);
32 = whole chunks only, so that the kernel's unconditional request for the chunk behind the last one is all there is beyond the input."""

# shape id -> stride -> (B, C_out, H, W) of the input
GEOMETRY = {
    1: {1: (8, 512, 5, 80), 2: (8, 512, 10, 160)},      # last row tile: 1 of 4 rows
    2: {1: (3, 512, 5, 40), 2: (3, 512, 10, 80)},       # 1 of 2 rows
    3: {1: (1, 16, 2, 80), 2: (1, 16, 4, 160)},         # the tile is one row: two row tiles
    4: {1: (1, 16, 3, 40), 2: (1, 16, 6, 80)},          # 1 of 2 rows
}
KERNEL_SIZES = (3, 5)
STRIDES = (1, 2)
INPUT_CHANNELS = (3, 37, 32)
TILE_OF_SHAPE = {0: 0, 1: 2, 2: 2, 3: 1, 4: 1}          # dvmvs_direct_conv_tile of dvmvs_direct_conv_shape
ALL_VARIANTS = sorted((shape, k, stride) for shape in GEOMETRY for k in KERNEL_SIZES for stride in STRIDES)

# problem (B, C_in, H, W, C_out, k, stride) -> the (shape id, k, stride) it is there to run
CASES = {}
for _shape, _by_stride in GEOMETRY.items():
    for _stride, (_B, _C_out, _H, _W) in _by_stride.items():
        for _k in KERNEL_SIZES:
            for _C_in in INPUT_CHANNELS:
                CASES[(_B, _C_in, _H, _W, _C_out, _k, _stride)] = (_shape, _k, _stride)


# the batch strides of the C entry need a second batch item to matter: per kernel its 37-channel case, at batch 2 where the case has batch 1
STRIDE_CASES = {(max(_c[0], 2),) + _c[1:]: _v for _c, _v in CASES.items() if _c[1] == 37}


def case_id(case):
    B, C_in, H, W, C_out, k, stride = case
    shape = CASES[case][0] if case in CASES else STRIDE_CASES[case][0]
    return f"shape{shape}-k{k}s{stride}-b{B}c{C_in}x{H}x{W}to{C_out}"
