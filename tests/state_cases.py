"""Inputs of the recurrent chain's forward tests (a helper module like direct_conv_cases.py: no fixtures, no test module imports
another): the gate maps on both sides of every layout boundary, the hard gate values, and hidden-warp geometries built so that each
class of sample -- inside, across each border, all taps outside, behind the source camera -- is there BY CONSTRUCTION.
tests/test_frame_reference.py proves the classes and the preconditions on the CPU; tests/test_state_kernels_gpu.py runs the kernels."""
import math

import torch

# H*W on both sides of every layout boundary of dispatch_gates: 1, 5, 15, 64 | 65, 80, 128 | 129, 256 | 257, 512 | 513, 1024
GATE_MAPS = [(1, 1), (1, 5), (3, 5), (8, 8), (5, 13), (8, 10), (8, 16), (3, 43), (16, 16), (1, 257), (16, 32), (19, 27), (32, 32)]


def gate_layout(HW):
    """(lanes per row, elements per lane) that dispatch_gates (csrc/lstm_gates.hip) picks for a plane of HW elements; None: refused."""
    for lanes, per_lane in ((16, 4), (64, 2), (64, 4), (64, 8), (64, 16)):
        if HW <= lanes * per_lane:
            return lanes, per_lane
    return None


def gate_inputs(B, hid, H, W, seed, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4 * hid, H, W, generator=g) * scale, torch.randn(B, hid, H, W, generator=g)


def hard_gate_inputs(kind, B, hid, H, W, seed):
    """``narrow``: g-gate rows of offset 5 and sigma 1e-3 (the LayerNorm amplifies by 1000).  ``saturated``: |cc| around 20 (saturated
    sigmoids), two g rows and one cell-state row with a single outlier that drives the normalised value deep into the CELU's tail."""
    g = torch.Generator().manual_seed(seed)
    cc, c = gate_inputs(B, hid, H, W, seed + 1)
    if kind == "narrow":
        cc[:, 3 * hid:] = 5.0 + 1e-3 * torch.randn(B, hid, H, W, generator=g)
        return cc, c
    assert kind == "saturated" and hid >= 2
    sat = 20.0 * torch.sign(torch.randn(B, 4 * hid, H, W, generator=g)) + 0.3 * torch.randn(B, 4 * hid, H, W, generator=g)
    sat[:, 3 * hid:3 * hid + 2] = 20.0 + 0.3 * torch.randn(B, 2, H, W, generator=g)
    sat[:, 3 * hid:3 * hid + 2, 0, 0] = -20.0
    c_sat = 20.0 * torch.randn(B, hid, H, W, generator=g)
    c_sat[:, 0] = 20.0
    c_sat[:, 0, H // 2, W // 2] = -20.0
    return sat, c_sat


# ----------------------------------------------------------------------------------------------------------------------
# hidden-state warp
# ----------------------------------------------------------------------------------------------------------------------
WARP_SHAPES = [(2, 7, 8, 8), (3, 1, 5, 9), (1, 2, 1, 7), (1, 2, 7, 1), (1, 512, 8, 10)]
WARP_GRID_STRIDE_SHAPE = (2, 1100, 15, 16)       # 528 000 elements: more than the 2048 x 256 threads launched
WARP_KINDS = ["sideways", "shift", "forward", "behind", "borders"]
SHIFTS = [(1.5, -0.5), (-2.25, 1.25), (0.75, 2.5)]            # "shift": pixels in x and y, per batch item
MIN_ABS_Z = 0.05            # every pixel's source-camera z before the clamp is farther than this from 0


def special_depths():
    """0, 0.01f exactly, and the next float above 0.01f: on either side of the cell's ``depth <= 0.01`` mask."""
    edge = torch.tensor(0.01, dtype=torch.float32)
    return torch.tensor(0.0), edge, torch.nextafter(edge, torch.tensor(1.0))


def _rot_y(deg):
    t = math.radians(deg)
    R = torch.eye(4, dtype=torch.float64)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = math.cos(t), math.sin(t), -math.sin(t), math.cos(t)
    return R


def warp_case(kind, B, H, W, seed):
    """(depth [B,1,H,W], T [B,4,4], K [B,3,3]) in float32, T and K different for every batch item.  The principal point is near the
    map's centre ((W-1)/2, (H-1)/2), the focal lengths near max(W, H, 2) pixels: rays reach about +-0.5 at the borders.

    * ``sideways``  a few degrees about y and a small translation with t_z >= 0.1; depths in [0.5, 3) with 0, 0.01f and the next
                    float sprinkled in -- a point of depth 0 lands at t itself, far outside the map (all four taps outside);
    * ``shift``     T = translation by (sx * d / fx, sy * d / fy, 0) at constant depth d = 2: every sample sits at (x + sx, y + sy);
    * ``forward``   t_z >= 1.5 at depths in [1, 2) (and the special ones): everything contracts towards the principal point by
                    d / (d + t_z) <= 0.58, all samples inside the map;
    * ``behind``    half a turn about y and t_z <= -0.3: every point has z <= -0.3 in the source camera and is clamped to 0;
    * ``borders``   constant depth d = 1.5 and t_z < 0 chosen so that the map is magnified about the principal point by
                    s = 1 + (0.5 + 0.1 b) / max(cx, cy): column 0 samples at cx (1 - s) in (-1, 0), column W-1 in (W-1, W), and the same
                    for the rows -- taps across each of the four borders."""
    g = torch.Generator().manual_seed(seed)
    lo, span = (1.0, 1.0) if kind == "forward" else (0.5, 2.5)
    depth = lo + span * torch.rand(B, 1, H, W, generator=g)
    if kind == "shift":
        depth[:] = 2.0
    elif kind == "borders":
        depth[:] = 1.5
    else:
        flat, idx = depth.view(-1), torch.arange(depth.numel())
        zero, edge, above = special_depths()
        flat[idx % 5 == 1], flat[idx % 7 == 3], flat[idx % 11 == 5] = zero, edge, above
    Ts, Ks = [], []
    for b in range(B):
        f = float(max(W, H, 2))
        K = torch.tensor([[f * (1.0 + 0.07 * b), 0.0, (W - 1) / 2 + 0.13 * b], [0.0, f * (1.1 - 0.05 * b), (H - 1) / 2 - 0.09 * b],
                          [0.0, 0.0, 1.0]], dtype=torch.float64)
        T = torch.eye(4, dtype=torch.float64)
        if kind == "sideways":
            T = _rot_y(3.0 * (b + 1))
            T[:3, 3] = torch.tensor([0.12 * (b + 1), -0.15, 0.1 + 0.05 * b], dtype=torch.float64)
        elif kind == "shift":
            sx, sy = SHIFTS[b]
            T[:3, 3] = torch.tensor([sx * 2.0 / float(K[0, 0]), sy * 2.0 / float(K[1, 1]), 0.0], dtype=torch.float64)
        elif kind == "forward":
            T[:3, 3] = torch.tensor([0.02 * b, 0.01, 1.5 + 0.2 * b], dtype=torch.float64)
        elif kind == "behind":
            T = _rot_y(180.0 + 5.0 * b)
            T[:3, 3] = torch.tensor([0.05, 0.02, -0.3 - 0.1 * b], dtype=torch.float64)
        elif kind == "borders":
            s = 1.0 + (0.5 + 0.1 * b) / max(float(K[0, 2]), float(K[1, 2]))
            T[2, 3] = 1.5 / s - 1.5
        else:
            raise ValueError(kind)
        Ts.append(T)
        Ks.append(K)
    return depth, torch.stack(Ts).float(), torch.stack(Ks).float()


def warp_classes(ix, iy, z, H, W):
    """How many pixels of each class the float64 positions ``ix, iy`` and source-camera z [B,H,W] hold: the north-west tap (floor of the
    position) in column -1 / W-1, in row -1 / H-1, all four taps outside the map, z clamped, and the sample position inside the map."""
    x0, y0 = torch.floor(ix), torch.floor(iy)
    count = lambda m: int(m.sum())      # noqa: E731
    return dict(west=count(x0 == -1), east=count(x0 == W - 1), north=count(y0 == -1), south=count(y0 == H - 1),
                outside=count((x0 < -1) | (x0 > W - 1) | (y0 < -1) | (y0 > H - 1)), clamped=count(z < 0), total=z.numel(),
                inside=count((ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)))


def check_warp_case(kind, depth, ix, iy, z, H, W):
    """The precondition and the classes a case of ``kind`` holds by construction, asserted from the float64 reference's positions."""
    assert float(z.abs().min()) > MIN_ABS_Z, (kind, float(z.abs().min()))       # no pixel near the clamp or the 1e-8 threshold
    assert bool(torch.isfinite(ix).all()) and bool(torch.isfinite(iy).all())
    n = warp_classes(ix, iy, z, H, W)
    if kind == "behind":
        assert n["clamped"] == n["total"], n
    else:
        assert n["clamped"] == 0, n
    if kind == "sideways":
        assert n["outside"] > 0 and n["inside"] > 0, n
    if kind == "forward":
        assert n["inside"] == n["total"], n
    if kind == "shift":
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        for b in range(ix.shape[0]):
            if W > 1:
                assert float((ix[b] - (xs + SHIFTS[b][0])).abs().max()) < 1e-5
            if H > 1:
                assert float((iy[b] - (ys + SHIFTS[b][1])).abs().max()) < 1e-5
    if kind == "borders":
        assert (W == 1 or (n["west"] > 0 and n["east"] > 0)) and (H == 1 or (n["north"] > 0 and n["south"] > 0)), n
    if kind in ("sideways", "forward", "behind"):
        for v in special_depths():
            assert bool((depth == v).any()), (kind, float(v))
    return n
