"""Plain references for the small frame-path kernels (a helper module like accuracy.py and splat_reference.py: no fixtures, no test
module imports another).  Each op is stated ONCE with torch ops on the CPU and parameterised by ``dtype``: the float32 call is
``ref32``, the float64 call is ``ref64`` (``accuracy.as_accurate_as_reference``), and gradients come from autograd through the very
same functions.  The contracts are those of include/dvmvs_hip.h:

* ``bias_act``      dvmvs_bias_act_fwd / _inplace  (csrc/frame_ops.hip)
* ``upsample2x``    dvmvs_upsample2x_fwd / _pair_fwd, and through autograd dvmvs_upsample2x_bwd  (csrc/train_ops.hip)
* ``depthwise``     dvmvs_depthwise_conv_fwd, and through autograd dvmvs_depthwise_conv_bwd
* ``partial_sums``  dvmvs_partial_sums_bias_act_fwd  (csrc/bottleneck_conv.hip)
* ``lstm_gates``    dvmvs_lstm_gates_fwd  (csrc/lstm_gates.hip)
* ``lstm_gates_partials``  dvmvs_lstm_gates_partials_fwd
* ``hidden_warp``   dvmvs_hidden_warp_fwd  (csrc/hidden_warp.hip)

Inputs are float32 tensors (what the kernels are given); ``dtype`` only chooses the arithmetic.  tests/test_frame_reference.py pins
this module on the CPU.
"""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SIGMOID_TO_DEPTH = 0, 1, 2, 3
RES_NONE, RES_SAME, RES_NEAREST_UP2 = 0, 1, 2


def _as(t, dtype):
    return None if t is None else t.to(dtype)


def _per_channel(v, dtype):
    return v.to(dtype).view(1, -1, 1, 1)


def _f32(p):
    """The kernels take p0 / p1 as C floats: the algebra in any precision starts from those rounded parameters."""
    return float(torch.tensor(float(p), dtype=torch.float32))


def activate(v, activation, p0=0.0, p1=0.0):
    """0 none, 1 ReLU, 2 sigmoid, 3 sigmoid then the decoder's depth mapping 1 / (p0 * s + p1): multiply, add, reciprocal."""
    if activation == ACT_NONE:
        return v
    if activation == ACT_RELU:
        return torch.relu(v)
    if activation == ACT_SIGMOID:
        return torch.sigmoid(v)
    if activation == ACT_SIGMOID_TO_DEPTH:
        return 1.0 / (_f32(p0) * torch.sigmoid(v) + _f32(p1))
    raise ValueError(f"activation {activation}")


def bias_act(x, bias=None, activation=ACT_NONE, residual=None, residual_mode=RES_NONE, p0=0.0, p1=0.0, dtype=torch.float32):
    """act(x + bias[c]) (+ residual AFTER the activation); residual_mode 1: same shape, 2: [B,C,H/2,W/2] nearest-up-sampled."""
    v = x.to(dtype)
    if bias is not None:
        v = v + _per_channel(bias, dtype)
    v = activate(v, activation, p0, p1)
    if residual_mode == RES_SAME:
        v = v + residual.to(dtype)
    elif residual_mode == RES_NEAREST_UP2:
        v = v + F.interpolate(residual.to(dtype), scale_factor=2, mode="nearest")
    elif residual_mode != RES_NONE:
        raise ValueError(f"residual_mode {residual_mode}")
    return v


def upsample2x(x, pre_bias=None, pre_activation=ACT_NONE, dtype=torch.float32):
    """F.interpolate(act(x + pre_bias[c]), scale_factor=2, mode="bilinear", align_corners=True).  ``pre_bias`` belongs to the
    pre-activation (1 ReLU, 2 sigmoid): without one the input is up-sampled as it is, whatever ``pre_bias`` holds."""
    if pre_activation not in (ACT_NONE, ACT_RELU, ACT_SIGMOID):
        raise ValueError(f"pre_activation {pre_activation}")
    v = x.to(dtype)
    if pre_activation != ACT_NONE:
        if pre_bias is not None:
            v = v + _per_channel(pre_bias, dtype)
        v = activate(v, pre_activation)
    return F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=True)


def depthwise(x, w, bias=None, stride=1, activation=ACT_NONE, pre_bias=None, pre_relu=False, dtype=torch.float32):
    """Depthwise k x k convolution (w [C,1,k,k], padding k // 2) + bias + activation (0..2).  With ``pre_relu`` the taps are
    relu(x + pre_bias[c]); the zero padding stays zero (it pads the ACTIVATED map); without it ``pre_bias`` has no effect."""
    if activation not in (ACT_NONE, ACT_RELU, ACT_SIGMOID):
        raise ValueError(f"activation {activation}")
    v = x.to(dtype)
    if pre_relu:
        if pre_bias is not None:
            v = v + _per_channel(pre_bias, dtype)
        v = torch.relu(v)
    k = w.shape[-1]
    y = F.conv2d(v, w.to(dtype), _as(bias, dtype), stride=stride, padding=k // 2, groups=x.shape[1])
    return activate(y, activation)


def partial_sums(parts, bias=None, activation=ACT_NONE, dtype=torch.float32):
    """act(parts[0] + parts[1] + ... + bias[c]): ``parts`` [S,B,C,H,W] added in ASCENDING order, then the bias, then none | ReLU."""
    if activation not in (ACT_NONE, ACT_RELU):
        raise ValueError(f"activation {activation}")
    v = parts[0].to(dtype)
    for s in range(1, parts.shape[0]):
        v = v + parts[s].to(dtype)
    if bias is not None:
        v = v + _per_channel(bias, dtype)
    return activate(v, activation)


def gradients(fn, inputs, grad_out, dtype=torch.float32):
    """Autograd through ``fn(*leaves, dtype=dtype)``: the gradients w.r.t. ``inputs`` (float32 tensors) for the upstream ``grad_out``."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in inputs]
    y = fn(*leaves, dtype=dtype)
    return torch.autograd.grad(y, leaves, grad_out.to(dtype))


# ----------------------------------------------------------------------------------------------------------------------
# the recurrent chain: ConvLSTM gates (whole and from partial sums) and the hidden-state warp
# ----------------------------------------------------------------------------------------------------------------------
LAYER_NORM_EPS = 1e-5         # torch.nn.LayerNorm's default
HOMOGENEOUS_EPS = 1e-8        # kornia.convert_points_from_homogeneous' default
INVALID_DEPTH = 0.01          # the cell zeroes the warped state where the depth estimate is <= 0.01 (as a float32 number)


def _layer_norm_hw(x):
    """LayerNorm over [H,W] per (batch, channel): biased variance, eps 1e-5, no affine."""
    mean = x.mean(dim=(-2, -1), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(-2, -1), keepdim=True)
    return (x - mean) / torch.sqrt(var + LAYER_NORM_EPS)


def _celu(x):
    """CELU with alpha 1: x above 0, expm1(x) below."""
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))


def lstm_gates(cc, c, dtype=torch.float32):
    """(h', c') of the cell from its convolution output ``cc`` [B,4*hid,H,W] (split order i, f, o, g) and the cell state ``c``:
    g = celu(LN(cc_g)), c' = LN(sigmoid(cc_f) * c + sigmoid(cc_i) * g), h' = sigmoid(cc_o) * celu(c')."""
    cc, c = cc.to(dtype), c.to(dtype)
    cc_i, cc_f, cc_o, cc_g = torch.split(cc, c.shape[1], dim=1)
    i, f, o = torch.sigmoid(cc_i), torch.sigmoid(cc_f), torch.sigmoid(cc_o)
    g = _celu(_layer_norm_hw(cc_g))
    c_next = _layer_norm_hw(f * c + i * g)
    return o * _celu(c_next), c_next


def lstm_gates_partials(parts, c, dtype=torch.float32):
    """``lstm_gates`` on a convolution output that arrives as partial sums ``parts`` [S,B,4*hid,H,W], added in ASCENDING order in
    ``dtype``: in float32 that is the kernel's stated contract (a fixed order of IEEE additions), in float64 it is the exact sum."""
    total = parts[0].to(dtype)
    for s in range(1, parts.shape[0]):
        total = total + parts[s].to(dtype)
    return lstm_gates(total, c, dtype)


def _dehomogenise(p):
    """kornia.convert_points_from_homogeneous: divide by the last coordinate where |it| > 1e-8, else by 1."""
    z = p[..., -1:]
    return torch.where(z.abs() > HOMOGENEOUS_EPS, 1.0 / z, torch.ones_like(z)) * p[..., :-1]


def warp_grid(depth, T, K, dtype=torch.float32):
    """The geometry of the hidden-state warp for destination depth [B,1,H,W], source-from-destination transform [B,4,4] and intrinsics
    [B,3,3]: un-project every destination pixel with its depth, move it into the source camera, clamp z at 0 (relu), project (kornia's
    de-homogenisation: 1 / z only where |z| > 1e-8) and normalise by 2 / max(size - 1, 1e-8).  Returns the normalised grid [B,H,W,2]
    that grid_sample takes and the source-camera z BEFORE the clamp [B,H,W]."""
    B, _, H, W = depth.shape
    depth, T, K = depth.to(dtype), T.to(dtype), K.to(dtype)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    fx, fy, cx, cy = (K[:, r, c].view(B, 1, 1) for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)))
    x, y = (xs.unsqueeze(0) - cx) / fx, (ys.unsqueeze(0) - cy) / fy
    pts = torch.stack([x, y, torch.ones_like(x)], dim=-1) * depth.permute(0, 2, 3, 1)                 # [B,H,W,3]
    moved = _dehomogenise(torch.einsum("bij,bhwj->bhwi", T, torch.cat([pts, torch.ones_like(pts[..., :1])], dim=-1)))
    xy = _dehomogenise(torch.cat([moved[..., :2], torch.relu(moved[..., 2:3])], dim=-1))
    u, v = xy[..., 0] * fx + cx, xy[..., 1] * fy + cy
    grid = torch.stack([u * (2.0 / max(W - 1, HOMOGENEOUS_EPS)) - 1, v * (2.0 / max(H - 1, HOMOGENEOUS_EPS)) - 1], dim=-1)
    return grid, moved[..., 2]


def grid_pixels(g, size):
    """grid_sample's [-1, 1] -> pixel map with align_corners=True."""
    return ((g + 1.0) / 2.0) * (size - 1)


def _bilinear_zeros(src, ix, iy):
    """Bilinear gather of src [B,C,H,W] at pixel positions ix, iy [B,H',W']; a tap outside [0,W-1] x [0,H-1] contributes nothing."""
    B, C, H, W = src.shape
    shape = ix.shape[1:]
    ix, iy = ix.reshape(B, -1), iy.reshape(B, -1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    flat = src.reshape(B, C, H * W)
    out = torch.zeros(B, C, ix.shape[1], dtype=src.dtype)
    for xs, ys, w in ((x0, y0, (x1 - ix) * (y1 - iy)), (x1, y0, (ix - x0) * (y1 - iy)), (x0, y1, (x1 - ix) * (iy - y0)), (x1, y1, (ix - x0) * (iy - y0))):
        inside = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1) & torch.isfinite(ix) & torch.isfinite(iy)
        lin = (torch.where(inside, ys, torch.zeros_like(ys)).long() * W + torch.where(inside, xs, torch.zeros_like(xs)).long())
        out = out + torch.gather(flat, 2, lin.unsqueeze(1).expand(B, C, -1)) * torch.where(inside, w, torch.zeros_like(w)).unsqueeze(1)
    return out.reshape(B, C, *shape)


def hidden_warp(src, depth, T, K, zero_invalid=False, dtype=torch.float32):
    """``src`` [B,C,H,W] sampled bilinearly (zero padding, align_corners=True) at ``warp_grid(depth, T, K)``; with ``zero_invalid`` the
    result is 0 where depth <= 0.01 (the float32 comparison of the float32 input, whatever ``dtype``).  Returns
    ``(out, ix, iy, z)``: the warped map in ``dtype`` and, always in float64, the sample positions in pixels and the source-camera z
    before the clamp ([B,H,W] each), by which a test classifies pixels."""
    B, C, H, W = src.shape
    grid, z = warp_grid(depth, T, K, dtype)
    out = _bilinear_zeros(src.to(dtype), grid_pixels(grid[..., 0], W), grid_pixels(grid[..., 1], H))
    if zero_invalid:
        out = torch.where(depth <= torch.tensor(INVALID_DEPTH, dtype=torch.float32), torch.zeros((), dtype=dtype), out)
    if dtype != torch.float64:
        grid, z = warp_grid(depth, T, K, torch.float64)
    return out, grid_pixels(grid[..., 0], W), grid_pixels(grid[..., 1], H), z
