"""Plain references for the small frame-path kernels (a helper module like accuracy.py and splat_reference.py: no fixtures, no test
module imports another).  Each op is stated ONCE with torch ops on the CPU and parameterised by ``dtype``: the float32 call is
``ref32``, the float64 call is ``ref64`` (``accuracy.as_accurate_as_reference``), and gradients come from autograd through the very
same functions.  The contracts are those of include/dvmvs_hip.h:

* ``bias_act``      dvmvs_bias_act_fwd / _inplace  (csrc/frame_ops.hip)
* ``upsample2x``    dvmvs_upsample2x_fwd / _pair_fwd, and through autograd dvmvs_upsample2x_bwd  (csrc/train_ops.hip)
* ``depthwise``     dvmvs_depthwise_conv_fwd, and through autograd dvmvs_depthwise_conv_bwd
* ``partial_sums``  dvmvs_partial_sums_bias_act_fwd  (csrc/bottleneck_conv.hip)

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
