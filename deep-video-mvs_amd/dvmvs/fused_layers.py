"""Layer rewriting for inference: eval-mode BatchNorm folded into its convolution, then convolution + bias + activation as ``FusedConv2d`` -- the
layer that takes the MFMA kernels of csrc/direct_conv.hip, csrc/bottleneck_conv.hip and csrc/pointwise_conv.hip where they take the problem and
MIOpen + one epilogue launch where they do not.  ``nn.Module``-level code with no notion of a frame: ``dvmvs.engine.DepthEngine`` and
``dvmvs.module_surface.accelerate`` both build on it."""
import copy

import torch
from torch import nn

from dvmvs.hip import ops as _ops


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm folding
# ----------------------------------------------------------------------------------------------------------------------
def _fold_pair(conv, bn):
    w = conv.weight
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    folded = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, stride=conv.stride, padding=conv.padding,
                       dilation=conv.dilation, groups=conv.groups, bias=True).to(w.device)
    with torch.no_grad():
        folded.weight.copy_(w * scale.reshape(-1, 1, 1, 1))
        bias = conv.bias if conv.bias is not None else torch.zeros_like(bn.running_mean)
        folded.bias.copy_((bias - bn.running_mean) * scale + bn.bias)
    return folded


def fold_batchnorm(module):
    """Returns a deep copy of ``module`` (eval mode) in which every Conv2d directly followed by a BatchNorm2d inside
    an ``nn.Sequential`` is replaced by one biased convolution."""
    module = copy.deepcopy(module).eval()
    for parent in module.modules():
        if not isinstance(parent, nn.Sequential):
            continue
        names = list(parent._modules.keys())
        for a, b in zip(names, names[1:]):
            conv, bn = parent._modules[a], parent._modules[b]
            if isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d):
                parent._modules[a] = _fold_pair(conv, bn)
                parent._modules[b] = nn.Identity()
    return module


# ----------------------------------------------------------------------------------------------------------------------
# epilogue fusion: conv (MIOpen, no bias) + one in-place HIP kernel for bias and activation
# ----------------------------------------------------------------------------------------------------------------------
def _graph_microseconds(fn, reps=10, rounds=3):
    """GPU time of one ``fn()``: ``reps`` of them captured into a hipGraph, best of ``rounds`` replays (HIP events)."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(rounds):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        graph.replay()
        end.record()
        torch.cuda.synchronize()
        best = min(best, start.elapsed_time(end) * 1e3 / reps)
    return best


_PLAN_TIMINGS = {}     # (device, input shape, weight shape, stride, padding, activation) -> FusedConv2d._time_plan's tuple


class _ShapeOn:
    """A (shape, device) pair where code written for a tensor only asks for those two."""

    def __init__(self, shape, device):
        self.shape, self.device = shape, device


class FusedConv2d(nn.Module):
    """Convolution whose bias add and activation run as ONE HIP kernel (dvmvs_bias_act_fwd) instead of two ATen launches
    after the MIOpen convolution.  Same arithmetic (add, then max / sigmoid), so results are identical.  Three launch savers:
    * ``out=``: the epilogue writes into a caller-supplied channel slice of a concatenation buffer (no torch.cat copy later);
    * ``defer_epilogue``: a ReLU convolution directly followed by a depthwise one hands over its RAW output, and the depthwise
      kernel applies bias + ReLU to its input taps on the fly (``pre_bias``): one launch per MnasNet block less;
    * depthwise layers are a single HIP launch (convolution + bias + activation)."""

    def __init__(self, conv, activation):
        super().__init__()
        self.weight = conv.weight
        self.bias = conv.bias if conv.bias is not None else None
        self.stride, self.padding, self.dilation, self.groups = conv.stride, conv.padding, conv.dilation, conv.groups
        self.activation = _ops.ACTIVATIONS[activation]
        self.register_buffer("_no_bias", torch.empty(0, device=conv.weight.device), persistent=False)
        self.defer_epilogue = False      # set by fuse_epilogues: the next (depthwise) layer applies this layer's bias + ReLU
        self.pre_bias = None             # set by fuse_epilogues on that depthwise layer: the deferred bias
        # Epilogue inside MIOpen's kernel (dvmvs_conv_bias_act_fwd): decided per input shape the first time the shape is seen outside a
        # stream capture -- taken only when its output is BIT-IDENTICAL to convolution + epilogue (the Winograd case) and it is faster;
        # {input shape: (use the plan, plan us, two-launch us, max |difference|)}
        self.plan_epilogue = False       # set by DepthEngine(conv_plans=True)
        self.plans = {}
        # 3x3 layers on the bottleneck maps (8x10, 16x20): the deterministic weight-streaming MFMA kernel instead of MIOpen's
        # atomically accumulated split-K kernels (csrc/bottleneck_conv.hip); {input shape: (splits, partial-sum buffer) or None}
        self.bottleneck = False          # set by DepthEngine(bottleneck_convs=True)
        self._bottleneck_packed = None
        self._bottleneck_buffers = {}
        # dense 3x3 / 5x5 layers on the larger maps and the one-channel depth heads: the direct MFMA convolution with bias + ReLU in
        # its store path instead of MIOpen's Winograd / GEMM kernel + epilogue launch (csrc/direct_conv.hip);
        # {input shape: output-channel tiles per wave the problem needs (0: not taken)}, {tiles: packed weights}
        self.direct_conv = False         # set by DepthEngine(direct_convs=True)
        self._direct_tiles = {}
        self._direct_packed = {}
        # 1x1 layers (MnasNet expansion / projection layers, FPN lateral layers): the MFMA GEMM with bias + ReLU + residual in its store path
        # instead of the library GEMM + epilogue launch (csrc/pointwise_conv.hip); {(input shape, activation, residual mode): taken}
        self.pointwise_conv = False      # set by DepthEngine(pointwise_convs=True)
        self._pointwise_taken = {}
        self._pointwise_packed = None

        k = conv.kernel_size
        self.depthwise = (conv.groups == conv.in_channels == conv.out_channels and conv.groups > 1 and k[0] == k[1] and k[0] in (3, 5)
                          and tuple(conv.padding) == (k[0] // 2, k[0] // 2) and tuple(conv.dilation) == (1, 1)
                          and conv.stride[0] == conv.stride[1] and conv.stride[0] in (1, 2))

    def forward(self, x, residual=None, residual_mode=0, out=None, activation=None, p0=0.0, p1=0.0, raw=False, out_nhwc=None):
        """``residual`` (mode 1: same shape, mode 2: half resolution, nearest-up-sampled) is added in the same epilogue; ``out``
        is the destination (default: the convolution's own output buffer); ``activation`` overrides the layer's; ``raw`` returns
        the convolution output without the epilogue (the consumer applies it: up-sampler, depthwise kernel).  ``out_nhwc``: a second
        destination that receives the same values channels-last -- in the direct kernel's own epilogue, else by one transposing launch."""
        if out_nhwc is not None:
            y = self._forward(x, residual, residual_mode, out, activation, p0, p1, raw, out_nhwc)
            if y is not None:
                return y
            y = self._forward(x, residual, residual_mode, out, activation, p0, p1, raw, None)
            _ops.nchw_to_nhwc_into(y, out_nhwc)
            return y
        return self._forward(x, residual, residual_mode, out, activation, p0, p1, raw, None)

    def _forward(self, x, residual, residual_mode, out, activation, p0, p1, raw, out_nhwc):
        """``forward``; with ``out_nhwc``: the layer through the dual-destination direct kernel, or None when it does not take the problem."""
        if out_nhwc is not None:
            if self.direct_conv and residual is None and x.is_contiguous() and not (raw or self.defer_epilogue):
                act = self.activation if activation is None else activation
                return self._direct_forward(x, out, act, p0, p1, False, out_nhwc)
            return None
        act = self.activation if activation is None else activation
        if (self.defer_epilogue or raw) and (out is not None or residual is not None or (activation is not None and not raw)):
            raise RuntimeError("this layer hands over its RAW convolution output (its consumer applies bias + activation): "
                               "out=, residual= and an activation override would be silently ignored")
        if self.depthwise and residual is None and out is None:
            pre = self.pre_bias
            return _ops.depthwise_conv(x, self.weight, self.bias if self.bias is not None else self._no_bias, self.stride[0], act,
                                       pre if pre is not None else self._no_bias, pre is not None)
        if self.pre_bias is not None:
            raise RuntimeError("a depthwise layer with a deferred input epilogue must take the depthwise kernel")
        if self.bottleneck and residual is None and not raw and not self.defer_epilogue and x.is_contiguous() and \
                act in (_ops.ACTIVATIONS["none"], _ops.ACTIVATIONS["relu"]):
            buffers = self._bottleneck_for(x)
            if buffers is not None:
                B, _, H, W = x.shape
                shape = (B, self.weight.shape[0], H // self.stride[0], W // self.stride[0])
                splits = _ops.bottleneck_conv_into(x, self._bottleneck_packed, shape[1], self.stride[0], buffers)
                dst = out if out is not None else torch.empty(shape, device=x.device, dtype=torch.float32)
                return _ops.partial_sums_bias_act_into(buffers, splits, dst, self.bias, act, shape)
        if self.direct_conv and residual is None and x.is_contiguous():
            y = self._direct_forward(x, out, act, p0, p1, raw or self.defer_epilogue)
            if y is not None:
                return y
        if self.pointwise_conv and x.is_contiguous() and (residual is None or residual.is_contiguous()):
            y = self._pointwise_forward(x, out, act, residual, residual_mode if residual is not None else 0, raw or self.defer_epilogue)
            if y is not None:
                return y
        if (self.plan_epilogue and residual is None and not raw and not self.defer_epilogue and self._plan_eligible(act)
                and x.is_contiguous()):
            key = tuple(x.shape)
            plan = self.plans.get(key)
            if plan is None and not torch.cuda.is_current_stream_capturing():
                # one timing per problem and process: engines built later (and this engine's other layers of the same shape) reuse it
                problem = (x.device.index, key, tuple(self.weight.shape), self.stride[0], self.padding[0], act)
                if problem not in _PLAN_TIMINGS:
                    _PLAN_TIMINGS[problem] = self._time_plan(x, act)
                plan = self.plans[key] = _PLAN_TIMINGS[problem]
            if plan is not None and plan[0]:
                y = _ops.conv_bias_act_into(x, self.weight, self.bias, out, self.stride[0], self.padding[0], act)
                if y is not None:
                    return y
        y = nn.functional.conv2d(x, self.weight, None, self.stride, self.padding, self.dilation, self.groups)
        if not y.is_contiguous():
            y = y.contiguous()
        if self.defer_epilogue or raw:
            return y
        return _ops.bias_act_into(y, y if out is None else out, self.bias, act, residual, residual_mode if residual is not None else 0, p0, p1)

    def _direct_forward(self, x, out, act, p0, p1, raw, out_nhwc=None):
        """The layer through csrc/direct_conv.hip, or None when that kernel does not take the problem (then MIOpen as before).  ``raw``:
        the convolution output without bias and activation (the consumer applies them)."""
        k = self.weight.shape
        if self.depthwise or self.groups != 1 or k[2] != k[3] or tuple(self.dilation) != (1, 1) or self.stride[0] != self.stride[1] or \
                tuple(self.padding) != (k[2] // 2, k[2] // 2):
            return None
        B, _, H, W = x.shape
        if x.data_ptr() % 16 != 0 or (out is not None and out.data_ptr() % 4 != 0):
            return None      # (the kernel stages aligned float4 rows; torch's own allocations always are)
        stride = self.stride[0]
        bias = None if raw or self.bias is None else self.bias
        if raw:
            act = _ops.ACTIVATIONS["none"]
        if k[0] == 1 and k[2] == 3 and stride == 1:      # depth head
            if out_nhwc is not None:
                return None
            dst = out if out is not None else torch.empty((B, 1, H, W), device=x.device, dtype=torch.float32)
            return _ops.conv_head_into(x, self.weight, bias, dst, act, p0, p1)
        if act not in (_ops.ACTIVATIONS["none"], _ops.ACTIVATIONS["relu"]):
            return None
        key = tuple(x.shape)
        tile = self._direct_tiles.get(key)
        if tile is None:
            tile = self._direct_tiles[key] = _ops.direct_conv_tile(B, k[1], H, W, k[0], k[2], stride)
        if tile == 0:
            return None
        packed = self._direct_packed.get(tile)
        if packed is None:
            if torch.cuda.is_current_stream_capturing():
                return None      # (packed at the next eager call: the first frame of every kind runs eagerly)
            packed = self._direct_packed[tile] = _ops.direct_conv_pack(self.weight.detach(), tile)
        dst = out if out is not None else torch.empty((B, k[0], H // stride, W // stride), device=x.device, dtype=torch.float32)
        return _ops.direct_conv_into(x, packed, tile, bias, dst, k[0], k[2], stride, act, dst_nhwc=out_nhwc)

    def forward_upsampled(self, x, out=None):
        """``self(upsample2x(x), out=out)`` -- the decoder's up-convolutions.  Where the bottleneck kernel takes the layer on the up-sampled map it
        interpolates while it stages its input (one launch less; the same bits: csrc/bottleneck_conv.hip, UP2X); else the two launches."""
        if self.bottleneck and not self.defer_epilogue and x.is_contiguous() and tuple(x.shape[2:]) == (8, 10) and self.stride[0] == 1 \
                and self.activation in (_ops.ACTIVATIONS["none"], _ops.ACTIVATIONS["relu"]):
            B, C = x.shape[0], x.shape[1]
            buffers = self._bottleneck_for(x, shape=(B, C, 16, 20))
            if buffers is not None:
                shape = (B, self.weight.shape[0], 16, 20)
                splits = _ops.bottleneck_conv_into(x, self._bottleneck_packed, shape[1], 1, buffers, upsample=True)
                dst = out if out is not None else torch.empty(shape, device=x.device, dtype=torch.float32)
                return _ops.partial_sums_bias_act_into(buffers, splits, dst, self.bias, self.activation, shape)
        return self(_ops.upsample2x(x), out=out)

    def _pointwise_forward(self, x, out, act, residual, residual_mode, raw):
        """The layer through csrc/pointwise_conv.hip, or None when that kernel does not take the problem (then the library GEMM + epilogue launch
        as before).  ``raw``: the convolution output without bias and activation (the depthwise consumer applies them)."""
        k = self.weight.shape
        if k[2] != 1 or k[3] != 1 or self.groups != 1 or tuple(self.stride) != (1, 1) or tuple(self.padding) != (0, 0):
            return None
        if raw:
            act = _ops.ACTIVATIONS["none"]
        key = (tuple(x.shape), act, residual_mode)
        taken = self._pointwise_taken.get(key)
        if taken is None:
            B, _, H, W = x.shape
            taken = self._pointwise_taken[key] = _ops.pointwise_conv_supported(B, k[1], H, W, k[0], act, residual_mode)
        if not taken or x.data_ptr() % 16 != 0 or (out is not None and out.data_ptr() % 16 != 0):
            return None
        if self._pointwise_packed is None:
            if torch.cuda.is_current_stream_capturing():
                return None      # (packed at the next eager call: the first frame of every kind runs eagerly)
            self._pointwise_packed = _ops.pointwise_conv_pack(self.weight.detach())
        B, _, H, W = x.shape
        dst = out if out is not None else torch.empty((B, k[0], H, W), device=x.device, dtype=torch.float32)
        return _ops.pointwise_conv_into(x, self._pointwise_packed, None if raw else self.bias, dst, k[0], act, residual, residual_mode)

    def _bottleneck_for(self, x, shape=None):
        """The partial-sum buffer for this input shape if the bottleneck kernel takes the problem (else None); packs the weights the
        first time (outside a stream capture: the first frame of every kind runs eagerly).  ``shape``: the shape of the map the layer convolves
        when that is not ``x`` itself (``forward_upsampled``)."""
        key = tuple(x.shape) if shape is None else tuple(shape)
        if shape is not None:
            x = _ShapeOn(key, x.device)
        if key not in self._bottleneck_buffers:
            k = self.weight.shape
            ok = (not self.depthwise and self.groups == 1 and k[2] == 3 and k[3] == 3 and tuple(self.padding) == (1, 1) and
                  tuple(self.dilation) == (1, 1) and self.stride[0] == self.stride[1])
            splits = _ops.bottleneck_conv_splits(x.shape[0], k[0], k[1], x.shape[2], x.shape[3], self.stride[0]) if ok else 0
            if splits == 0:
                self._bottleneck_buffers[key] = None
            elif torch.cuda.is_current_stream_capturing():
                return None      # (not cached: decided at the next eager call)
            else:
                if self._bottleneck_packed is None:
                    self._bottleneck_packed = _ops.bottleneck_conv_pack(self.weight.detach())
                P = (x.shape[2] // self.stride[0]) * (x.shape[3] // self.stride[0])
                self._bottleneck_buffers[key] = torch.empty(splits * x.shape[0] * k[0] * P, device=x.device, dtype=torch.float32)
        return self._bottleneck_buffers[key]

    def repack(self):
        """Re-packs this layer's packed weight copies from ``weight`` (after new parameters were loaded) IN PLACE: captured graphs that read them
        stay valid.  Copies that were never made are made at first use, as ever."""
        if self._bottleneck_packed is not None:
            self._bottleneck_packed.copy_(_ops.bottleneck_conv_pack(self.weight.detach()))
        for tile, packed in self._direct_packed.items():
            packed.copy_(_ops.direct_conv_pack(self.weight.detach(), tile))
        if self._pointwise_packed is not None:
            self._pointwise_packed.copy_(_ops.pointwise_conv_pack(self.weight.detach()))

    def _plan_eligible(self, act):
        k = self.weight.shape
        return (not self.depthwise and self.groups == 1 and self.bias is not None and k[2] == k[3] and self.stride[0] == self.stride[1]
                and self.padding[0] == self.padding[1] and tuple(self.dilation) == (1, 1)
                and act in (_ops.ACTIVATIONS["none"], _ops.ACTIVATIONS["relu"]))


    def _time_plan(self, x, act):
        """(use the MIOpen fusion plan for this input shape?, plan us, convolution + epilogue us, max |difference|).
        The plan is used only when its result is bit-identical to the two-launch form on this input AND faster: which of two
        differently-rounded fp32 results a layer produces must not depend on a timing (the timing then only decides
        between two ways of computing the same bits)."""
        with torch.no_grad():
            probe = _ops.conv_bias_act_into(x, self.weight, self.bias, None, self.stride[0], self.padding[0], act)
            if probe is None:
                return (False, float("nan"), float("nan"), float("nan"))

            def two_launches():
                y = nn.functional.conv2d(x, self.weight, None, self.stride, self.padding, self.dilation, self.groups)
                return _ops.bias_act_into(y, y, self.bias, act)

            difference = float((two_launches() - probe).abs().max())
            t_two = _graph_microseconds(two_launches)
            t_plan = _graph_microseconds(lambda: _ops.conv_bias_act_into(x, self.weight, self.bias, probe, self.stride[0], self.padding[0], act))
        return (difference == 0.0 and t_plan < t_two, t_plan, t_two, difference)


def fuse_epilogues(module):
    """In place on an eval-mode (BN-folded) copy: Conv2d [+ Identity] + ReLU / Sigmoid, and bare biased Conv2d, become
    FusedConv2d.  Convolutions without bias and without activation are left alone."""
    for parent in module.modules():
        names = list(parent._modules.keys())
        if isinstance(parent, nn.Sequential):
            i = 0
            while i < len(names):
                m = parent._modules[names[i]]
                if isinstance(m, nn.Conv2d):
                    j = i + 1
                    while j < len(names) and isinstance(parent._modules[names[j]], nn.Identity):
                        j += 1
                    nxt = parent._modules[names[j]] if j < len(names) else None
                    if isinstance(nxt, nn.ReLU):
                        parent._modules[names[i]] = FusedConv2d(m, "relu")
                        parent._modules[names[j]] = nn.Identity()
                    elif isinstance(nxt, nn.Sigmoid):
                        parent._modules[names[i]] = FusedConv2d(m, "sigmoid")
                        parent._modules[names[j]] = nn.Identity()
                    elif m.bias is not None:
                        parent._modules[names[i]] = FusedConv2d(m, "none")
                i += 1
        else:
            for name in names:
                m = parent._modules[name]
                if isinstance(m, nn.Conv2d) and m.bias is not None:
                    parent._modules[name] = FusedConv2d(m, "none")
    # a ReLU convolution directly followed by a depthwise layer: its epilogue moves into the depthwise kernel's input read
    for parent in module.modules():
        if not isinstance(parent, nn.Sequential):
            continue
        fused = [m for m in parent._modules.values() if not isinstance(m, nn.Identity)]
        for first, second in zip(fused, fused[1:]):
            if isinstance(first, FusedConv2d) and isinstance(second, FusedConv2d) and second.depthwise and not first.depthwise and \
                    first.activation == _ops.ACTIVATIONS["relu"] and first.bias is not None and first.groups == 1:
                first.defer_epilogue = True
                second.pre_bias = first.bias
    # shortcut sums folded into the producing convolution's epilogue
    from dvmvs.backbone import FeaturePyramidNetwork, InvertedResidual
    for m in module.modules():
        if isinstance(m, InvertedResidual) and m.apply_residual and isinstance(m.layers[6], FusedConv2d):
            m.fused_head, m.fused_tail = nn.Sequential(*list(m.layers)[:6]), m.layers[6]
        if isinstance(m, FeaturePyramidNetwork) and all(isinstance(b, FusedConv2d) for b in m.inner_blocks):
            m.fused_top_down = True
    return module


# (environment variable, constructor argument of DepthEngine / accelerate = the engine's attribute, FusedConv2d attribute) of the kernel families that
# can be switched off ("0": MIOpen + epilogue launch instead); each needs the fused epilogues and contiguous maps
_KERNEL_SWITCHES = (
    ("DVMVS_CONV_PLANS", "conv_plans", "plan_epilogue"),      # epilogues inside MIOpen's Winograd kernels where that is measurably faster (FusedConv2d.plans)
    ("DVMVS_BOTTLENECK_CONVS", "bottleneck_convs", "bottleneck"),      # 3x3 layers on the 8x10 / 16x20 maps, ConvLSTM convolution: csrc/bottleneck_conv.hip
    ("DVMVS_DIRECT_CONVS", "direct_convs", "direct_conv"),      # dense 3x3 / 5x5 layers of the 1/8 ... full-resolution maps, depth heads: csrc/direct_conv.hip
    ("DVMVS_POINTWISE_CONVS", "pointwise_convs", "pointwise_conv"),      # 1x1 layers (feature extractor, FPN lateral layers): csrc/pointwise_conv.hip
)


def set_kernel_families(module, conv_plans=False, bottleneck_convs=False, direct_convs=False, pointwise_convs=False):
    """Switches the kernel families of ``_KERNEL_SWITCHES`` on or off on every FusedConv2d of ``module``."""
    wanted = dict(conv_plans=conv_plans, bottleneck_convs=bottleneck_convs, direct_convs=direct_convs, pointwise_convs=pointwise_convs)
    for sub in module.modules():
        if isinstance(sub, FusedConv2d):
            for _, argument, layer_attribute in _KERNEL_SWITCHES:
                setattr(sub, layer_attribute, bool(wanted[argument]))
