"""The three hand-written backward kernels of training -- gates (csrc/lstm_gates.hip), hidden-state warp (csrc/hidden_warp.hip) and
fused cost volume (csrc/cost_volume_bwd.hip) -- on every code path their launchers pick from the shape, against autograd through the
CPU oracle.

The arbiter is float64: the oracle is differentiated twice, in float32 and in float64, and the kernel's gradient may be at most three
times as far from the float64 one as the float32 oracle's is (``accuracy.as_accurate_as_reference``).  Paths without atomics (the
gate backward, the reference-feature gradient, the measurement-feature gather) must also repeat bit for bit; the warp backward and the
scatter of 1-pixel-high or -wide maps use float atomics and are checked against float64 only.

Paths, by shape:
* gate backward: one LayerNorm row per 16 lanes for H*W <= 64 (16 rows per workgroup), one wave per row with 2, 4, 8, 16 elements
  per lane up to 128, 256, 512, 1024 (4 rows per workgroup); larger planes are refused.
* warp backward: one thread per element up to 2048 x 256 elements, a grid-stride loop beyond.
* cost-volume backward: reference gradient in chunks of 8 channels; measurement gradient gathered 32 channels per pass with LDS
  sized by D, or scattered with atomics when H == 1 or W == 1.
"""
import types

import numpy as np
import pytest
import torch

import dvmvs_oracle as orc
import hipcall
import synthetic as syn
from accuracy import as_accurate_as_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_device):
    from dvmvs.hip import _capi
    _capi.lib()  # the HIP library must be there: no fallback
    return hip_device


@pytest.fixture(scope="module")
def ops(dev):
    from dvmvs.hip import ops as o
    return o


def _leaves(ts, dev=None, dtype=None, grad=True):
    return [t.detach().to(device=dev, dtype=dtype).clone().requires_grad_(grad) for t in ts]


# ----------------------------------------------------------------------------------------------------------------------
# gate backward (ops.lstm_gates under autograd)
# ----------------------------------------------------------------------------------------------------------------------
# H*W on both sides of every layout boundary: 1, 5, 15, 64 (training) | 65, 80, 128 | 129, 256 | 257, 512 | 513, 1024
GATE_MAPS = [(1, 1), (1, 5), (3, 5), (8, 8), (5, 13), (8, 10), (8, 16), (3, 43), (16, 16), (1, 257), (16, 32), (19, 27), (32, 32)]


def gate_inputs(B, hid, H, W, seed, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4 * hid, H, W, generator=g) * scale, torch.randn(B, hid, H, W, generator=g)


def both_outputs(wh, wc):
    return lambda h, c: (h * wh.to(h)).sum() + (c * wc.to(c)).sum()


def gate_grads(fn, cc, c, loss, dev=None, dtype=None):
    a, b = _leaves((cc, c), dev, dtype)
    h, cn = fn(a, b)
    loss(h, cn).backward()
    return a.grad, b.grad


def check_gate_backward(ops, dev, cc, c, loss):
    """Kernel gradients w.r.t. (cc, c) vs float32 / float64 oracle autograd; a second run must repeat them bit for bit."""
    got = gate_grads(ops.lstm_gates, cc, c, loss, dev)
    ref32 = gate_grads(orc.lstm_gates, cc, c, loss)
    ref64 = gate_grads(orc.lstm_gates, cc, c, loss, dtype=torch.float64)
    for name, x, r32, r64 in zip(("grad_cc", "grad_c"), got, ref32, ref64):
        assert torch.isfinite(x).all(), name
        as_accurate_as_reference(x, r32, r64)
    again = gate_grads(ops.lstm_gates, cc, c, loss, dev)
    assert all(torch.equal(x, y) for x, y in zip(got, again)), "gate backward is not bit-reproducible"
    return got, ref64


@pytest.mark.parametrize("H,W", GATE_MAPS)
def test_gate_backward_every_layout(ops, dev, H, W):
    """15 rows: a partial workgroup in every layout (16 rows per workgroup at H*W <= 64, 4 above)."""
    B, hid = 3, 5
    cc, c = gate_inputs(B, hid, H, W, seed=100 + H * W)
    g = torch.Generator().manual_seed(7 + H * W)
    check_gate_backward(ops, dev, cc, c, both_outputs(torch.randn(B, hid, H, W, generator=g), torch.randn(B, hid, H, W, generator=g)))


@pytest.mark.parametrize("B,hid,H,W", [(4, 512, 8, 8), (1, 64, 8, 10), (2, 33, 16, 16)])
def test_gate_backward_full_workgroups(ops, dev, B, hid, H, W):
    """(4, 512, 8, 8) is the training cell itself (256x256 input: 8x8 bottleneck maps, the 16-lane layout)."""
    cc, c = gate_inputs(B, hid, H, W, seed=B * hid + H)
    g = torch.Generator().manual_seed(11)
    check_gate_backward(ops, dev, cc, c, both_outputs(torch.randn(B, hid, H, W, generator=g), torch.randn(B, hid, H, W, generator=g)))


@pytest.mark.parametrize("H,W", [(8, 8), (8, 10), (19, 27)])
def test_gate_backward_upstream_gradient_forms(ops, dev, H, W):
    """Only h' used, only c' used (the other gradient arrives as None / zeros), a strided slice of h', a transposed (non-contiguous)
    gradient of h' and an expanded (stride-0) gradient of c'."""
    B, hid = 2, 6
    cc, c = gate_inputs(B, hid, H, W, seed=300 + H * W)
    g = torch.Generator().manual_seed(301)
    wh, wc = torch.randn(B, hid, H, W, generator=g), torch.randn(B, hid, H, W, generator=g)
    wt = torch.randn(B, hid, W, H, generator=g)
    row = torch.randn(1, 1, 1, W, generator=g)
    losses = {
        "h only": lambda h, cn: (h * wh.to(h)).sum(),
        "c only": lambda h, cn: (cn * wc.to(cn)).sum(),
        "h strided": lambda h, cn: h[..., ::2].sum(),
        "h transposed, c expanded": lambda h, cn: (h.transpose(-1, -2) * wt.to(h)).sum() + (cn * row.to(cn)).sum(),
    }
    for name, loss in losses.items():
        (gcc, _), _ = check_gate_backward(ops, dev, cc, c, loss)
        if name == "c only":     # h' is not used: its gate (o) gets no gradient at all
            assert float(gcc[:, 2 * hid:3 * hid].abs().max()) == 0.0
    # whichever form autograd hands over for the unused output, None and zeros give the same gradients, bit for bit
    ctx = types.SimpleNamespace(saved_tensors=(cc.to(dev), c.to(dev)))
    gh, gc = wh.to(dev), wc.to(dev)
    for none_form, zero_form in ((ops.frame._lstm_gates_backward(ctx, gh, None), ops.frame._lstm_gates_backward(ctx, gh, torch.zeros_like(gc))),
                                 (ops.frame._lstm_gates_backward(ctx, None, gc), ops.frame._lstm_gates_backward(ctx, torch.zeros_like(gh), gc))):
        assert all(torch.equal(x, y) for x, y in zip(none_form, zero_form))


@pytest.mark.parametrize("H,W", [(8, 8), (8, 10), (19, 27)])
def test_gate_backward_hard_values(ops, dev, H, W):
    """g-gate rows of offset 5 and sigma 1e-3 (the LayerNorm amplifies by 1000), and |cc| around 20: saturated sigmoids, and rows
    with one outlier that drive the normalised value deep into the CELU's negative tail."""
    B, hid = 2, 8
    g = torch.Generator().manual_seed(400 + H * W)
    wh, wc = torch.randn(B, hid, H, W, generator=g), torch.randn(B, hid, H, W, generator=g)
    cc, c = gate_inputs(B, hid, H, W, seed=401 + H * W)
    cc[:, 3 * hid:] = 5.0 + 1e-3 * torch.randn(B, hid, H, W, generator=g)
    check_gate_backward(ops, dev, cc, c, both_outputs(wh, wc))

    sat = 20.0 * torch.sign(torch.randn(B, 4 * hid, H, W, generator=g)) + 0.3 * torch.randn(B, 4 * hid, H, W, generator=g)
    sat[:, 3 * hid:3 * hid + 2] = 20.0 + 0.3 * torch.randn(B, 2, H, W, generator=g)
    sat[:, 3 * hid:3 * hid + 2, 0, 0] = -20.0                      # g-gate outlier: normalised to about -sqrt(H*W - 1)
    c_sat = 20.0 * torch.randn(B, hid, H, W, generator=g)
    c_sat[:, 0] = 20.0
    c_sat[:, 0, H // 2, W // 2] = -20.0                            # and one in the cell state that feeds LayerNorm(c')
    check_gate_backward(ops, dev, sat, c_sat, both_outputs(wh, wc))


@pytest.mark.parametrize("H,W", [(8, 8), (8, 10), (3, 43), (16, 16), (16, 32), (32, 32)])
@pytest.mark.parametrize("n_partials", [2, 3, 16])
def test_gate_partial_sums(ops, dev, H, W, n_partials):
    """``lstm_gates_partials_into`` (K-split convolution partial sums, added in ascending order inside the gate kernel; its own kernel
    at 65 .. 128 elements) equals ``lstm_gates_into`` on the ascending-order sum bit for bit, and the oracle."""
    B, hid = 2, 12
    g = torch.Generator().manual_seed(500 + H * W + n_partials)
    parts = torch.randn(n_partials, B, 4 * hid, H, W, generator=g) * (1.5 / n_partials ** 0.5)
    c = torch.randn(B, hid, H, W, generator=g)
    total = parts[0].clone()
    for k in range(1, n_partials):
        total = total + parts[k]                                   # fp32, ascending order (exact IEEE additions on either device)
    pd = parts.to(dev)
    c_part, h_part = c.to(dev).clone(), torch.full((B, hid, H, W), float("nan"), device=dev)
    ops.lstm_gates_partials_into(pd, n_partials, c_part, h_part)
    c_sum, h_sum = c.to(dev).clone(), torch.full((B, hid, H, W), float("nan"), device=dev)
    sd = pd[0].clone()
    for k in range(1, n_partials):
        sd = sd + pd[k]
    ops.lstm_gates_into(sd, c_sum, h_sum)
    assert torch.equal(sd.cpu(), total)
    assert torch.equal(h_part, h_sum) and torch.equal(c_part, c_sum)
    h32, c32 = orc.lstm_gates(total, c)
    h64, c64 = orc.lstm_gates(total.double(), c.double())
    as_accurate_as_reference(h_part, h32, h64)
    as_accurate_as_reference(c_part, c32, c64)


def test_gate_planes_above_1024_elements_are_refused(ops, dev):
    """33x32 = 1056 elements: no layout holds the row; every entry point raises from _capi.check and leaves its outputs alone."""
    B, hid, H, W = 1, 3, 33, 32
    cc = torch.randn(B, 4 * hid, H, W, device=dev)
    c = torch.randn(B, hid, H, W, device=dev)
    with pytest.raises(RuntimeError, match="dvmvs_lstm_gates_fwd"):
        ops.lstm_gates(cc, c)
    with pytest.raises(RuntimeError, match="dvmvs_lstm_gates_bwd"):
        ops.frame._lstm_gates_backward(types.SimpleNamespace(saved_tensors=(cc, c)), torch.ones_like(c), torch.ones_like(c))
    c_state, h_state = c.clone(), torch.zeros_like(c)
    with pytest.raises(RuntimeError, match="dvmvs_lstm_gates_fwd"):
        ops.lstm_gates_into(cc, c_state, h_state)
    with pytest.raises(RuntimeError, match="dvmvs_lstm_gates_partials_fwd"):
        ops.lstm_gates_partials_into(torch.stack([cc, cc]), 2, c_state, h_state)
    torch.cuda.synchronize()
    assert torch.equal(c_state, c) and float(h_state.abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# hidden-warp backward (ops.hidden_warp under autograd)
# ----------------------------------------------------------------------------------------------------------------------
WARP_KINDS = ["identity", "moderate", "outside", "behind", "special depths"]


def _rot_y(deg):
    t = np.deg2rad(deg)
    R = torch.eye(4, dtype=torch.float64)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(t), np.sin(t), -np.sin(t), np.cos(t)
    return R


def warp_geometry(kind, B, H, W, seed):
    """(depth [B,1,H,W], T [B,4,4], K [B,3,3]), float32, with a different T and K for every batch item."""
    g = torch.Generator().manual_seed(seed)
    depth = 0.5 + 2.5 * torch.rand(B, 1, H, W, generator=g)
    if kind == "special depths":
        flat = depth.view(-1)
        n = flat.numel()
        idx = torch.arange(n)
        flat[idx % 5 == 1] = 0.0
        flat[idx % 7 == 3] = -0.7
        flat[idx % 4 == 2] = 0.01
        if n == B:                                     # 1x1 maps: one of each over the batch
            flat[:] = torch.tensor([0.01, 0.0, -0.7, 1.3])[:n]
    Ts, Ks = [], []
    for b in range(B):
        K = syn.scaled_K(syn.full_K(), 32.0 * 10.0 / max(W, 2))[0].double()
        K[0, 0] *= 1.0 + 0.07 * b
        K[1, 2] += 0.3 * b
        T = torch.eye(4, dtype=torch.float64)
        if kind in ("moderate", "special depths"):
            T = _rot_y(4.0 * (b + 1))
            T[:3, 3] = torch.tensor([0.15 * (b + 1), 0.05, 0.1 - 0.05 * b], dtype=torch.float64)
        elif kind == "outside":                        # most samples leave the image
            T[:3, 3] = torch.tensor([3.0 * (b + 1), -2.0, 0.0], dtype=torch.float64)
        elif kind == "behind":                         # most points end up behind the source camera: Z clamped at 0
            T = _rot_y(150.0 + 10.0 * b)
            T[:3, 3] = torch.tensor([0.1, 0.0, 0.3], dtype=torch.float64)
        Ts.append(T)
        Ks.append(K)
    return depth, torch.stack(Ts).float(), torch.stack(Ks).float()


def warp_grad(fn, src, depth, T, K, zero_invalid, go, dev=None, dtype=None):
    s, = _leaves((src,), dev, dtype)
    d, t, k = (x.to(device=dev, dtype=dtype) for x in (depth, T, K))
    out = fn(s, d, t, k, zero_invalid)
    out.backward(go.to(device=dev, dtype=dtype))
    return out.detach(), s.grad


def hit_pixels_outside_support(got, ref):
    """(b, y, x) source pixels where ``got`` has a gradient in some channel while ``ref`` has none in any."""
    g, r = got.detach().cpu(), ref.detach().cpu()
    return int(((g != 0).any(dim=1) & ~(r != 0).any(dim=1)).sum())


def check_warp_backward(ops, dev, src, depth, T, K, zero_invalid, go):
    out, got = warp_grad(ops.hidden_warp, src, depth, T, K, zero_invalid, go, dev)
    out32, ref32 = warp_grad(orc.warp_hidden_state, src, depth, T, K, zero_invalid, go)
    out64, ref64 = warp_grad(orc.warp_hidden_state, src, depth, T, K, zero_invalid, go, dtype=torch.float64)
    as_accurate_as_reference(out, out32, out64)
    as_accurate_as_reference(got, ref32, ref64)
    # no tap lands (float64 gradient exactly 0) -> no gradient: up to the float32 oracle's own boundary roundings, plus two
    assert hit_pixels_outside_support(got, ref64) <= hit_pixels_outside_support(ref32, ref64) + 2
    return got, ref64


WARP_SHAPES = [(1, 7, 8, 8), (3, 7, 8, 10), (4, 1, 1, 10), (3, 7, 10, 1), (4, 3, 1, 1), (3, 512, 8, 8)]


@pytest.mark.parametrize("kind", WARP_KINDS)
@pytest.mark.parametrize("B,C,H,W", WARP_SHAPES)
def test_warp_backward(ops, dev, B, C, H, W, kind):
    depth, T, K = warp_geometry(kind, B, H, W, seed=600 + B * C + H * W)
    g = torch.Generator().manual_seed(601 + H * W)
    src = torch.randn(B, C, H, W, generator=g)
    go = torch.randn(B, C, H, W, generator=g)
    for zero_invalid in (False, True):
        check_warp_backward(ops, dev, src, depth, T, K, zero_invalid, go)


@pytest.mark.parametrize("kind", ["moderate", "behind"])
def test_warp_backward_grid_stride(ops, dev, kind):
    """4 x 512 x 16 x 20 = 655360 elements: more than the 2048 x 256 threads launched, so the grid-stride loop runs."""
    B, C, H, W = 4, 512, 16, 20
    depth, T, K = warp_geometry(kind, B, H, W, seed=700)
    g = torch.Generator().manual_seed(701)
    check_warp_backward(ops, dev, torch.randn(B, C, H, W, generator=g), depth, T, K, True, torch.randn(B, C, H, W, generator=g))


def test_warp_gradient_is_not_masked(ops, dev):
    """The forward zeroes outputs where the destination depth is <= 0.01; the gradient flows there all the same (the reference
    masks through ``.data``, convlstm.py:41).  Checked on a random case against float64 autograd of the UNMASKED warp, and that
    a masked gradient would have been told apart."""
    B, C, H, W = 3, 16, 8, 10
    depth, T, K = warp_geometry("special depths", B, H, W, seed=800)
    g = torch.Generator().manual_seed(801)
    src, go = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    masked = depth <= 0.01
    assert masked.float().mean().item() > 0.3
    out, got = warp_grad(ops.hidden_warp, src, depth, T, K, True, go, dev)
    assert float(out.cpu().masked_fill(~masked, 0.0).abs().max()) == 0.0           # the forward is masked ...
    _, ref32 = warp_grad(orc.warp_hidden_state, src, depth, T, K, False, go)
    _, ref64 = warp_grad(orc.warp_hidden_state, src, depth, T, K, False, go, dtype=torch.float64)
    as_accurate_as_reference(got, ref32, ref64)                                     # ... its gradient is the unmasked one
    _, if_masked = warp_grad(orc.warp_hidden_state, src, depth, T, K, False, go.masked_fill(masked, 0.0), dtype=torch.float64)
    assert (if_masked - ref64).abs().max().item() > 0.1


# ----------------------------------------------------------------------------------------------------------------------
# cost-volume backward (ops.cost_volume(dot_product=True) under autograd)
# ----------------------------------------------------------------------------------------------------------------------
def cv_geometry(B, M, H, W):
    """Host poses and intrinsics of the sample scene: a different reference frame, measurement frames and focal length per item."""
    p1 = torch.cat([syn.pose(30 + 50 * b) for b in range(B)])
    p2s = [torch.cat([syn.pose(30 + 50 * b - 3 * (m + 1)) for b in range(B)]) for m in range(M)]
    Ks = []
    for b in range(B):
        K = syn.scaled_K(syn.full_K(), 320.0 / max(W, 2)).clone()
        K[:, 0, 0] *= 1.0 + 0.05 * b
        K[:, 1, 1] *= 1.0 - 0.03 * b
        Ks.append(K)
    return p1, p2s, torch.cat(Ks)


def cv_inputs(B, M, C, H, W, D, seed):
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(B, C, H, W, generator=g)
    f2s = [torch.randn(B, C, H, W, generator=g) for _ in range(M)]
    go = torch.randn(B, D, H, W, generator=g) * (M * C)       # O(1) gradients: the 1/(M*C) of the mean is undone
    return f1, f2s, go


def cv_kernel_grads(ops, dev, f1, f2s, geo, D, go, need1=True, need2=None, channels_last=False):
    p1, p2s, K = geo
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    a = f1.to(dev).clone().contiguous(memory_format=fmt).requires_grad_(need1)
    need2 = [True] * len(f2s) if need2 is None else need2
    bs = [t.to(dev).clone().contiguous(memory_format=fmt).requires_grad_(n) for t, n in zip(f2s, need2)]
    hipcall.cost_volume(ops, a, bs, p1, p2s, K, 0.25, 20.0, D, True, 0).backward(go.to(dev))
    return a.grad, [t.grad for t in bs]


def cv_oracle_grads(f1, f2s, geo, D, go, dtype):
    p1, p2s, K = geo
    a, *bs = _leaves([f1] + list(f2s), dtype=dtype)
    orc.cost_volume_fusion(a, bs, p1.to(dtype), [p.to(dtype) for p in p2s], K.to(dtype), 0.25, 20.0, D, True).backward(go.to(dtype))
    return a.grad, [t.grad for t in bs]


CV_CASES = [   # B, M, C, H, W, D
    (1, 1, 1, 12, 16, 2),
    (1, 3, 3, 16, 20, 63),
    (1, 8, 17, 12, 16, 8),        # DVMVS_MAX_MEASUREMENTS: one gather grid row per frame
    (1, 2, 33, 16, 20, 256),      # DVMVS_MAX_DEPTH_LEVELS: the gather's dynamic LDS at its maximum
    (3, 2, 48, 20, 24, 16),
    (1, 3, 5, 16, 20, 1),         # one plane: zero plane step
    (1, 8, 48, 8, 12, 63),
    (2, 3, 8, 1, 24, 16),         # H == 1: atomic scatter
    (1, 2, 17, 20, 1, 12),        # W == 1: atomic scatter
    (1, 1, 3, 1, 1, 4),
    (3, 3, 33, 1, 24, 2),
]


@pytest.mark.parametrize("B,M,C,H,W,D", CV_CASES)
def test_cost_volume_backward(ops, dev, B, M, C, H, W, D):
    f1, f2s, go = cv_inputs(B, M, C, H, W, D, seed=900 + B * 1000 + M * 100 + C + H * W + D)
    geo = cv_geometry(B, M, H, W)
    g1, g2s = cv_kernel_grads(ops, dev, f1, f2s, geo, D, go)
    r1_32, r2s_32 = cv_oracle_grads(f1, f2s, geo, D, go, torch.float32)
    r1_64, r2s_64 = cv_oracle_grads(f1, f2s, geo, D, go, torch.float64)
    assert r1_64.abs().max().item() > 0.1 and min(r.abs().max().item() for r in r2s_64) > 0.1     # the frames do overlap
    as_accurate_as_reference(g1, r1_32, r1_64)
    for m, (x, r32, r64) in enumerate(zip(g2s, r2s_32, r2s_64)):
        assert x.shape == r64.shape, m
        as_accurate_as_reference(x, r32, r64)
    again1, again2s = cv_kernel_grads(ops, dev, f1, f2s, geo, D, go)
    assert torch.equal(again1, g1), "reference-feature gradient is not bit-reproducible"
    if H > 1 and W > 1:           # the gather; the H == 1 / W == 1 scatter adds with atomics
        assert all(torch.equal(x, y) for x, y in zip(again2s, g2s)), "measurement-feature gather is not bit-reproducible"


def test_cost_volume_backward_one_sided(ops, dev):
    """Gradient requested for the reference map only, or for one of three measurement maps: what is computed equals, bit for bit,
    the same gradient of the run that computes all of them."""
    B, M, C, H, W, D = 2, 3, 17, 16, 20, 12
    f1, f2s, go = cv_inputs(B, M, C, H, W, D, seed=950)
    geo = cv_geometry(B, M, H, W)
    g1, g2s = cv_kernel_grads(ops, dev, f1, f2s, geo, D, go)
    r1_32, r2s_32 = cv_oracle_grads(f1, f2s, geo, D, go, torch.float32)
    r1_64, r2s_64 = cv_oracle_grads(f1, f2s, geo, D, go, torch.float64)
    as_accurate_as_reference(g1, r1_32, r1_64)
    as_accurate_as_reference(g2s[1], r2s_32[1], r2s_64[1])
    only1, none2 = cv_kernel_grads(ops, dev, f1, f2s, geo, D, go, need2=[False] * M)
    assert torch.equal(only1, g1) and all(x is None for x in none2)
    no1, one2 = cv_kernel_grads(ops, dev, f1, f2s, geo, D, go, need1=False, need2=[False, True, False])
    assert no1 is None and one2[0] is None and one2[2] is None
    assert torch.equal(one2[1], g2s[1])


def test_cost_volume_backward_channels_last(ops, dev):
    """Channels-last feature maps at 64x64, C = 32 (the forward's NHWC path): the gradients equal those of NCHW inputs bit for bit."""
    B, M, C, H, W, D = 1, 2, 32, 64, 64, 8
    f1, f2s, go = cv_inputs(B, M, C, H, W, D, seed=960)
    geo = cv_geometry(B, M, H, W)
    probe = f2s[0].to(dev).contiguous(memory_format=torch.channels_last)
    assert probe.is_contiguous(memory_format=torch.channels_last) and not probe.is_contiguous()
    n1, n2s = cv_kernel_grads(ops, dev, f1, f2s, geo, D, go)
    c1, c2s = cv_kernel_grads(ops, dev, f1, f2s, geo, D, go, channels_last=True)
    assert torch.equal(c1, n1) and all(torch.equal(x, y) for x, y in zip(c2s, n2s))
    r1_32, r2s_32 = cv_oracle_grads(f1, f2s, geo, D, go, torch.float32)
    r1_64, r2s_64 = cv_oracle_grads(f1, f2s, geo, D, go, torch.float64)
    as_accurate_as_reference(c1, r1_32, r1_64)
    for x, r32, r64 in zip(c2s, r2s_32, r2s_64):
        as_accurate_as_reference(x, r32, r64)
