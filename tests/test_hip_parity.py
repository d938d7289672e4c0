"""GPU parity tests: every HIP op, called through the C ABI (ctypes -> libdvmvs_hip.so), against the CPU oracle on the
same inputs and against the golden vectors produced by the reference.

Tolerances (floating point, fp32 everywhere):
* cost volume, dot mode: max |err| <= 2e-5 on values of mean magnitude ~0.06-0.09 (SURVEY: an independent float64
  restatement is within 2.8e-5 of the reference); SAD mode 1e-4 on values ~1.3-7.
* hidden warp / gates: 5e-6 / 2e-5 absolute on O(1) values.
* depth re-projection: bit-exact except at round-to-nearest ties of the projected pixel (<= 0.1 % of pixels may move
  by one pixel when the fp32 projection differs in the last ulp); measured: 0 mismatches.
"""
import json
import os

import numpy as np
import pytest
import torch

import dvmvs_oracle as orc
import hipcall
import synthetic as syn
from accuracy import as_accurate_as_reference, f64  # noqa: F401  (also imported from here by test_sweep_mfma_gpu)

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


@pytest.fixture(scope="module")
def utils(dev):
    from dvmvs import utils as u
    return u


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def to(dev, *ts):
    return [t.to(dev) for t in ts]


def maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def check_pins(t, z, prefix, atol):
    t = t.detach().cpu()
    assert list(t.shape) == list(z[f"{prefix}_shape"])
    idx = syn.sample_indices(t.numel())
    np.testing.assert_allclose(t.reshape(-1)[idx].numpy(), z[f"{prefix}_samples"], atol=atol, rtol=0)
    scale = float(z[f"{prefix}_abs_sum"])
    assert abs(t.double().sum().item() - float(z[f"{prefix}_sum"])) <= 2e-5 * scale


VARIANTS = [0, 1, 2, 3, 4, 5, 6, 7]   # 0 automatic, 1 generic, 2 / 3 the two configurations of the LDS-tiled sweep, 4 / 5 the same without a second pass,
                                      # 6 the correlate-then-interpolate sweep on the fp32 matrix cores (csrc/sweep_mfma.hip; persistent form where
                                      # eligible), 7 its one-item-per-workgroup form


def run_cv(ops, dev, f1, f2s, p1, p2s, K, lo, hi, D, dot, variant):
    """Features to the device; poses / intrinsics stay on the host, where the reference-mode pose algebra runs."""
    return hipcall.cost_volume(ops, f1.to(dev), [t.to(dev) for t in f2s], p1, p2s, K, lo, hi, D, dot, variant)


# ----------------------------------------------------------------------------------------------------------------------
# cost volume
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_cost_volume_small_goldens(ops, dev, golden_dir, variant, fixture_host_algebra):
    z = load(golden_dir, "cost_volume_small")
    K = torch.from_numpy(z["K"])
    feats = [syn.analytic_features(s, 8, 32, 40) for s in range(4)]
    for tag, (r, ms) in json.loads(str(z["pose_sets"])).items():
        for dot in (True, False):
            if variant in (2, 3, 4, 5, 6, 7) and not dot:
                continue
            got = run_cv(ops, dev, feats[0], [feats[1 + i] for i in range(len(ms))], syn.pose(r), [syn.pose(m) for m in ms], K,
                         0.25, 20.0, 16, dot, variant)
            exp = torch.from_numpy(z[f"{tag}_{'dot' if dot else 'sad'}"])
            # one bound for every pair, including "behind" (the sweep crosses Z = 0 for 38 % of the samples): the kernels are
            # handed the reference's own fp32 matrices (dvmvs.pose_algebra), so positions next to the singularity agree too
            tol = 2e-5 if dot else 1e-4
            err = (got.cpu() - exp).abs()
            assert err.max().item() < tol and err.mean().item() < tol / 20, (tag, dot, err.max().item(), err.mean().item())


@pytest.mark.parametrize("variant", VARIANTS)
def test_cost_volume_full_size_known_answers(ops, dev, golden_dir, variant, fixture_host_algebra):
    """320x256 -> 160x128 features, 32 channels, 64 planes (BASELINE.json config): KAT-CV, behind-camera pair, noise."""
    z = load(golden_dir, "cost_volume_full_pins")
    halfK = syn.scaled_K(syn.full_K(), 2.0)
    f = [syn.analytic_features(s) for s in range(3)]
    cv = run_cv(ops, dev, f[0], [f[1], f[2]], syn.pose(9), [syn.pose(6), syn.pose(0)], halfK, 0.25, 20.0, 64, True, variant)
    assert abs(cv.double().sum().item() - 78687.558811) < 1.0
    assert abs(cv[0, 0, 64, 80].item() - 0.31054920) < 2e-5
    assert abs(cv[0, 31, 10, 20].item() - 0.36512548) < 2e-5
    assert abs(cv[0, 63, 127, 159].item() - 0.02026378) < 2e-5
    check_pins(cv, z, "kat_cv", atol=5e-5)
    exp = orc.cost_volume_fusion(f[0], [f[1], f[2]], syn.pose(9), [syn.pose(6), syn.pose(0)], halfK, 0.25, 20.0, 64, True)
    exp64 = orc.cost_volume_fusion(*f64(f[0], [f[1], f[2]], syn.pose(9), [syn.pose(6), syn.pose(0)], halfK), 0.25, 20.0, 64, True)
    d = (cv.cpu() - exp).abs()
    assert d.max().item() < 5e-5 and d.mean().item() < 2e-6          # SURVEY: fp32 reference vs float64 is 2.8e-5 / 1.3e-6
    as_accurate_as_reference(cv, exp, exp64)
    back = run_cv(ops, dev, f[0], [f[1]], syn.pose(141), [syn.pose(135)], halfK, 0.25, 20.0, 64, True, variant)
    check_pins(back, z, "behind", atol=5e-5)   # Z = 0 crossings: same bound as everywhere else
    nf = [syn.smooth_noise((1, 32, 128, 160), seed=40 + i) for i in range(3)]
    ncv = run_cv(ops, dev, nf[0], [nf[1], nf[2]], syn.pose(13), [syn.pose(12), syn.pose(9)], halfK, 0.25, 20.0, 64, True, variant)
    check_pins(ncv, z, "noise", atol=5e-5)


def test_cost_volume_sad_known_answer(ops, dev, golden_dir, fixture_host_algebra):
    """The baselines' mode: RGB (C=3), SAD, 0.5-50 m (KAT-SAD)."""
    z = load(golden_dir, "cost_volume_full_pins")
    halfK = syn.scaled_K(syn.full_K(), 2.0)
    f = [syn.analytic_features(s)[:, :3].contiguous() for s in range(2)]
    sad = run_cv(ops, dev, f[0], [f[1]], syn.pose(9), [syn.pose(6)], halfK, 0.5, 50.0, 64, False, 0)
    assert abs(sad.double().sum().item() - 1749443.403785) < 20.0
    assert abs(sad[0, 5, 64, 80].item() - 2.28013682) < 1e-4
    check_pins(sad, z, "kat_sad", atol=1e-4)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(2, 5, 33, 47, 10, 3), (3, 32, 16, 24, 64, 1), (1, 1, 7, 5, 3, 2), (2, 32, 64, 80, 64, 2)])
def test_cost_volume_ragged_shapes_and_batches(ops, dev, shape, variant):
    """Sizes that are not multiples of the workgroup tile, odd channel counts, per-batch poses/intrinsics."""
    B, C, H, W, D, M = shape
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + H)
    f1 = torch.randn(B, C, H, W, generator=g)
    f2s = [torch.randn(B, C, H, W, generator=g) for _ in range(M)]
    pose_ids = [9, 10, 13, 16, 20, 141]
    p1 = torch.cat([syn.pose(pose_ids[b % 6]) for b in range(B)])
    p2s = [torch.cat([syn.pose(pose_ids[(b + 1 + m) % 6] - 3) for b in range(B)]) for m in range(M)]
    K = torch.cat([syn.scaled_K(syn.full_K(), 320.0 / W) * torch.tensor([1.0 + 0.01 * b]) for b in range(B)])
    K[:, 2, 2] = 1.0
    for dot in (True, False):
        if variant in (2, 3, 4, 5, 6, 7) and not dot:
            continue
        got = run_cv(ops, dev, f1, f2s, p1, p2s, K, 0.25, 20.0, D, dot, variant)
        exp = orc.cost_volume_fusion(f1, f2s, p1, p2s, K, 0.25, 20.0, D, dot)
        exp64 = orc.cost_volume_fusion(*f64(f1, f2s, p1, p2s, K), 0.25, 20.0, D, dot)
        # white-noise features: the worst case for sample-position round-off (gradient ~ 1 per pixel)
        assert maxerr(got, exp) < (5e-4 if dot else 2e-3) * max(1.0, exp.abs().max().item()), (shape, dot)
        as_accurate_as_reference(got, exp, exp64, floor=(2e-6 if dot else 2e-5))


@pytest.mark.parametrize("variant", VARIANTS)
def test_cost_volume_properties_full_size(ops, dev, variant):
    """Size-independent properties at the BASELINE.json size: linearity in the reference features (dot mode),
    fusion == mean of the single-frame volumes, identity pose == plain per-pixel correlation at the rescaled grid."""
    halfK = syn.scaled_K(syn.full_K(), 2.0)
    f = [syn.smooth_noise((1, 32, 128, 160), seed=90 + i) for i in range(4)]
    args = dict(lo=0.25, hi=20.0, D=64, dot=True, variant=variant)
    cv_a = run_cv(ops, dev, f[0], [f[2]], syn.pose(10), [syn.pose(9)], halfK, **args)
    cv_b = run_cv(ops, dev, f[1], [f[2]], syn.pose(10), [syn.pose(9)], halfK, **args)
    cv_ab = run_cv(ops, dev, 0.5 * f[0] - 2.0 * f[1], [f[2]], syn.pose(10), [syn.pose(9)], halfK, **args)
    assert maxerr(cv_ab, 0.5 * cv_a - 2.0 * cv_b) < 2e-5
    cv_c = run_cv(ops, dev, f[0], [f[3]], syn.pose(10), [syn.pose(6)], halfK, **args)
    fused = run_cv(ops, dev, f[0], [f[2], f[3]], syn.pose(10), [syn.pose(9), syn.pose(6)], halfK, **args)
    assert maxerr(fused, (cv_a + cv_c) / 2) < 1e-6
    # identical poses: every plane samples at u*(W-1)/W, v*(H-1)/H, independent of depth.  (With the "exact" pose algebra:
    # inverse(P) @ P is the identity only up to fp32 round-off in the reference's own arithmetic, which leaves a K t of ~1e-6 that
    # the near planes turn into a 5e-5 difference between plane 0 and plane 63 -- faithfully reproduced in the default mode.)
    same = hipcall.cost_volume(ops, f[0].to(dev), [f[2].to(dev)], syn.pose(10).to(dev), [syn.pose(10).to(dev)], halfK.to(dev),
                               0.25, 20.0, 64, True, variant, mode="exact")
    assert maxerr(same[:, 0], same[:, 63]) < 2e-5
    ys, xs = torch.meshgrid(torch.arange(128.0), torch.arange(160.0), indexing="ij")
    warped = orc.bilinear_zeros_gather(f[2], (xs * 159 / 160).reshape(1, -1), (ys * 127 / 128).reshape(1, -1)).reshape(1, 32, 128, 160)
    assert maxerr(same[:, 17], (f[0] * warped).sum(1) / 32) < 2e-5


def test_cost_volume_channels_last_measurement_maps(ops, dev):
    """DVMVS_LAYOUT_NHWC: measurement maps handed over channels-last give the same volume as NCHW ones (staged and
    spill paths: the second geometry has tiles whose footprint does not fit in LDS)."""
    halfK = syn.scaled_K(syn.full_K(), 2.0)
    f = [syn.smooth_noise((2, 32, 128, 160), seed=70 + i) for i in range(3)]
    for (r, ms) in ((9, (6, 0)), (202, (196, 188)), (141, (135, 130))):
        p1 = torch.cat([syn.pose(r), syn.pose(r)])
        p2s = [torch.cat([syn.pose(m), syn.pose(max(m - 1, 0))]) for m in ms]
        K = torch.cat([halfK, halfK])
        nchw = hipcall.cost_volume(ops, f[0].to(dev), [t.to(dev) for t in f[1:]], p1.to(dev), [p.to(dev) for p in p2s], K.to(dev), 0.25, 20.0, 64, True, 2)
        cl = [t.to(dev).contiguous(memory_format=torch.channels_last) for t in f[1:]]
        assert all(not t.is_contiguous() for t in cl)
        nhwc = hipcall.cost_volume(ops, f[0].to(dev), cl, p1.to(dev), [p.to(dev) for p in p2s], K.to(dev), 0.25, 20.0, 64, True, 0)
        assert maxerr(nhwc, nchw) < 1e-6
        # every tiled instantiation reads channels-last maps too (the frame engine keeps its maps channels-last): both LDS configurations,
        # two-pass and single-pass forms (the wide configuration's channels-last instantiations have their own prefetch depth)
        for variant in (2, 3, 4, 5):
            forced = hipcall.cost_volume(ops, f[0].to(dev), cl, p1.to(dev), [p.to(dev) for p in p2s], K.to(dev), 0.25, 20.0, 64, True, variant)
            assert maxerr(forced, nchw) < 2e-6, (r, variant)
        exp = orc.cost_volume_fusion(f[0][:1], [t[:1] for t in f[1:]], p1[:1], [p[:1] for p in p2s], K[:1], 0.25, 20.0, 64, True)
        exp64 = orc.cost_volume_fusion(*f64(f[0][:1], [t[:1] for t in f[1:]], p1[:1], [p[:1] for p in p2s], K[:1]), 0.25, 20.0, 64, True)
        as_accurate_as_reference(nhwc[:1], exp, exp64, floor=1e-5)


def test_cost_volume_two_pass_is_bit_reproducible(ops, dev):
    """SURVEY section 5 / VERDICT r1: the two-pass sweep queues runs of planes it cannot stage (here: forward motion and a
    behind-camera pair, three measurement frames so that several frames spill the same pixel and plane) and finishes them in
    a second launch.  That launch applies a (pixel, plane)'s contributions in frame order from a single writer, so repeated
    runs must agree BIT FOR BIT, and must agree with the single-pass form (inline gather) to fp32 round-off."""
    halfK = syn.scaled_K(syn.full_K(), 2.0)
    f = [syn.smooth_noise((2, 32, 128, 160), seed=170 + i) for i in range(4)]
    for (r, ms) in ((202, (196, 188, 180)), (141, (135, 130, 120)), (170, (168, 167, 160))):
        p1 = torch.cat([syn.pose(r), syn.pose(r)]).to(dev)
        p2s = [torch.cat([syn.pose(m), syn.pose(max(m - 2, 0))]).to(dev) for m in ms]
        K = torch.cat([halfK, halfK]).to(dev)
        f1 = f[0].to(dev)
        for layout in ("nchw", "nhwc"):
            f2s = [t.to(dev) for t in f[1:]]
            if layout == "nhwc":
                f2s = [t.contiguous(memory_format=torch.channels_last) for t in f2s]
            runs = [hipcall.cost_volume(ops, f1, f2s, p1, p2s, K, 0.25, 20.0, 64, True, 2).clone() for _ in range(4)]
            for other in runs[1:]:
                assert torch.equal(runs[0], other), (r, layout)
            # the wide-baseline configuration (72 KB boxes, 512-thread workgroups): bit-reproducible as well, and the same volume
            wide = [hipcall.cost_volume(ops, f1, f2s, p1, p2s, K, 0.25, 20.0, 64, True, 3).clone() for _ in range(4)]
            for other in wide[1:]:
                assert torch.equal(wide[0], other), (r, layout, "wide")
            assert maxerr(wide[0], runs[0]) < 1e-6, (r, layout)
            # the single-pass variants on geometries that DO need unstageable runs: gathered inline, same volume, bit-reproducible
            for variant in (4, 5, 6):
                one = [hipcall.cost_volume(ops, f1, f2s, p1, p2s, K, 0.25, 20.0, 64, True, variant).clone() for _ in range(2)]
                assert torch.equal(one[0], one[1]), (r, layout, variant)
                assert maxerr(one[0], runs[0]) < (2e-6 if variant == 6 else 1e-6), (r, layout, variant)   # (6: another order of the channel sum)
            saved = ops.sweep.COST_VOLUME_TWO_PASS
            ops.sweep.COST_VOLUME_TWO_PASS = False
            try:
                single = hipcall.cost_volume(ops, f1, f2s, p1, p2s, K, 0.25, 20.0, 64, True, 2)
            finally:
                ops.sweep.COST_VOLUME_TWO_PASS = saved
            assert maxerr(single, runs[0]) < 1e-6, (r, layout)
            generic = hipcall.cost_volume(ops, f1, [t.contiguous() for t in f2s], p1, p2s, K, 0.25, 20.0, 64, True, 1)
            assert maxerr(generic, runs[0]) < 3e-5, (r, layout)   # different (reference-order) arithmetic, same volume


def test_cost_volume_limits(ops, dev):
    """Maximum measurement-frame and plane counts the ABI accepts (8 and 256), one step beyond, and degenerate arguments."""
    g = torch.Generator().manual_seed(31)
    B, C, H, W, D, M = 1, 4, 64, 64, 256, 8
    f1 = torch.randn(B, C, H, W, generator=g)
    f2s = [torch.randn(B, C, H, W, generator=g) for _ in range(M)]
    p1 = syn.pose(20)
    p2s = [syn.pose(20 - 1 - m) for m in range(M)]
    K = syn.scaled_K(syn.full_K(), 320.0 / W)
    exp = orc.cost_volume_fusion(f1, f2s, p1, p2s, K, 0.25, 20.0, D, True)
    for variant in (1, 2, 3, 4, 5, 6):
        got = run_cv(ops, dev, f1, f2s, p1, p2s, K, 0.25, 20.0, D, True, variant)
        assert maxerr(got, exp) < 5e-4 * max(1.0, exp.abs().max().item()), variant
    with pytest.raises(RuntimeError, match="not supported"):      # 9 measurement frames
        run_cv(ops, dev, f1, f2s + [f2s[0]], p1, p2s + [p2s[0]], K, 0.25, 20.0, 16, True, 0)
    with pytest.raises(RuntimeError, match="not supported"):      # 257 planes
        run_cv(ops, dev, f1, f2s[:1], p1, p2s[:1], K, 0.25, 20.0, 257, True, 0)
    with pytest.raises(RuntimeError, match="invalid argument"):   # non-positive depth range
        run_cv(ops, dev, f1, f2s[:1], p1, p2s[:1], K, 0.0, 20.0, 16, True, 0)
    with pytest.raises(ValueError):                                # no measurement frame at all
        run_cv(ops, dev, f1, [], p1, [], K, 0.25, 20.0, 16, True, 0)
    with pytest.raises(RuntimeError, match="not supported"):      # SAD has no tiled kernel
        run_cv(ops, dev, f1, f2s[:1], p1, p2s[:1], K, 0.25, 20.0, 16, False, 2)


def test_cost_volume_surface_and_errors(utils, dev):
    halfK = syn.scaled_K(syn.full_K(), 2.0)
    f = [syn.analytic_features(s, 8, 32, 40) for s in range(2)]
    K = syn.scaled_K(halfK, 4.0)
    grid = utils.get_warp_grid_for_cost_volume_calculation(40, 32, dev)
    assert tuple(grid.shape) == (3, 32 * 40) and grid[0, 41].item() == 1.0 and grid[1, 41].item() == 1.0
    one = utils.calculate_cost_volume_by_warping(f[0].to(dev), f[1].to(dev), syn.pose(9).to(dev), syn.pose(6).to(dev), K.to(dev), grid,
                                                 0.25, 20.0, 16, dev, True)
    fused = utils.cost_volume_fusion(f[0].to(dev), [f[1].to(dev)], syn.pose(9).to(dev), [syn.pose(6).to(dev)], K.to(dev), grid,
                                     0.25, 20.0, 16, dev, True)
    assert torch.equal(one, fused) and tuple(one.shape) == (1, 16, 32, 40)
    with pytest.raises(RuntimeError):  # CPU tensors: no fallback
        utils.cost_volume_fusion(f[0], [f[1]], syn.pose(9), [syn.pose(6)], K, None, 0.25, 20.0, 16, "cpu", True)
    with pytest.raises(ValueError):
        utils.cost_volume_fusion(f[0].to(dev), [f[1].to(dev)], syn.pose(9).to(dev), [syn.pose(6).to(dev)], K.to(dev),
                                 grid[:, :100], 0.25, 20.0, 16, dev, True)


def test_cost_volume_gradients(ops, dev, golden_dir):
    """Autograd through the custom op (dvmvs_cost_volume_bwd) vs the reference's autograd (golden) and the oracle's."""
    z = load(golden_dir, "cost_volume_small_grad")
    K = torch.from_numpy(load(golden_dir, "cost_volume_small")["K"])
    sf = [syn.analytic_features(s, 8, 32, 40) for s in range(3)]
    f1 = sf[0].to(dev).requires_grad_(True)
    f2 = [sf[1].to(dev).requires_grad_(True), sf[2].to(dev).requires_grad_(True)]
    # the golden was captured on the fixture host: feed the kernel that host's matrices (tests/synthetic.py, "host pose algebra")
    Hm, kt = syn.FixtureHostAlgebra().sweep_matrices_host(syn.pose(12), [syn.pose(9), syn.pose(3)], K)
    out = ops.cost_volume(f1, f2, Hm.to(dev), kt.to(dev), 0.25, 20.0, 16, True, 0)
    out.backward(torch.from_numpy(z["grad_out"]).to(dev))
    # the same gradients in float64 (oracle autograd) arbitrate between the reference's fp32 round-off and ours
    d1 = sf[0].double().requires_grad_(True)
    d2 = [sf[1].double().requires_grad_(True), sf[2].double().requires_grad_(True)]
    orc.cost_volume_fusion(d1, d2, syn.pose(12).double(), [syn.pose(9).double(), syn.pose(3).double()], K.double(), 0.25, 20.0, 16,
                           True).backward(torch.from_numpy(z["grad_out"]).double())
    for got, key, ref64 in ((f1.grad, "grad_image1", d1.grad), (f2[0].grad, "grad_image2_0", d2[0].grad),
                            (f2[1].grad, "grad_image2_1", d2[1].grad)):
        ref32 = torch.from_numpy(z[key])
        assert maxerr(got, ref32) < 1e-4 * max(1.0, ref32.abs().max().item()), key
        as_accurate_as_reference(got, ref32, ref64)
    # a second geometry (behind-camera pair, B=2) against the oracle's autograd
    g = torch.Generator().manual_seed(3)
    a = torch.randn(2, 6, 20, 28, generator=g)
    b = torch.randn(2, 6, 20, 28, generator=g)
    p1, p2 = torch.cat([syn.pose(141), syn.pose(10)]), torch.cat([syn.pose(135), syn.pose(9)])
    K2 = torch.cat([syn.scaled_K(syn.full_K(), 320.0 / 28)] * 2)
    go = torch.randn(2, 12, 20, 28, generator=g)
    ac, bc = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    orc.cost_volume_fusion(ac, [bc], p1, [p2], K2, 0.25, 20.0, 12, True).backward(go)
    ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    hipcall.cost_volume(ops, ad, [bd], p1.to(dev), [p2.to(dev)], K2.to(dev), 0.25, 20.0, 12, True, 0).backward(go.to(dev))
    assert maxerr(ad.grad, ac.grad) < 5e-4 * max(1.0, ac.grad.abs().max().item())
    assert maxerr(bd.grad, bc.grad) < 5e-4 * max(1.0, bc.grad.abs().max().item())


def test_convolution_with_its_epilogue_as_one_miopen_plan(ops, dev):
    """dvmvs_conv_bias_act_fwd (MIOpen fusion plan convolution + bias [+ ReLU]) against torch's convolution + bias + ReLU, into a
    new tensor and into a channel slice of a larger buffer.  MIOpen may pick a different algorithm (Winograd) than torch's call
    does: stated bound 1e-4 of the largest output."""
    g = torch.Generator().manual_seed(5)
    supported = 0
    for (cin, cout, h, w, k, stride, act) in ((32, 32, 64, 80, 5, 1, "relu"), (64, 64, 32, 40, 3, 1, "relu"), (16, 24, 20, 28, 3, 1, "none"),
                                              (32, 64, 32, 40, 3, 2, "relu"), (96, 32, 128, 160, 5, 1, "relu")):
        x = torch.randn(1, cin, h, w, generator=g).to(dev)
        wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(dev)
        b = torch.randn(cout, generator=g).to(dev)
        exp = torch.nn.functional.conv2d(x, wt, b, stride, k // 2)
        exp = torch.relu(exp) if act == "relu" else exp
        got = ops.conv_bias_act_into(x, wt, b, None, stride, k // 2, ops.ACTIVATIONS[act])
        if got is None:                      # MIOpen has no plan for this problem: the engine keeps the two launches
            continue
        supported += 1
        assert got.shape == exp.shape and maxerr(got, exp) < 1e-4 * exp.abs().max().item(), (cin, cout, k, stride)
        cat = torch.zeros(1, cout + 5, exp.shape[2], exp.shape[3], device=dev)
        ops.conv_bias_act_into(x, wt, b, cat[:, 2:2 + cout], stride, k // 2, ops.ACTIVATIONS[act])
        assert torch.equal(cat[:, 2:2 + cout], got) and float(cat[:, :2].abs().max()) == 0.0 and float(cat[:, 2 + cout:].abs().max()) == 0.0
    assert supported >= 2


def test_cost_volume_gradients_near_the_vanishing_line(ops, dev):
    """The measurement-feature gradient is a gather over the inverse homography of each plane (csrc/cost_volume_bwd.hip); where a
    pixel's 2x2 footprint straddles a plane's vanishing line the inverse is not a search window and the kernel scans the whole
    reference image instead.  Wide field of view + a 50 / 75 degree rotation puts that line inside the image; float64 autograd
    through the oracle is the expected value."""
    g = torch.Generator().manual_seed(21)

    def rot_y(deg):
        t = np.deg2rad(deg)
        R = torch.eye(4)
        R[0, 0], R[0, 2], R[2, 0], R[2, 2] = float(np.cos(t)), float(np.sin(t)), float(-np.sin(t)), float(np.cos(t))
        return R[None]

    for deg, focal_scale, (C, H, W, D) in ((50.0, 0.35, (8, 48, 64, 8)), (75.0, 0.2, (5, 40, 56, 6))):
        a, b = torch.randn(1, C, H, W, generator=g), torch.randn(1, C, H, W, generator=g)
        go = torch.randn(1, D, H, W, generator=g)
        p1 = syn.pose(10)
        p2 = p1 @ rot_y(deg)
        K = syn.scaled_K(syn.full_K(), 320.0 / W).clone()
        K[:, 0, 0] *= focal_scale
        K[:, 1, 1] *= focal_scale
        ac, bc = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        orc.cost_volume_fusion(ac, [bc], p1, [p2], K, 0.25, 20.0, D, True).backward(go)
        assert (bc.grad != 0).float().mean().item() > 0.2          # the pair does overlap
        ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
        hipcall.cost_volume(ops, ad, [bd], p1.to(dev), [p2.to(dev)], K.to(dev), 0.25, 20.0, D, True, 0).backward(go.to(dev))
        assert maxerr(ad.grad, ac.grad) < 5e-4 * max(1.0, ac.grad.abs().max().item())
        assert maxerr(bd.grad, bc.grad) < 5e-4 * max(1.0, bc.grad.abs().max().item()), deg


def test_cost_volume_gradients_larger_maps(ops, dev):
    """Feature maps of 64x80 and more, wide pairs (sample footprints of eight planes several times the tile), a pair with a
    behind-camera corner, odd sizes and more than 32 channels (two channel passes); checked against autograd through the oracle."""
    g = torch.Generator().manual_seed(9)
    # the 128x128 cases: wide pairs whose eight-plane boxes are several LDS windows high (the kernel walks them row block by row block)
    for (B, C, H, W, D, pairs) in ((2, 8, 64, 80, 16, ((12, (9, 3)), (202, (196, 188)))), (1, 20, 72, 100, 24, ((141, (135,)),)),
                                   (2, 8, 128, 128, 16, ((202, (188,)), (86, (83,)))), (1, 36, 128, 160, 8, ((170, (160,)),))):
        a = torch.randn(B, C, H, W, generator=g)
        bs = [torch.randn(B, C, H, W, generator=g) for _ in range(len(pairs[0][1]))]
        p1 = torch.cat([syn.pose(pairs[b % len(pairs)][0]) for b in range(B)])
        p2s = [torch.cat([syn.pose(pairs[b % len(pairs)][1][m]) for b in range(B)]) for m in range(len(bs))]
        K = torch.cat([syn.scaled_K(syn.full_K(), 320.0 / W)] * B)
        go = torch.randn(B, D, H, W, generator=g)
        ac, bc = a.clone().requires_grad_(True), [t.clone().requires_grad_(True) for t in bs]
        orc.cost_volume_fusion(ac, bc, p1, p2s, K, 0.25, 20.0, D, True).backward(go)
        ad, bd = a.to(dev).requires_grad_(True), [t.to(dev).requires_grad_(True) for t in bs]
        hipcall.cost_volume(ops, ad, bd, p1.to(dev), [p.to(dev) for p in p2s], K.to(dev), 0.25, 20.0, D, True, 0).backward(go.to(dev))
        assert maxerr(ad.grad, ac.grad) < 5e-4 * max(1.0, ac.grad.abs().max().item())
        for x, y in zip(bd, bc):
            assert maxerr(x.grad, y.grad) < 5e-4 * max(1.0, y.grad.abs().max().item()), (B, C, H, W)
            assert (x.grad.cpu() - y.grad).abs().mean().item() < 2e-5 * max(1.0, y.grad.abs().mean().item())


# ----------------------------------------------------------------------------------------------------------------------
# depth re-projection
# ----------------------------------------------------------------------------------------------------------------------
def splat_agrees(got, exp, max_moved=20, rtol=2e-6):
    """Same set of hit pixels (up to ``max_moved`` round-to-nearest ties) and the same z on the common ones.  z itself
    is a 4-term fp32 dot product whose summation order (FMA or not) differs between the CPU matmul and the kernel."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    moved = int(((got != 0) != (exp != 0)).sum())
    both = (got != 0) & (exp != 0)
    rel = np.abs(got[both] - exp[both]) / np.abs(exp[both])
    # a pixel hit by two surfaces can flip to the other surface at a tie: count large deviations with the moved ones
    flipped = int((rel > rtol).sum())
    assert moved + flipped <= max_moved, f"{moved} pixels hit/miss differently, {flipped} carry a different surface"
    return moved + flipped


def test_depth_reprojection(ops, utils, dev, golden_dir, fixture_host_algebra):
    z = load(golden_dir, "reproject")
    fullK = syn.full_K()
    halfK = syn.scaled_K(fullK, 2.0)
    prev = syn.analytic_depth()
    out = utils.get_non_differentiable_rectangle_depth_estimation(*to(dev, syn.pose(10), syn.pose(9), prev, fullK, halfK), 320, 256)
    assert tuple(out.shape) == (1, 1, 128, 160)
    got = out.cpu().numpy()
    n_off = splat_agrees(got, z["kat"])
    assert abs(float(got.astype(np.float64).sum()) - 30690.716363) < 0.05 + 3.0 * n_off   # KAT-REPROJ
    assert abs(int((got != 0).sum()) - 20307) <= n_off and abs(got[0, 0, 64, 80] - 1.03667092) < 1e-5
    full, low = hipcall.depth_reproject(ops, syn.pose(10), syn.pose(9), *to(dev, prev, fullK, halfK), 16)
    assert torch.equal(full, out) and torch.equal(low, out[..., ::16, ::16])
    splat_agrees(low.cpu().numpy(), z["kat_low"], max_moved=1)
    # harder case: zeros in the source depth, a far wall, larger motion; and a batch of two different problems
    prev2 = prev.clone()
    prev2[:, :, 40:90, 100:180] = 0.0
    prev2[:, :, 150:, :] = 6.0
    out2 = hipcall.depth_reproject(ops, torch.cat([syn.pose(16), syn.pose(10)]), torch.cat([syn.pose(9), syn.pose(9)]),
                                   *to(dev, torch.cat([prev2, prev]), torch.cat([fullK, fullK]), torch.cat([halfK, halfK])))
    splat_agrees(out2[0, 0].cpu().numpy(), z["hard"][0, 0])
    assert torch.equal(out2[1], out[0])
    # order independence: the atomic z-buffer is deterministic (bitwise) run to run
    again = hipcall.depth_reproject(ops, syn.pose(10), syn.pose(9), *to(dev, prev, fullK, halfK))
    assert torch.equal(again, out)
    # "exact" pose algebra (fp64 on the device): a different last-ulp rounding of the relative pose, the same surface
    exact = hipcall.depth_reproject(ops, *to(dev, syn.pose(10), syn.pose(9), prev, fullK, halfK), mode="exact")
    splat_agrees(exact.cpu().numpy(), z["kat"])


def test_relative_pose(ops, dev):
    a = torch.cat([syn.pose(i) for i in (9, 40, 141, 200)])
    c = torch.cat([syn.pose(i) for i in (10, 9, 135, 3)])
    got = ops.relative_pose(a.to(dev), c.to(dev)).cpu()
    exp = (torch.linalg.inv(a.double()) @ c.double())
    assert (got.double() - exp).abs().max().item() < 1e-6
    assert torch.equal(got[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(4, 4))


def test_exact_sweep_matrices_and_modes(ops, dev):
    """dvmvs_sweep_matrices (fp64 on the device, the opt-in "exact" pose algebra) against float64 torch, and both modes
    through the surface: "reference" hands the kernel the reference's own fp32 matrices bit for bit."""
    from dvmvs import pose_algebra
    p1 = torch.cat([syn.pose(i) for i in (9, 141, 202)])
    p2s = [torch.cat([syn.pose(i) for i in (6, 135, 196)]), torch.cat([syn.pose(i) for i in (0, 130, 188)])]
    K = torch.cat([syn.scaled_K(syn.full_K(), 2.0)] * 3)
    Hm, kt = ops.sweep_matrices(p1.to(dev), [p.to(dev) for p in p2s], K.to(dev))
    assert tuple(Hm.shape) == (3, 2, 9) and tuple(kt.shape) == (3, 2, 3)
    for m, p2 in enumerate(p2s):
        H64, k64 = orc.plane_sweep_setup(p1.double(), p2.double(), K.double())
        assert (Hm[:, m].cpu().double() - H64.reshape(3, 9)).abs().max().item() < 2e-7 * H64.abs().max().item()
        assert (kt[:, m].cpu().double() - k64.reshape(3, 3)).abs().max().item() < 2e-7 * max(1.0, k64.abs().max().item())
        H32, k32 = orc.plane_sweep_setup(p1, p2, K)     # the reference's arithmetic (oracle pinned to it)
        Hr, kr = pose_algebra.sweep_matrices(p1, p2s, K, dev, "reference")
        assert torch.equal(Hr[:, m].cpu(), H32.reshape(3, 9)) and torch.equal(kr[:, m].cpu(), k32.reshape(3, 3))
    f = [syn.smooth_noise((3, 32, 128, 160), seed=300 + i) for i in range(3)]
    a = hipcall.cost_volume(ops, f[0].to(dev), [t.to(dev) for t in f[1:]], p1, p2s, K, 0.25, 20.0, 64, True, 0, mode="reference")
    b = hipcall.cost_volume(ops, f[0].to(dev), [t.to(dev) for t in f[1:]], p1.to(dev), [p.to(dev) for p in p2s], K.to(dev),
                            0.25, 20.0, 64, True, 0, mode="exact")
    # two roundings of the same matrices: equal up to the position round-off they cause (never bit-equal, never far apart)
    assert 0.0 < maxerr(a, b) < 2e-3 * a.abs().max().item()


# ----------------------------------------------------------------------------------------------------------------------
# hidden-state warp
# ----------------------------------------------------------------------------------------------------------------------
def test_hidden_warp_goldens(ops, utils, dev, golden_dir):
    z = load(golden_dir, "hidden_warp")
    lK = syn.scaled_K(syn.full_K(), 32.0)
    _, _, h0, _ = syn.analytic_lstm_inputs()
    t = lambda k: torch.from_numpy(z[k])
    got = utils.warp_frame_depth(*to(dev, h0, t("depth"), t("T"), lK))
    assert maxerr(got, t("warped")) < 5e-6
    got = ops.hidden_warp(*to(dev, h0, t("depth_masked"), t("T"), lK), True)
    assert maxerr(got, t("warped_masked")) < 5e-6
    assert float(got[0, :, 2:5, 3:7].abs().max()) == 0.0
    got = utils.warp_frame_depth(*to(dev, h0, t("depth"), t("T_far"), lK))
    assert maxerr(got, t("warped_far")) < 5e-6
    with pytest.raises(ValueError):
        utils.warp_frame_depth(*to(dev, h0[0], t("depth"), t("T"), lK))
    with pytest.raises(TypeError):
        utils.warp_frame_depth(h0.numpy(), t("depth"), t("T"), lK)


def test_hidden_warp_other_shapes(ops, dev):
    g = torch.Generator().manual_seed(11)
    for (B, C, H, W) in ((2, 7, 8, 8), (1, 512, 15, 20), (3, 1, 5, 9)):
        src = torch.randn(B, C, H, W, generator=g)
        depth = torch.rand(B, 1, H, W, generator=g) * 3.0
        depth[:, :, 0, :] = 0.0
        T = torch.linalg.inv(torch.cat([syn.pose(9 + b) for b in range(B)])) @ torch.cat([syn.pose(10 + 2 * b) for b in range(B)])
        K = torch.cat([syn.scaled_K(syn.full_K(), 320.0 / W)] * B)
        for mask in (False, True):
            got = ops.hidden_warp(*to(dev, src, depth, T, K), mask)
            assert maxerr(got, orc.warp_hidden_state(src, depth, T, K, zero_invalid=mask)) < 2e-5


def test_hidden_warp_gradient_is_not_masked(ops, dev, golden_dir):
    z = load(golden_dir, "lstm_grads")
    hw = load(golden_dir, "hidden_warp")
    lK = syn.scaled_K(syn.full_K(), 32.0)
    _, _, h0, _ = syn.analytic_lstm_inputs()
    src = h0[:, :64].to(dev).requires_grad_(True)
    out = ops.hidden_warp(src, torch.from_numpy(hw["depth_masked"]).to(dev), torch.from_numpy(hw["T"]).to(dev), lK.to(dev), True)
    out.backward(torch.from_numpy(z["warp_grad_out"]).to(dev))
    assert maxerr(src.grad, torch.from_numpy(z["warp_grad_src"])) < 1e-5


# ----------------------------------------------------------------------------------------------------------------------
# ConvLSTM
# ----------------------------------------------------------------------------------------------------------------------
def analytic_cc():
    o = np.arange(2048, dtype=np.float64).reshape(-1, 1, 1)
    yy = np.arange(8, dtype=np.float64).reshape(1, -1, 1)
    xx = np.arange(10, dtype=np.float64).reshape(1, 1, -1)
    return torch.from_numpy((2.0 * np.sin(0.013 * o + 0.7 * yy + 0.3 * xx) + 0.5 * np.cos(0.05 * o * xx)).astype(np.float32)).unsqueeze(0)


def test_lstm_gates_goldens(ops, dev, golden_dir):
    z = load(golden_dir, "lstm_gates")
    _, _, _, c0 = syn.analytic_lstm_inputs()
    h, c = ops.lstm_gates(analytic_cc().to(dev), c0.to(dev))
    assert maxerr(h, torch.from_numpy(z["h_next"])) < 1e-5 and maxerr(c, torch.from_numpy(z["c_next"])) < 1e-5
    # LayerNorm property: every (b, channel) plane of c' has mean 0 and biased variance 1 (up to eps)
    assert c.mean(dim=(-2, -1)).abs().max().item() < 1e-5
    assert (c.var(dim=(-2, -1), unbiased=False) - 1).abs().max().item() < 1e-3


@pytest.mark.parametrize("shape", [(4, 512, 8, 8), (1, 512, 8, 10), (2, 24, 15, 20), (1, 8, 3, 5), (2, 16, 20, 30), (1, 4, 32, 32)])
def test_lstm_gates_shapes(ops, dev, shape):
    B, hid, H, W = shape
    g = torch.Generator().manual_seed(H * W + hid)
    cc = torch.randn(B, 4 * hid, H, W, generator=g) * 1.5
    c = torch.randn(B, hid, H, W, generator=g)
    h, cn = ops.lstm_gates(cc.to(dev), c.to(dev))
    eh, ec = orc.lstm_gates(cc, c)
    assert maxerr(h, eh) < 2e-5 and maxerr(cn, ec) < 2e-5


def test_lstm_gates_gradients(ops, dev, golden_dir):
    z = load(golden_dir, "lstm_grads")
    cc = torch.from_numpy(z["cc"]).to(dev).requires_grad_(True)
    c = torch.from_numpy(z["c"]).to(dev).requires_grad_(True)
    h, cn = ops.lstm_gates(cc, c)
    ((h * torch.from_numpy(z["grad_h"]).to(dev)).sum() + (cn * torch.from_numpy(z["grad_c"]).to(dev)).sum()).backward()
    assert maxerr(cc.grad, torch.from_numpy(z["grad_cc"])) < 2e-5
    assert maxerr(c.grad, torch.from_numpy(z["grad_c_cur"])) < 2e-5


def test_convlstm_cell_known_answer(dev, golden_dir):
    """KAT-LSTM: the module (pose op + warp/mask kernel + MIOpen conv + gate kernel) against the reference cell."""
    from dvmvs.convlstm import MVSLayernormConvLSTMCell
    z = load(golden_dir, "lstm_gates")
    weight, x, h0, c0 = syn.analytic_lstm_inputs()
    lK = syn.scaled_K(syn.full_K(), 32.0)
    de16 = torch.from_numpy(load(golden_dir, "reproject")["kat_low"])
    cell = MVSLayernormConvLSTMCell(512, 512, (3, 3), torch.celu).to(dev)
    assert list(cell.state_dict().keys()) == ["conv.weight"]
    with torch.no_grad():
        cell.conv.weight.copy_(weight.to(dev))
        hn, cn = cell(*to(dev, x), to(dev, h0, c0), *to(dev, syn.pose(9), syn.pose(10), de16, lK))
        # K = 9216 fp32 reduction inside the conv: summation order differs between MIOpen and the CPU reference
        assert maxerr(hn, torch.from_numpy(z["kat_h"])) < 2e-4 and maxerr(cn, torch.from_numpy(z["kat_c"])) < 2e-4
        assert abs(hn.double().abs().sum().item() - 14085.416424) < 0.5
        # first step of a sequence: no previous pose -> no warp
        h1, c1 = cell(*to(dev, x), list(cell.init_hidden(1, (8, 10))), None, syn.pose(9).to(dev), de16.to(dev), lK.to(dev))
        eh, ec = orc.convlstm_cell(weight, x, torch.zeros_like(h0), torch.zeros_like(c0), None, syn.pose(9), de16, lK)
        assert maxerr(h1, eh) < 2e-4 and maxerr(c1, ec) < 2e-4


# ----------------------------------------------------------------------------------------------------------------------
# frame-path epilogues
# ----------------------------------------------------------------------------------------------------------------------
def test_bias_activation_epilogue_is_exact(ops, dev):
    g = torch.Generator().manual_seed(21)
    for shape in ((1, 32, 128, 160), (2, 7, 5, 3), (1, 1, 256, 320), (3, 96, 16, 20)):
        x = torch.randn(*shape, generator=g)
        b = torch.randn(shape[1], generator=g)
        for name, fn in (("none", lambda t: t), ("relu", torch.relu), ("sigmoid", torch.sigmoid)):
            none = torch.empty(0, device=dev)
            y = x.to(dev).clone()
            ops.bias_act_(y, b.to(dev), ops.ACTIVATIONS[name], none, ops.RESIDUAL_NONE)
            exp = fn(x + b.view(1, -1, 1, 1))
            assert maxerr(y, exp) <= (0.0 if name != "sigmoid" else 2e-7), (shape, name)
            r = torch.randn(*shape, generator=g)
            y = x.to(dev).clone()
            ops.bias_act_(y, b.to(dev), ops.ACTIVATIONS[name], r.to(dev), ops.RESIDUAL_SAME)       # MnasNet shortcut
            assert maxerr(y, exp + r) <= (0.0 if name != "sigmoid" else 5e-7), (shape, name)
            if shape[2] % 2 == 0 and shape[3] % 2 == 0:
                rh = torch.randn(shape[0], shape[1], shape[2] // 2, shape[3] // 2, generator=g)
                y = x.to(dev).clone()
                ops.bias_act_(y, b.to(dev), ops.ACTIVATIONS[name], rh.to(dev), ops.RESIDUAL_NEAREST_UP2)   # FPN top-down sum
                up = torch.nn.functional.interpolate(rh, size=shape[2:], mode="nearest")
                assert maxerr(y, exp + up) <= (0.0 if name != "sigmoid" else 5e-7), (shape, name)
        y = x.to(dev).clone()
        ops.bias_act_(y, torch.empty(0, device=dev), ops.ACTIVATIONS["relu"], torch.empty(0, device=dev), ops.RESIDUAL_NONE)
        assert maxerr(y, torch.relu(x)) == 0.0


def test_upsample2x_matches_aten(ops, dev):
    g = torch.Generator().manual_seed(22)
    for shape in ((1, 512, 8, 10), (1, 32, 128, 160), (2, 3, 5, 7), (1, 1, 64, 80), (1, 4, 1, 1)):
        x = torch.randn(*shape, generator=g)
        got = ops.upsample2x(x.to(dev))
        exp = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        assert tuple(got.shape) == tuple(exp.shape)
        err = maxerr(got, exp)
        assert err < 5e-6 * max(1.0, exp.abs().max().item()), (shape, err)   # same formula, different FMA contraction
        if shape[3] % 2 == 0:
            # round 6: four outputs per thread where the destination allows 16-byte stores; a destination that is only 4-byte aligned takes the
            # one-output-per-thread kernel -- the same expression per output, so the same bits
            B, C, H, W = shape
            misaligned = torch.empty(B * C * 4 * H * W + 1, device=dev)[1:].view(B, C, 2 * H, 2 * W)
            ops.upsample2x_into(x.to(dev), misaligned)
            assert torch.equal(misaligned, got), shape


def test_paired_upsampling_gives_the_bits_of_the_two_launches(ops, dev):
    """dvmvs_upsample2x_pair_fwd (round 6): a decoder level's feature map and its one-channel depth head (raw convolution output, bias + sigmoid on
    the taps) up-sampled in ONE launch -- channel-slice destinations, batches, and a destination that forces the two-launch fallback."""
    g = torch.Generator().manual_seed(23)
    for (B, C, H, W) in ((1, 128, 32, 40), (2, 5, 6, 8), (1, 32, 128, 160), (1, 3, 5, 7)):
        x, raw, hb = torch.randn(B, C, H, W, generator=g).to(dev), (torch.randn(B, 1, H, W, generator=g) * 2).to(dev), torch.randn(1, generator=g).to(dev)
        cat_two, cat_one = (torch.full((B, C + 3, 2 * H, 2 * W), 7.0, device=dev) for _ in range(2))
        up_two, up_one = (torch.full((B, C, 2 * H, 2 * W), float("nan"), device=dev) for _ in range(2))
        ops.upsample2x_into(x, up_two)
        ops.upsample2x_into(raw, cat_two[:, -1:], hb, ops.ACTIVATIONS["sigmoid"])
        ops.upsample2x_pair_into(x, up_one, raw, cat_one[:, -1:], hb, ops.ACTIVATIONS["sigmoid"])
        assert torch.equal(up_one, up_two) and torch.equal(cat_one, cat_two), (B, C, H, W)
        misaligned = torch.empty(B * C * 4 * H * W + 1, device=dev)[1:].view(B, C, 2 * H, 2 * W)      # 4-byte aligned: the fallback
        ops.upsample2x_pair_into(x, misaligned, raw, cat_one[:, -1:], hb, ops.ACTIVATIONS["sigmoid"])
        assert torch.equal(misaligned, up_two) and torch.equal(cat_one, cat_two)
    with pytest.raises(ValueError):
        ops.upsample2x_pair_into(torch.zeros(1, 4, 8, 8, device=dev), torch.zeros(1, 4, 16, 16, device=dev), torch.zeros(1, 1, 4, 4, device=dev),
                                 torch.zeros(1, 1, 8, 8, device=dev))


def test_fused_modules_match_plain_modules(dev):
    """BN folding + epilogue fusion (what the engine runs) against the untouched modules on the GPU."""
    from dvmvs.engine import fold_batchnorm, fuse_epilogues
    from dvmvs.fusionnet.model import CostVolumeDecoder, FeatureExtractor, FeatureShrinker
    fe = syn.deterministic_init(FeatureExtractor(), 0).eval().to(dev)
    fs = FeatureShrinker().eval().to(dev)
    dec = syn.deterministic_init(CostVolumeDecoder(), 4).eval().to(dev)
    x = syn.smooth_noise((1, 3, 256, 320), seed=5).to(dev)
    with torch.no_grad():
        plain = fs(*fe(x))
        fused = fuse_epilogues(fold_batchnorm(fs))(*fuse_epilogues(fold_batchnorm(fe))(x))
        for a, b in zip(plain, fused):
            assert maxerr(a, b) <= 2e-4 * max(1.0, a.abs().max().item())
        skips = [torch.randn(1, c, 128 // s, 160 // s, device=dev) for c, s in ((32, 1), (64, 2), (128, 4), (256, 8), (512, 16))]
        d_plain = dec(x, *skips)
        d_fused = fuse_epilogues(fold_batchnorm(dec))(x, *skips, full_resolution_only=True)
        assert d_fused[1] is None
        rel = ((d_plain[0] - d_fused[0]).abs() / d_plain[0]).mean().item()
        assert rel < 1e-4


def test_depthwise_conv_matches_torch(ops, dev):
    g = torch.Generator().manual_seed(23)
    none = torch.empty(0, device=dev)
    for (B, C, H, W, k, stride) in ((1, 32, 128, 160, 3, 1), (1, 48, 128, 160, 3, 2), (2, 72, 33, 41, 5, 2), (1, 240, 32, 40, 5, 1),
                                    (1, 1152, 8, 10, 3, 1), (1, 3, 7, 5, 5, 1)):
        x = torch.randn(B, C, H, W, generator=g)
        w = torch.randn(C, 1, k, k, generator=g) * 0.3
        b = torch.randn(C, generator=g)
        for name, fn in (("none", lambda t: t), ("relu", torch.relu), ("sigmoid", torch.sigmoid)):
            got = ops.depthwise_conv(x.to(dev), w.to(dev), b.to(dev), stride, ops.ACTIVATIONS[name], none, False)
            exp = fn(torch.nn.functional.conv2d(x, w, b, stride=stride, padding=k // 2, groups=C))
            assert tuple(got.shape) == tuple(exp.shape)
            assert maxerr(got, exp) < 2e-5 * max(1.0, exp.abs().max().item()), (B, C, H, W, k, stride, name)
        got = ops.depthwise_conv(x.to(dev), w.to(dev), none, stride, 0, none, False)
        assert maxerr(got, torch.nn.functional.conv2d(x, w, None, stride=stride, padding=k // 2, groups=C)) < 2e-5 * 10
        # the preceding 1x1 convolution's epilogue (bias + ReLU) applied to the input taps on the fly; the zero padding stays zero
        pb = torch.randn(C, generator=g)
        got = ops.depthwise_conv(x.to(dev), w.to(dev), b.to(dev), stride, ops.ACTIVATIONS["relu"], pb.to(dev), True)
        exp = torch.relu(torch.nn.functional.conv2d(torch.relu(x + pb.view(1, -1, 1, 1)), w, b, stride=stride, padding=k // 2, groups=C))
        assert maxerr(got, exp) < 2e-5 * max(1.0, exp.abs().max().item()), (B, C, H, W, k, stride, "pre-activated")


# ----------------------------------------------------------------------------------------------------------------------
# destination-passing forms (the frame engine's launch savers)
# ----------------------------------------------------------------------------------------------------------------------
def test_epilogues_write_into_channel_slices(ops, dev):
    """dvmvs_bias_act_fwd / dvmvs_upsample2x_fwd with a channel slice of a larger buffer as destination (what replaces torch.cat),
    batch 1 and batch 2 (batch stride of the big buffer), and the sigmoid -> depth mapping of the decoder's last layer."""
    g = torch.Generator().manual_seed(41)
    for B in (1, 2):
        x = torch.randn(B, 7, 12, 20, generator=g)
        bias = torch.randn(7, generator=g)
        big = torch.full((B, 16, 12, 20), -5.0, device=dev)
        ops.bias_act_into(x.to(dev), big[:, 4:11], bias.to(dev), ops.ACTIVATIONS["relu"])
        exp = torch.relu(x + bias.view(1, -1, 1, 1))
        assert torch.equal(big[:, 4:11].cpu(), exp) and bool((big[:, :4] == -5.0).all()) and bool((big[:, 11:] == -5.0).all())
        r = torch.randn(B, 7, 12, 20, generator=g)
        ops.bias_act_into(x.to(dev), big[:, 9:16], None, ops.ACTIVATIONS["none"], r.to(dev), ops.RESIDUAL_SAME)
        assert maxerr(big[:, 9:16], x + r) == 0.0
        up = torch.full((B, 9, 24, 40), 7.0, device=dev)
        ops.upsample2x_into(x.to(dev), up[:, 1:8])
        ref = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        assert maxerr(up[:, 1:8], ref) < 1e-6 and bool((up[:, 0] == 7.0).all()) and bool((up[:, 8] == 7.0).all())
    # coarse depth heads: sigmoid(conv + bias) applied inside the up-sampler
    raw, hb = torch.randn(1, 1, 16, 20, generator=g) * 2, torch.randn(1, generator=g)
    cat = torch.zeros(1, 5, 32, 40, device=dev)
    ops.upsample2x_into(raw.to(dev), cat[:, -1:], hb.to(dev), ops.ACTIVATIONS["sigmoid"])
    exp = torch.nn.functional.interpolate(torch.sigmoid(raw + hb.view(1, 1, 1, 1)), scale_factor=2, mode="bilinear", align_corners=True)
    assert maxerr(cat[:, -1:], exp) < 1e-6 and float(cat[:, :4].abs().max()) == 0.0
    # last decoder layer: depth = 1 / (multiplier * sigmoid(conv + bias) + base)   (fusionnet/model.py:231-232, 297-303)
    y = torch.randn(1, 1, 256, 320, generator=g) * 3
    b1 = torch.randn(1, generator=g)
    mult, base = 1 / 0.25 - 1 / 20.0, 1 / 20.0
    store = torch.zeros(1, 256, 320, device=dev)
    ops.bias_act_into(y.to(dev), store.view(1, 1, 256, 320), b1.to(dev), ops.ACTIVATION_SIGMOID_TO_DEPTH, p0=mult, p1=base)
    exp = 1.0 / (mult * torch.sigmoid(y + b1.view(1, 1, 1, 1)) + base).squeeze(1)
    assert float(((store.cpu() - exp).abs() / exp).max()) < 2e-6
    with pytest.raises(ValueError):
        ops.bias_act_into(y.to(dev), torch.zeros(1, 1, 256, 320, device=dev)[:, :, ::2], None, 0)   # not a channel slice


def test_state_updates_in_place(ops, dev):
    """lstm_gates_into (c and h updated in their own buffers) and depth_reproject_lowres_into (z-buffer left all-zero) equal the
    allocating ops bit for bit."""
    g = torch.Generator().manual_seed(43)
    cc, c0 = torch.randn(2, 2048, 8, 10, generator=g).to(dev), torch.randn(2, 512, 8, 10, generator=g).to(dev)
    h_ref, c_ref = ops.lstm_gates(cc, c0)
    c_state, h_state = c0.clone(), torch.full_like(c0, 9.0)
    ops.lstm_gates_into(cc, c_state, h_state)
    assert torch.equal(c_state, c_ref) and torch.equal(h_state, h_ref)
    fullK = syn.full_K()
    halfK = syn.scaled_K(fullK, 2.0)
    prev = syn.analytic_depth()
    full, low = hipcall.depth_reproject(ops, syn.pose(10), syn.pose(9), *to(dev, prev, fullK, halfK), 16)
    from dvmvs import pose_algebra
    T = pose_algebra.relative_pose(syn.pose(10), syn.pose(9), dev)
    zbuffer, estimate = torch.zeros(1, 128, 160, device=dev), torch.full((1, 1, 8, 10), -1.0, device=dev)
    for _ in range(3):     # repeated use of the same z-buffer: it must come back all-zero every time
        ops.depth_reproject_lowres_into(T, prev.to(dev), fullK.to(dev), halfK.to(dev), zbuffer, estimate, 16)
        assert torch.equal(estimate, low) and float(zbuffer.abs().max()) == 0.0
    # ABI 6: the frame path's one-launch form -- straight into the 8x10 estimate, two buffers alternating, each launch zero-fills the other one
    est = [torch.zeros(1, 1, 8, 10, device=dev), torch.full((1, 1, 8, 10), 7.0, device=dev)]
    for n in range(4):
        cur, other = est[n % 2], est[1 - n % 2]
        ops.depth_reproject_estimate_into(T, prev.to(dev), fullK.to(dev), halfK.to(dev), cur, other, 16)
        assert torch.equal(cur, low) and float(other.abs().max()) == 0.0, n
    with pytest.raises(ValueError):
        ops.depth_reproject_estimate_into(T, prev.to(dev), fullK.to(dev), halfK.to(dev), est[0], est[0], 16)
    dst = torch.zeros(1, 1024, 8, 10, device=dev)
    hw = load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), "hidden_warp")
    h0 = syn.analytic_lstm_inputs()[2]
    lK = syn.scaled_K(syn.full_K(), 32.0)
    args = to(dev, h0, torch.from_numpy(hw["depth_masked"]), torch.from_numpy(hw["T"]), lK)
    ops.hidden_warp_into(*args, True, dst[:, 512:])
    assert torch.equal(dst[:, 512:], ops.hidden_warp(*args, True)) and float(dst[:, :512].abs().max()) == 0.0


def test_destination_passing_engine_equals_the_concatenating_one(dev):
    """The headline engine (one sequence, BN folded, epilogues fused, every producer writing into its consumer's buffer) against
    the same engine with torch.cat / copy_ launches (direct = False): same convolutions, same kernels, same arithmetic -- the depth
    must agree to float32 round-off (measured 2.6e-6 rel-L1)."""
    from dvmvs.engine import DepthEngine
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    ctors = (FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)
    mods = syn.build_e2e_modules(ctors)
    direct = DepthEngine(*mods, device=dev, use_graphs=False, conv_plans=False)
    plain = DepthEngine(*mods, device=dev, use_graphs=False, conv_plans=False)
    assert direct.direct
    plain.direct = False
    fullK = syn.full_K()
    for n, (r, ms) in enumerate(list(syn.E2E_FRAMES) + [(12, (11, 9))]):
        args = (syn.e2e_image(r).to(dev), syn.pose(r), [syn.e2e_image(i).to(dev) for i in ms], [syn.pose(i) for i in ms], fullK)
        a = direct.step(*args, frame_id=r, measurement_ids=list(ms)).clone()
        b = plain.step(*args, frame_id=r, measurement_ids=list(ms)).clone()
        err = float(((a - b).abs() / b).mean())
        print(f"frame {n}: destination-passing vs concatenating engine, depth rel-L1 {err:.3e}")
        assert err <= 1e-5, (n, err)     # measured 2.6e-6: MIOpen picks per-call algorithms for the differently placed buffers
        assert float((direct._static["h"] - plain._static["h"]).abs().max()) <= 1e-3


def test_engine_with_epilogues_inside_miopen_equals_the_two_launch_engine(dev):
    """DepthEngine(conv_plans=True) -- the default: per convolution problem the epilogue rides inside MIOpen's kernel where that
    gives the SAME BITS as convolution + dvmvs_bias_act_fwd and was measured faster at warm-up -- against conv_plans=False (two
    launches everywhere), eagerly and through the captured graph.  A plan whose probe output differs in any bit is never taken
    (round 3 took whichever was faster in a 3-round timing: the arithmetic depended on timing noise)."""
    from dvmvs.engine import DepthEngine
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    ctors = (FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)
    mods = syn.build_e2e_modules(ctors)
    # (pointwise_convs=False: since round 6 the 1x1 layers -- the last ones MIOpen ran in a default engine -- have their own kernel with the epilogue
    # in its store path, csrc/pointwise_conv.hip; without it they are the problems the plans are decided for)
    planned = DepthEngine(*mods, device=dev, use_graphs=True, conv_plans=True, pointwise_convs=False)
    plain = DepthEngine(*mods, device=dev, use_graphs=True, conv_plans=False, pointwise_convs=False)
    assert planned.conv_plans and not plain.conv_plans
    fullK = syn.full_K()
    frames = list(syn.E2E_FRAMES) + [(12, (11, 9)), (13, (12, 10)), (14, (13, 11))]       # the later ones replay the captured graph
    for n, (r, ms) in enumerate(frames):
        args = (syn.e2e_image(r).to(dev), syn.pose(r), [syn.e2e_image(i).to(dev) for i in ms], [syn.pose(i) for i in ms], fullK)
        a = planned.step(*args, frame_id=r, measurement_ids=list(ms)).clone()
        b = plain.step(*args, frame_id=r, measurement_ids=list(ms)).clone()
        err = float(((a - b).abs() / b).mean())
        print(f"frame {n}: epilogues inside MIOpen vs two launches, depth rel-L1 {err:.3e}")
        assert err <= 1e-5, (n, err)
    report = planned.conv_plan_report()
    chosen = [row for row in report if row[2]]
    for shape, wshape, use, t_plan, t_two, diff in sorted(report, key=lambda row: -row[4] if row[4] == row[4] else 0):
        print(f"  in {shape} w {wshape}: plan {t_plan:7.2f} us, two launches {t_two:7.2f} us, max|diff| {diff:.1e} -> {'plan' if use else 'two launches'}")
    print(f"{len(chosen)} of {len(report)} dense convolution problems take the MIOpen fusion plan")
    assert report and not plain.conv_plan_report()
    for row in chosen:
        assert row[5] == 0.0           # against the two-launch result of the same layer: bit-identical or not taken
    for row in report:
        if row[5] == row[5] and row[5] != 0.0:
            assert not row[2], row     # a differently-rounded plan is rejected however fast it is


def test_cost_volume_backward_is_bit_reproducible(ops, dev):
    """SURVEY section 5 / VERDICT r2: rounds 1-2 computed the measurement-feature gradient as an atomic scatter whose summation
    order varied from run to run (stated bound 1e-5 of the largest entry).  Since round 3 both gradients are gathers without
    atomics: at the training feature size (128x128, 32 channels, 64 planes) repeated runs must agree bit for bit."""
    g = torch.Generator().manual_seed(77)
    f1 = torch.randn(2, 32, 128, 128, generator=g).to(dev)
    f2 = torch.randn(2, 32, 128, 128, generator=g).to(dev)
    go = torch.randn(2, 64, 128, 128, generator=g).to(dev)
    K = torch.cat([syn.scaled_K(syn.full_K(width=256, height=256), 2.0)] * 2)
    p1, p2 = torch.cat([syn.pose(10), syn.pose(202)]), torch.cat([syn.pose(9), syn.pose(196)])     # an easy pair and a spilling one
    runs = []
    for _ in range(4):
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        hipcall.cost_volume(ops, a, [b], p1, [p2], K, 0.25, 20.0, 64, True, 0).backward(go)
        runs.append((a.grad.clone(), b.grad.clone()))
    scale = runs[0][1].abs().max().item()
    worst = 0.0
    for ga, gb in runs[1:]:
        assert torch.equal(ga, runs[0][0])
        worst = max(worst, (gb - runs[0][1]).abs().max().item())
    print(f"measurement-feature gradient, run-to-run max |diff| {worst:.3e} of max |g| {scale:.3e} = {worst / scale:.2e}")
    assert worst == 0.0
