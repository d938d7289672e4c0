"""GPU: the TSDF ray-caster (csrc/tsdf_raycast.hip, dvmvs.hip.ops.tsdf_raycast, TSDFVolume.render, python -m dvmvs.tsdf
--render_keyframes) against the float64 restatement of its definition (tests/raycast_reference.py).

On unambiguous pixels (the rule is in raycast_reference.py; the caps on its use are checked on the CPU) hit / miss equals the float64
reference's, depth and normals are as accurate as the float32 restatement (accuracy.as_accurate_as_reference: no tolerance constant
of their own) and colours are equal.  On ambiguous pixels the depth is 0 or a finite depth inside the range; their share is printed."""
import os

import numpy as np
import pytest
import torch

import raycast_reference as rr
from accuracy import as_accurate_as_reference

pytestmark = pytest.mark.gpu

ALL_CASES = sorted(rr.CASES)


def get_case(name):
    return rr.oracle_case(int(name[-1])) if name.startswith("oracle") else rr.case(name)


def device_volume(vol, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (vol.tsdf, vol.weight, vol.color))


def render(c, dev, skip_empty=True, views=None, **options):
    """The op on a case's volume and views; ``views``: indices (default all)."""
    from dvmvs.hip import ops
    tsdf, weight, color = device_volume(c.vol, dev)
    poses = torch.from_numpy(c.poses if views is None else c.poses[list(views)]).to(dev)
    K = torch.from_numpy(np.broadcast_to(c.K, (len(c.poses), 3, 3)).copy() if c.K.ndim == 2 else c.K)
    K = (K if views is None else K[list(views)]).to(dev)
    mask = ops.tsdf_raycast_mask(tsdf, weight) if skip_empty else None
    kwargs = dict(c.kwargs, **options)
    return ops.tsdf_raycast(tsdf, weight, color, c.vol.origin, c.vol.voxel_size, K, poses, c.image[0], c.image[1], mask=mask, **kwargs)


@pytest.mark.parametrize("name", ALL_CASES + ["oracle_2"])
def test_matches_the_float64_reference(hip_device, name):
    c = get_case(name)
    depth, normal, rgb = (t.cpu().numpy() for t in render(c, hip_device))
    r32, r64 = c.ref32, c.ref64
    near, far = c.kwargs.get("near", 0.0), c.kwargs.get("far", np.inf)
    assert depth.shape == r64.depth.shape and normal.shape == r64.normal.shape and rgb.shape == r64.rgb.shape and rgb.dtype == np.uint8
    for i in range(len(depth)):
        clear, amb = ~r64.ambiguous[i], r64.ambiguous[i]
        hit = depth[i] != 0
        print(f"{name} view {i}: {100 * amb.mean():.2f} % ambiguous pixels, {100 * hit.mean():.1f} % hits (reference {100 * r64.hit[i].mean():.1f} %), "
              f"max |depth - float64| {np.abs(depth[i] - r64.depth[i])[clear].max():.2e} m (float32 restatement "
              f"{np.abs(r32.depth[i] - r64.depth[i])[clear].max():.2e})")
        assert np.array_equal(hit[clear], r64.hit[i][clear])
        both = clear & r64.hit[i]
        as_accurate_as_reference(torch.from_numpy(depth[i][both]), torch.from_numpy(r32.depth[i][both]), torch.from_numpy(r64.depth[i][both]))
        for_normals = both & ~r64.normal_excluded[i]
        as_accurate_as_reference(torch.from_numpy(normal[i][for_normals]), torch.from_numpy(r32.normal[i][for_normals]),
                                 torch.from_numpy(r64.normal[i][for_normals]))
        for_colours = both & ~r64.colour_excluded[i]
        assert np.array_equal(rgb[i][for_colours], r64.rgb[i][for_colours])
        # misses carry nothing; ambiguous pixels are a miss or a finite depth inside the range
        assert not normal[i][~hit].any() and not rgb[i][~hit].any()
        d = depth[i][amb]
        assert (np.isfinite(d) & ((d == 0) | ((d >= np.float32(max(near, 0.0))) & (d <= np.float32(far))))).all()
        assert np.isfinite(depth[i]).all() and np.isfinite(normal[i]).all()


@pytest.mark.parametrize("name", [n for n in ALL_CASES if n.startswith("plane")])
def test_known_answer_plane(hip_device, name):
    """The kernel against the closed-form ray-plane depth, by the same criterion (the float32 restatement's own distance from it)."""
    c = get_case(name)
    depth = render(c, hip_device, normals=False, colour=False)[0].cpu().numpy()
    for i, pose in enumerate(c.poses):
        closed = rr.plane_depth(c.vol, c.K, pose, *c.image)
        both = ~c.ref64.ambiguous[i] & c.ref64.hit[i]
        assert both.mean() >= rr.HIT_FLOOR
        as_accurate_as_reference(torch.from_numpy(depth[i][both]), torch.from_numpy(c.ref32.depth[i][both]), torch.from_numpy(closed[both]))


@pytest.mark.parametrize("name", ALL_CASES + ["oracle_2", "oracle_1"])
def test_skipping_empty_space_changes_no_bit(hip_device, name):
    from dvmvs.hip import ops
    c = get_case(name)
    tsdf, weight, _ = device_volume(c.vol, hip_device)
    mask = ops.tsdf_raycast_mask(tsdf, weight).cpu().numpy()
    # the mask is what its definition says -- and it leaves something to skip and something to march through
    assert np.array_equal(mask, rr.brick_mask(c.vol.tsdf, c.vol.weight)) and mask.any() and not mask.all()
    for step in (0.5, 1.0, 2.0):
        dense, skipped = render(c, hip_device, skip_empty=False, step=step), render(c, hip_device, skip_empty=True, step=step)
        for a, b in zip(dense, skipped):
            assert torch.equal(a, b)
        assert bool((dense[0] > 0).any())


def test_views_in_one_launch_equal_single_launches_and_repeat(hip_device):
    for name in ("plane_odd_n3_half_step", "sphere_odd_n3"):
        c = get_case(name)
        batch, again = render(c, hip_device), render(c, hip_device)
        for a, b in zip(batch, again):
            assert torch.equal(a, b)                       # run to run
        for i in range(len(c.poses)):
            single = render(c, hip_device, views=[i])
            for a, b in zip(batch, single):
                assert torch.equal(a[i], b[0])             # N = 3 in one call against three calls


def test_degenerate_inputs_give_zeros_and_leave_the_stream_usable(hip_device):
    from types import SimpleNamespace
    c = get_case("plane_small_n3")
    K = rr.intrinsics(rr.IMAGE_B)
    bad_pose = np.stack([rr.view("frontal")] * 4)
    bad_pose[0, 0, 3], bad_pose[1, 1, 1], bad_pose[2, :3, :3] = np.nan, np.inf, 0.0
    bad_K = np.stack([K] * 4)
    bad_K[3, 0, 0] = 0.0
    cases = [SimpleNamespace(vol=rr.empty_volume(rr.DIMS_SMALL), K=K, poses=np.stack([rr.view("frontal"), rr.view("yaw-inside")]), image=rr.IMAGE_B, kwargs={}),
             SimpleNamespace(vol=c.vol, K=K, poses=rr.view("away")[None], image=rr.IMAGE_B, kwargs={}),
             SimpleNamespace(vol=c.vol, K=bad_K, poses=bad_pose, image=rr.IMAGE_B, kwargs={}),
             SimpleNamespace(vol=c.vol, K=K, poses=rr.view("frontal")[None], image=rr.IMAGE_B, kwargs={"near": 0.5, "far": 0.2})]
    for case in cases:
        for skip_empty in (True, False):
            depth, normal, rgb = render(case, hip_device, skip_empty=skip_empty)
            assert not bool(depth.any()) and not bool(normal.any()) and not bool(rgb.any())
    depth = render(c, hip_device)[0]                       # the next launch on the stream
    torch.cuda.synchronize()
    clear = ~c.ref64.ambiguous
    assert np.array_equal((depth.cpu().numpy() != 0)[clear], c.ref64.hit[clear])


def oracle_frames_volume(dev, n_frames):
    from dvmvs.tsdf import TSDFVolume
    src = rr.oracle_volume(2)
    vol = TSDFVolume(src.bounds.copy(), src.voxel_size, device=dev)
    for n, (rgb, depth, K, pose) in enumerate(src.frames[:n_frames]):
        vol.integrate(rgb, depth, K, pose, obs_weight=1.0 + n)
    return vol, src


def test_render_rebuilds_its_mask_after_integrate(hip_device):
    """Render the still empty volume (which caches a mask without a single flagged brick), integrate a frame, render, integrate one
    more, render again: each result is that of a fresh volume holding the same data and that of the dense march.  A mask kept from
    before an ``integrate`` would differ: every brick the frame's surface lies in is unflagged in the older mask
    (tests/test_raycast_reference.py checks that on the CPU), so its rays would jump over the surface."""
    from dvmvs.tsdf import TSDFVolume
    src = rr.oracle_volume(2)
    K = np.stack([f[2] for f in src.frames])
    poses = np.stack([f[3] for f in src.frames])
    h, w = src.frames[0][1].shape
    vol = TSDFVolume(src.bounds.copy(), src.voxel_size, device=hip_device)
    before = vol.render(K, poses, h, w)
    assert not bool(before[0].any())
    for n, (rgb, depth, Kf, pose) in enumerate(src.frames):
        vol.integrate(rgb, depth, Kf, pose, obs_weight=1.0 + n)
        after = vol.render(K, poses, h, w)
        fresh_vol, _ = oracle_frames_volume(hip_device, n + 1)
        fresh, dense = fresh_vol.render(K, poses, h, w), vol.render(K, poses, h, w, skip_empty=False)
        for a, b, c in zip(after, fresh, dense):
            assert torch.equal(a, b) and torch.equal(a, c)
        assert not torch.equal(before[0], after[0])        # the frame changed the view
        # the device volume is the oracle's, so the reference of scene (c) applies to render() as it stands
        ref = rr.oracle_case(n + 1).ref64
        clear = ~ref.ambiguous
        assert np.array_equal((after[0].cpu().numpy() != 0)[clear], ref.hit[clear])
        before = after


def test_ops_reject_bad_tensors(hip_device):
    from dvmvs.hip import ops
    c = get_case("plane_small_n3")
    tsdf, weight, color = device_volume(c.vol, hip_device)
    K = torch.from_numpy(np.stack([c.K] * 3)).to(hip_device)
    poses = torch.from_numpy(c.poses).to(hip_device)
    mask = ops.tsdf_raycast_mask(tsdf, weight)

    def call(tsdf=tsdf, weight=weight, color=color, K=K, poses=poses, **kw):
        return ops.tsdf_raycast(tsdf, weight, color, c.vol.origin, c.vol.voxel_size, K, poses, 8, 8, **kw)

    for bad in (dict(tsdf=tsdf.double()), dict(weight=weight.half()), dict(color=color[:, :, :-1]), dict(tsdf=tsdf.transpose(0, 1)),
                dict(weight=weight[::2]), dict(tsdf=tsdf[:1], weight=weight[:1], color=color[:1]), dict(color=None),
                dict(K=K[:2]), dict(K=K.double()), dict(poses=poses[:, :3]), dict(K=K[0]),
                dict(mask=mask[:-1]), dict(mask=mask.float()), dict(mask=mask.transpose(0, 2)), dict(step=0.0), dict(near=-0.5)):
        with pytest.raises(ValueError):
            call(**bad)
    assert call(color=None, colour=False)[2] is None
    for bad in (dict(out=mask[:-1]), dict(out=mask.int()), dict(out=mask.transpose(0, 2))):
        with pytest.raises(ValueError):
            ops.tsdf_raycast_mask(tsdf, weight, **bad)
    with pytest.raises(ValueError):
        ops.tsdf_raycast_mask(tsdf.transpose(0, 2), weight.transpose(0, 2))
    with pytest.raises(ValueError):
        ops.tsdf_raycast_mask(tsdf, weight.double())
    assert torch.equal(ops.tsdf_raycast_mask(tsdf, weight, out=torch.empty_like(mask)), mask)


def test_render_surface(hip_device):
    vol, src = oracle_frames_volume(hip_device, 2)
    rgb, depth, K, pose = src.frames[0]
    h, w = depth.shape
    d, n, c = vol.render(K, pose, h, w)                                   # one numpy K, one numpy pose
    assert d.shape == (1, h, w) and n.shape == (1, h, w, 3) and c.shape == (1, h, w, 3) and c.dtype == torch.uint8 and d.is_cuda
    poses = torch.from_numpy(np.stack([f[3] for f in src.frames])).float().to(hip_device)
    d2, n2, c2 = vol.render(torch.from_numpy(K).to(hip_device), poses, h, w, normals=False, colour=False)       # tensors, one K for two poses
    assert d2.shape == (2, h, w) and n2 is None and c2 is None and torch.equal(d2[0], d[0])
    unit = n.norm(dim=-1)
    assert bool(((unit - 1).abs()[unit > 0] < 1e-5).all()) and bool((unit > 0).any())
    for bad in (dict(step=0.0), dict(step=5.5), dict(near=-1.0), dict(far=float("nan"))):
        with pytest.raises(ValueError):
            vol.render(K, pose, h, w, **bad)
    with pytest.raises(ValueError):
        vol.render(K, np.eye(3), h, w)
    with pytest.raises(ValueError):
        vol.render(np.stack([K] * 3), np.stack([pose] * 2), h, w)


def test_round_trip_of_one_frame(hip_device):
    """One frame integrated, rendered from its own pose: the rendered depth tracks the input depth.  The bound is the float64
    reference's own deviation from the input on this scene (integrate projects every voxel to its NEAREST pixel) times 1.5, computed
    here from the reference, never from the kernel."""
    vol, src = oracle_frames_volume(hip_device, 1)
    rgb, depth_in, K, pose = src.frames[0]
    h, w = depth_in.shape
    ref = rr.oracle_case(1).ref64
    seen = ref.hit[0] & ~ref.ambiguous[0] & (depth_in > 0)
    ref_dev = np.abs(ref.depth[0] - depth_in)[seen].max()
    got = vol.render(K, pose, h, w)[0][0].cpu().numpy()
    dev = np.abs(got - depth_in)[seen].max()
    print(f"round trip: {seen.sum()} of {seen.size} pixels, max |rendered - input| = {dev * 1e3:.3f} mm, float64 reference {ref_dev * 1e3:.3f} mm")
    assert seen.mean() >= rr.HIT_FLOOR and 0 < ref_dev < 0.5 * src.voxel_size
    assert (got[seen] > 0).all() and dev <= 1.5 * ref_dev


def test_program_renders_keyframes(hip_device, golden_dir, tmp_path):
    """``python -m dvmvs.tsdf --render_keyframes`` on two keyframes of the sample scene (their depth maps as 'predictions'): writes the
    <system>+tsdf predictions and errors next to the meshes; without the flag the program writes exactly what it wrote before."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.tsdf import main
    src = os.path.join(golden_dir, "sample_scene")
    scene = tmp_path / "data" / "hololens-dataset" / "000"
    (scene / "images").mkdir(parents=True)
    (scene / "depth").mkdir()
    names = ["00012.png", "00013.png"]
    for name in names:
        Image.open(os.path.join(src, "images", name)).save(scene / "images" / name)
        Image.open(os.path.join(src, "depth", name)).save(scene / "depth" / name)
    np.savetxt(scene / "poses.txt", np.loadtxt(os.path.join(golden_dir, "hololens_000_poses.txt")).reshape(-1, 16)[[9, 10]])
    np.savetxt(scene / "K.txt", np.loadtxt(os.path.join(golden_dir, "hololens_000_K.txt")))
    (tmp_path / "data" / "indices").mkdir()
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("00012.png 00009.png\nTRACKING LOST\n00013.png 00012.png\n")
    preds = np.stack([resize_nearest(load_depth_png(os.path.join(src, "depth", n)), 320, 256) for n in names]).astype(np.float32)
    (tmp_path / "pred").mkdir()
    np.savez(tmp_path / "pred" / "keyframe_hololens-dataset_320_256_3_dvmvs_fusionnet_online_predictions_000.npz", preds)
    written = {}
    for tag, flag in (("plain", []), ("rendered", ["--render_keyframes"])):
        out = tmp_path / tag
        main(["--reconstruction_folder", str(out), "--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"),
              "--voxel_size", "0.05"] + flag)
        written[tag] = {w: open(out / w, "rb").read() for w in sorted(os.listdir(out))}
    assert len(written["plain"]) == 1 and all(w.endswith("_complete.ply") for w in written["plain"])
    system = "keyframe_hololens-dataset_320_256_3_dvmvs_fusionnet_online+tsdf"
    extra = {system + "_predictions_000.npz", system + "_errors_000.npz"}
    assert set(written["rendered"]) == set(written["plain"]) | extra
    for w, data in written["plain"].items():
        assert written["rendered"][w] == data
    fused = np.load(tmp_path / "rendered" / (system + "_predictions_000.npz"))["arr_0"]
    errors = np.load(tmp_path / "rendered" / (system + "_errors_000.npz"))["arr_0"]
    assert fused.shape == preds.shape and fused.dtype == np.float32 and errors.shape == (2, 8)
    hit = fused > 0
    print(f"fused keyframe depth: {100 * hit.mean():.1f} % of the pixels hit a surface; mean abs error against the depth maps {errors[:, 0]}")
    assert hit.mean() > 0.2 and np.isfinite(errors).all()
    # the fused depth of views whose own depth went into the volume stays close to it (5 cm voxels)
    both = hit & (preds > 0)
    assert np.median(np.abs(fused - preds)[both]) < 0.05
