"""GPU: ray-casting ``dvmvs.tsdf.SparseTSDFVolume`` straight from its pool (csrc/sparse_raycast.hip).  The
yardstick is existing code -- ``volume.dense(box).render(...)`` with the same arguments -- and "equal" is ``torch.equal`` on depth, normals
and colours; one test holds the sparse image to the float64 restatement of the definition directly (tests/raycast_reference.py)."""
import os

import numpy as np
import pytest
import torch

import raycast_reference as rr
import sparse_scene as sc
import tsdf_fuse_scene
from accuracy import as_accurate_as_reference
from dvmvs import sparse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = ((24, 32), (17, 23))              # both leave partial 8x8 tiles
CUT_FIRST, CUT_LAST = (5, 5, 4), (9, 8, 18)
MARCHES = ({}, {"step": 0.5}, {"step": 2.0}, {"near": 0.9, "far": 1.5}, {"skip_empty": False}, {"step": 2.0, "skip_empty": False},
           {"near": 0.9, "far": 1.5, "skip_empty": False, "step": 0.5})


@pytest.fixture(scope="module")
def scene():
    depth, rgb = sc.frames()
    return {"depth": depth, "rgb": rgb, "poses": sc.poses(), "K": sc.K}


def make(max_bricks=1024, origin=None):
    from dvmvs.tsdf import SparseTSDFVolume
    return SparseTSDFVolume(sc.VOXEL, origin=sc.BOX_ORIGIN if origin is None else origin, max_bricks=max_bricks, device=DEV)


def feed(volume, scene, views, split, poses=None):
    poses = scene["poses"] if poses is None else poses
    first = 0
    for n in split:
        part = list(views[first:first + n])
        volume.integrate_frames(scene["rgb"][part], scene["depth"][part], scene["K"], poses[part], max_depth=5.0)
        first += n
    assert first == len(views)


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def hit_shares(depth):
    return [float((d != 0).float().mean()) for d in depth]


@pytest.fixture(scope="module")
def six_frames(scene):
    """Six frames in one flush on the lattice that starts at the box, and its dense yardsticks by box: shared, never written."""
    volume = make()
    feed(volume, scene, range(6), (6,))
    assert volume.n_bricks == 306 and volume.overflow == 0
    boxes = {"no bounds": None, "the scene's box": sc.box_bounds(), "a box cut through the surface": volume.brick_bounds(CUT_FIRST, CUT_LAST)}
    return volume, boxes, {name: volume.dense(bounds) for name, bounds in boxes.items()}


@pytest.mark.parametrize("box", ["no bounds", "the scene's box", "a box cut through the surface"])
def test_scene_from_its_own_poses_equals_the_dense_render(scene, six_frames, box):
    volume, boxes, yardsticks = six_frames
    bounds, dense = boxes[box], yardsticks[box]
    coords = volume.bricks()[0]
    if box == "a box cut through the surface":
        assert tuple(dense._tsdf.shape) == tuple(8 * (b - a + 1) for a, b in zip(CUT_FIRST, CUT_LAST))
        for a in range(3):      # allocated bricks lie outside the box on every side
            assert (coords[:, a] < CUT_FIRST[a]).any() and (coords[:, a] > CUT_LAST[a]).any()
    elif box == "the scene's box":
        assert tuple(dense._tsdf.shape) == sc.BOX_DIMS and (coords.min(axis=0) >= 1).all() and (coords.max(axis=0) <= sc.BOX_BRICKS - 2).all()
    for height, width in SIZES:
        K = tsdf_fuse_scene.scaled_K(height, width)
        for march in MARCHES:
            want = dense.render(K, scene["poses"], height, width, **march)
            got = volume.render(K, scene["poses"], height, width, bounds=bounds, **march)
            shares = hit_shares(want[0])
            print(f"{box} {height}x{width} {march}: hits per view {[round(100 * s, 1) for s in shares]} %")
            assert same(got, want), (box, height, width, march)
            if "near" not in march:
                assert min(shares) >= rr.HIT_FLOOR      # the yardstick sees the surface in every view, on every box
            else:
                # near / far are there to cut the march short of part of the surface (depth 0.8 .. 1.8 m), so these renders hit less by
                # construction and the floor, which is for views meant to see the surface, is not theirs: every view must still hit
                assert min(shares) > 0.0
    # depth alone, and depth with one of the two
    K = sc.K
    for normals, colour in ((False, False), (True, False), (False, True)):
        want = dense.render(K, scene["poses"], sc.HEIGHT, sc.WIDTH, normals=normals, colour=colour)
        got = volume.render(K, scene["poses"], sc.HEIGHT, sc.WIDTH, bounds=bounds, normals=normals, colour=colour)
        assert (got[1] is None) == (not normals) and (got[2] is None) == (not colour) and same(got, want)


def test_held_to_the_float64_reference(scene, six_frames):
    """The sparse image against ``raycast_reference.raycast(..., float64)`` on the arrays of ``dense(box)``: hit / miss equal on unambiguous
    pixels, depth and normals as accurate as the float32 restatement, colours equal."""
    volume, boxes, yardsticks = six_frames
    dense = yardsticks["the scene's box"]
    views = [sc.POSE_NAMES.index(v) for v in ("front", "inside", "graze", "tilt", "far")]
    poses = scene["poses"][views]
    arrays = (dense._tsdf.cpu().numpy(), dense._weight.cpu().numpy(), dense._color.cpu().numpy(), dense._vol_origin, dense._voxel_size)
    r32 = rr.raycast(*arrays, sc.K, poses, sc.HEIGHT, sc.WIDTH, dtype=np.float32)
    r64 = rr.raycast(*arrays, sc.K, poses, sc.HEIGHT, sc.WIDTH, dtype=np.float64)
    shares = rr.check_caps(r64)
    depth, normal, rgb = (t.cpu().numpy() for t in volume.render(sc.K, poses, sc.HEIGHT, sc.WIDTH, bounds=boxes["the scene's box"]))
    for i in range(len(views)):
        amb, hits, n_ex, c_ex = shares[i]
        print(f"view {sc.POSE_NAMES[views[i]]}: {100 * amb:.2f} % ambiguous, {100 * hits:.1f} % hits, {100 * n_ex:.2f} % / {100 * c_ex:.2f} % excluded")
        clear = ~r64.ambiguous[i]
        assert np.array_equal((depth[i] != 0)[clear], r64.hit[i][clear])
        both = clear & r64.hit[i]
        as_accurate_as_reference(torch.from_numpy(depth[i][both]), torch.from_numpy(r32.depth[i][both]), torch.from_numpy(r64.depth[i][both]))
        for_normals = both & ~r64.normal_excluded[i]
        as_accurate_as_reference(torch.from_numpy(normal[i][for_normals]), torch.from_numpy(r32.normal[i][for_normals]),
                                 torch.from_numpy(r64.normal[i][for_normals]))
        for_colours = both & ~r64.colour_excluded[i]
        assert np.array_equal(rgb[i][for_colours], r64.rgb[i][for_colours])
        assert not normal[i][depth[i] == 0].any() and not rgb[i][depth[i] == 0].any()


def fill_with_noise(volume, n, seed):
    """tsdf <- uniform [-1, 1], colour <- folded integers < 2^24, weight <- 1 in the first n pool slots, then a seeded 10 % of the voxels
    get weight 0; in place.  Every face, edge and corner of every brick then carries crossings and validity changes."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    tsdf, weight, colour = volume.pool()
    tsdf[:n] = torch.rand((n, 512), generator=gen, device=DEV) * 2.0 - 1.0
    colour[:n] = torch.randint(0, 1 << 24, (n, 512), generator=gen, device=DEV).float()
    weight[:n] = (torch.rand((n, 512), generator=gen, device=DEV) >= 0.1).float()


def test_noise_pool_every_face_edge_and_corner(scene):
    volume = make()
    feed(volume, scene, range(6), (6,))
    fill_with_noise(volume, volume.n_bricks, 1)
    dense = volume.dense(sc.box_bounds())
    for march in ({}, {"skip_empty": False}, {"step": 0.5}):
        want = dense.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, **march)
        got = volume.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, bounds=sc.box_bounds(), **march)
        assert same(got, want) and min(hit_shares(want[0])) > 0.2
        assert bool((want[1].abs().sum(-1) == 0)[want[0] != 0].any()) and bool((want[1].abs().sum(-1) > 0).any())      # normals kept and dropped


BLOCK2 = [(x, y, z) for x in (2, 3) for y in (2, 3) for z in (2, 3)]
LAYOUTS = {
    "one brick": [(2, 2, 2)],
    "two sharing a face": [(2, 2, 2), (2, 3, 2)],
    "two sharing an edge": [(2, 2, 2), (3, 2, 3)],
    "two sharing a corner": [(2, 2, 2), (3, 3, 3)],
    "2x2x2 minus one": [b for b in BLOCK2 if b != (2, 3, 2)],
    "3x3x3 minus its centre": [(x, y, z) for x in (2, 3, 4) for y in (2, 3, 4) for z in (2, 3, 4) if (x, y, z) != (3, 3, 3)],
    "2x2x2 minus one, slots in descending key order": [b for b in BLOCK2 if b != (2, 3, 2)][::-1],
}


def look_at(eye, target):
    """float32 camera-to-world: the camera at ``eye`` looks along +z at ``target``."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross([0.0, 1.0, 0.13], z)
    x /= np.linalg.norm(x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, np.cross(z, x), z, eye
    return pose.astype(np.float32)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_hand_made_layouts(name):
    """``pool_key[:n]``, ``status[0]`` and noise written directly into a fresh state: the volume's hash table stays empty, and is not read."""
    coords = np.array(LAYOUTS[name])
    n = len(coords)
    volume = make(32)
    state = volume._state
    state.pool_key[:n] = torch.from_numpy(sparse.pack_keys(coords)).to(DEV)
    state.status[0] = n
    fill_with_noise(volume, n, 2 + n)
    assert np.array_equal(volume.bricks()[0], coords)
    bounds = volume.brick_bounds((0, 0, 0), coords.max(axis=0) + 1)
    dense = volume.dense(bounds)
    brick = 8 * sc.VOXEL
    o = sc.BOX_ORIGIN.astype(np.float64)
    centre = o + 3.5 * brick                   # the centre of brick (3, 3, 3): the missing one of the 3x3x3 layout
    first = o + 2.5 * brick                    # the centre of brick (2, 2, 2): in every layout
    poses = np.stack([look_at(o + [-0.3, 1.2, 1.3], first),            # from outside the box
                      look_at(o + [1.3, 1.1, 0.1], first + [0.05, 0.1, 0.2]),      # from brick (2, 2, 0): through empty bricks
                      look_at(o + [0.2, 0.3, 0.2], centre),            # along the diagonal from brick (0, 0, 0)
                      look_at(centre + [0.02, -0.03, 0.01], centre + [1.0, 0.6, 0.8])])      # from inside brick (3, 3, 3)
    assert torch.all(state.table_keys == (1 << 63) - 1)
    hits = []
    for march in ({}, {"skip_empty": False}, {"step": 2.0}):
        want = dense.render(sc.K, poses, sc.HEIGHT, sc.WIDTH, **march)
        got = volume.render(sc.K, poses, sc.HEIGHT, sc.WIDTH, bounds=bounds, **march)
        assert same(got, want)
        hits.append(hit_shares(want[0]))
        print(f"{name} {march}: hits per view {[round(100 * s, 1) for s in hits[-1]]} %")
    # the yardstick is not empty: every camera outside sees the block at every step, the one in the missing centre sees the shell
    assert min(min(h[:3]) for h in hits) > 0.0 and (n < 26 or min(h[3] for h in hits) > 0.0)


def world_points(K, pose, depth):
    """float64 [H,W,3]: the points at camera depth ``depth`` along the pixels' rays."""
    K, pose = np.asarray(K, np.float32).astype(np.float64), np.asarray(pose, np.float32).astype(np.float64)
    h, w = depth.shape
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1) @ pose[:3, :3].T
    return pose[:3, 3] + depth[..., None].astype(np.float64) * d


def test_two_clusters_256_metres_apart(scene):
    """With ``bounds`` around one cluster the image is that of ``dense(that box)``; without, the box is more than 4096 voxels per axis,
    which no dense volume can hold: it must run, and every hit must lie on an allocated brick."""
    from dvmvs.tsdf import SparseTSDFVolume
    far_poses = scene["poses"].copy()
    far_poses[:, :3, 3] += 256.0
    both = SparseTSDFVolume(sc.VOXEL, origin=sc.ORIGIN, max_bricks=1024, device=DEV)
    feed(both, scene, [0, 1, 2], (3,))
    feed(both, scene, [0, 1, 2], (3,), poses=far_poses)
    coords = both.bricks()[0]
    near_side = coords[:, 0] < 256
    assert both.overflow == 0 and near_side.sum() * 2 == len(coords) and ((coords.max(axis=0) - coords.min(axis=0) + 1) * 8 > 4096).all()
    lo = both.origin.astype(np.float64) + coords * 8 * sc.VOXEL
    for side, poses in ((near_side, scene["poses"][:3]), (~near_side, far_poses[:3])):
        box = both.brick_bounds(coords[side].min(axis=0), coords[side].max(axis=0))
        want = both.dense(box).render(sc.K, poses, sc.HEIGHT, sc.WIDTH)
        got = both.render(sc.K, poses, sc.HEIGHT, sc.WIDTH, bounds=box)
        print(f"hits per view with bounds {[round(100 * h, 1) for h in hit_shares(want[0])]} %")
        assert same(got, want) and min(hit_shares(want[0])) > 0.0
        # the whole volume: a box that cannot be made dense
        depth = both.render(sc.K, poses, sc.HEIGHT, sc.WIDTH)[0].cpu().numpy()
        print(f"hits per view without bounds {[round(100 * float((d != 0).mean()), 1) for d in depth]} %")
        assert min(float((d != 0).mean()) for d in depth) > 0.0
        for i in range(len(poses)):
            points = world_points(sc.K, poses[i], depth[i])[depth[i] != 0]
            inside = ((points[:, None, :] >= lo[None] - sc.VOXEL) & (points[:, None, :] <= lo[None] + 8 * sc.VOXEL + sc.VOXEL)).all(-1).any(-1)
            assert inside.all()


def test_caches_and_determinism(scene, six_frames):
    volume, boxes, _ = six_frames
    first = volume.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH)
    tables, read = volume._render_tables, volume._render_read
    assert tables is not None and read is not None
    coords = volume.bricks()[0]
    assert np.array_equal(volume.brick_extent[0], coords.min(axis=0)) and np.array_equal(volume.brick_extent[1], coords.max(axis=0))
    assert same(first, volume.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH))
    assert volume._render_tables is tables and volume._render_read is read      # built once, read once
    fresh = make()
    feed(fresh, scene, range(6), (6,))
    assert same(first, fresh.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH))
    for i in range(6):      # N views in one launch against N launches
        single = volume.render(sc.K, scene["poses"][i], sc.HEIGHT, sc.WIDTH)
        assert all(torch.equal(a[i], b[0]) for a, b in zip(first, single))
    # a volume that has rendered once, then receives more frames: index, flags and box are rebuilt
    grown = make()
    feed(grown, scene, [0, 1], (2,))
    small = grown.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH)
    assert grown._render_tables is not None and grown._render_read is not None and grown._neighbour is not None
    feed(grown, scene, [2, 3, 4, 5], (4,))
    assert grown._render_tables is None and grown._render_read is None and grown._neighbour is None
    other = make()
    feed(other, scene, [0, 1], (2,))
    feed(other, scene, [2, 3, 4, 5], (4,))
    big = grown.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH)
    assert same(big, other.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH)) and not torch.equal(big[0], small[0])
    assert same(big, first)      # ... and equals the volume fed the same six frames in one go
    # the index's entries may be placed differently from build to build; what it answers is the same
    from dvmvs.hip import sparse as hip_sparse
    index = hip_sparse.sparse_raycast_index(volume._state).cpu().numpy()
    keys = volume._state.pool_key[:306].cpu().numpy()
    used = index[:, 0] != (1 << 63) - 1
    assert used.sum() == 306 and np.array_equal(np.sort(index[used, 0]), np.sort(keys))
    assert np.array_equal(keys[index[used, 1]], index[used, 0])      # value = the slot that holds the key (no flag yet)
    flags = tables[1].cpu().numpy()
    flagged = tables[0].cpu().numpy()
    used = flagged[:, 0] != (1 << 63) - 1
    assert np.array_equal(flags[flagged[used, 1] & 0x7FFFFFFF], (flagged[used, 1] >> 32) & 1) and 0 < flags[:306].sum() < 306


def test_edges(scene, six_frames):
    from dvmvs.hip import sparse as hip_sparse
    empty = make(16)
    with pytest.raises(ValueError, match="no brick"):
        empty.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH)
    assert empty.brick_extent is None
    depth, normal, rgb = empty.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, bounds=sc.box_bounds())
    assert depth.shape == (6, sc.HEIGHT, sc.WIDTH) and depth.dtype == torch.float32 and normal.shape == (6, sc.HEIGHT, sc.WIDTH, 3)
    assert normal.dtype == torch.float32 and rgb.shape == (6, sc.HEIGHT, sc.WIDTH, 3) and rgb.dtype == torch.uint8 and depth.is_cuda
    assert not bool(depth.any()) and not bool(normal.any()) and not bool(rgb.any())
    full = make(4)
    feed(full, scene, [0], (1,))
    assert full.overflow > 0
    with pytest.raises(RuntimeError, match="did not fit"):
        full.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH)
    got = full.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, allow_overflow=True)
    assert same(got, full.dense(allow_overflow=True).render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH))
    # degenerate cameras and ranges: zeros, as the dense path, and the stream stays usable
    volume, boxes, yardsticks = six_frames
    dense = yardsticks["the scene's box"]
    bad_pose = np.stack([scene["poses"][0]] * 4)
    bad_pose[0, 0, 3], bad_pose[1, 1, 1], bad_pose[2, :3, :3] = np.nan, np.inf, 0.0
    bad_K = np.stack([sc.K] * 4)
    bad_K[3, 0, 0] = 0.0
    for K, poses, march in ((bad_K, bad_pose, {}), (sc.K, scene["poses"][:1], {"near": 2.0, "far": 1.0})):
        for skip_empty in (True, False):
            got = volume.render(K, poses, sc.HEIGHT, sc.WIDTH, bounds=sc.box_bounds(), skip_empty=skip_empty, **march)
            assert not bool(got[0].any()) and not bool(got[1].any()) and not bool(got[2].any())
            assert same(got, dense.render(K, poses, sc.HEIGHT, sc.WIDTH, skip_empty=skip_empty, **march))
    again = volume.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, bounds=sc.box_bounds())
    torch.cuda.synchronize()
    assert same(again, dense.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH)) and bool(again[0].any())
    # refusals before a launch
    with pytest.raises(ValueError, match="step"):
        volume.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, step=6.0)
    with pytest.raises(ValueError, match="bounds="):
        volume.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, bounds=[[0.0, 40000.0], [0.0, 1.0], [0.0, 1.0]], step=0.5)
    state, (index, flags), neighbour = volume._state, volume._render_tables, volume.neighbours()
    K = torch.from_numpy(np.stack([sc.K] * 6)).to(DEV)
    P = torch.from_numpy(scene["poses"]).to(DEV)
    good = dict(state=state, index=index, flags=flags, neighbour=neighbour, first_brick=(0, 0, 0), count=(17, 17, 25), origin=sc.BOX_ORIGIN,
                voxel_size=sc.VOXEL, cam_intr=K, cam_pose=P, height=sc.HEIGHT, width=sc.WIDTH)
    assert same(hip_sparse.sparse_raycast(**good), again)
    for bad in ({"cam_pose": P.double()}, {"cam_intr": K[:5]}, {"cam_pose": P.cpu()}, {"index": index[:-1]}, {"index": index.int()},
                {"flags": flags.float()}, {"neighbour": neighbour[:, :26]}, {"flags": flags.cpu()}, {"count": (0, 17, 25)}, {"near": -1.0},
                {"far": float("nan")}, {"height": 0}):
        with pytest.raises((ValueError, RuntimeError, TypeError)):
            hip_sparse.sparse_raycast(**dict(good, **bad))


def live_fusion(scene, bounds, **kwargs):
    from dvmvs.tsdf import LiveFusion
    fuse = LiveFusion(bounds, voxel_size=sc.VOXEL, max_depth=5.0, batch=4, device=DEV, **kwargs)
    for view in range(6):
        fuse.add(torch.from_numpy(scene["depth"][view]).to(DEV), scene["rgb"][view], scene["K"], scene["poses"][view])
    return fuse


def test_live_fusion_renders_from_the_pool_without_bounds(scene):
    fuse = live_fusion(scene, None, max_bricks=1024, sparse_origin=sc.ORIGIN)
    got = fuse.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, step=0.5)      # flushes the two pending frames; no dense()
    assert fuse.sparse.frames == 6 and fuse._volume is None
    assert same(got, fuse.sparse.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, step=0.5)) and min(hit_shares(got[0])) >= rr.HIT_FLOOR
    assert fuse._volume is None and same(got, fuse.volume.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH, step=0.5))


def test_live_fusion_with_bounds_renders_its_dense_volume(scene):
    fuse = live_fusion(scene, sc.box_bounds())
    got = fuse.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH)
    assert fuse.sparse is None and same(got, fuse.volume.render(sc.K, scene["poses"], sc.HEIGHT, sc.WIDTH)) and bool(got[0].any())


def test_program_renders_the_keyframes_from_the_pool(hip_device, golden_dir, tmp_path, monkeypatch):
    """``python -m dvmvs.tsdf --sparse_volume --render_keyframes --sparse_volume_render`` on two keyframes of the sample scene (the set-up
    of tests/test_sparse_extract_gpu.py, restated): with ``--sparse_volume_extract`` as well ``dense()`` is never called, and the rendered
    files are byte for byte those of the run without the new flag."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.tsdf import SparseTSDFVolume, main
    src = os.path.join(golden_dir, "sample_scene")
    scene_dir = tmp_path / "data" / "hololens-dataset" / "000"
    (scene_dir / "images").mkdir(parents=True)
    (scene_dir / "depth").mkdir()
    names = ["00012.png", "00013.png"]
    for name in names:
        Image.open(os.path.join(src, "images", name)).save(scene_dir / "images" / name)
        Image.open(os.path.join(src, "depth", name)).save(scene_dir / "depth" / name)
    np.savetxt(scene_dir / "poses.txt", np.loadtxt(os.path.join(golden_dir, "hololens_000_poses.txt")).reshape(-1, 16)[[9, 10]])
    np.savetxt(scene_dir / "K.txt", np.loadtxt(os.path.join(golden_dir, "hololens_000_K.txt")))
    (tmp_path / "data" / "indices").mkdir()
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("00012.png 00009.png\nTRACKING LOST\n00013.png 00012.png\n")
    preds = np.stack([resize_nearest(load_depth_png(os.path.join(src, "depth", n)), 320, 256) for n in names]).astype(np.float32)
    (tmp_path / "pred").mkdir()
    np.savez(tmp_path / "pred" / "keyframe_hololens-dataset_320_256_3_dvmvs_fusionnet_online_predictions_000.npz", preds)
    calls = []
    dense = SparseTSDFVolume.dense
    monkeypatch.setattr(SparseTSDFVolume, "dense", lambda self, *a, **k: calls.append(1) or dense(self, *a, **k))
    written, dense_calls = {}, {}
    common = ["--sparse_volume", "--sparse_volume_bricks", "4096", "--render_keyframes"]
    for tag, flags in (("dense", ["--sparse_volume_extract"]), ("pool", ["--sparse_volume_extract", "--sparse_volume_render"]),
                       ("pool_rendered_only", ["--sparse_volume_render"])):
        out = tmp_path / tag
        del calls[:]
        main(["--reconstruction_folder", str(out), "--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"),
              "--voxel_size", "0.05"] + common + flags)
        dense_calls[tag] = len(calls)
        written[tag] = {w: open(out / w, "rb").read() for w in sorted(os.listdir(out))}
    assert dense_calls == {"dense": 1, "pool": 0, "pool_rendered_only": 1}      # (the last: for the mesh, not for the rendering)
    assert set(written["pool"]) == set(written["dense"]) == set(written["pool_rendered_only"])
    rendered = [w for w in written["dense"] if not w.endswith("_complete.ply")]
    assert len(rendered) == 2 and all("+sparse" in w for w in rendered)
    for w in rendered:
        assert written["pool"][w] == written["dense"][w] and written["pool_rendered_only"][w] == written["dense"][w]
    meshes = [w for w in written["dense"] if w.endswith("_complete.ply")]
    assert len(meshes) == 1 and written["pool"][meshes[0]] == written["dense"][meshes[0]]      # both from the pool
