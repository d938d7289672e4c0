"""GPU: marching cubes straight from the pool of ``dvmvs.tsdf.SparseTSDFVolume`` (csrc/sparse_extract.hip).
The yardstick is always existing code -- ``marching_cubes`` of the arrays of ``volume.dense(box)`` for a brick-aligned box that starts at
brick 0 and leaves a brick of margin -- and every comparison is equality of bits, as multisets (the order of the sparse mesh is by
handling brick, the dense one's by voxel), except the one stated bound of the shifted lattice."""
import numpy as np
import pytest
import torch

import sparse_scene as sc
from dvmvs import sparse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = [1.0, 2.0, 0.5, 1.0, 3.0, 1.0]


@pytest.fixture(scope="module")
def scene():
    depth, rgb = sc.frames()
    return {"depth": depth, "rgb": rgb, "poses": sc.poses(), "K": sc.K}


def make(max_bricks=1024, origin=None):
    from dvmvs.tsdf import SparseTSDFVolume
    return SparseTSDFVolume(sc.VOXEL, origin=sc.BOX_ORIGIN if origin is None else origin, max_bricks=max_bricks, device=DEV)


def feed(volume, scene, views, split, max_depth=5.0, weights=None, poses=None):
    poses = scene["poses"] if poses is None else poses
    first = 0
    for n in split:
        part = list(views[first:first + n])
        volume.integrate_frames(scene["rgb"][part], scene["depth"][part], scene["K"], poses[part],
                                obs_weight=1.0 if weights is None else [weights[v] for v in part], max_depth=max_depth)
        first += n
    assert first == len(views)


def extract(volume, **kwargs):
    """(verts, faces, normals, colours) device tensors of the sparse path."""
    return volume._surface(True, None, None, None, **kwargs)


def bits(mesh):
    """int64 host arrays (vertex rows [V,9], triangle rows [F,27]): position, normal and colour of a vertex as their bits."""
    verts, faces, normals, colours = (t.cpu().numpy() for t in mesh)
    assert verts.dtype == np.float32 and normals.dtype == np.float32 and colours.dtype == np.uint8 and faces.dtype == np.int32
    rows = np.concatenate([verts.view(np.int32).astype(np.int64), normals.view(np.int32).astype(np.int64), colours.astype(np.int64)], axis=1)
    assert faces.size == 0 or (faces.min() >= 0 and faces.max() < len(rows))
    return rows, rows[faces.astype(np.int64)].reshape(len(faces), 27)


def sort_rows(a):
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def same_mesh(got, want):
    """V, F, the multiset of vertex rows and the multiset of triangles (3 x vertex row, in corner order), bit for bit."""
    (gv, gt), (wv, wt) = bits(got), bits(want)
    return gv.shape == wv.shape and gt.shape == wt.shape and np.array_equal(sort_rows(gv), sort_rows(wv)) and np.array_equal(sort_rows(gt), sort_rows(wt))


def dense_mesh(volume, last=None):
    """The yardstick: ``marching_cubes`` of ``dense(box)``, the box from brick 0 to ``last`` (default: the scene's box).  Asserts the margin."""
    from dvmvs.hip.volume import marching_cubes
    coords = volume.bricks()[0]
    last = sc.BOX_BRICKS - 1 if last is None else np.asarray(last)
    assert len(coords) == 0 or (coords.min(axis=0) >= 1).all() and (coords.max(axis=0) <= last - 1).all()      # >= 1 brick of margin
    dense = volume.dense(volume.brick_bounds((0, 0, 0), last))
    assert np.array_equal(dense._vol_origin, volume.origin) and tuple(dense._tsdf.shape) == tuple(int(c) * 8 for c in last + 1)
    return marching_cubes(dense._tsdf, 0.0, dense._color, dense._vol_origin, dense._voxel_size)


@pytest.fixture(scope="module")
def six_frames(scene):
    """Six frames in one flush at max_depth 5 on the lattice that starts at the box: the volume and its sparse mesh, shared, never written."""
    volume = make()
    feed(volume, scene, range(6), (6,))
    assert volume.n_bricks == 306 and volume.overflow == 0
    return volume, extract(volume)


def test_scene_equals_the_dense_mesh(six_frames):
    volume, got = six_frames
    want = dense_mesh(volume)
    print(f"V {len(want[0])} F {len(want[1])}")
    assert len(want[0]) > 1000 and len(want[1]) > 1000
    assert same_mesh(got, want)


def test_scene_with_a_depth_clamp_and_frame_weights(scene):
    volume = make()
    feed(volume, scene, range(6), (6,), max_depth=1.4, weights=WEIGHTS)
    want = dense_mesh(volume)
    assert len(want[1]) > 300 and same_mesh(extract(volume), want)


def fill_with_noise(volume, n, seed):
    """tsdf <- uniform [-1, 1], colour <- folded integers < 2^24, weight <- 1 in the first n pool slots, in place."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    tsdf, weight, colour = volume.pool()
    tsdf[:n] = torch.rand((n, 512), generator=gen, device=DEV) * 2.0 - 1.0
    colour[:n] = torch.randint(0, 1 << 24, (n, 512), generator=gen, device=DEV).float()
    weight[:n] = 1.0


def test_noise_pool_every_face_edge_and_corner(scene):
    volume = make()
    feed(volume, scene, range(6), (6,))
    n = volume.n_bricks
    fill_with_noise(volume, n, 1)
    want = dense_mesh(volume)
    assert same_mesh(extract(volume), want)
    # the dense mesh has vertices whose owner voxel, and triangles whose cube, lie in an unallocated brick
    allocated = np.zeros(tuple(int(b) for b in sc.BOX_BRICKS), dtype=bool)
    coords = volume.bricks()[0]
    allocated[coords[:, 0], coords[:, 1], coords[:, 2]] = True
    verts, faces = want[0].cpu().numpy().astype(np.float64), want[1].cpu().numpy()
    p = (verts - volume.origin.astype(np.float64)) / sc.VOXEL
    owner = np.floor(p).astype(np.int64) // 8
    cube = np.floor(p[faces].mean(axis=1)).astype(np.int64) // 8
    assert (~allocated[owner[:, 0], owner[:, 1], owner[:, 2]]).sum() > 0 and (~allocated[cube[:, 0], cube[:, 1], cube[:, 2]]).sum() > 0


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


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_hand_made_layouts(name):
    """``pool_key[:n]``, ``status[0]`` and noise written directly into a fresh state: the hash table stays empty, and is not read."""
    coords = np.array(LAYOUTS[name])
    n = len(coords)
    volume = make(32)
    state = volume._state
    state.pool_key[:n] = torch.from_numpy(sparse.pack_keys(coords)).to(DEV)
    state.status[0] = n
    fill_with_noise(volume, n, 2 + n)
    assert np.array_equal(volume.bricks()[0], coords)
    want = dense_mesh(volume, last=coords.max(axis=0) + 1)
    assert len(want[1]) > 500 and same_mesh(extract(volume), want)


def test_negative_coordinates_on_a_shifted_lattice(scene, six_frames):
    volume_a, mesh_a = six_frames
    origin_b = (sc.BOX_ORIGIN.astype(np.float64) + 8 * 20 * sc.VOXEL).astype(np.float32)
    volume_b = make(origin=origin_b)
    feed(volume_b, scene, range(6), (6,))
    coords_a, coords_b = volume_a.bricks()[0], volume_b.bricks()[0]
    # (x and y of every brick are negative on lattice B; z reaches brick 0: the scene's highest bricks are 20 above the box's first)
    assert np.array_equal(coords_b, coords_a - 20) and coords_b.max() == 0 and coords_b[:, :2].max() < 0 and (coords_b[:, 2] < 0).mean() > 0.5
    for a, b in zip(volume_a.pool(), volume_b.pool()):
        assert torch.equal(a, b)
    mesh_b = extract(volume_b)
    assert mesh_a[0].shape == mesh_b[0].shape and torch.equal(mesh_a[1], mesh_b[1]) and torch.equal(mesh_a[2], mesh_b[2])
    va, vb = mesh_a[0].cpu().numpy().astype(np.float64), mesh_b[0].cpu().numpy().astype(np.float64)
    index_a = np.abs(va - sc.BOX_ORIGIN.astype(np.float64)).max()          # |index| * voxel on lattice A
    index_b = np.abs(vb - origin_b.astype(np.float64)).max()
    M = max(index_a, index_b, np.abs(va).max(), np.abs(vb).max())
    worst = np.abs(va - vb).max()
    print(f"positions differ by at most {worst:.3e}; bound {2.0 ** -22 * M:.3e}")
    assert worst <= 2.0 ** -22 * M


def test_two_clusters_256_metres_apart(scene):
    """What ``dense()`` cannot do: the bounding box is more than 4096 voxels on each axis.  No dense volume is allocated here."""
    from dvmvs.tsdf import SparseTSDFVolume
    far_poses = scene["poses"].copy()
    far_poses[:, :3, 3] += 256.0
    both = SparseTSDFVolume(sc.VOXEL, origin=sc.ORIGIN, max_bricks=1024, device=DEV)
    feed(both, scene, [0, 1, 2], (3,))
    feed(both, scene, [0, 1, 2], (3,), poses=far_poses)
    near = SparseTSDFVolume(sc.VOXEL, origin=sc.ORIGIN, max_bricks=1024, device=DEV)
    feed(near, scene, [0, 1, 2], (3,))
    coords = both.bricks()[0]
    n_near = near.n_bricks
    assert both.overflow == 0 and both.rejected_pixels == 0 and len(coords) == 2 * n_near
    assert np.array_equal(np.sort(sparse.pack_keys(coords[n_near:] - 512)), np.sort(sparse.pack_keys(coords[:n_near])))
    assert ((coords.max(axis=0) - coords.min(axis=0) + 1) * 8 > 4096).all()
    mesh = extract(both)
    rows, triangles = bits(mesh)                                           # (asserts every face index < V)
    x = mesh[0][:, 0].cpu().numpy()[mesh[1].cpu().numpy().astype(np.int64)]
    near_side, far_side = (x < 100).all(axis=1), (x > 100).all(axis=1)
    assert near_side.sum() + far_side.sum() == len(triangles) and far_side.sum() > 100
    want = bits(extract(near))[1]
    assert len(want) > 100 and np.array_equal(sort_rows(triangles[near_side]), sort_rows(want))


def test_determinism_and_the_cached_neighbour_table(scene, six_frames):
    volume, first = six_frames
    again = extract(volume)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    fresh = make()
    feed(fresh, scene, range(6), (6,))
    assert all(torch.equal(a, b) for a, b in zip(first, extract(fresh)))
    # a volume that has extracted once, then receives more frames: the table is rebuilt
    grown = make()
    feed(grown, scene, [0, 1], (2,))
    small = extract(grown)
    table = grown._neighbour
    assert table is not None and grown.neighbours() is table
    feed(grown, scene, [2, 3, 4, 5], (4,))
    assert grown._neighbour is None
    other = make()
    feed(other, scene, [0, 1], (2,))
    feed(other, scene, [2, 3, 4, 5], (4,))
    big = extract(grown)
    assert len(big[1]) > len(small[1]) and all(torch.equal(a, b) for a, b in zip(big, extract(other)))


def test_an_empty_volume_gives_typed_empties():
    verts, faces, normals, colours = extract(make(16))
    assert tuple(verts.shape) == (0, 3) and verts.dtype == torch.float32 and tuple(faces.shape) == (0, 3) and faces.dtype == torch.int32
    assert tuple(normals.shape) == (0, 3) and normals.dtype == torch.float32 and tuple(colours.shape) == (0, 3) and colours.dtype == torch.uint8
    assert verts.is_cuda and faces.is_cuda
    arrays = make(16).get_mesh()
    assert [a.shape for a in arrays] == [(0, 3)] * 4


def test_an_overflowed_pool_raises_unless_allowed(scene):
    volume = make(4)
    feed(volume, scene, [0], (1,))
    assert volume.overflow > 0 and volume.n_bricks == 4
    with pytest.raises(RuntimeError, match="did not fit"):
        volume.mesh_tensors()
    verts, faces = volume.mesh_tensors(allow_overflow=True)
    assert verts.shape[1] == 3 and faces.shape[1] == 3 and (faces.numel() == 0 or int(faces.max()) < len(verts))
    fill_with_noise(volume, 4, 9)
    verts, faces = volume.mesh_tensors(allow_overflow=True)
    assert len(faces) > 500 and int(faces.max()) < len(verts) and int(faces.min()) >= 0


def test_get_mesh_stages_are_the_device_functions_on_the_extracted_mesh(six_frames):
    from dvmvs.components import ComponentFilter, filter_components_device
    from dvmvs.simplify import SimplifySettings, simplify_mesh_device
    from dvmvs.smooth import SmoothSettings, smooth_mesh_device
    volume, mesh = six_frames
    assert all(torch.equal(a, b) for a, b in zip(volume.mesh_tensors(), mesh[:2])) and torch.equal(volume.vertices(), mesh[0])
    clean, smooth, simplify = ComponentFilter(min_faces=20), SmoothSettings(2), SimplifySettings(2 * sc.VOXEL)
    want = filter_components_device(mesh[0], mesh[1], clean, mesh[2], mesh[3])
    assert len(want[1]) < len(mesh[1])
    want = smooth_mesh_device(want[0], want[1], smooth, want[2], want[3])
    want = simplify_mesh_device(want[0], want[1], simplify, want[2], want[3])
    got = volume.get_mesh(clean=clean, smooth=smooth, simplify=simplify)
    assert len(got[1]) > 100
    for g, w in zip(got, want):
        assert np.array_equal(g, w.cpu().numpy())
    cloud = volume.get_point_cloud()
    assert cloud.shape == (len(mesh[0]), 6) and np.array_equal(cloud[:, :3], mesh[0].cpu().numpy())
    points = volume.surface_points()
    assert torch.equal(points, mesh[0])
    row = volume.score_against(volume.mesh_tensors(), threshold=0.05).cpu().numpy()
    assert row.shape == (6,) and row[0] == 0.0 and row[5] == 1.0


def live_fusion(scene, bounds, **kwargs):
    from dvmvs.tsdf import LiveFusion
    fuse = LiveFusion(bounds, voxel_size=sc.VOXEL, max_depth=5.0, batch=4, device=DEV, **kwargs)
    for view in range(6):
        fuse.add(torch.from_numpy(scene["depth"][view]).to(DEV), scene["rgb"][view], scene["K"], scene["poses"][view])
    return fuse


def test_live_fusion_meshes_from_the_pool_without_bounds(scene):
    fuse = live_fusion(scene, None, max_bricks=1024, sparse_origin=sc.ORIGIN)
    got = fuse.get_mesh()                                       # flushes the two pending frames; no dense()
    assert fuse.sparse.frames == 6 and fuse._volume is None
    want = fuse.sparse.get_mesh()
    assert len(got[1]) > 1000 and all(np.array_equal(g, w) for g, w in zip(got, want))
    verts, faces = fuse.mesh_tensors()
    assert verts.is_cuda and np.array_equal(verts.cpu().numpy(), want[0]) and np.array_equal(faces.cpu().numpy(), want[1])


def test_live_fusion_with_bounds_meshes_its_dense_volume(scene):
    fuse = live_fusion(scene, sc.box_bounds())
    got = fuse.get_mesh()
    assert fuse.sparse is None
    want = fuse.volume.get_mesh()
    assert len(got[1]) > 1000 and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_program_meshes_and_scores_from_the_pool(hip_device, golden_dir, tmp_path, monkeypatch):
    """``python -m dvmvs.tsdf --sparse_volume --sparse_volume_extract`` on two keyframes of the sample scene (their depth maps as
    'predictions', 5 cm voxels): the same files under ``<system>+sparse`` as without the flag; ``dense()`` is called for
    ``--render_keyframes`` only, whose files are then those of the run without the flag, byte for byte; mesh and scores are those of the
    dense box up to what crosses the box's faces."""
    import os
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.tsdf import SparseTSDFVolume, TSDFFusion, main
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
    common = ["--sparse_volume", "--sparse_volume_bricks", "4096", "--evaluate_3d", "--threshold_3d", "0.1"]
    for tag, flags in (("dense", ["--render_keyframes"]), ("pool", ["--sparse_volume_extract"]),
                       ("pool_rendered", ["--sparse_volume_extract", "--render_keyframes"])):
        out = tmp_path / tag
        del calls[:]
        main(["--reconstruction_folder", str(out), "--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"),
              "--voxel_size", "0.05"] + common + flags)
        dense_calls[tag] = len(calls)
        written[tag] = {w: open(out / w, "rb").read() for w in sorted(os.listdir(out))}
    assert dense_calls == {"dense": 1, "pool": 0, "pool_rendered": 1}
    assert set(written["pool_rendered"]) == set(written["dense"]) and all("+sparse" in w for w in written["dense"])
    meshes = [w for w in written["dense"] if w.endswith("_complete.ply")]
    scores = [w for w in written["dense"] if w.endswith("_errors3d.npz")]
    rendered = set(written["dense"]) - set(meshes) - set(scores)
    assert len(meshes) == 1 and len(scores) == 1 and len(rendered) == 2 and set(written["pool"]) == set(meshes + scores)
    for w in rendered:                                            # rendered from dense() in both runs
        assert written["pool_rendered"][w] == written["dense"][w]
    assert written["pool"][meshes[0]] == written["pool_rendered"][meshes[0]]
    faces_dense = len(TSDFFusion.meshread(str(tmp_path / "dense" / meshes[0]))[1])
    faces_pool = len(TSDFFusion.meshread(str(tmp_path / "pool" / meshes[0]))[1])
    row_dense, row_pool = (np.load(tmp_path / tag / scores[0])["arr_0"] for tag in ("dense", "pool"))
    print(f"faces: dense box {faces_dense}, pool {faces_pool}; rows {row_dense} {row_pool}")
    # the dense box of the allocated bricks has no margin: it lacks the triangles of cubes that cross its faces, and nothing else
    assert faces_dense > 1000 and faces_dense <= faces_pool <= 1.05 * faces_dense
    assert np.isfinite(row_pool).all() and np.abs(row_pool - row_dense).max() < 0.02
