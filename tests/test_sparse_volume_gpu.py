"""GPU: ``dvmvs.tsdf.SparseTSDFVolume`` (csrc/sparse_volume.hip) -- the bricks a flush allocates against the host
definition (dvmvs/sparse.py), the contents of every allocated brick against the dense kernel under the birth rule, batching, determinism,
negative coordinates, hash collisions, both kinds of overflow, and ``LiveFusion`` without bounds.  Everything compares with equality:
there is no tolerance in this file."""
import numpy as np
import pytest
import torch

import sparse_grid_program
import sparse_scene as sc
from dvmvs import sparse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = [1.0, 2.0, 0.5, 1.0, 3.0, 1.0]


@pytest.fixture(scope="module")
def scene():
    depth, rgb = sc.frames()
    return {"depth": depth, "rgb": rgb, "poses": sc.poses(), "K": sc.K}


def make(max_bricks=1024, table_slots=None):
    from dvmvs.tsdf import SparseTSDFVolume
    return SparseTSDFVolume(sc.VOXEL, origin=sc.ORIGIN, max_bricks=max_bricks, table_slots=table_slots, device=DEV)


def feed(volume, scene, views, split, max_depth, weights=None, depth=None):
    """Gives the frames ``views`` of the scene to ``volume`` in flushes of the sizes ``split``."""
    depth = scene["depth"] if depth is None else depth
    first = 0
    for n in split:
        part = list(views[first:first + n])
        volume.integrate_frames(scene["rgb"][part], depth[part], scene["K"], scene["poses"][part],
                                obs_weight=1.0 if weights is None else [weights[v] for v in part], max_depth=max_depth)
        first += n
    assert first == len(views)


def arrays(dense):
    return dense._tsdf, dense._weight, dense._color


def yardstick(scene, views, max_depth, weights=None, depth=None):
    """What the issue defines as the contents, from existing code only: a dense ``TSDFVolume`` on the box, ``integrate`` called frame by
    frame, and after frame g every brick with birth > g, or never born, set back to (1, 0, 0).  Returns the three device tensors."""
    from dvmvs.tsdf import TSDFVolume
    depth = scene["depth"] if depth is None else depth
    views = list(views)
    coords, birth = sparse.brick_births(depth[views], scene["K"], scene["poses"][views], sc.ORIGIN, sc.VOXEL, sc.TRUNC, max_depth)
    assert sc.bricks_in_box(coords).all()
    dense = TSDFVolume(sc.box_bounds(), sc.VOXEL, device=DEV)
    assert tuple(int(d) for d in dense.vol_dim) == sc.BOX_DIMS and np.array_equal(dense._vol_origin, sc.BOX_ORIGIN)
    for g, view in enumerate(views):
        dense.integrate(scene["rgb"][view], sc.clamp(depth[view], max_depth), scene["K"], scene["poses"][view],
                        obs_weight=1.0 if weights is None else weights[view])
        born = torch.from_numpy(sc.brick_mask(coords[birth <= g])).to(DEV)
        dense._tsdf[~born] = 1.0
        dense._weight[~born] = 0.0
        dense._color[~born] = 0.0
    return arrays(dense)


@pytest.fixture(scope="module")
def six_frames(scene):
    """The six frames in one flush at max_depth 5, and their yardstick: computed once, shared, never written."""
    volume = make()
    feed(volume, scene, range(6), (6,), 5.0)
    return volume, arrays(volume.dense(sc.box_bounds())), yardstick(scene, range(6), 5.0)


def equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("view", range(6))
def test_one_flush_allocates_the_bricks_of_the_host_definition(scene, view):
    """(b) of the issue, per view; the pixels that must mark nothing are planted in the frame."""
    depth = scene["depth"].copy()
    depth[view] = sc.planted_depth(depth[view])
    for max_depth in sc.MAX_DEPTHS:
        volume = make(256)
        feed(volume, scene, [view], (1,), max_depth, depth=depth)
        coords, birth = volume.bricks()
        want = sparse.mark_bricks(depth[view], scene["K"], scene["poses"][view], sc.ORIGIN, sc.VOXEL, sc.TRUNC, max_depth)
        assert coords.dtype == np.int32 and np.array_equal(coords, want) and len(want) > 30      # pool order of one flush = key order
        assert birth.dtype == np.int32 and not birth.any()
        assert volume.n_bricks == len(want) and volume.overflow == 0 and volume.rejected_pixels == 0


@pytest.mark.parametrize("voxel,origin,view", [(0.05, (0.013, -0.7, 2.1), 4), (0.0437, (-0.31, 0.77, -1.9), 1), (0.003, (-1.0, -0.75, 0.0), 3)])
def test_marking_on_lattices_that_are_not_dyadic_and_rejected_pixels(scene, voxel, origin, view):
    """The marking is bit for bit the host definition's on any lattice: positions that round, and a 3 mm voxel at which most pixels
    span more than 4 bricks, mark nothing and are counted."""
    from dvmvs.tsdf import SparseTSDFVolume
    volume = SparseTSDFVolume(voxel, origin=origin, max_bricks=16384, device=DEV)      # (the 3 mm case allocates 13 277 bricks)
    depth = sc.planted_depth(scene["depth"][view])
    volume.integrate(scene["rgb"][view], depth, scene["K"], scene["poses"][view], max_depth=5.0)
    want, rejected = sparse.mark_bricks(depth, scene["K"], scene["poses"][view], np.asarray(origin, dtype=np.float32), voxel, volume.trunc_margin,
                                        5.0, return_rejected=True)
    assert np.array_equal(volume.bricks()[0], want) and volume.rejected_pixels == rejected and volume.overflow == 0
    assert (rejected > 100) if voxel < 0.01 else (rejected == 0 and len(want) > 30)


def test_six_frames_at_once_allocate_the_bricks_and_births_of_the_host_definition(scene):
    depth = scene["depth"].copy()
    depth[2] = sc.planted_depth(depth[2])
    volume = make()
    feed(volume, scene, range(6), (6,), 5.0, depth=depth)
    coords, birth = volume.bricks()
    want, want_birth = sparse.brick_births(depth, scene["K"], scene["poses"], sc.ORIGIN, sc.VOXEL, sc.TRUNC, 5.0)
    assert np.array_equal(coords, want) and np.array_equal(birth, want_birth) and set(birth.tolist()) == set(range(6))
    assert volume.overflow == 0 and volume.rejected_pixels == 0 and volume.frames == 6


def test_contents_are_the_dense_kernels_bits_under_the_birth_rule(six_frames):
    _, got, want = six_frames
    observed = int((want[1] > 0).sum())
    print(f"{observed} voxels with weight > 0; {int((want[0] < 1).sum())} with tsdf < 1")
    assert observed >= 3000
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_contents_with_a_weight_per_frame_and_a_depth_clamp(scene):
    volume = make()
    feed(volume, scene, range(6), (4, 2), 1.4, weights=WEIGHTS)
    got = arrays(volume.dense(sc.box_bounds()))
    want = yardstick(scene, range(6), 1.4, weights=WEIGHTS)
    assert int((want[1] > 0).sum()) >= 3000 and len(torch.unique(want[1])) > 6
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("split", [(1, 5), (3, 3), (1, 1, 1, 1, 1, 1)])
def test_batching_does_not_change_the_volume(scene, six_frames, split):
    volume = make()
    feed(volume, scene, range(6), split, 5.0)
    assert equal(arrays(volume.dense(sc.box_bounds())), six_frames[1])
    # the pool's order is by flush, ascending key inside; the set of bricks and their births are those of one flush
    coords, birth = volume.bricks()
    one_coords, one_birth = six_frames[0].bricks()
    order = np.argsort(sparse.pack_keys(coords))
    assert np.array_equal(coords[order], one_coords) and np.array_equal(birth[order], one_birth)
    flush_of_frame = np.repeat(np.arange(len(split)), split)
    assert np.array_equal(np.lexsort((sparse.pack_keys(coords), flush_of_frame[birth])), np.arange(len(coords)))     # by flush, then key


def test_more_than_64_frames_in_one_flush(scene):
    """70 frames (the six, over and over, each with a weight of its own) in ONE flush, which the integrate entry cuts into launches of 64 and
    6 frames, against flushes of 35 + 35 and of 64 + 6: the same pool, bit for bit."""
    views = [i % 6 for i in range(70)]
    weights = [1.0 + 0.25 * (i % 7) for i in range(70)]
    pools = []
    for split in ((70,), (35, 35), (64, 6)):
        volume, first = make(512), 0
        for n in split:
            part = views[first:first + n]
            volume.integrate_frames(scene["rgb"][part], scene["depth"][part], scene["K"], scene["poses"][part], obs_weight=weights[first:first + n],
                                    max_depth=5.0)
            first += n
        assert volume.frames == 70 and volume.overflow == 0
        pools.append([*volume.pool(), volume._state.pool_key, volume._state.pool_birth])
    assert equal(pools[0], pools[1]) and equal(pools[0], pools[2])
    assert float(pools[0][1].max()) > 20 and set(volume.bricks()[1].tolist()) == set(range(6))


def test_the_same_split_twice_gives_the_same_pool(scene):
    pools = []
    for _ in range(2):
        volume = make(512, 1024)
        feed(volume, scene, range(6), (2, 4), 5.0, weights=WEIGHTS)
        state = volume._state
        pools.append([t.clone() for t in (*volume.pool(), state.pool_key, state.pool_birth, state.status)])
    assert equal(pools[0], pools[1])
    assert int(pools[0][5][0]) == 306 and not pools[0][5][1:].any()


def test_the_same_frame_again_allocates_nothing_and_still_updates(scene):
    volume = make(256)
    feed(volume, scene, [0], (1,), 5.0)
    first, bricks = volume.n_bricks, volume.bricks()
    once = [t.clone() for t in arrays(volume.dense(sc.box_bounds()))]
    feed(volume, scene, [0], (1,), 5.0)
    assert volume.n_bricks == first and volume.frames == 2 and volume.overflow == 0
    again = volume.bricks()
    assert np.array_equal(bricks[0], again[0]) and np.array_equal(bricks[1], again[1])
    twice = arrays(volume.dense(sc.box_bounds()))
    assert torch.equal(twice[1], 2 * once[1]) and int((once[1] > 0).sum()) > 1000
    assert equal(twice, yardstick(scene, [0, 0], 5.0))


def test_negative_coordinates_the_far_view_alone(scene):
    volume = make(256)
    feed(volume, scene, [5], (1,), 5.0)
    coords, birth = volume.bricks()
    assert np.array_equal(coords, sparse.mark_bricks(scene["depth"][5], scene["K"], scene["poses"][5], sc.ORIGIN, sc.VOXEL, sc.TRUNC, 5.0))
    assert coords[:, 2].max() < -5 and coords[:, 2].min() <= -10 and coords.min() < 0 and not birth.any()
    want = yardstick(scene, [5], 5.0)
    assert int((want[1] > 0).sum()) >= 3000
    assert equal(arrays(volume.dense(sc.box_bounds())), want)
    own = volume.dense()                                        # over the allocated bricks alone: the same voxels, elsewhere in the array
    first = coords.min(axis=0)
    assert tuple(own._tsdf.shape) == tuple(int(d) for d in (coords.max(axis=0) - first + 1) * 8)
    assert np.array_equal(own._vol_origin, (sc.ORIGIN.astype(np.float64) + first * 8 * sc.VOXEL).astype(np.float32))
    at = (first - sc.BOX_FIRST) * 8
    for mine, boxed in zip(arrays(own), want):
        assert torch.equal(mine, boxed[at[0]:at[0] + mine.shape[0], at[1]:at[1] + mine.shape[1], at[2]:at[2] + mine.shape[2]])


@pytest.mark.parametrize("max_bricks,table_slots,max_depth,keys", [(128, 256, 1.1, 103), (512, 512, 5.0, 306)])
def test_a_crowded_table_gives_the_result_of_the_default_table(scene, max_bricks, table_slots, max_depth, keys):
    """103 keys in 256 slots, 306 in 512: probing is certain (the expected number of keys that do not sit in their first slot is about
    20 and 90)."""
    crowded, roomy = make(max_bricks, table_slots), make()
    for volume in (crowded, roomy):
        feed(volume, scene, range(6), (3, 3), max_depth)
    assert crowded.table_slots == table_slots and roomy.table_slots == 2048
    assert crowded.n_bricks == keys and crowded.overflow == 0
    for a, b in zip(crowded.bricks(), roomy.bricks()):
        assert np.array_equal(a, b)
    assert equal(arrays(crowded.dense(sc.box_bounds())), arrays(roomy.dense(sc.box_bounds())))
    table = crowded._state.table_keys.cpu().numpy()
    slots = np.flatnonzero(table != (1 << 63) - 1)
    assert len(slots) == keys and len(np.unique(table[slots])) == keys          # every key once


def test_overflow_of_the_pool(scene):
    volume = make(4, 256)
    feed(volume, scene, [0], (1,), 5.0)                        # 73 keys: the table takes them all, the pool four
    want = sparse.mark_bricks(scene["depth"][0], scene["K"], scene["poses"][0], sc.ORIGIN, sc.VOXEL, sc.TRUNC, 5.0)
    assert volume.overflow == len(want) - 4 and volume.n_bricks == 4
    coords, birth = volume.bricks()
    assert np.array_equal(coords, want[:4]) and not birth.any()            # the four smallest keys of the first flush
    feed(volume, scene, [1, 2], (2,), 5.0)
    assert volume.overflow > len(want) - 4 and volume.n_bricks == 4 and np.array_equal(volume.bricks()[0], want[:4])
    with pytest.raises(RuntimeError, match="did not fit"):
        volume.dense()
    partial = volume.dense(allow_overflow=True)
    assert int((partial._weight > 0).sum()) > 0


def test_overflow_of_the_table(scene):
    status, output = sparse_grid_program.run(sanitize=False)   # the bounded probe passes on the host (a plain build) before it runs here
    if status is None:
        pytest.skip("no host compiler: the probe sequence was not checked on the CPU")
    assert status == 0, output
    volume = make(4, 8)
    feed(volume, scene, range(6), (6,), 5.0)
    assert volume.overflow > 0 and volume.n_bricks <= 4


def live_fusion(scene, bounds, **kwargs):
    from dvmvs.tsdf import LiveFusion
    fuse = LiveFusion(bounds, voxel_size=sc.VOXEL, max_depth=5.0, batch=4, device=DEV, **kwargs)
    for view in range(6):
        fuse.add(torch.from_numpy(scene["depth"][view]).to(DEV), scene["rgb"][view], scene["K"], scene["poses"][view])
    return fuse


def test_live_fusion_without_bounds(scene, six_frames):
    fuse = live_fusion(scene, None, max_bricks=1024, sparse_origin=sc.ORIGIN)
    volume = fuse.volume                                       # flushes the two pending frames, then dense()
    assert fuse.sparse is not None and fuse.sparse.frames == 6 and fuse.volume is volume          # cached until the next add
    want = six_frames[0].dense()
    assert np.array_equal(volume._vol_origin, want._vol_origin) and equal(arrays(volume), arrays(want))
    verts, faces, normals, colours = volume.get_mesh()
    assert len(faces) > 100 and len(verts) > 100 and faces.max() < len(verts) and len(normals) == len(colours) == len(verts)
    fuse.add(torch.from_numpy(scene["depth"][0]).to(DEV), scene["rgb"][0], scene["K"], scene["poses"][0])
    assert fuse.volume is not volume and fuse.sparse.frames == 7


def test_live_fusion_with_bounds_is_what_it_was(scene):
    from dvmvs.tsdf import TSDFVolume
    fuse = live_fusion(scene, sc.box_bounds())
    assert fuse.sparse is None
    dense = TSDFVolume(sc.box_bounds(), sc.VOXEL, device=DEV)
    dense.integrate_frames(scene["rgb"][:4], scene["depth"][:4], scene["K"], scene["poses"][:4], max_depth=5.0)
    dense.integrate_frames(scene["rgb"][4:], scene["depth"][4:], scene["K"], scene["poses"][4:], max_depth=5.0)
    assert equal(arrays(fuse.volume), arrays(dense))


def test_predict_online_reconstructs_a_scene_without_its_poses_in_advance(tmp_path):
    """``predict_online(..., fuse=LiveFusion(None, ...))``: nothing of the scene is read before its frames arrive; the live volume equals
    what the logged frames give when they are fused one by one into a second sparse volume, and the downstream chain takes it.
    14 frames of a synthetic scene through a full ``DepthEngine``: 4.4 s on an MI355X, nearly all of it building and warming the engine
    (the runner tests of tests/test_tsdf_fuse_gpu.py share one engine among themselves and take as long for their first); it is the one
    test here that runs what the feature is for, end to end."""
    import os
    import synthetic as syn
    from test_runner import _write_scene
    from dvmvs.dataset_loader import PreprocessImage, load_image, resize_nearest
    from dvmvs.engine import DepthEngine
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    from dvmvs.runner import Scene, predict_online
    from dvmvs.tsdf import LiveFusion, SparseTSDFVolume
    folder = str(tmp_path / "scene")
    _write_scene(folder, 30)
    engine = DepthEngine(*syn.build_e2e_modules((FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)), device=DEV)
    live = LiveFusion(None, voxel_size=0.1, max_depth=5.0, batch=2, device=DEV, max_bricks=8192)
    log = []
    predictions = predict_online(engine, folder, evaluate=False, max_frames=14, frame_log=log, fuse=live)[0]
    names = [line.split(" ")[0] for line in log if line != "TRACKING LOST"]
    assert len(names) == len(predictions) > 2 and live.frames == len(predictions)      # more than one flush of two
    volume = live.volume                                        # flushes a pending frame
    assert live.sparse.frames == len(predictions) and live.sparse.overflow == 0 and live.sparse.n_bricks > 10 and int((volume._weight > 0).sum()) > 1000
    scene = Scene(folder)
    first = load_image(os.path.join(folder, "images", scene.image_names[0]))
    K = PreprocessImage(K=scene.K, old_width=first.shape[1], old_height=first.shape[0], new_width=320, new_height=256, distortion_crop=0,
                        perform_crop=False).get_updated_intrinsics()
    again = SparseTSDFVolume(0.1, max_bricks=8192, device=DEV)
    for name, prediction in zip(names, predictions):
        image = resize_nearest(load_image(os.path.join(folder, "images", name)), 320, 256).astype(np.uint8)
        again.integrate(image, np.asarray(prediction, dtype=np.float32), K, scene.poses[scene.image_names.index(name)], max_depth=5.0)
    (coords, birth), (coords_again, birth_again) = live.sparse.bricks(), again.bricks()      # pool order follows the flushes: compare by key
    order, order_again = np.argsort(sparse.pack_keys(coords)), np.argsort(sparse.pack_keys(coords_again))
    assert np.array_equal(coords[order], coords_again[order_again]) and np.array_equal(birth[order], birth_again[order_again])
    assert equal(arrays(volume), arrays(again.dense()))
    depth, _, _ = volume.render(K, scene.poses[scene.image_names.index(names[0])], 256, 320, normals=False, colour=False)
    assert int((depth > 0).sum()) > 0 and len(volume.get_mesh()[1]) > 0
