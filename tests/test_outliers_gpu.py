"""GPU: the k-nearest-neighbour search, the radius count and the outlier filters (csrc/point_neighbours.hip, dvmvs.hip.neighbours) against
the host definitions of dvmvs/outliers.py, bit for bit in every case: ``dist``, ``index``, ``count``, ``mean``, ``stats``, ``keep`` and the
filtered cloud; up to the program's ``--clean_points_*`` flags.  A row of the k-nearest search is the prefix of the row for a larger k, so
the brute force is computed once per case for k = 32 and shared; it is never modified."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import consistency_reference as cr
from dvmvs import outliers
from dvmvs.outliers import OutlierFilter

pytestmark = pytest.mark.gpu
KS = (1, 8, 20, 32)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def gaussian(n, seed):
    return f32(np.random.default_rng(seed).normal(size=(n, 3)))


def lattice(n):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def blob_with_far_points():
    rng = np.random.default_rng(41)
    far = rng.normal(size=(20, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(3, 5, (20, 1))        # the box is ~20 cell edges wide
    return f32(np.concatenate([rng.normal(0, 0.05, (2000, 3)), far]))


# name -> (query, target or None for the query itself, exclude_same_index, max_distance)
@functools.lru_cache(maxsize=None)
def case(name):
    sizes = {1: 5, 2: 1, 255: 300, 257: 129, 3001: 2500}
    if name.startswith("self"):
        n = int(name[4:])
        query, target, exclude, limit = gaussian(n, 100 + n), None, True, math.inf
    elif name.startswith("other"):
        n = int(name[5:])
        query, target, exclude, limit = gaussian(n, 200 + n), gaussian(sizes[n], 300 + n), False, math.inf
    elif name == "lattice":
        query, target, exclude, limit = lattice(6), None, True, math.inf
    elif name == "lattice_limit":                          # the limit is exactly a lattice distance: inclusive
        query, target, exclude, limit = 2 * lattice(6), None, True, 2.0
    elif name == "duplicates":                             # a box without extent: the one-cell grid
        query, target, exclude, limit = np.repeat(f32([[0.3, -1.2, 2.5]]), 77, axis=0), None, True, math.inf
    elif name == "duplicates_and_off":
        target = np.repeat(f32([[0.3, -1.2, 2.5]]), 40, axis=0)
        query, exclude, limit = np.concatenate([target[:10], gaussian(30, 5)]), False, math.inf
    elif name == "collinear":
        t = np.random.default_rng(6).uniform(-1, 1, 300)
        query, target, exclude, limit = f32(np.outer(t, [1.0, 2.0, -0.5]) + [0.1, 0.2, 0.3]), None, True, math.inf
    elif name == "coplanar":
        uv = np.random.default_rng(7).uniform(-1, 1, (600, 2))
        query, target, exclude, limit = f32(uv @ np.array([[1.0, 0.2, 0.0], [0.0, 1.0, 0.7]])), None, True, math.inf
    elif name == "coplanar_off":
        uv = np.random.default_rng(7).uniform(-1, 1, (600, 2))
        target = f32(np.concatenate([uv, np.zeros((600, 1))], axis=1))            # an axis without extent: one layer of cells
        query, exclude, limit = gaussian(200, 8), False, math.inf
    elif name == "far_points":
        query, target, exclude, limit = blob_with_far_points(), None, True, math.inf
    elif name == "far_points_limit":
        query, target, exclude, limit = blob_with_far_points(), None, True, 0.25
    elif name == "outside":
        target = f32(np.random.default_rng(9).uniform(0, 1, (1500, 3)))
        rng = np.random.default_rng(10)
        query = f32(np.concatenate([rng.uniform(-3, 4, (300, 3)), [[50, 0.5, 0.5], [0.5, -40, 0.5], [-30, -30, 60]]]))
        exclude, limit = False, math.inf
    elif name == "outside_limit":
        query, target, exclude, _ = case("outside")[:4]
        limit = 1.5
    elif name == "few_targets":                            # k greater than M - 1
        query, target, exclude, limit = gaussian(6, 12), None, True, math.inf
    else:
        raise KeyError(name)
    reference = outliers.nearest_neighbours(query, query if target is None else target, 32, limit, exclude)
    for a in (query, target) + reference:
        if a is not None:
            a.setflags(write=False)
    return query, target, exclude, limit, reference


def upload(dev, a):
    return torch.tensor(a, device=dev)               # (a copy: the cached arrays are read-only)


def same_bits(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    if got.size == 0:
        return
    if got.dtype.kind == "f":
        got, want = got.view(f"i{got.dtype.itemsize}"), want.view(f"i{want.dtype.itemsize}")
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)) if got.ndim else np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {len(got)} rows differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def assert_knn(dev, name, ks=KS):
    from dvmvs.hip import neighbours
    query, target, exclude, limit, (want_d, want_i) = case(name)
    q = upload(dev, query)
    t = q if target is None else upload(dev, target)
    for k in ks:
        dist, index = neighbours.knn(q, t, k, limit, exclude)
        assert dist.dtype == torch.float32 and index.dtype == torch.int32 and dist.shape == index.shape == (len(query), k)
        same_bits(index, np.ascontiguousarray(want_i[:, :k]))
        same_bits(dist, np.ascontiguousarray(want_d[:, :k]))
    return want_d, want_i


@pytest.mark.parametrize("N", [1, 2, 255, 257, 3001])
def test_cloud_against_itself(hip_device, N):
    want_d, want_i = assert_knn(hip_device, f"self{N}")
    assert (want_i != np.arange(N)[:, None]).all() and (want_i[:, min(N - 1, 32):] == -1).all()


@pytest.mark.parametrize("N", [1, 2, 255, 257, 3001])
def test_cloud_against_another(hip_device, N):
    assert_knn(hip_device, f"other{N}")


def test_one_neighbour_is_the_nearest_point_op(hip_device):
    from dvmvs.hip import neighbours, ops
    q, t = upload(hip_device, gaussian(1000, 20)), upload(hip_device, gaussian(700, 21))
    dist, index = neighbours.knn(q, t, 1)
    want_d, want_i = ops.nearest_distance(q, t, return_index=True)
    assert torch.equal(dist[:, 0].view(torch.int32), want_d.view(torch.int32)) and torch.equal(index[:, 0], want_i)
    grid = ops.nearest_build(t)                           # a prebuilt grid gives the same
    again = neighbours.knn(q, t, 1, grid=grid)
    assert torch.equal(again[0].view(torch.int32), dist.view(torch.int32)) and torch.equal(again[1], index)


@pytest.mark.parametrize("name", ["lattice", "lattice_limit", "duplicates", "duplicates_and_off"])
def test_ties_and_duplicates(hip_device, name):
    want_d, want_i = assert_knn(hip_device, name)
    if name == "lattice":                                  # ties everywhere: an inner point has 6 at 1, 12 at sqrt 2, 8 at sqrt 3
        inner = (1 * 6 + 1) * 6 + 1
        assert (want_d[inner, :6] == 1).all() and (np.diff(want_i[inner, :6]) > 0).all() and (np.diff(want_i[inner, 6:18]) > 0).all()
    if name == "lattice_limit":
        assert (np.count_nonzero(want_i >= 0, axis=1) <= 6).all() and np.count_nonzero(want_i[(1 * 6 + 1) * 6 + 1] >= 0) == 6
    if name == "duplicates":                               # every other copy, in index order, at distance 0
        assert (want_d == 0).all() and want_i[5].tolist() == [j for j in range(33) if j != 5]


@pytest.mark.parametrize("name", ["collinear", "coplanar", "coplanar_off"])
def test_degenerate_clouds(hip_device, name):
    assert_knn(hip_device, name)


@pytest.mark.parametrize("name", ["far_points", "far_points_limit"])
def test_far_points_walk_far_unless_bounded(hip_device, name):
    want_d, want_i = assert_knn(hip_device, name, ks=(8, 20))
    if name == "far_points":
        to_blob = np.where(want_i[-20:] < 2000, want_d[-20:], np.inf).min(axis=1)       # at most 19 of the 32 are other far points
        assert (to_blob > 2.0).all() and (to_blob < np.inf).all() and (want_i[-20:, :20] >= 0).all()
    else:
        assert (want_i[-20:] == -1).all() and (want_i[:2000, :20] >= 0).all()          # the far points find nothing within the limit


@pytest.mark.parametrize("name", ["outside", "outside_limit", "few_targets"])
def test_queries_outside_the_box_and_few_targets(hip_device, name):
    want_d, want_i = assert_knn(hip_device, name)
    if name == "few_targets":
        assert (want_i[:, 5:] == -1).all() and (want_i[:, :5] >= 0).all()
    if name == "outside_limit":
        assert (want_i[-3:] == -1).all() and (want_i[:300, 0] >= 0).any()


def test_radius_count(hip_device):
    from dvmvs.hip import neighbours
    cloud = gaussian(3001, 30)
    q = upload(hip_device, cloud)
    for radius, cap in ((0.25, 1), (0.25, 6), (0.25, 10000), (0.0, 3), (100.0, 3000), (100.0, 3001)):
        want = outliers.radius_count(cloud, cloud, radius, cap, exclude_same_index=True)
        count = neighbours.radius_count(q, q, radius, cap, True)
        assert count.dtype == torch.int32
        same_bits(count, want)
    want = outliers.radius_count(cloud, cloud, 0.25, 6, exclude_same_index=True)
    assert (want < 6).any() and (want == 6).any() and outliers.radius_count(cloud, cloud, 0.25, 10000, True).max() > 6     # below, at, above
    other, lat = gaussian(500, 31), lattice(6)
    same_bits(neighbours.radius_count(upload(hip_device, other), q, 0.3, 4), outliers.radius_count(other, cloud, 0.3, 4))
    same_bits(neighbours.radius_count(upload(hip_device, other), q, 0.0, 4), outliers.radius_count(other, cloud, 0.0, 4))
    for radius in (0.0, 1.0, float(np.sqrt(np.float32(2))), 2.0):                       # ties at the limit; radius 0 counts the point itself
        for exclude in (False, True):
            same_bits(neighbours.radius_count(upload(hip_device, lat), upload(hip_device, lat), radius, 7, exclude),
                      outliers.radius_count(lat, lat, radius, 7, exclude))
    duplicates = np.repeat(f32([[1, 2, 3]]), 50, axis=0)
    same_bits(neighbours.radius_count(upload(hip_device, duplicates), upload(hip_device, duplicates), 0.0, 60, True),
              np.full(50, 49, dtype=np.int32))
    same_bits(outliers.radius_outliers_device(q, 0.25, 6).cpu().numpy(), outliers.radius_outliers(cloud, 0.25, 6))


def test_repeatable_on_any_stream_and_at_any_alignment(hip_device):
    from dvmvs.hip import neighbours
    query, _, _, _, (want_d, want_i) = case("self3001")
    q = upload(hip_device, query)
    first = neighbours.knn(q, q, 20, exclude_same_index=True)
    second = neighbours.knn(q, q, 20, exclude_same_index=True)
    same_bits(first[0], np.ascontiguousarray(want_d[:, :20]))
    same_bits(first[1], np.ascontiguousarray(want_i[:, :20]))
    assert torch.equal(first[0].view(torch.int32), second[0].view(torch.int32)) and torch.equal(first[1], second[1])
    buffer = torch.zeros(3 * len(query) + 5, device=hip_device)
    shifted = buffer[1:1 + 3 * len(query)].view(-1, 3)                       # 4-byte aligned and no more
    shifted.copy_(q)
    assert shifted.data_ptr() % 8 == 4 and shifted.is_contiguous()
    third = neighbours.knn(shifted, shifted, 20, exclude_same_index=True)
    count = neighbours.radius_count(shifted, shifted, 0.25, 6, True)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        fourth = neighbours.knn(q, q, 20, exclude_same_index=True)
        count_side = neighbours.radius_count(q, q, 0.25, 6, True)
        keep_side = neighbours.outlier_statistics(*fourth, 1.0)
    side.synchronize()
    torch.cuda.current_stream(hip_device).wait_stream(side)
    for other in (third, fourth):
        assert torch.equal(first[0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(first[1], other[1])
    assert torch.equal(count, count_side)
    keep = neighbours.outlier_statistics(*first, 1.0)
    for a, b in zip(keep, keep_side):
        same_bits(a, b.cpu().numpy())


@functools.lru_cache(maxsize=None)
def noisy_cloud():
    """A sheet, a blob and stray points, with colours: [N,6]."""
    rng = np.random.default_rng(50)
    sheet = np.concatenate([rng.uniform(-1, 1, (1500, 2)), rng.normal(0, 0.01, (1500, 1))], axis=1)
    blob = rng.normal([0.3, 0.2, 0.5], 0.06, (700, 3))
    stray = rng.uniform(-3, 3, (40, 3))
    xyz = np.concatenate([sheet, blob, stray])
    order = rng.permutation(len(xyz))
    cloud = f32(np.concatenate([xyz[order], rng.integers(0, 256, (len(xyz), 3))], axis=1))
    cloud.setflags(write=False)
    return cloud


@pytest.mark.parametrize("neighbours,ratio,limit", [(20, 2.0, math.inf), (8, 0.0, math.inf), (32, 1.0, 0.3), (1, 3.0, 0.05)])
def test_statistical_outliers(hip_device, neighbours, ratio, limit):
    cloud = noisy_cloud()
    want_keep, want_mean, want_stats = outliers.statistical_outliers(cloud[:, :3], neighbours, ratio, limit)
    keep, mean, stats = outliers.statistical_outliers_device(upload(hip_device, cloud[:, :3]), neighbours, ratio, limit)
    assert keep.dtype == torch.bool and mean.dtype == torch.float32 and stats.dtype == torch.float64 and stats.shape == (4,)
    print(f"neighbours {neighbours} ratio {ratio} limit {limit}: stats {stats.cpu().tolist()} want {want_stats.tolist()}, kept {int(keep.sum())}")
    same_bits(mean, want_mean)
    same_bits(stats, want_stats)
    same_bits(keep, want_keep)
    assert 0 < want_keep.sum() < len(cloud)
    if limit < 1:
        assert np.isinf(want_mean).any() and want_stats[0] == np.isfinite(want_mean).sum() < len(cloud)     # points without a neighbour


def test_statistics_of_few_points(hip_device):
    """n = 0, 1, 2 valid points, and rows of every length."""
    from dvmvs.hip import neighbours
    for points, k, limit in ((f32([[0, 0, 0]]), 3, math.inf), (f32([[0, 0, 0], [0, 0, 1], [9, 9, 9]]), 1, 0.5),
                             (f32([[0, 0, 0], [0, 0, 1], [0, 0, 3]]), 1, 1.5), (f32([[0, 0, 0], [0, 0, 1], [0, 0, 3]]), 2, math.inf),
                             (gaussian(1025, 60), 5, math.inf)):
        want = outliers.statistical_outliers(points, k, 2.0, limit)
        got = neighbours.statistical_outliers(upload(hip_device, points), k, 2.0, limit)
        for g, w in zip(got, want):
            same_bits(g, w)
    dist = upload(hip_device, f32([[2.0, np.inf], [np.inf, np.inf]]))
    index = torch.tensor([[4, -1], [-1, -1]], dtype=torch.int32, device=hip_device)
    keep, mean, stats = neighbours.outlier_statistics(dist, index, 2.0)                  # n = 1: sigma is 0, the point stays
    assert keep.cpu().tolist() == [True, False] and mean.cpu().tolist() == [2.0, math.inf] and stats.cpu().tolist() == [1, 2, 0, 2]


@pytest.mark.parametrize("filter", [OutlierFilter(neighbours=20), OutlierFilter(neighbours=8, ratio=1.0, max_distance=0.3),
                                    OutlierFilter(radius=0.08, min_neighbours=5), OutlierFilter(12, 1.5, None, 0.08, 5)])
def test_filter_outliers(hip_device, filter):
    cloud = noisy_cloud()
    want, want_mask = outliers.filter_outliers(cloud, filter, return_mask=True)
    got, mask = outliers.filter_outliers_device(upload(hip_device, cloud), filter, return_mask=True)
    same_bits(mask, want_mask)
    same_bits(got, want)
    same_bits(outliers.filter_outliers_device(upload(hip_device, cloud), filter), want)
    assert got.shape[1] == 6 and 0 < len(want) < len(cloud)
    xyz_only = outliers.filter_outliers_device(upload(hip_device, cloud[:, :3]), filter)
    same_bits(xyz_only, np.ascontiguousarray(want[:, :3]))


def test_filter_of_an_empty_cloud_and_argument_checks(hip_device):
    from dvmvs.hip import neighbours
    empty = torch.zeros((0, 6), device=hip_device)
    for filter in (OutlierFilter(neighbours=20), OutlierFilter(radius=0.1, min_neighbours=2), OutlierFilter(5, 2.0, 1.0, 0.1, 2)):
        got, mask = outliers.filter_outliers_device(empty, filter, return_mask=True)
        assert got.shape == (0, 6) and mask.shape == (0,) and mask.dtype == torch.bool
    keep, mean, stats = neighbours.statistical_outliers(empty[:, :3])
    assert keep.shape == mean.shape == (0,) and stats.cpu().tolist() == [0, 0, 0, 0]
    q = torch.zeros((4, 3), device=hip_device)
    dist, index = neighbours.knn(empty[:, :3], q, 3)
    assert dist.shape == index.shape == (0, 3) and neighbours.radius_count(empty[:, :3], q, 1.0, 2).shape == (0,)
    with pytest.raises(ValueError, match="empty"):
        neighbours.knn(q, empty[:, :3], 3)
    with pytest.raises(ValueError, match="k must"):
        neighbours.knn(q, q, 0)
    with pytest.raises(ValueError, match="max_distance"):
        neighbours.knn(q, q, 3, max_distance=-1.0)
    with pytest.raises(ValueError, match="radius"):
        neighbours.radius_count(q, q, float("nan"), 3)
    with pytest.raises(ValueError, match="grid"):
        neighbours.knn(q, q, 3, grid=torch.zeros(16, dtype=torch.uint8, device=hip_device))
    with pytest.raises(ValueError, match="C >= 3"):
        neighbours.filter_outliers(torch.zeros((4, 2), device=hip_device), OutlierFilter(neighbours=3))
    with pytest.raises(ValueError):
        neighbours.knn(q.double(), q, 3)


# ---- the program --------------------------------------------------------------------------------------------------------------------
def test_program_cleans_the_point_cloud(hip_device, tmp_path, capsys):
    """``python -m dvmvs.tsdf --filter_consistency --save_point_cloud --clean_points_*`` on five 24x32 keyframes of the analytic scene of the
    consistency tests: ``_pointcloud_clean.ply`` holds exactly the rows of ``_pointcloud.ply`` that the host definition keeps of the cloud
    that was written, and every other file is what it is without the flags, byte for byte."""
    from PIL import Image
    from dvmvs.consistency import filter_depths, fused_point_cloud, nearest_sources
    from dvmvs.dataset_loader import PreprocessImage
    from dvmvs.tsdf import main
    depths, Ks, poses = (a[:5] for a in cr.clean_scene("24x32"))                   # five views: fewer than 4 000 points
    h, w = depths.shape[1:]
    scene_dir = tmp_path / "data" / "hololens-dataset" / "000"
    (scene_dir / "images").mkdir(parents=True)
    rng = np.random.default_rng(5)
    names = [f"{i:05d}.png" for i in range(5)]
    for name in names:
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(scene_dir / "images" / name)
    np.savetxt(scene_dir / "poses.txt", poses.reshape(-1, 16).astype(np.float64))
    np.savetxt(scene_dir / "K.txt", Ks[0].astype(np.float64))
    (tmp_path / "data" / "indices").mkdir()
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("\n".join(f"{n} {n}" for n in names) + "\n")
    (tmp_path / "pred").mkdir()
    system = "320_256_3_dvmvs_fusionnet_online"
    np.savez(tmp_path / "pred" / f"keyframe_hololens-dataset_{system}_predictions_000.npz", depths)
    common = ["--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"), "--voxel_size", "0.05",
              "--filter_consistency", "--save_point_cloud"]
    flags = OutlierFilter(neighbours=8, ratio=1.0, max_distance=0.5, radius=0.12, min_neighbours=25)
    main(["--reconstruction_folder", str(tmp_path / "plain")] + common)
    capsys.readouterr()
    main(["--reconstruction_folder", str(tmp_path / "cleaned"), "--clean_points_neighbours", "8", "--clean_points_ratio", "1.0",
          "--clean_points_max_distance", "0.5", "--clean_points_radius", "0.12", "--clean_points_min_neighbours", "25"] + common)
    printed = capsys.readouterr().out

    stem = f"reconstruction_voxelsize-0.05_maxdepth-5.0_anchor-False_{system}+consistent_hololens-dataset_000"
    before = sorted(os.listdir(tmp_path / "plain"))
    assert before == [stem + "_complete.ply", stem + "_pointcloud.ply"]
    assert sorted(os.listdir(tmp_path / "cleaned")) == sorted(before + [stem + "_pointcloud_clean.ply"])
    for name in before:
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "cleaned" / name, "rb").read(), name

    # the cloud that was written, with its float32 coordinates (the file holds six decimals of them), and what the host definition keeps
    scaled_K = PreprocessImage(K=Ks[0], old_width=w, old_height=h, new_width=w, new_height=h, distortion_crop=0,
                               perform_crop=False).get_updated_intrinsics()
    averaged, _, points = filter_depths(depths, scaled_K, poses, nearest_sources(5, 4), min_views=2, average=True, with_points=True,
                                        device=hip_device)
    xyz = fused_point_cloud(averaged, points).cpu().numpy()
    header, body = open(tmp_path / "cleaned" / (stem + "_pointcloud.ply")).read().split("end_header\n")
    rows = body.splitlines()
    assert len(rows) == len(xyz) <= 4000 and f"element vertex {len(xyz)}\n" in header
    assert np.abs(np.array([r.split()[:3] for r in rows], dtype=np.float64) - xyz).max() < 2e-6
    _, mask = outliers.filter_outliers(xyz, flags, return_mask=True)
    statistical = outliers.statistical_outliers(xyz, 8, 1.0, 0.5)[0]
    print(f"{len(xyz)} points, the statistical filter keeps {statistical.sum()}, both keep {mask.sum()}")
    assert 0 < mask.sum() < statistical.sum() < len(xyz)                           # each filter removes something
    clean_header, clean_body = open(tmp_path / "cleaned" / (stem + "_pointcloud_clean.ply")).read().split("end_header\n")
    assert clean_body.splitlines() == [row for row, kept in zip(rows, mask) if kept]
    assert clean_header == header.replace(f"element vertex {len(xyz)}\n", f"element vertex {int(mask.sum())}\n")
    assert f"Outlier filter: kept {100.0 * mask.sum() / len(xyz):.1f} % of the {len(xyz)} points" in printed
