"""GPU: the implicit surface of an oriented cloud on the device (csrc/implicit_surface.hip through dvmvs/hip/implicit.py) against the host
definition (dvmvs/implicit.py), bit for bit at every node of every case of tests/implicit_cases.py (which also shows that the band misses
nothing), chunking, alignment, streams, the trim flags, the meshes of a sphere and a plane, and the program's ``--point_mesh_*`` flags."""
import os

import numpy as np
import pytest
import torch

import consistency_reference as cr
import implicit_cases as ic
from dvmvs import implicit as im

pytestmark = pytest.mark.gpu

CASES = ic.cases()


def upload(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_arguments(dev, c):
    return (upload(dev, c["points"]), upload(dev, c["normals"]), c["origin"], c["voxel"], c["dims"], c["radius"], c["neighbours"],
            c["min_neighbours"])


def same_volume(got, want):
    """``(volume, valid)`` of the device against the host's: dtypes, shapes and every bit."""
    for name, g, w in zip(("volume", "valid"), got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bits = np.uint32 if g.dtype == np.float32 else np.uint8
            different = np.argwhere(g.view(bits) != w.view(bits))
            first = tuple(different[0])
            raise AssertionError(f"{name}: {len(different)} of {g.size} nodes differ, first {first}: {g[first]!r} != {w[first]!r}")


@pytest.mark.parametrize("name", list(CASES))
def test_every_node_of_every_case(hip_device, name):
    """The device's banded evaluation equals the dense host form at EVERY node, in volume and in valid: no node with a candidate was left
    out of the band, and the values are the host's bits.  The inputs are left as they were."""
    c = CASES[name]
    args = device_arguments(hip_device, c)
    got = im.implicit_volume_device(*args)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.bool and got[0].device == hip_device
    same_volume(got, ic.host_volume(name))
    assert np.array_equal(args[0].cpu().numpy(), c["points"]) and np.array_equal(args[1].cpu().numpy(), c["normals"])


def test_band_is_a_superset_and_stays_inside_the_grid(hip_device):
    """The mask holds every node with a candidate of the float32 search (dense brute force on the host), on the case with d2 == radius^2
    and on the one with points outside the grid on every side; written between guard bytes that stay as they were."""
    from dvmvs.hip import implicit as binding
    from dvmvs.outliers import nearest_neighbours
    for name in ("exact-boundary", "points-outside", "small-radius", "thin-x-1x9x7"):
        c = CASES[name]
        mask = binding.band(upload(hip_device, c["points"]), c["origin"], c["voxel"], c["dims"], c["radius"]).cpu().numpy()
        assert mask.dtype == np.uint8 and mask.shape == c["dims"] and set(np.unique(mask)) <= {0, 1}
        nodes = im.node_positions(c["origin"], c["voxel"], c["dims"])
        has = (nearest_neighbours(nodes, c["points"], 1, np.float32(c["radius"]), False)[1][:, 0] >= 0).reshape(c["dims"])
        assert has.any() and (mask[has] == 1).all(), name
    assert mask_of_case_in_guarded_buffer(hip_device, CASES["points-outside"])


def mask_of_case_in_guarded_buffer(dev, c):
    """The band entry called on a mask in the middle of a buffer of 7s: the bytes around it are untouched."""
    from dvmvs.hip.ops._common import launch, ptr
    total = int(np.prod(c["dims"]))
    buffer = torch.full((total + 4096,), 7, dtype=torch.uint8, device=dev)
    buffer[2048:2048 + total] = 0
    points = upload(dev, c["points"])
    o = [float(v) for v in c["origin"]]
    launch("dvmvs_implicit_band_fwd", dev, ptr(points), len(c["points"]), o[0], o[1], o[2], float(np.float32(c["voxel"])), *c["dims"],
           float(np.float32(c["radius"])), buffer[2048:].data_ptr())
    buffer = buffer.cpu().numpy()
    return (buffer[:2048] == 7).all() and (buffer[2048 + total:] == 7).all() and buffer[2048:2048 + total].any()


def test_chunks_alignment_layout_and_streams(hip_device):
    """``nodes_per_chunk = 64`` (dozens of chunks, the last one short), tensors offset by one element (4-byte and not 16-byte aligned),
    inputs that are not contiguous, a given grid and a side stream: the bytes of the default call."""
    from dvmvs.hip import implicit as binding, ops
    name = "sheet-k32-33x17x12"
    c = CASES[name]
    want = ic.host_volume(name)
    points, normals = upload(hip_device, c["points"]), upload(hip_device, c["normals"])
    rest = (c["origin"], c["voxel"], c["dims"], c["radius"], c["neighbours"], c["min_neighbours"])
    same_volume(binding.implicit_volume(points, normals, *rest), want)
    same_volume(binding.implicit_volume(points, normals, *rest, nodes_per_chunk=64), want)
    same_volume(binding.implicit_volume(points, normals, *rest, nodes_per_chunk=257), want)
    same_volume(binding.implicit_volume(points, normals, *rest, grid=ops.nearest_build(points)), want)

    def shifted(a):
        buffer = torch.zeros(a.numel() + 5, dtype=a.dtype, device=hip_device)
        out = buffer[1:1 + a.numel()].view(a.shape)
        out.copy_(a)
        assert out.data_ptr() % 8 == 4 and out.is_contiguous()
        return out

    same_volume(binding.implicit_volume(shifted(points), shifted(normals), *rest), want)

    def strided(a):
        wide = torch.zeros(a.shape[:-1] + (2 * a.shape[-1],), dtype=a.dtype, device=hip_device)
        out = wide[..., ::2]
        out.copy_(a)
        assert not out.is_contiguous()
        return out

    same_volume(binding.implicit_volume(strided(points), strided(normals), *rest), want)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        other = binding.implicit_volume(points, normals, *rest)
    side.synchronize()
    torch.cuda.current_stream(hip_device).wait_stream(side)
    same_volume(other, want)
    assert np.array_equal(points.cpu().numpy(), c["points"]) and np.array_equal(normals.cpu().numpy(), c["normals"])


def test_nothing_outside_the_cloud_is_read(hip_device):
    """The cloud and its normals between eight rows of NaN on either side: a slot of -1 (the short rows of the bounded search) or any
    index outside [0, M) that were read would bring a NaN into the sums."""
    from dvmvs.hip import implicit as binding
    for name in ("cloud-n2-9x7x5", "small-radius", "sheet-k32-33x17x12"):
        c = CASES[name]
        M = len(c["points"])
        padded = [torch.full((M + 16, 3), float("nan"), device=hip_device) for _ in range(2)]
        padded[0][8:8 + M] = upload(hip_device, c["points"])
        padded[1][8:8 + M] = upload(hip_device, c["normals"])
        got = binding.implicit_volume(padded[0][8:8 + M], padded[1][8:8 + M], c["origin"], c["voxel"], c["dims"], c["radius"], c["neighbours"],
                                      c["min_neighbours"])
        same_volume(got, ic.host_volume(name))


@pytest.mark.parametrize("name", list(CASES))
def test_trim_flags_on_the_device_s_own_mesh(hip_device, name):
    """Marching cubes of the device's volume in index space, then the trim kernel: its flags, and the compacted mesh, are ``trim_mesh``'s
    on the same vertices and faces."""
    from dvmvs.hip import implicit as binding
    from dvmvs.tsdf import marching_cubes
    volume, valid = im.implicit_volume_device(*device_arguments(hip_device, CASES[name]))
    verts, faces, _, _ = marching_cubes(volume, 0.0, None, (0.0, 0.0, 0.0), 1.0)
    keep_vertex, keep_face = binding.trim_flags(verts, faces, valid)
    assert keep_vertex.dtype == torch.bool and keep_face.dtype == torch.bool
    v, f, ok = verts.cpu().numpy(), faces.cpu().numpy(), valid.cpu().numpy()
    want_verts, want_faces, kept = im.trim_mesh(v, f, ok)
    want_vertex = np.zeros(len(v), bool)
    want_vertex[kept] = True
    assert np.array_equal(keep_vertex.cpu().numpy(), want_vertex)
    assert np.array_equal(keep_face.cpu().numpy(), want_vertex[f].all(axis=1) if len(f) else np.zeros(0, bool))
    got = im.trim_mesh_device(verts, faces, valid)
    assert got[1].dtype == torch.int32 and got[2].dtype == torch.int64
    assert got[0].cpu().numpy().tobytes() == want_verts.tobytes() and np.array_equal(got[1].cpu().numpy(), want_faces)
    assert np.array_equal(got[2].cpu().numpy(), kept)
    if len(v):                                                            # two whole coordinates, the third on a grid edge
        assert ((v == np.floor(v)).sum(axis=1) >= 2).all()
    if name in ("sphere", "plane", "sheet-k32-33x17x12"):
        assert 0 < want_vertex.sum() < len(v)                             # the fill invents crossings, and the trim removes them


def edges_of(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    return np.unique(np.sort(e, axis=1), axis=0, return_counts=True)


def nearest_index(verts, points):
    """The smallest index of a nearest point under the float32 contract ``(dx dx + dy dy) + dz dz``."""
    out = np.zeros(len(verts), np.int64)
    for begin in range(0, len(verts), 512):
        d = verts[begin:begin + 512, None, :] - points[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[begin:begin + 512] = d2.argmin(axis=1)
    return out


def test_sphere_mesh_is_closed_and_where_it_must_be(hip_device):
    """A crossing lies on an edge between a valid node with value < 0, which has r^2 < R^2 + radius^2, and one with value >= 0, which has
    r^2 >= R^2 (tests/test_implicit_reference.py derives both), one voxel apart: R - voxel <= |v| <= sqrt(R^2 + radius^2) + voxel.  A
    closed surface of genus 0: every edge in exactly two faces, V - E + F = 2.  Without the trim the crossings to the fill inside and
    outside the band are further shells."""
    c = CASES["sphere"]
    rng = np.random.default_rng(1)
    colours = rng.integers(0, 256, size=(len(c["points"]), 3)).astype(np.float32)
    cloud = upload(hip_device, np.concatenate([c["points"], colours], axis=1))
    verts, faces, normals, colors = im.mesh_points_device(cloud, upload(hip_device, c["normals"]), ic.SPHERE_VOXEL, ic.SPHERE_RADIUS)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and normals.dtype == torch.float32 and colors.dtype == torch.uint8
    v, f, n, col = (a.cpu().numpy() for a in (verts, faces, normals, colors))
    assert v.shape[1:] == (3,) and f.shape[1:] == (3,) and n.shape == v.shape and col.shape == v.shape and len(v) > 1000
    assert f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    voxel, radius = float(np.float32(ic.SPHERE_VOXEL)), float(np.float32(ic.SPHERE_RADIUS))
    print(f"sphere mesh: {len(v)} vertices, {len(f)} faces, |v| in [{r.min():.4f}, {r.max():.4f}]")
    assert (r >= ic.SPHERE_R - voxel).all() and (r <= np.sqrt(ic.SPHERE_R ** 2 + radius ** 2) + voxel).all()
    edges, counts = edges_of(f)
    assert (counts == 2).all()
    assert len(v) - len(edges) + len(f) == 2
    # normals and colours are those of the nearest cloud point; the normals point outward, the faces are counter-clockwise from outside
    nearest = nearest_index(v, c["points"])
    assert n.tobytes() == c["normals"][nearest].tobytes() and np.array_equal(col, colours[nearest].astype(np.uint8))
    assert ((n.astype(np.float64) * v).sum(axis=1) > 0).all()
    a, b, d = (v[f[:, i]].astype(np.float64) for i in range(3))
    assert ((np.cross(b - a, d - a) * (a + b + d)).sum(axis=1) > 0).all()
    # the untrimmed surface has the extra shells: more than one closed piece, so this test fails without the trim
    from dvmvs.tsdf import marching_cubes
    volume, _ = im.implicit_volume_device(upload(hip_device, c["points"]), upload(hip_device, c["normals"]), c["origin"], c["voxel"],
                                          c["dims"], c["radius"])
    raw = marching_cubes(volume, 0.0, None, (0.0, 0.0, 0.0), 1.0)
    assert raw[0].shape[0] > len(v) and raw[1].shape[0] > len(f)


def test_plane_mesh(hip_device):
    c = CASES["plane"]
    verts, faces, normals, colors = im.mesh_points_device(upload(hip_device, c["points"]), upload(hip_device, c["normals"]), 0.05, 0.125)
    assert colors is None
    v, f, n = verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy()
    assert len(v) > 100 and len(f) > 100 and f.max() < len(v)
    print("plane mesh: max |z - c| =", np.abs(v[:, 2].astype(np.float64) - float(ic.PLANE_C)).max())
    assert (np.abs(v[:, 2].astype(np.float64) - float(ic.PLANE_C)) <= 1e-5).all()
    a, b, d = (v[f[:, i]].astype(np.float64) for i in range(3))
    assert (np.cross(b - a, d - a)[:, 2] > 0).all()                       # counter-clockwise seen from +z, the side the normals point to
    assert (n == np.array([0, 0, 1], np.float32)).all()
    # the same through bounds: the grid of the case, which the cloud does not fill
    bounded = im.mesh_points_device(upload(hip_device, c["points"]), upload(hip_device, c["normals"]), c["voxel"], c["radius"],
                                    bounds=(c["origin"], c["dims"]))
    assert bounded[0].shape[0] > 100 and (np.abs(bounded[0].cpu().numpy()[:, 2].astype(np.float64) - float(ic.PLANE_C)) <= 1e-5).all()


def test_points_outside_the_given_bounds(hip_device):
    """A cloud that reaches past the grid of ``bounds`` on every side: the mesh is the trimmed marching cubes of the host's dense volume
    on that grid, and lies inside it."""
    from dvmvs.tsdf import marching_cubes
    c = CASES["points-outside"]
    points, normals = upload(hip_device, c["points"]), upload(hip_device, c["normals"])
    verts, faces, _, _ = im.mesh_points_device(points, normals, c["voxel"], c["radius"], c["neighbours"], c["min_neighbours"],
                                               bounds=(c["origin"], c["dims"]))
    volume, valid = ic.host_volume("points-outside")
    raw = marching_cubes(upload(hip_device, np.array(volume)), 0.0, None, (0.0, 0.0, 0.0), 1.0)
    want_verts, want_faces, _ = im.trim_mesh(raw[0].cpu().numpy(), raw[1].cpu().numpy(), valid)
    world = want_verts * np.float32(c["voxel"]) + c["origin"]
    assert len(want_faces) > 0 and np.array_equal(faces.cpu().numpy(), want_faces) and verts.cpu().numpy().tobytes() == world.tobytes()
    low, high = c["origin"], c["origin"] + np.float32(c["voxel"]) * (np.array(c["dims"], np.float32) - 1)
    assert (verts.cpu().numpy() >= low).all() and (verts.cpu().numpy() <= high).all()      # rounding is monotone: the last node bounds them


def test_empty_band_and_no_valid_normal(hip_device):
    points, normals = upload(hip_device, CASES["tiny-radius"]["points"]), upload(hip_device, CASES["tiny-radius"]["normals"])
    c = CASES["tiny-radius"]
    for mesh in (im.mesh_points_device(points, normals, c["voxel"], c["radius"], bounds=(c["origin"], c["dims"])),
                 im.mesh_points_device(points, torch.zeros_like(normals), 0.15, 0.35),
                 im.mesh_points_device(torch.cat([points, 255 * torch.rand_like(points)], dim=1), torch.zeros_like(normals), 0.15, 0.35)):
        assert mesh[0].shape == (0, 3) and mesh[1].shape == (0, 3) and mesh[2].shape == (0, 3)
        assert mesh[0].dtype == torch.float32 and mesh[1].dtype == torch.int32
    assert mesh[3].shape == (0, 3) and mesh[3].dtype == torch.uint8
    with pytest.raises(ValueError, match="empty"):
        im.mesh_points_device(points[:0], normals[:0], 0.15, 0.35)
    with pytest.raises(ValueError, match="cloud"):
        im.mesh_points_device(torch.zeros((5, 4), device=hip_device), normals[:5], 0.15, 0.35)
    with pytest.raises(ValueError, match="normals"):
        im.mesh_points_device(points, normals[:5], 0.15, 0.35)
    with pytest.raises(ValueError, match="neighbours"):
        im.mesh_points_device(points, normals, 0.15, 0.35, neighbours=33)
    with pytest.raises(ValueError, match="radius"):
        im.mesh_points_device(points, normals, 0.15, float("inf"))


def test_clean_passes_through_to_the_component_filter(hip_device):
    """The plane patch and a small one far from it: two components; ``clean`` keeps the largest, as ``filter_components_device`` does on
    the unfiltered mesh."""
    from dvmvs.components import ComponentFilter, filter_components_device
    points, normals = ic.plane_patch()
    small, small_normals = ic.plane_patch(4)
    cloud = upload(hip_device, np.concatenate([points, small + np.array([2.0, 0.0, 0.0], np.float32)]))
    normals = upload(hip_device, np.concatenate([normals, small_normals]))
    clean = ComponentFilter(keep_largest=True)
    plain = im.mesh_points_device(cloud, normals, 0.05, 0.125)
    cleaned = im.mesh_points_device(cloud, normals, 0.05, 0.125, clean=clean)
    want = filter_components_device(plain[0], plain[1], clean, plain[2], plain[3])
    assert 0 < cleaned[1].shape[0] < plain[1].shape[0] and (plain[0][:, 0] > 1.5).any() and not (cleaned[0][:, 0] > 1.5).any()
    for got, expected in zip(cleaned[:3], want[:3]):
        assert torch.equal(got, expected)


# ---- the program --------------------------------------------------------------------------------------------------------------------
def write_scene(tmp_path, depths, Ks, poses, system):
    """Five keyframes of the analytic scene of the consistency tests as the folders ``python -m dvmvs.tsdf`` reads."""
    from PIL import Image
    h, w = depths.shape[1:]
    scene_dir = tmp_path / "data" / "hololens-dataset" / "000"
    (scene_dir / "images").mkdir(parents=True)
    rng = np.random.default_rng(5)
    names = [f"{i:05d}.png" for i in range(len(depths))]
    for name in names:
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(scene_dir / "images" / name)
    np.savetxt(scene_dir / "poses.txt", poses.reshape(-1, 16).astype(np.float64))
    np.savetxt(scene_dir / "K.txt", Ks[0].astype(np.float64))
    (tmp_path / "data" / "indices").mkdir()
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("\n".join(f"{n} {n}" for n in names) + "\n")
    (tmp_path / "pred").mkdir()
    np.savez(tmp_path / "pred" / f"keyframe_hololens-dataset_{system}_predictions_000.npz", depths)
    return ["--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"), "--voxel_size", "0.05",
            "--filter_consistency", "--save_point_cloud", "--point_normals_neighbours", "10", "--point_normals_max_distance", "0.15"]


def test_program_writes_the_mesh(hip_device, tmp_path, capsys):
    """``python -m dvmvs.tsdf ... --point_mesh_voxel`` on five 24x32 keyframes: ``_pointcloud_mesh.ply`` is a readable mesh, the one
    ``mesh_points_device`` makes of the cloud in ``_pointcloud_normals.ply``, and every other file is what it is without the flags."""
    from dvmvs.tsdf import TSDFFusion, main
    depths, Ks, poses = (a[:5] for a in cr.clean_scene("24x32"))
    system = "320_256_3_dvmvs_fusionnet_online"
    common = write_scene(tmp_path, depths, Ks, poses, system)
    main(["--reconstruction_folder", str(tmp_path / "plain")] + common)
    capsys.readouterr()
    main(["--reconstruction_folder", str(tmp_path / "mesh"), "--point_mesh_voxel", "0.05", "--point_mesh_radius", "0.15",
          "--point_mesh_neighbours", "16", "--point_mesh_min_neighbours", "2"] + common)
    printed = capsys.readouterr().out
    stem = f"reconstruction_voxelsize-0.05_maxdepth-5.0_anchor-False_{system}+consistent_hololens-dataset_000"
    before = sorted(os.listdir(tmp_path / "plain"))
    assert sorted(os.listdir(tmp_path / "mesh")) == sorted(before + [stem + "_pointcloud_mesh.ply"])
    for name in before:
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "mesh" / name, "rb").read(), name
    verts, faces = TSDFFusion.meshread(str(tmp_path / "mesh" / (stem + "_pointcloud_mesh.ply")))
    assert len(verts) > 0 and len(faces) > 0 and faces.min() >= 0 and faces.max() < len(verts)
    assert f"Point mesh: {len(verts)} vertices and {len(faces)} faces" in printed
    # the mesh of the cloud that the normals file holds, made again from the scene: the same faces, the same vertices as the file prints them
    from dvmvs.consistency import filter_depths, fused_point_cloud, fused_point_views, nearest_sources
    from dvmvs.dataset_loader import PreprocessImage
    from dvmvs.normals import estimate_normals_device
    h, w = depths.shape[1:]
    scaled_K = PreprocessImage(K=Ks[0], old_width=w, old_height=h, new_width=w, new_height=h, distortion_crop=0,
                               perform_crop=False).get_updated_intrinsics()
    averaged, _, points = filter_depths(depths, scaled_K, poses, nearest_sources(5, 4), min_views=2, average=True, with_points=True,
                                        device=hip_device)
    xyz = fused_point_cloud(averaged, points)
    centres = upload(hip_device, poses.astype(np.float32)[:, :3, 3])
    normals, _, valid = estimate_normals_device(xyz, 10, 0.15, centres, fused_point_views(averaged))
    assert int(valid.sum()) > 100
    want = im.mesh_points_device(xyz[valid], normals[valid], 0.05, 0.15, 16, 2)
    assert np.array_equal(want[1].cpu().numpy(), faces)
    printed_verts = np.array([["%f" % x for x in row] for row in want[0].cpu().numpy()]).astype(np.float32)
    assert np.array_equal(printed_verts, verts)
    # the flag combinations that must raise do
    for drop in ("--point_normals_neighbours", "--save_point_cloud", "--filter_consistency"):
        argv = ["--reconstruction_folder", str(tmp_path / "refused"), "--point_mesh_voxel", "0.05"] + common
        at = argv.index(drop)
        del argv[at:at + (2 if drop == "--point_normals_neighbours" else 1)]
        if drop == "--point_normals_neighbours":
            at = argv.index("--point_normals_max_distance")
            del argv[at:at + 2]
        with pytest.raises(ValueError):
            main(argv)
    with pytest.raises(ValueError, match="point_mesh_voxel"):
        main(["--reconstruction_folder", str(tmp_path / "refused"), "--point_mesh_radius", "0.1"] + common)
    assert not (tmp_path / "refused").exists()
