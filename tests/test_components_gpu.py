"""GPU: connected components and cleaning of a mesh (csrc/mesh_components.hip, dvmvs.hip.components) against the host definition
(dvmvs/components.py) bit for bit, on the meshes of tests/components_reference.py, and the surface built on them: ``TSDFVolume``'s ``clean``
keywords and the program's ``--clean_mesh_*`` flags.  The host definition of a case is computed once and never modified."""
import os

import numpy as np
import pytest
import torch

import components_reference as cr
from dvmvs.components import ComponentFilter, filter_components, mesh_components

pytestmark = pytest.mark.gpu

PARTS = ("labels", "face_labels", "face_count", "area")


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def upload(dev, case):
    return {k: torch.from_numpy(np.array(v)).to(dev) for k, v in case.items()}          # (a copy: the cases are read-only)


def assert_parts(got, want, label):
    for key in PARTS:
        g = got[key].cpu().numpy()
        assert g.dtype == want[key].dtype and g.shape == want[key].shape and bits(g) == bits(want[key]), (label, key)
    assert got["n_components"].dtype == torch.int64 and got["n_components"].dim() == 0 and got["n_components"].is_cuda
    assert int(got["n_components"]) == want["n_components"] and int(got["status"]) == 0, label


def assert_filtered(got, want, label):
    """``filter_components(..., return_index=True)`` of the device against ``components_reference.host_filtered``."""
    flat = list(got[:4]) + list(got[4])
    for name, g, w in zip(("verts", "faces", "normals", "colors", "vertex_index", "face_index"), flat, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and bits(g) == bits(w), (label, name, g.shape, w.shape)


@pytest.mark.parametrize("name", sorted(cr.CASES))
def test_components_and_filters_equal_the_host_definition(hip_device, name):
    from dvmvs.hip import components
    case, want = cr.case(name), cr.host(name)
    dev = upload(hip_device, case)
    V = len(case["verts"])
    got = components.mesh_components(dev["faces"], V, dev["verts"])
    assert_parts(got, want, name)
    bare = components.mesh_components(dev["faces"], V)
    assert "area" not in bare and bits(bare["labels"].cpu().numpy()) == bits(want["labels"])
    assert bits(bare["face_count"].cpu().numpy()) == bits(want["face_count"]) and int(bare["n_components"]) == want["n_components"]
    for rule in cr.filters(name):
        filtered = components.filter_components(dev["verts"], dev["faces"], rule, dev["normals"], dev["colors"], return_index=True)
        assert_filtered(filtered, cr.host_filtered(name, rule), (name, rule))
    # without the optional arrays and the indices
    rule = cr.filters(name)[0]
    verts, faces, normals, colors = components.filter_components(dev["verts"], dev["faces"], rule)
    want_filtered = cr.host_filtered(name, rule)
    assert normals is None and colors is None
    assert bits(verts.cpu().numpy()) == bits(want_filtered[0]) and bits(faces.cpu().numpy()) == bits(want_filtered[1])
    if name == "ties":                                                                 # the tie rules, on the device
        kept = components.filter_components(dev["verts"], dev["faces"], ComponentFilter(keep_largest=True), return_index=True)[4]
        assert kept[0].tolist() == [3, 4, 5, 6] and kept[1].tolist() == [1, 2]


def test_empty_results_and_the_module_level_twins(hip_device):
    from dvmvs import components
    case = cr.case("tetrahedra")
    dev = upload(hip_device, case)
    verts, faces, normals, colors, (vertex_index, face_index) = components.filter_components_device(
        dev["verts"], dev["faces"], ComponentFilter(min_faces=5), dev["normals"], dev["colors"], return_index=True)
    assert tuple(verts.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and tuple(normals.shape) == (0, 3) and tuple(colors.shape) == (0, 3)
    assert vertex_index.numel() == 0 and face_index.numel() == 0 and verts.is_cuda and colors.dtype == torch.uint8
    got = components.mesh_components_device(dev["faces"], len(case["verts"]), dev["verts"])
    assert_parts(got, cr.host("tetrahedra"), "twin")
    assert got["labels"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8] and got["face_labels"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, -1, -1]


@pytest.mark.parametrize("name", ["tetrahedra", "soup", "sized_1025_1025"])
def test_views_and_odd_offsets(hip_device, name):
    """Inputs that are non-contiguous views (every second row of a larger tensor, three of six columns) and views that begin one element
    past an aligned address."""
    from dvmvs.hip import components
    case, want = cr.case(name), cr.host(name)
    V, F = len(case["verts"]), len(case["faces"])
    rule = cr.filters(name)[2]

    def strided(a, dtype):
        wide = torch.zeros((2 * a.shape[0], 6), dtype=dtype, device=hip_device)
        view = wide[::2, 1:4]
        view.copy_(torch.from_numpy(np.array(a)))
        assert not view.is_contiguous()
        return view

    def offset(a, dtype):
        flat = torch.zeros(a.size + 1, dtype=dtype, device=hip_device)
        view = flat[1:].view(-1, 3)
        view.copy_(torch.from_numpy(np.array(a)))
        assert view.data_ptr() % (2 * view.element_size()) == view.element_size()
        return view

    for make in (strided, offset):
        verts, faces = make(case["verts"], torch.float32), make(case["faces"], torch.int32)
        normals, colors = make(case["normals"], torch.float32), make(case["colors"], torch.uint8)
        assert_parts(components.mesh_components(faces, V, verts), want, (name, make.__name__))
        filtered = components.filter_components(verts, faces, rule, normals, colors, return_index=True)
        assert_filtered(filtered, cr.host_filtered(name, rule), (name, make.__name__))


def test_two_calls_give_identical_bytes(hip_device):
    from dvmvs.hip import components
    for name in ("strip", "soup"):
        case = cr.case(name)
        dev = upload(hip_device, case)
        runs = []
        for _ in range(2):
            parts = components.mesh_components(dev["faces"], len(case["verts"]), dev["verts"])
            out = components.filter_components(dev["verts"], dev["faces"], cr.filters(name)[0], dev["normals"], dev["colors"], return_index=True)
            runs.append([bits(parts[k].cpu().numpy()) for k in PARTS] + [bits(t.cpu().numpy()) for t in list(out[:4]) + list(out[4])])
        assert runs[0] == runs[1], name


def test_status_1_is_a_value_error(hip_device):
    from dvmvs.hip import components
    case = cr.nan_face()
    dev = upload(hip_device, case)
    got = components.mesh_components(dev["faces"], len(case["verts"]), dev["verts"])
    assert int(got["status"]) == components.STATUS_AREA
    assert bits(got["labels"].cpu().numpy()) == bits(mesh_components(case["faces"], len(case["verts"]))["labels"])      # the labels need no area
    with pytest.raises(ValueError, match="not finite"):
        components.filter_components(dev["verts"], dev["faces"], ComponentFilter())
    # each face below 2^31 square metres, the four together above: decided exactly from the summed halves
    huge = torch.tensor([[0, 0, 0], [4e4, 0, 0], [0, 4e4, 0], [0, 0, 4e4]], dtype=torch.float32, device=hip_device)
    tet = torch.from_numpy(cr.TET.astype(np.int32)).to(hip_device)
    assert int(components.mesh_components(tet, 4, huge)["status"]) == components.STATUS_AREA
    with pytest.raises(ValueError, match="2\\^31 square metres"):
        components.filter_components(huge, tet, ComponentFilter())
    two = components.mesh_components(tet[:2].contiguous(), 4, huge)
    assert int(two["status"]) == 0 and int(two["area"][0]) == 2 * int(8e8 * 2 ** 32)
    for bad in (ComponentFilter(min_area=-1.0), ComponentFilter(min_faces=0.5), ComponentFilter(keep_largest=1)):
        with pytest.raises(ValueError):
            components.filter_components(huge, tet, bad)


# ---- the volume ---------------------------------------------------------------------------------------------------------------------------
VOXEL = 0.05
SPHERES = (((0.65, 1.2, 1.2), 0.4), ((1.75, 1.2, 1.2), 0.4))
BLOB = ((1.2, 0.4, 0.4), (1.3, 0.4, 0.4), 0.03)       # 3 cm around a segment from one grid corner to the next but one: 3 corners inside


def sphere_volume(dev, with_blob):
    """A 48^3 volume of 5 cm voxels whose zero iso-surface is two spheres of 40 cm and, ``with_blob``, a shell around three grid corners."""
    from dvmvs.tsdf import TSDFVolume
    vol = TSDFVolume(np.array([[0.0, 2.4]] * 3), VOXEL, device=dev)
    assert tuple(vol.vol_dim) == (48, 48, 48)
    grid = np.stack(np.meshgrid(*[np.arange(48) * VOXEL] * 3, indexing="ij"), axis=-1)
    sdf = np.full((48, 48, 48), np.inf)
    for centre, radius in SPHERES:
        sdf = np.minimum(sdf, np.linalg.norm(grid - np.array(centre), axis=-1) - radius)
    if with_blob:
        a, b, radius = (np.array(BLOB[0]), np.array(BLOB[1]), BLOB[2])
        along = np.clip((grid - a) @ (b - a) / ((b - a) @ (b - a)), 0.0, 1.0)
        sdf = np.minimum(sdf, np.linalg.norm(grid - (a + along[..., None] * (b - a)), axis=-1) - radius)
    vol._tsdf.copy_(torch.from_numpy(np.clip(sdf / (5 * VOXEL), -1.0, 1.0).astype(np.float32)))
    vol._color.copy_(torch.from_numpy(np.random.default_rng(3).integers(0, 2 ** 24, (48, 48, 48)).astype(np.float32)))
    return vol


def test_volume_cleaning_end_to_end(hip_device):
    from dvmvs import errors
    vol, reference = sphere_volume(hip_device, True), sphere_volume(hip_device, False)
    raw = vol.get_mesh()
    parts = mesh_components(raw[1], len(raw[0]), raw[0])
    counts = np.sort(parts["face_count"][parts["face_count"] > 0])
    print(f"{len(raw[0])} vertices, {len(raw[1])} faces in {parts['n_components']} components of {counts.tolist()} faces")
    assert parts["n_components"] == 3 and 8 <= counts[0] < 50 and counts[1] > 100     # the shell around the three corners, and the two spheres
    blob_label = int(np.flatnonzero(parts["face_count"] == counts[0])[0])
    rule = ComponentFilter(min_faces=100)
    want = filter_components(*raw[:2], rule, raw[2], raw[3])
    got = vol.get_mesh(clean=rule)
    assert len(got[1]) == len(raw[1]) - counts[0] and len(got[0]) == len(raw[0]) - int((parts["labels"] == blob_label).sum())
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and bits(g) == bits(w)
    # an area threshold does the same here, and the device tensors are the same mesh
    by_area = vol.get_mesh(clean=ComponentFilter(min_area=0.1))
    assert all(bits(g) == bits(w) for g, w in zip(by_area, want))
    verts, faces = vol.mesh_tensors(clean=rule)
    assert verts.is_cuda and bits(verts.cpu().numpy()) == bits(want[0]) and bits(faces.cpu().numpy()) == bits(want[1])
    assert bits(vol.vertices(clean=rule).cpu().numpy()) == bits(want[0])
    # the blob-free volume's mesh is what cleaning leaves (the blob is more than the truncation away from the spheres' faces)
    assert bits(reference.get_mesh()[0]) == bits(want[0]) and bits(reference.get_mesh()[1]) == bits(want[1])
    # scores: the reference is a cloud that the spheres alone explain
    cloud = reference.vertices()
    threshold = 0.02
    plain = vol.score_against(cloud, threshold=threshold)
    clean = vol.score_against(cloud, threshold=threshold, clean=rule)
    on_host_cleaned = errors.compute_reconstruction_errors_device(torch.from_numpy(want[0]).to(hip_device), cloud, threshold)
    assert bits(clean.cpu().numpy()) == bits(on_host_cleaned.cpu().numpy())
    unchanged = errors.compute_reconstruction_errors_device(torch.from_numpy(raw[0]).to(hip_device), cloud, threshold)
    assert bits(plain.cpu().numpy()) == bits(unchanged.cpu().numpy())                 # without the keyword: what it always was
    assert bits(vol.score_against(cloud, threshold=threshold, clean=None).cpu().numpy()) == bits(plain.cpu().numpy())
    print(f"precision at {threshold} m: {float(plain[3]):.6f} with the blob, {float(clean[3]):.6f} cleaned")
    assert float(plain[3]) < 1.0 and float(clean[3]) == 1.0 and float(clean[0]) == 0.0
    # sampled and down-sampled, with the reference as a volume: the prediction alone is cleaned
    density, voxel = 2000.0, 0.04
    sampled, sizes = vol.score_against(reference, threshold=threshold, return_sizes=True, sample_density=density, voxel=voxel, clean=rule)
    same, same_sizes = reference.score_against(reference, threshold=threshold, return_sizes=True, sample_density=density, voxel=voxel)
    assert sizes == same_sizes and bits(sampled.cpu().numpy()) == bits(same.cpu().numpy())
    swapped = reference.score_against(vol, threshold=threshold, sample_density=density, voxel=voxel, clean=rule)     # the reference keeps its blob
    assert float(swapped[4]) < 1.0
    points = vol.surface_points(density, voxel, clean=rule)
    assert bits(points.cpu().numpy()) == bits(reference.surface_points(density, voxel).cpu().numpy())


# ---- the program -------------------------------------------------------------------------------------------------------------------------
def test_program_cleans(hip_device, golden_dir, tmp_path):
    """``python -m dvmvs.tsdf --evaluate_3d`` on the two keyframes of the sample scene: without the flags two runs write the same bytes under
    the names and keys they always had; with ``--clean_mesh_faces`` the ``+clean`` files hold the cleaned mesh and the new keys."""
    from PIL import Image
    from dvmvs.components import filter_components_device
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.tsdf import TSDFFusion, main
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
    system = "320_256_3_dvmvs_fusionnet_online"
    np.savez(tmp_path / "pred" / f"keyframe_hololens-dataset_{system}_predictions_000.npz", preds)

    def run(tag, flags, evaluate=("--evaluate_3d", "--threshold_3d", "0.1")):
        out = tmp_path / tag
        main(["--reconstruction_folder", str(out), "--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"),
              "--voxel_size", "0.05"] + list(evaluate) + flags)
        return {w: open(out / w, "rb").read() for w in sorted(os.listdir(out))}

    plain, again = run("plain", []), run("again", [])
    assert plain == again and len(plain) == 2
    mesh_file, = [w for w in plain if w.endswith("_complete.ply")]
    errors_file, = [w for w in plain if w.endswith("_errors3d.npz")]
    assert f"_{system}_hololens" in mesh_file and "+clean" not in mesh_file
    saved = np.load(tmp_path / "plain" / errors_file)
    assert sorted(saved.files) == ["arr_0", "counts", "names", "threshold"]
    # the threshold: as many faces as the largest component has, so that every smaller one goes (connectivity alone decides: the
    # vertices of a .ply are rounded to six decimals, its faces are exact)
    verts, faces = TSDFFusion.meshread(str(tmp_path / "plain" / mesh_file))
    parts = mesh_components(faces, len(verts))
    most = int(parts["face_count"].max())
    print(f"the system's mesh: {len(faces)} faces in {parts['n_components']} components, the largest of {most}")
    rule = ComponentFilter(min_faces=most)
    cleaned = run("cleaned", ["--clean_mesh_faces", str(most)])
    assert sorted(cleaned) == sorted(w.replace(system, system + "+clean") for w in plain)
    want = filter_components(verts, faces, rule)
    got_verts, got_faces = TSDFFusion.meshread(str(tmp_path / "cleaned" / mesh_file.replace(system, system + "+clean")))
    assert bits(got_verts) == bits(want[0]) and bits(got_faces) == bits(want[1])
    on_device = filter_components_device(torch.from_numpy(verts).to(hip_device), torch.from_numpy(faces).to(hip_device), rule)
    assert bits(on_device[0].cpu().numpy()) == bits(got_verts) and bits(on_device[1].cpu().numpy()) == bits(got_faces)
    scored = np.load(tmp_path / "cleaned" / errors_file.replace(system, system + "+clean"))
    assert sorted(scored.files) == sorted(saved.files + ["clean_min_area", "clean_min_faces", "clean_largest", "clean_faces"])
    assert scored["clean_faces"].dtype == np.int64 and scored["clean_faces"].tolist() == [len(got_faces), len(faces)]
    assert scored["clean_min_area"] == 0.0 and scored["clean_min_faces"] == most and not scored["clean_largest"]
    assert scored["counts"][0] == len(got_verts) and scored["counts"][1] == saved["counts"][1]          # the ground truth is not cleaned
    assert scored["arr_0"].dtype == np.float32 and scored["arr_0"].shape == (6,)
    # with the consistency filter as well: "+clean" comes after "+consistent"
    both = run("both", ["--clean_mesh_faces", "2", "--clean_mesh_largest", "--filter_consistency"], evaluate=())
    assert list(both) == [mesh_file.replace(system, system + "+consistent+clean")]
