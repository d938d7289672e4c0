"""GPU: mesh simplification (csrc/mesh_simplify.hip, dvmvs.hip.simplify) against the host definition (dvmvs/simplify.py) bit for bit, on the
meshes of tests/simplify_reference.py, and the surface built on it: ``TSDFVolume``'s ``simplify`` keywords and the program's
``--simplify_mesh_voxel`` flag.  The host definition of a case is computed once and never modified."""
import os

import numpy as np
import pytest
import torch

import simplify_reference as sr
from dvmvs.simplify import CONTRACTIONS, SimplifySettings, simplify_mesh

pytestmark = pytest.mark.gpu

NAMES = ("verts", "faces", "normals", "colors", "vertex_cluster", "face_index")


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def upload(dev, case):
    return {k: torch.from_numpy(np.array(v)).to(dev) for k, v in case.items() if isinstance(v, np.ndarray)}      # (a copy: the cases are read-only)


def assert_simplified(got, want, label):
    """``simplify_mesh(..., return_index=True)`` of the device against ``simplify_reference.host``."""
    flat = list(got[:4]) + list(got[4])
    for name, g, w in zip(NAMES, flat, want):
        assert (g is None) == (w is None), (label, name)
        if g is None:
            continue
        assert g.is_cuda, (label, name)
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and bits(g) == bits(w), (label, name, g.shape, w.shape)


@pytest.mark.parametrize("contraction", CONTRACTIONS)
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_simplify_equals_the_host_definition(hip_device, name, contraction):
    from dvmvs.hip import simplify
    case = sr.case(name)
    dev = upload(hip_device, case)
    got = simplify.simplify_mesh(dev["verts"], dev["faces"], case["voxel"], dev["normals"], dev["colors"], contraction, return_index=True)
    assert_simplified(got, sr.host(name, contraction), (name, contraction))
    # without the optional arrays, and without the indices
    bare = simplify.simplify_mesh(dev["verts"], dev["faces"], case["voxel"], contraction=contraction, return_index=True)
    assert_simplified(bare, sr.host(name, contraction, attributes=False), (name, contraction, "bare"))
    plain = simplify.simplify_mesh(dev["verts"], dev["faces"], SimplifySettings(case["voxel"], contraction), dev["normals"], dev["colors"])
    assert len(plain) == 4
    for g, w in zip(plain, sr.host(name, contraction)):
        assert bits(g.cpu().numpy()) == bits(w), (name, contraction, "settings")


def test_empty_results_and_the_module_level_twin(hip_device):
    from dvmvs import simplify
    for name in ("empty_both", "empty_faces", "single_cell"):
        case = sr.case(name)
        dev = upload(hip_device, case)
        verts, faces, normals, colors, (vertex_cluster, face_index) = simplify.simplify_mesh_device(
            dev["verts"], dev["faces"], case["voxel"], dev["normals"], dev["colors"], return_index=True)
        assert tuple(verts.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and tuple(normals.shape) == (0, 3) and tuple(colors.shape) == (0, 3)
        assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and normals.dtype == torch.float32 and colors.dtype == torch.uint8
        assert vertex_cluster.dtype == torch.int32 and face_index.dtype == torch.int32 and face_index.numel() == 0
        assert tuple(vertex_cluster.shape) == (len(case["verts"]),) and bool((vertex_cluster == -1).all())
        assert all(t.device == hip_device for t in (verts, faces, normals, colors, vertex_cluster, face_index))
        verts, faces, normals, colors = simplify.simplify_mesh_device(dev["verts"], dev["faces"], case["voxel"])
        assert normals is None and colors is None and tuple(verts.shape) == (0, 3) and tuple(faces.shape) == (0, 3)


@pytest.mark.parametrize("name", ["cube", "duplicates", "sized_1025"])
def test_views_and_odd_offsets(hip_device, name):
    """Inputs that are non-contiguous views (every second row of a larger tensor, three of six columns) and views that begin one element
    past an aligned address."""
    from dvmvs.hip import simplify
    case = sr.case(name)

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
        for contraction in CONTRACTIONS:
            got = simplify.simplify_mesh(verts, faces, case["voxel"], normals, colors, contraction, return_index=True)
            assert_simplified(got, sr.host(name, contraction), (name, make.__name__, contraction))


def test_two_calls_give_identical_bytes(hip_device):
    from dvmvs.hip import simplify
    for name in ("long_run", "far"):
        case = sr.case(name)
        dev = upload(hip_device, case)
        runs = []
        for _ in range(2):
            out = simplify.simplify_mesh(dev["verts"], dev["faces"], case["voxel"], dev["normals"], dev["colors"], return_index=True)
            runs.append([bits(t.cpu().numpy()) for t in list(out[:4]) + list(out[4])])
        assert runs[0] == runs[1], name


def test_status_and_settings_raise_the_hosts_exceptions(hip_device):
    from dvmvs.hip import simplify
    for name in sorted(sr.ERROR_CASES):
        case = sr.case(name)
        dev = upload(hip_device, case)
        with pytest.raises(ValueError, match="2\\^21 voxels"):
            simplify_mesh(case["verts"], case["faces"], case["voxel"])
        for contraction in CONTRACTIONS:
            with pytest.raises(ValueError, match="2\\^21 voxels"):
                simplify.simplify_mesh(dev["verts"], dev["faces"], case["voxel"], contraction=contraction)
    case = sr.case("duplicates")
    dev = upload(hip_device, case)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel"):
            simplify.simplify_mesh(dev["verts"], dev["faces"], bad)
    with pytest.raises(ValueError, match="contraction"):
        simplify.simplify_mesh(dev["verts"], dev["faces"], 0.5, contraction="median")
    with pytest.raises(ValueError, match="normals"):
        simplify.simplify_mesh(dev["verts"], dev["faces"], 0.5, normals=dev["normals"][:-1])
    with pytest.raises(ValueError, match="faces"):
        simplify.simplify_mesh(dev["verts"], dev["faces"].long(), 0.5)
    # the call after a refused one is what it always was
    got = simplify.simplify_mesh(dev["verts"], dev["faces"], case["voxel"], dev["normals"], dev["colors"], return_index=True)
    assert_simplified(got, sr.host("duplicates"), "after the refusals")


# ---- the volume ---------------------------------------------------------------------------------------------------------------------------
VOXEL = 0.05
CELL = 0.15


def box_volume(dev):
    """A 32^3 volume of 5 cm voxels whose zero iso-surface is a box of 0.8 x 0.7 x 0.6 m with faces, edges and corners, and a small shell
    around two grid corners next to it."""
    from dvmvs.tsdf import TSDFVolume
    vol = TSDFVolume(np.array([[0.0, 1.6]] * 3), VOXEL, device=dev)
    assert tuple(vol.vol_dim) == (32, 32, 32)
    grid = np.stack(np.meshgrid(*[np.arange(32) * VOXEL] * 3, indexing="ij"), axis=-1)
    q = np.abs(grid - np.array([0.8, 0.8, 0.8])) - np.array([0.4, 0.35, 0.3]) + 0.012
    sdf = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
    a, b = np.array([0.2, 0.2, 0.2]), np.array([0.25, 0.2, 0.2])
    along = np.clip((grid - a) @ (b - a) / ((b - a) @ (b - a)), 0.0, 1.0)
    sdf = np.minimum(sdf, np.linalg.norm(grid - (a + along[..., None] * (b - a)), axis=-1) - 0.03)
    vol._tsdf.copy_(torch.from_numpy(np.clip(sdf / (5 * VOXEL), -1.0, 1.0).astype(np.float32)))
    vol._color.copy_(torch.from_numpy(np.random.default_rng(5).integers(0, 2 ** 24, (32, 32, 32)).astype(np.float32)))
    return vol


def test_volume_simplifies_end_to_end(hip_device):
    from dvmvs import errors
    from dvmvs.components import ComponentFilter, filter_components
    vol = box_volume(hip_device)
    raw = vol.get_mesh()
    rule, settings = ComponentFilter(min_faces=100), SimplifySettings(CELL)
    for simplify in (settings, SimplifySettings(CELL, "average")):
        want = simplify_mesh(raw[0], raw[1], simplify, raw[2], raw[3])
        got = vol.get_mesh(simplify=simplify)
        print(f"{simplify.contraction}: {len(raw[0])} vertices and {len(raw[1])} faces -> {len(got[0])} and {len(got[1])}")
        assert 0 < len(got[1]) < len(raw[1]) // 4
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and bits(g) == bits(w)
        verts, faces = vol.mesh_tensors(simplify=simplify)
        assert verts.is_cuda and bits(verts.cpu().numpy()) == bits(want[0]) and bits(faces.cpu().numpy()) == bits(want[1])
        assert bits(vol.vertices(simplify=simplify).cpu().numpy()) == bits(want[0])
    # after cleaning, and the same as the two stages on the host
    cleaned = filter_components(raw[0], raw[1], rule, raw[2], raw[3])
    assert len(cleaned[1]) < len(raw[1])
    want = simplify_mesh(cleaned[0], cleaned[1], settings, cleaned[2], cleaned[3])
    got = vol.get_mesh(simplify=settings, clean=rule)
    assert all(bits(g) == bits(w) for g, w in zip(got, want))
    assert all(bits(g) == bits(w) for g, w in zip(vol.get_mesh(rule), cleaned))                # a filter by position is still the filter
    # simplify=None: the bytes of the path without the keyword
    assert all(bits(g) == bits(w) for g, w in zip(vol.get_mesh(simplify=None), raw))
    assert all(bits(g) == bits(w) for g, w in zip(vol.get_mesh(simplify=None, clean=rule), cleaned))
    plain_verts, plain_faces = vol.mesh_tensors()
    assert bits(plain_verts.cpu().numpy()) == bits(raw[0]) and bits(plain_faces.cpu().numpy()) == bits(raw[1])
    # scores: the prediction alone is simplified
    cloud = vol.vertices()
    threshold = 0.02
    plain = vol.score_against(cloud, threshold=threshold)
    assert bits(vol.score_against(cloud, threshold=threshold, simplify=None).cpu().numpy()) == bits(plain.cpu().numpy())
    scored = vol.score_against(cloud, threshold=threshold, simplify=settings, clean=rule)
    on_host = errors.compute_reconstruction_errors_device(torch.from_numpy(want[0]).to(hip_device), cloud, threshold)
    assert bits(scored.cpu().numpy()) == bits(on_host.cpu().numpy())
    density, voxel = 2000.0, 0.04
    points = vol.surface_points(density, voxel, simplify=settings, clean=rule)
    want_points = errors.prepare_points_device(torch.from_numpy(want[0]).to(hip_device), torch.from_numpy(want[1]).to(hip_device), density, voxel)
    assert bits(points.cpu().numpy()) == bits(want_points.cpu().numpy())
    sampled, sizes = vol.score_against(vol, threshold=threshold, return_sizes=True, sample_density=density, voxel=voxel, simplify=settings)
    assert sizes[0] != sizes[1] and float(sampled[2]) > 0.0                                     # the reference keeps its density


# ---- the program -------------------------------------------------------------------------------------------------------------------------
def test_program_simplifies(hip_device, golden_dir, tmp_path, monkeypatch):
    """``python -m dvmvs.tsdf --evaluate_3d`` on the two keyframes of the sample scene: with ``--simplify_mesh_voxel`` the ``+simple`` files hold
    the simplified mesh and the new keys; it composes with ``--clean_mesh_faces``."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.tsdf import TSDFFusion, main, program
    volumes = []                                       # the system's volume of every run, to take its mesh at full precision
    fuse_system = program._fuse_system

    def recording(*args):
        volumes.append(fuse_system(*args))
        return volumes[-1]

    monkeypatch.setattr(program, "_fuse_system", recording)
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

    plain = run("plain", [])
    mesh_file, = [w for w in plain if w.endswith("_complete.ply")]
    errors_file, = [w for w in plain if w.endswith("_errors3d.npz")]
    assert "+simple" not in mesh_file
    saved = np.load(tmp_path / "plain" / errors_file)
    assert sorted(saved.files) == ["arr_0", "counts", "names", "threshold"]
    simple = run("simple", ["--simplify_mesh_voxel", "0.15"])
    assert sorted(simple) == sorted(w.replace(system, system + "+simple") for w in plain)
    # the file is the host definition of the volume's own mesh through the same writer (a .ply rounds vertices to six decimals, so the
    # mesh that the plain run wrote is not what was simplified: its vertices on cell borders would change cells)
    full = volumes[-1][0].get_mesh()
    want = simplify_mesh(full[0], full[1], 0.15, full[2], full[3])
    TSDFFusion.meshwrite(str(tmp_path / "want.ply"), *want)
    simple_file = mesh_file.replace(system, system + "+simple")
    assert simple[simple_file] == open(tmp_path / "want.ply", "rb").read()
    want_verts, want_faces = TSDFFusion.meshread(str(tmp_path / "want.ply"))
    got_verts, got_faces = TSDFFusion.meshread(str(tmp_path / "simple" / mesh_file.replace(system, system + "+simple")))
    full_verts, full_faces = TSDFFusion.meshread(str(tmp_path / "plain" / mesh_file))
    print(f"the system's mesh: {len(full_faces)} faces, simplified {len(got_faces)}")
    assert bits(got_verts) == bits(want_verts) and bits(got_faces) == bits(want_faces) and bits(got_faces) == bits(want[1])
    assert 0 < len(got_faces) < len(full_faces) // 4 and len(got_verts) < len(full_verts) // 4
    scored = np.load(tmp_path / "simple" / errors_file.replace(system, system + "+simple"))
    assert sorted(scored.files) == sorted(saved.files + ["simplify_voxel", "simplify_average", "simplify_faces"])
    assert scored["simplify_faces"].dtype == np.int64 and scored["simplify_faces"].tolist() == [len(got_faces), len(full_faces)]
    assert scored["simplify_voxel"] == 0.15 and not scored["simplify_average"]
    assert scored["counts"][0] == len(got_verts) and scored["counts"][1] == saved["counts"][1]          # the ground truth is not simplified
    again = run("again", ["--simplify_mesh_voxel", "0.15"])
    assert list(again.values()) == list(simple.values())                                        # the same bytes twice
    average = run("average", ["--simplify_mesh_voxel", "0.15", "--simplify_mesh_average"], evaluate=())
    average_verts, average_faces = TSDFFusion.meshread(str(tmp_path / "average" / mesh_file.replace(system, system + "+simple")))
    assert bits(average_faces) == bits(got_faces) and average_verts.shape == got_verts.shape and bits(average_verts) != bits(got_verts)
    both = run("both", ["--clean_mesh_faces", "2", "--simplify_mesh_voxel", "0.15", "--filter_consistency"], evaluate=())
    assert list(both) == [mesh_file.replace(system, system + "+consistent+clean+simple")]
