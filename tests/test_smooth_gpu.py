"""GPU: mesh smoothing and vertex normals (csrc/mesh_smooth.hip, dvmvs.hip.smooth) against the host definition (dvmvs/smooth.py) bit for
bit, on the meshes and settings of tests/smooth_reference.py, and the surface built on it: ``TSDFVolume``'s ``smooth`` keywords and the
program's ``--smooth_mesh_iterations`` flag.  The host definition of a case is computed once and never modified."""
import os

import numpy as np
import pytest
import torch

import smooth_reference as sr
from dvmvs.smooth import SmoothSettings, smooth_mesh

pytestmark = pytest.mark.gpu

NAMES = ("verts", "faces", "normals", "colors")
INPUTS = ("verts", "faces", "normals", "colors")


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def upload(dev, case):
    return {k: torch.from_numpy(np.array(v)).to(dev) for k, v in case.items() if isinstance(v, np.ndarray)}      # (a copy: the cases are read-only)


def assert_smoothed(got, want, label):
    assert len(got) == 4, label
    for name, g, w in zip(NAMES, got, want):
        assert (g is None) == (w is None), (label, name)
        if g is None:
            continue
        assert g.is_cuda and g.is_contiguous(), (label, name)
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and bits(g) == bits(w), (label, name, g.shape, w.shape)


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_smooth_equals_the_host_definition(hip_device, name):
    from dvmvs.hip import smooth
    case = sr.case(name)
    dev = upload(hip_device, case)
    for setting, settings in sr.SETTINGS.items():
        got = smooth.smooth_mesh(dev["verts"], dev["faces"], settings, dev["normals"], dev["colors"])
        assert_smoothed(got, sr.host(name, setting), (name, setting))
        for g, key in zip(got, INPUTS):                                         # copies: no output is an input
            assert g.data_ptr() != dev[key].data_ptr() or g.numel() == 0, (name, setting, key)
        bare = smooth.smooth_mesh(dev["verts"], dev["faces"], settings.iterations, method=settings.method, lam=settings.lam, mu=settings.mu,
                                  boundary=settings.boundary, recompute_normals=settings.recompute_normals)
        assert_smoothed(bare, sr.host(name, setting, attributes=False), (name, setting, "bare"))
    for key in INPUTS:                                                          # the inputs are what they were
        assert bits(dev[key].cpu().numpy()) == bits(case[key]), (name, key)


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_rows_equal_the_host_definition(hip_device, name):
    from dvmvs.hip import smooth
    case = sr.case(name)
    faces = torch.from_numpy(np.array(case["faces"])).to(hip_device)
    got = smooth.vertex_rows(faces, len(case["verts"]))
    for label, g, w in zip(("offsets", "neighbours", "boundary"), got, sr.host_rows(name)):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and bits(g) == bits(w), (name, label)


@pytest.mark.parametrize("name", ["cube", "sphere_noisy", "junk", "strip_1025", "empty_faces", "empty_both"])
def test_vertex_normals_alone(hip_device, name):
    from dvmvs import smooth
    case = sr.case(name)
    dev = upload(hip_device, case)
    got = smooth.vertex_normals_device(dev["verts"], dev["faces"])
    assert got.is_cuda and got.dtype == torch.float32 and bits(got.cpu().numpy()) == bits(sr.host_normals(name))
    got = smooth.vertex_normals_device(dev["verts"], dev["faces"], dev["normals"])
    assert bits(got.cpu().numpy()) == bits(sr.host_normals(name, fallback=True))
    assert got.data_ptr() != dev["normals"].data_ptr() or got.numel() == 0
    for key in ("verts", "faces", "normals"):
        assert bits(dev[key].cpu().numpy()) == bits(case[key])


@pytest.mark.parametrize("name", ["cube", "junk", "strip_1025"])
def test_views_and_odd_offsets(hip_device, name):
    """Inputs that are non-contiguous views (every second row of a larger tensor, three of six columns) and views that begin one element
    past an aligned address."""
    from dvmvs.hip import smooth
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
        for setting in ("taubin_2_free", "laplacian_3_fixed", "none"):
            got = smooth.smooth_mesh(verts, faces, sr.SETTINGS[setting], normals, colors)
            assert_smoothed(got, sr.host(name, setting), (name, make.__name__, setting))
        assert bits(smooth.vertex_normals(verts, faces, normals).cpu().numpy()) == bits(sr.host_normals(name, fallback=True))
        for view, key in ((verts, "verts"), (faces, "faces"), (normals, "normals"), (colors, "colors")):
            assert bits(view.cpu().numpy()) == bits(case[key]), (name, make.__name__, key)


def test_two_calls_give_identical_bytes(hip_device):
    from dvmvs.hip import smooth
    for name in ("fan", "shuffled", "far"):
        case = sr.case(name)
        dev = upload(hip_device, case)
        runs = []
        for _ in range(2):
            out = smooth.smooth_mesh(dev["verts"], dev["faces"], 3, dev["normals"], dev["colors"])
            runs.append([bits(t.cpu().numpy()) for t in out])
        assert runs[0] == runs[1], name


def test_packed_positions_give_the_same_bits(hip_device):
    """The 12-byte iterate that tools/mesh_smooth_bench.py compares with the 16-byte one is the same arithmetic."""
    from dvmvs.hip import smooth
    for name in ("sphere_noisy", "strip_1025"):
        case = sr.case(name)
        verts, faces = (torch.from_numpy(np.array(case[k])).to(hip_device) for k in ("verts", "faces"))
        V, F = verts.shape[0], faces.shape[0]
        workspace, nbytes = smooth._workspace_of("smooth_mesh", hip_device, V, F)
        smooth.build_rows(faces, V, workspace, nbytes)
        for setting in ("taubin_2_free", "laplacian_1_fixed", "laplacian_3_free"):
            s = sr.SETTINGS[setting]
            got = smooth.run_steps(verts, F, workspace, nbytes, s.iterations, s.method, s.lam, s.mu, s.boundary, packed=True)
            assert bits(got.cpu().numpy()) == bits(sr.host(name, setting)[0]), (name, setting)


def test_settings_and_tensors_raise(hip_device):
    from dvmvs.hip import smooth
    case = sr.case("cube")
    dev = upload(hip_device, case)
    for bad in (SmoothSettings(-1), SmoothSettings(2, lam=0.0), SmoothSettings(2, mu=-0.2), SmoothSettings(2, "umbrella"),
                SmoothSettings(2, boundary="open")):
        with pytest.raises(ValueError):
            smooth.smooth_mesh(dev["verts"], dev["faces"], bad)
    with pytest.raises(ValueError, match="normals"):
        smooth.smooth_mesh(dev["verts"], dev["faces"], 2, normals=dev["normals"][:-1])
    with pytest.raises(ValueError, match="colors"):
        smooth.smooth_mesh(dev["verts"], dev["faces"], 2, colors=dev["colors"].float())
    with pytest.raises(ValueError, match="faces"):
        smooth.smooth_mesh(dev["verts"], dev["faces"].long(), 2)
    with pytest.raises(ValueError, match="fallback"):
        smooth.vertex_normals(dev["verts"], dev["faces"], dev["normals"][:-1])
    got = smooth.smooth_mesh(dev["verts"], dev["faces"], sr.SETTINGS["taubin_2_free"], dev["normals"], dev["colors"])
    assert_smoothed(got, sr.host("cube", "taubin_2_free"), "after the refusals")


# ---- the volume ---------------------------------------------------------------------------------------------------------------------------
def sphere_volume(dev, n=32, r=10.0):
    """A 32^3 volume of unit voxels whose zero iso-surface is a sphere of radius 10 about its centre (as tests/test_marching_cubes.py
    builds one), with a small second sphere next to it for ``clean`` to remove."""
    from dvmvs.tsdf import TSDFVolume
    vol = TSDFVolume(np.array([[0.0, float(n)]] * 3), 1.0, device=dev)
    assert tuple(vol.vol_dim) == (n, n, n)
    g = np.indices((n, n, n)).astype(np.float32)
    big = np.sqrt(((g - np.float32((n - 1) / 2)) ** 2).sum(0)) - np.float32(r)
    small = np.sqrt(((g - np.float32(2.6)) ** 2).sum(0)) - np.float32(1.7)
    vol._tsdf.copy_(torch.from_numpy(np.clip(np.minimum(big, small) / 5.0, -1.0, 1.0).astype(np.float32)))
    vol._color.copy_(torch.from_numpy(np.random.default_rng(5).integers(0, 2 ** 24, (n, n, n)).astype(np.float32)))
    return vol


def test_volume_smooths_end_to_end(hip_device):
    from dvmvs.components import ComponentFilter, filter_components
    from dvmvs.simplify import SimplifySettings, simplify_mesh
    vol = sphere_volume(hip_device)
    raw = vol.get_mesh()
    S, Q, C = SmoothSettings(3), SimplifySettings(4.0), ComponentFilter(min_faces=200)
    want = smooth_mesh(raw[0], raw[1], S, raw[2], raw[3])
    got = vol.get_mesh(smooth=S)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and bits(g) == bits(w)
    assert bits(got[0]) != bits(raw[0]) and bits(got[1]) == bits(raw[1]) and bits(got[3]) == bits(raw[3])
    verts, faces = vol.mesh_tensors(smooth=S)
    assert verts.is_cuda and bits(verts.cpu().numpy()) == bits(want[0]) and bits(faces.cpu().numpy()) == bits(want[1])
    assert bits(vol.vertices(smooth=S).cpu().numpy()) == bits(want[0])
    assert all(bits(g) == bits(w) for g, w in zip(vol.get_mesh(S), want))                       # settings by position, in another stage's slot
    # clean -> smooth -> simplify, as the three stages on the host
    cleaned = filter_components(raw[0], raw[1], C, raw[2], raw[3])
    assert 0 < len(cleaned[1]) < len(raw[1])
    smoothed = smooth_mesh(cleaned[0], cleaned[1], S, cleaned[2], cleaned[3])
    composed = simplify_mesh(smoothed[0], smoothed[1], Q, smoothed[2], smoothed[3])
    got = vol.get_mesh(simplify=Q, smooth=S, clean=C)
    assert all(g.shape == w.shape and bits(g) == bits(w) for g, w in zip(got, composed))
    assert all(bits(g) == bits(w) for g, w in zip(vol.get_mesh(Q, C, S), composed))             # by position, by type
    assert all(bits(g) == bits(w) for g, w in zip(vol.get_mesh(clean=C, smooth=S), smoothed))
    # smooth=None: the bytes of the path without the keyword
    assert all(bits(g) == bits(w) for g, w in zip(vol.get_mesh(smooth=None), raw))
    assert all(bits(g) == bits(w) for g, w in zip(vol.get_mesh(C), cleaned))
    # scores and points: the prediction alone is smoothed
    from dvmvs import errors
    cloud = vol.vertices()
    plain = vol.score_against(cloud, threshold=0.5)
    assert bits(vol.score_against(cloud, threshold=0.5, smooth=None).cpu().numpy()) == bits(plain.cpu().numpy())
    scored = vol.score_against(cloud, threshold=0.5, smooth=S, clean=C)
    on_host = errors.compute_reconstruction_errors_device(torch.from_numpy(smoothed[0]).to(hip_device), cloud, 0.5)
    assert bits(scored.cpu().numpy()) == bits(on_host.cpu().numpy())
    points = vol.surface_points(0.5, 2.0, smooth=S, clean=C)
    want_points = errors.prepare_points_device(torch.from_numpy(smoothed[0]).to(hip_device), torch.from_numpy(smoothed[1]).to(hip_device), 0.5, 2.0)
    assert bits(points.cpu().numpy()) == bits(want_points.cpu().numpy())


def radius_deviation(verts, n=32):
    return float(np.linalg.norm(verts.astype(np.float64) - np.float64((n - 1) / 2), axis=1).std())


def test_smoothed_sphere_has_less_radius_deviation(hip_device):
    """The radius deviation of the smoothed sphere is below the extracted one's, on the exact distance field of a sphere of radius 10
    voxels, as tests/test_marching_cubes.py builds it.

    The factor is chosen for what there is to smooth.  Marching cubes interpolates an exact distance field almost exactly: the extracted
    vertices have a radius deviation of 0.0034 voxels.  A step moves a vertex by lam times its umbrella vector u, so the variance of
    the radius becomes Var(r) + 2 lam Cov(r, u_n) + lam^2 Var(u_n).  The covariance is negative (a vertex that sticks out is pulled in: that
    is what makes the operator a smoother), so a small enough lam lowers the deviation; the last term is what the uniform weights cost
    on unevenly spaced neighbours: on a sphere of radius R the umbrella vector of a vertex with edges h has a normal part of about
    -mean(h^2) / (2 R), here -1.2 / 20 = -0.06 voxels for edges between 0 and 1.7 voxels, and it varies from row to row as the edges of a
    marching-cubes mesh do (on the extracted mesh: mean -0.052, deviation 0.013).  lam * 0.013 has to stay below the 0.0034 that is
    there: lam < 0.26.  The test takes one Laplacian step
    with lam = 0.125.  The default lam = 0.5 is meant for noise at the scale of a voxel and RAISES the deviation of this noise-free surface
    (measured with the host definition: 0.00486 after one Laplacian step, 0.00388 / 0.00675 / 0.00961 after 1 / 3 / 10 Taubin iterations);
    that figure is printed, and ``test_smoothed_noisy_sphere_has_less_radius_deviation`` is the case the defaults are for."""
    from dvmvs.tsdf import TSDFVolume
    n, r = 32, 10.0
    vol = TSDFVolume(np.array([[0.0, float(n)]] * 3), 1.0, device=hip_device)
    g = np.indices((n, n, n)).astype(np.float32) - np.float32((n - 1) / 2)
    vol._tsdf.copy_(torch.from_numpy(np.clip((np.sqrt((g * g).sum(0)) - np.float32(r)) / 5.0, -1.0, 1.0).astype(np.float32)))
    extracted = radius_deviation(vol.get_mesh()[0])
    smoothed = radius_deviation(vol.get_mesh(smooth=SmoothSettings(1, "laplacian", lam=0.125))[0])
    default = radius_deviation(vol.get_mesh(smooth=SmoothSettings(3))[0])
    print(f"radius deviation of the exact sphere: {extracted:.5f} voxels extracted, {smoothed:.5f} after one Laplacian step with lam 0.125, "
          f"{default:.5f} after 3 Taubin iterations with the default factors")
    assert smoothed < extracted


def test_smoothed_noisy_sphere_has_less_radius_deviation(hip_device):
    """The same sphere with noise of 0.1 voxels (standard deviation) on the distance values, as fused depth predictions carry it: thirty
    times the ripple that marching cubes leaves on the exact field.  Every filter setting of the defaults lowers the deviation."""
    from dvmvs.tsdf import TSDFVolume
    n, r = 32, 10.0
    vol = TSDFVolume(np.array([[0.0, float(n)]] * 3), 1.0, device=hip_device)
    g = np.indices((n, n, n)).astype(np.float32) - np.float32((n - 1) / 2)
    noise = np.float32(0.1) * np.random.default_rng(3).standard_normal((n, n, n)).astype(np.float32)
    vol._tsdf.copy_(torch.from_numpy(np.clip((np.sqrt((g * g).sum(0)) - np.float32(r) + noise) / 5.0, -1.0, 1.0).astype(np.float32)))
    extracted = radius_deviation(vol.get_mesh()[0])
    for settings in (SmoothSettings(1), SmoothSettings(3), SmoothSettings(1, "laplacian")):
        smoothed = radius_deviation(vol.get_mesh(smooth=settings)[0])
        print(f"radius deviation of the noisy sphere: {extracted:.5f} voxels extracted, {smoothed:.5f} after {settings}")
        assert smoothed < extracted, settings


# ---- the program -------------------------------------------------------------------------------------------------------------------------
def test_program_smooths(hip_device, golden_dir, tmp_path, monkeypatch):
    """``python -m dvmvs.tsdf --evaluate_3d`` on the two keyframes of the sample scene: with ``--smooth_mesh_iterations 2`` the ``+smooth``
    files hold the smoothed mesh and the new keys."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.tsdf import TSDFFusion, main, program
    volumes = []                                       # the system's volume of the run, to take its mesh at full precision
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

    out = tmp_path / "smooth"
    main(["--reconstruction_folder", str(out), "--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"),
          "--voxel_size", "0.05", "--evaluate_3d", "--threshold_3d", "0.1", "--smooth_mesh_iterations", "2"])
    written = sorted(os.listdir(out))
    mesh_file, = [w for w in written if w.endswith("_complete.ply")]
    errors_file, = [w for w in written if w.endswith("_errors3d.npz")]
    assert len(written) == 2 and system + "+smooth_" in mesh_file and system + "+smooth_" in errors_file
    # the file is the host definition of the volume's own mesh through the same writer
    full = volumes[-1][0].get_mesh()
    want = smooth_mesh(full[0], full[1], 2, full[2], full[3])
    TSDFFusion.meshwrite(str(tmp_path / "want.ply"), *want)
    assert open(out / mesh_file, "rb").read() == open(tmp_path / "want.ply", "rb").read()
    TSDFFusion.meshwrite(str(tmp_path / "plain.ply"), *full)
    assert open(out / mesh_file, "rb").read() != open(tmp_path / "plain.ply", "rb").read()
    direct = volumes[-1][0].get_mesh(smooth=SmoothSettings(2))
    assert all(bits(g) == bits(w) for g, w in zip(direct, want))
    scored = np.load(out / errors_file)
    assert sorted(scored.files) == sorted(["arr_0", "counts", "names", "threshold", "smooth_iterations", "smooth_method", "smooth_lambda",
                                           "smooth_mu", "smooth_fixed_boundary"])
    assert scored["smooth_iterations"] == 2 and str(scored["smooth_method"]) == "taubin" and scored["smooth_lambda"] == 0.5
    assert scored["smooth_mu"] == -0.53 and not scored["smooth_fixed_boundary"] and scored["counts"][0] == len(full[0])
