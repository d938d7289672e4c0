"""CPU: the marching-cubes case tables (csrc/marching_cubes_tables.h), the numpy restatement of the kernel's contract
(tests/marching_cubes_cpu.py) on closed surfaces, and the mesh / point-cloud post-processing and .ply writers against the
reference script's own output (tests/golden/tsdf_mesh.npz, from tests/golden/make_mesh_goldens.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import marching_cubes_cpu as mc
import synthetic as syn

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]


def edge_corners(e):
    return [int(c) for c in mc.tables()["edge_corners"][e]]


def on_common_face(e1, e2):
    pts = np.array([CORNERS[c] for c in edge_corners(e1) + edge_corners(e2)])
    return bool(((pts == 0).all(axis=0) | (pts == 1).all(axis=0)).any())


def case_triangles(case):
    tab = mc.tables()
    row = tab["tri_table"][case]
    n = int(tab["tri_count"][case])
    assert (row[3 * n:] == -1).all() and (row[:3 * n] >= 0).all()
    return row[:3 * n].reshape(n, 3)


def test_tables_self_consistent_for_all_256_cases():
    tab = mc.tables()
    for e in range(12):      # edge = corner pair differing in one axis; its owner is the low corner
        a, b = edge_corners(e)
        d = np.array(CORNERS[b]) - np.array(CORNERS[a])
        assert sorted(d.tolist()) == [0, 0, 1]
        assert list(tab["edge_owner"][e]) == list(CORNERS[a]) + [int(np.argmax(d))]
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        crossing = {e for e in range(12) if inside[edge_corners(e)[0]] != inside[edge_corners(e)[1]]}
        assert tab["edge_table"][case] == sum(1 << e for e in crossing)
        tris = case_triangles(case)
        assert set(tris.reshape(-1).tolist()) == crossing, case
        count = {}
        for t in tris:
            assert len(set(t.tolist())) == 3
            for i in range(3):
                key = tuple(sorted((int(t[i]), int(t[(i + 1) % 3]))))
                count[key] = count.get(key, 0) + 1
        for (e1, e2), n in count.items():
            if on_common_face(e1, e2):
                assert n == 1, (case, e1, e2)        # a boundary edge: on a cube face, one triangle inside this cube
            else:
                assert n == 2, (case, e1, e2)        # an interior edge: between two triangles of this cube


def test_generated_header_is_current():
    gen = os.path.join(os.path.dirname(mc.TABLES_H), "..", "..", "tools", "gen_marching_cubes_tables.py")
    assert subprocess.run([sys.executable, gen, "--check"]).returncode == 0


def noise_volume(shape, seed, border=True):
    v = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    if border:
        v[0] = v[-1] = 1.0
        v[:, 0] = v[:, -1] = 1.0
        v[:, :, 0] = v[:, :, -1] = 1.0
    return v


def sphere(n, r):
    g = np.indices((n, n, n)).astype(np.float32) - np.float32((n - 1) / 2)
    return (np.sqrt((g * g).sum(0)) - np.float32(r)).astype(np.float32)


def torus(n, big, small):
    x, y, z = np.indices((n, n, n)).astype(np.float32) - np.float32((n - 1) / 2)
    return (np.sqrt((np.sqrt(x * x + y * y) - big) ** 2 + z * z) - small).astype(np.float32)


def mesh_edges(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    return e, np.unique(np.sort(e, axis=1), axis=0, return_counts=True)


def check_closed(verts, faces):
    """Every edge between exactly two faces, traversed once in each direction; returns the Euler characteristic."""
    directed, (undirected, counts) = mesh_edges(faces)
    assert (counts == 2).all(), f"{int((counts != 2).sum())} edges not shared by exactly two faces"
    assert len(np.unique(directed, axis=0)) == len(directed), "two faces traverse an edge the same way (inconsistent orientation)"
    return len(verts) - len(undirected) + len(faces)


def enclosed_volume(verts, faces):
    p = verts.astype(np.float64)
    return float(np.einsum("ij,ij->i", p[faces[:, 0]], np.cross(p[faces[:, 1]], p[faces[:, 2]])).sum() / 6.0)


def test_vertex_set_is_the_sign_change_edges_in_order():
    vol = noise_volume((7, 9, 11), 3, border=False)
    verts, faces, normals, _ = mc.marching_cubes(vol, 0.25)
    X, Y, Z = vol.shape
    expect = []
    for lin in range(X * Y * Z):
        i, j, k = np.unravel_index(lin, vol.shape)
        for axis, (di, dj, dk) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            if i + di < X and j + dj < Y and k + dk < Z and (vol[i, j, k] < 0.25) != (vol[i + di, j + dj, k + dk] < 0.25):
                va, vb = vol[i, j, k], vol[i + di, j + dj, k + dk]
                p = [np.float32(i), np.float32(j), np.float32(k)]
                p[axis] = np.float32(p[axis] + (np.float32(0.25) - va) / (vb - va))
                expect.append(p)
    assert np.array_equal(verts, np.array(expect, dtype=np.float32))
    assert faces.min() >= 0 and faces.max() < len(verts)
    np.testing.assert_allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_noise_volumes_are_closed(seed):
    verts, faces, _, _ = mc.marching_cubes(noise_volume((18, 21, 23), seed))
    assert len(faces) > 1000
    check_closed(verts, faces)
    assert enclosed_volume(verts, faces) > 0


def test_sphere_is_a_closed_oriented_sphere():
    r = 20.0
    verts, faces, normals, _ = mc.marching_cubes(sphere(64, r))
    assert check_closed(verts, faces) == 2
    dist = np.linalg.norm(verts.astype(np.float64) - 31.5, axis=1)
    assert np.abs(dist - r).max() < 0.02
    vol = enclosed_volume(verts, faces)
    assert vol > 0 and abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1) < 0.01
    p = verts.astype(np.float64)
    face_n = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    vert_n = normals[faces].mean(axis=1)
    assert (np.einsum("ij,ij->i", face_n, vert_n) > 0).all()
    np.testing.assert_allclose(np.einsum("ij,ij->i", normals, (p - 31.5) / dist[:, None]), 1.0, atol=2e-3)   # outward


def test_torus_is_a_closed_torus():
    verts, faces, normals, _ = mc.marching_cubes(torus(64, 16.0, 6.0))
    assert check_closed(verts, faces) == 0
    assert enclosed_volume(verts, faces) > 0
    p = verts.astype(np.float64)
    face_n = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    assert (np.einsum("ij,ij->i", face_n, normals[faces].mean(axis=1)) > 0).all()


def test_empty_and_thin_volumes():
    for vol in (np.ones((4, 5, 6), np.float32), noise_volume((1, 8, 8), 0, border=False), noise_volume((8, 1, 8), 1, border=False)):
        verts, faces, normals, colors = mc.marching_cubes(vol, color=np.zeros_like(vol))
        assert verts.shape == (0, 3) and faces.shape == (0, 3) and normals.shape == (0, 3) and colors.shape == (0, 3)


# ---- the reference's post-processing: tests/golden/tsdf_mesh.npz -------------------------------------------------------------

@pytest.fixture(scope="module")
def pin(golden_dir):
    return np.load(os.path.join(golden_dir, "tsdf_mesh.npz"))


def test_world_vertices_colours_and_point_cloud_match_the_reference(pin):
    verts, faces, normals, colors = mc.marching_cubes(pin["tsdf"], 0.0, pin["color"], pin["vol_origin"], float(pin["voxel_size"]))
    assert len(verts) > 300
    assert np.array_equal(verts, pin["verts"]) and verts.dtype == pin["verts"].dtype
    assert np.array_equal(colors, pin["colors"]) and colors.dtype == np.uint8
    assert np.array_equal(faces, pin["faces"]) and np.array_equal(normals, pin["norms"])
    pc = np.hstack([verts, colors])
    assert pc.dtype == np.float32 and np.array_equal(pc, pin["point_cloud"])


def test_ply_writers_match_the_reference_bytes(pin, tmp_path):
    from dvmvs.tsdf import TSDFFusion
    TSDFFusion.meshwrite(str(tmp_path / "mesh.ply"), pin["verts"], pin["faces"], pin["norms"], pin["colors"])
    TSDFFusion.pcwrite(str(tmp_path / "pc.ply"), pin["point_cloud"])
    assert (tmp_path / "mesh.ply").read_bytes() == pin["mesh_ply"].tobytes()
    assert (tmp_path / "pc.ply").read_bytes() == pin["pc_ply"].tobytes()
    # an empty mesh still writes a valid header
    TSDFFusion.meshwrite(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32),
                         np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    text = (tmp_path / "empty.ply").read_text()
    assert "element vertex 0\n" in text and "element face 0\n" in text and text.endswith("end_header\n")


def test_calculate_volume_bounds_matches_the_reference(pin):
    from dvmvs.tsdf import TSDFFusion
    frames, _, _ = syn.tsdf_inputs()
    bounds = TSDFFusion.calculate_volume_bounds([f[1] for f in frames], [f[3] for f in frames], frames[0][2])
    assert np.array_equal(bounds, pin["bounds"])
    # it starts from zero, unlike volume_bounds (which starts from +-inf)
    shifted = [f[3] + np.diag([0.0, 0.0, 0.0, 0.0]) for f in frames]
    for pose in shifted:
        pose[:3, 3] += 5.0
    assert (TSDFFusion.calculate_volume_bounds([f[1] for f in frames], shifted, frames[0][2])[:, 0] == 0.0).all()
    assert (TSDFFusion.volume_bounds([(f[1], f[2], pose) for f, pose in zip(frames, shifted)])[:, 0] > 4.0).all()


def test_c_abi_argument_validation_without_gpu():
    """Negative codes come before anything is enqueued: safe without a device."""
    from dvmvs.hip import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _capi.lib()
    n = lib.dvmvs_marching_cubes_workspace_bytes(256, 256, 256)
    assert 4 * 256 ** 3 <= n <= 4 * 256 ** 3 + 32 * 256 ** 2
    assert lib.dvmvs_marching_cubes_workspace_bytes(0, 4, 4) == 0
    assert lib.dvmvs_marching_cubes_workspace_bytes(2048, 2048, 1024) == 0          # 2^32 voxels: unsupported
    assert lib.dvmvs_marching_cubes_count(None, 4, 4, 4, 0.0, None, 0, None, None) == -1
    assert lib.dvmvs_marching_cubes_count(1, 4, 4, 4, 0.0, 1, 8, 1, None) == -1        # workspace too small
    assert lib.dvmvs_marching_cubes_count(1, 2048, 2048, 1024, 0.0, 1, 1 << 40, 1, None) == -2
    assert lib.dvmvs_marching_cubes_emit(1, None, 4, 4, 4, 0.0, 0, 0, 0, 1.0, 1, None, None, None, None, 5, 0, None) == -1
    assert lib.dvmvs_marching_cubes_emit(1, None, 4, 4, 4, 0.0, 0, 0, 0, 1.0, 1, 1, 1, None, 1, 1 << 31, 1, None) == -2
    assert lib.dvmvs_marching_cubes_emit(1, None, 4, 4, 4, 0.0, 0, 0, 0, 1.0, 1, 1, 1, None, 1, -1, 1, None) == -1
