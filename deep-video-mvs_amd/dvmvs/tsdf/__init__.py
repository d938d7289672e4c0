"""Volumetric TSDF fusion of posed RGB-D frames on an MI355X (surface of the ``TSDFVolume`` / ``TSDFFusion`` classes of the
reference's reconstruction script, sample-data/run-tsdf-reconstruction.py, lines 30-330 there; the line numbers that the docstrings of
this package give are that file's).

``TSDFVolume.integrate`` is the hot function: one HIP launch (``dvmvs_tsdf_integrate``) updates the whole voxel volume in
place in HBM; the volumes never leave the device until ``get_volume()``.  The reference compiles an equivalent CUDA kernel
with pycuda and launches it once per "gpu loop"; its numba CPU fall-back has no counterpart here (GPU only, like the rest of
the package).

``get_mesh`` / ``get_point_cloud`` extract the zero iso-surface on the device with ``marching_cubes`` (csrc/marching_cubes.hip,
four launches), where the reference calls scikit-image's ``marching_cubes_lewiner`` on the host.  Vertices are the same (one on
every grid edge whose sign changes, linearly interpolated); in cubes with an ambiguous face or interior the Lewiner (MC33) cases
of scikit-image may triangulate differently, so face counts can differ slightly from the reference's; normals are the
interpolated ``np.gradient`` of the volume.  ``TSDFFusion`` carries the script's helpers (``meshwrite`` / ``pcwrite`` write the
same bytes, ``integrate``, ``calculate_volume_bounds``) and ``run`` is its main program: ``python -m dvmvs.tsdf --help``.

The modules, each importing only those before it: ``dvmvs.hip.volume`` (the two bindings: ``marching_cubes`` and the per-frame
integration), ``mesh_views`` (``render_mesh``, ``visible_mesh``, the camera tensors), ``volume`` (``TSDFVolume``, ``fold_color``), ``ply``
(the PLY reader and writers), ``scoring`` (the work of ``TSDFVolume.score_against``, which that method imports when it is called),
``sparse_volume`` (``SparseTSDFVolume``, the volume that needs no bounds: a hash table of bricks over a pool; ``dense()`` gives a
``TSDFVolume``, ``mesh_tensors`` / ``get_mesh`` extract the surface straight from the pool; ``dvmvs.tsdf.SparseTSDFVolume`` resolves to it on first use, so importing the package loads what it always loaded),
``fusion`` (``TSDFFusion``, ``LiveFusion``) and ``program`` (``run``, its stages and the parser).
"""
from dvmvs.hip.volume import marching_cubes
from dvmvs.tsdf.fusion import LiveFusion, TSDFFusion
from dvmvs.tsdf.mesh_views import VISIBLE_MESH_CHUNK, render_mesh, visible_mesh
from dvmvs.tsdf.program import apply_transform, build_parser, load_transform, main, run
from dvmvs.tsdf.volume import TSDFVolume, fold_color

__all__ = ["fold_color", "marching_cubes", "render_mesh", "visible_mesh", "VISIBLE_MESH_CHUNK", "TSDFVolume", "TSDFFusion", "LiveFusion", "run",
           "build_parser", "main", "load_transform", "apply_transform"]


def __getattr__(name):
    """``dvmvs.tsdf.SparseTSDFVolume``: imported when it is first asked for (PEP 562)."""
    if name == "SparseTSDFVolume":
        from dvmvs.tsdf.sparse_volume import SparseTSDFVolume
        return SparseTSDFVolume
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
