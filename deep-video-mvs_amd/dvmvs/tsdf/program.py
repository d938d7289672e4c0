"""The command-line program ``python -m dvmvs.tsdf``: ``run`` and the stages it is made of, its settings and its parser."""
import glob
import os
from argparse import ArgumentParser
from dataclasses import dataclass
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import torch

from dvmvs.tsdf.fusion import TSDFFusion
from dvmvs.tsdf.scoring import _aligned_score
from dvmvs.tsdf.volume import TSDFVolume


def run(reconstruction_folder, prediction_folder, data_folder, dataset_name, scene_name, system_name, voxel_size, max_depth,
        use_groundtruth_to_anchor, save_progressive, save_groundtruth, device="cuda", device_preprocess=False, render_keyframes=False,
        evaluate_3d=False, threshold_3d=0.05, filter_consistency=False, consistency_views=2, consistency_sources=4, consistency_pixel=1.0,
        consistency_relative=0.01, save_point_cloud=False, evaluate_3d_density=None, evaluate_3d_voxel=None, groundtruth_mesh=None,
        evaluate_3d_visible=False, evaluate_3d_min_views=1, evaluate_3d_align=None, evaluate_3d_align_scale=False, evaluate_3d_align_plane=False,
        evaluate_3d_align_neighbours=20, evaluate_3d_align_normal_distance=None, point_mesh_voxel=None, point_mesh_radius=None,
        point_mesh_neighbours=32, point_mesh_min_neighbours=3,
        sparse_volume=False, sparse_volume_bricks=65536, sparse_volume_extract=False, sparse_volume_render=False,      # (here, not last: the places of the parameters behind them are pinned by tests)
        simplify_mesh_voxel=None, simplify_mesh_average=False,
        smooth_mesh_iterations=None, smooth_mesh_laplacian=False, smooth_mesh_lambda=None, smooth_mesh_mu=None, smooth_mesh_fixed_boundary=False,
        groundtruth_transform=None, point_normals_neighbours=None,
        point_normals_max_distance=None, clean_points_neighbours=None, clean_points_ratio=2.0, clean_points_max_distance=None,
        clean_points_radius=None, clean_points_min_neighbours=None, clean_mesh_area=None, clean_mesh_faces=None, clean_mesh_largest=False):
    """The reconstruction script's main program (run-tsdf-reconstruction.py:477-636): fuses a scene's saved keyframe depth
    predictions (``keyframe_<dataset>_<system>_predictions_<scene>*.npz`` in ``prediction_folder``) into a TSDF volume and writes
    the mesh; optionally the same from the ground-truth depth maps.  Images and depth PNGs are read with the package's own
    loaders (no OpenCV).  ``device_preprocess`` (the switch the scene runners share): this program resamples its colour images with
    nearest selection only and integrates them as 8-bit, so all the switch does here is keep them 8-bit from the decoder on
    (``load_image_u8``: no float32 round trip); the values, and the meshes, are the same.

    ``render_keyframes``: after fusion, ray-cast the volume from every fused keyframe's own view at the prediction size (one launch,
    ``TSDFVolume.render``) and save the fused depth maps next to the meshes as ``keyframe_<dataset>_<system>+tsdf_predictions_<scene>.npz``,
    the layout of the network's predictions; if the scene has ground-truth depth, also their error metrics (``..._errors_<scene>.npz``),
    evaluated on the device over the pixels where a surface was hit.  Without the flag nothing else is written or changed.

    ``evaluate_3d``: also fuse the ground-truth depth maps (as ``save_groundtruth`` does; its mesh file is written only with that flag),
    keep that surface's vertices on the device, score the system's surface against them (``TSDFVolume.score_against`` with
    ``threshold_3d`` metres), print the six metrics on one line and save them as ``<mesh name of the system>_errors3d.npz``: ``arr_0``
    float32 [6], ``names``, ``counts`` int64 [2] (vertices of the prediction and of the ground truth) and ``threshold``.  Without the flag
    the program writes what it writes without it, byte for byte.

    ``evaluate_3d_density`` (points per square metre), ``evaluate_3d_voxel`` (metres), ``groundtruth_mesh`` (a .ply file), each with
    ``evaluate_3d``: the usual evaluation protocol instead of the vertex-to-vertex one.  With a density both surfaces are sampled on their
    faces, with a voxel both point sets are down-sampled to one point per voxel (``TSDFVolume.score_against``); with a ground-truth mesh
    (``TSDFFusion.meshread``) the system's surface is scored against that mesh, the ground-truth depth maps are not fused for the score
    (and not even loaded unless another flag needs them).  With any of the three, ``_errors3d.npz`` additionally holds ``sample_density``
    and ``voxel`` (NaN where not given) and ``points`` int64 [2], the sizes of the two point sets that were scored; ``counts`` stays the
    vertices of the two surfaces.  Without them the file is what it is without them, byte for byte.

    ``evaluate_3d_visible`` (needs ``evaluate_3d``, ``groundtruth_mesh`` and ``evaluate_3d_density``): the ground-truth mesh is first
    restricted to what the sequence observed, the faces whose three vertices are each seen by at least ``evaluate_3d_min_views`` of the
    fused keyframes' views at the prediction size (``visible_mesh``: the mesh is rasterised from those views on the device), so that the
    parts of a scan that the camera never faced do not count against completeness and recall.  ``_errors3d.npz`` then also holds
    ``visible_faces`` and ``total_faces``.

    ``evaluate_3d_align`` (metres; needs ``evaluate_3d``): the system's point set is registered to the ground truth's by trimmed ICP with
    that inlier distance before it is scored (``TSDFVolume.score_against(align_distance=...)``), ``evaluate_3d_align_scale`` (needs
    ``evaluate_3d_align``) with a scale.  ``_errors3d.npz`` then also holds ``transform`` float64 [4,4] (system -> ground truth),
    ``align_iterations``, ``align_status`` (an index of ``dvmvs.errors.REGISTRATION_STATUS``), ``align_fitness`` and ``align_rmse`` (of the
    last recorded iteration); they come down with the row, in the one download.  ``groundtruth_transform`` (needs
    ``groundtruth_mesh``): a text file of 16 numbers, the 4x4 that takes the mesh's frame into the dataset's world frame, applied to the
    mesh's vertices (in float64, rounded once) when the mesh is read, before visibility culling and sampling.  Without these flags the
    files are what they are without them, byte for byte.

    ``evaluate_3d_align_plane`` (needs ``evaluate_3d_align``, excludes ``evaluate_3d_align_scale``): the registration is point-to-plane
    (``TSDFVolume.score_against(align_plane=True)``) on normals estimated from the ground truth's point set, from
    ``evaluate_3d_align_neighbours`` nearest points within ``evaluate_3d_align_normal_distance`` metres (None: any distance).
    ``align_status`` is then an index of ``dvmvs.errors.REGISTRATION_PLANE_STATUS``, ``align_rmse`` the RMSE of the plane residual, and
    ``_errors3d.npz`` also holds ``align_status_name`` and ``align_rmse_point``.

    ``filter_consistency``: after the masks above, the keyframe predictions go up once and are filtered by multi-view geometric consistency
    in one launch (``dvmvs.consistency.filter_depths``): a pixel is kept, with its own depth, where at least ``consistency_views`` of the
    ``consistency_sources`` keyframes nearest to it in keyframe order (never across a "TRACKING LOST" line) agree within
    ``consistency_pixel`` pixels and ``consistency_relative`` of the depth.  The filtered predictions come down and are fused as before; the
    volume bounds are still those of the UNFILTERED predictions, so the meshes with and without the filter share a grid.  The system's mesh
    and the files of ``evaluate_3d`` and ``render_keyframes`` are written under ``<system_name>+consistent``; the kept share of the valid
    pixels is printed.  ``save_point_cloud`` (needs ``filter_consistency``): also writes ``<mesh name>_pointcloud.ply``, the kept pixels of
    a second call that averages the agreeing depths, as coloured world-space points.  Without these flags the program writes what it
    writes without them, byte for byte.

    ``clean_mesh_area`` (square metres), ``clean_mesh_faces`` (a count), ``clean_mesh_largest``: the system's mesh goes through
    ``dvmvs.components.filter_components`` on the device, which removes the connected components (floaters) with less area or fewer faces
    and, with ``clean_mesh_largest``, all but the largest (``ComponentFilter``).  With any of the three the system's files are written
    under ``<system_name>+clean`` (after ``+consistent`` when both are given), its ``.ply`` files, the progressive ones included, are the
    cleaned meshes, and ``evaluate_3d`` scores the cleaned surface; ``_errors3d.npz`` then also holds ``clean_min_area``,
    ``clean_min_faces``, ``clean_largest`` and ``clean_faces`` int64 [2], the kept and all faces of the system's mesh.  The ground-truth
    side is never cleaned, and ``render_keyframes`` ray-casts the VOLUME, which cleaning a mesh does not touch: its depth maps are what
    they are without these flags (under the ``+clean`` name).  Without these flags every file is what it is without them, byte for byte.

    ``simplify_mesh_voxel`` (metres) with ``simplify_mesh_average``: the system's mesh, after ``clean_mesh_*`` where those are given, goes
    through ``dvmvs.simplify.simplify_mesh`` on the device: one vertex per occupied cell of that edge, placed where the summed plane
    quadrics of the faces around it are smallest, so that edges and corners stay sharp; with ``simplify_mesh_average`` at the cell mean
    (``SimplifySettings``).  The system's files are then written under ``<system_name>+simple`` (after ``+consistent`` and ``+clean``), its
    ``.ply`` files, the progressive ones included, are the simplified meshes, and ``evaluate_3d`` scores the simplified surface;
    ``_errors3d.npz`` then also holds ``simplify_voxel``, ``simplify_average`` and ``simplify_faces`` int64 [2], the faces after and
    before the simplification.  The ground-truth side is never simplified, ``render_keyframes`` ray-casts the volume, and the mesh of
    ``point_mesh_voxel`` is not simplified.  Without these flags every file is what it is without them, byte for byte.

    ``smooth_mesh_iterations`` (a count, 0 .. 1024) with ``smooth_mesh_laplacian``, ``smooth_mesh_lambda``, ``smooth_mesh_mu`` and
    ``smooth_mesh_fixed_boundary``: the system's mesh, after ``clean_mesh_*`` and before ``simplify_mesh_*`` where those are given, goes
    through ``dvmvs.smooth.smooth_mesh`` on the device: that many iterations of Taubin's filter (a step with ``smooth_mesh_lambda``,
    default 0.5, then one with ``smooth_mesh_mu``, default -0.53, which does not shrink the surface), with ``smooth_mesh_laplacian`` of the
    plain Laplacian filter (a step with lambda), with ``smooth_mesh_fixed_boundary`` without moving the vertices on an open edge
    (``SmoothSettings``); the normals are recomputed from the smoothed faces.  The system's files are then written under
    ``<system_name>+smooth`` (after ``+clean``, before ``+simple``), its ``.ply`` files, the progressive ones included, are the smoothed
    meshes, and ``evaluate_3d`` scores the smoothed surface; ``_errors3d.npz`` then also holds ``smooth_iterations``, ``smooth_method``,
    ``smooth_lambda``, ``smooth_mu`` and ``smooth_fixed_boundary``.  The ground-truth side is never smoothed, ``render_keyframes``
    ray-casts the volume, and the mesh of ``point_mesh_voxel`` is not smoothed (its implicit surface is smooth already).  Without these
    flags every file is what it is without them, byte for byte.

    ``clean_points_neighbours`` (a count, 1 .. 32) with ``clean_points_ratio`` and ``clean_points_max_distance`` (metres),
    ``clean_points_radius`` (metres) with ``clean_points_min_neighbours`` (each needs ``save_point_cloud``): the fused point cloud goes
    through ``dvmvs.outliers.filter_outliers`` on the device before it comes down (``OutlierFilter``).  The first removes the points whose
    mean distance to their ``clean_points_neighbours`` nearest points is more than ``clean_points_ratio`` sample deviations above the
    cloud's mean (statistical outlier removal; ``clean_points_max_distance`` bounds the neighbour search, which otherwise follows a far
    outlier until it has its neighbours, and a point without a neighbour inside it is removed), the second those with fewer than
    ``clean_points_min_neighbours`` points within ``clean_points_radius``; with both, the second runs on what the first keeps.  The
    filtered cloud is written ADDITIONALLY as ``<mesh name>_pointcloud_clean.ply`` and the kept share of the points is printed;
    ``_pointcloud.ply`` and every other file are what they are without these flags, byte for byte.

    ``point_normals_neighbours`` (a count, 3 .. 32) with ``point_normals_max_distance`` (metres; None: unbounded), each needing
    ``save_point_cloud``: the point cloud, the cleaned one where ``clean_points_*`` are given and the fused one otherwise, gets oriented
    normals on the device (``dvmvs.normals.estimate_normals``): the direction of least spread of each point's ``point_normals_neighbours``
    nearest points within ``point_normals_max_distance``, the point itself among them, turned toward the camera centre of the keyframe
    the point came from (``dvmvs.consistency.fused_point_views``).  The cloud with its normals is written ADDITIONALLY as
    ``<mesh name>_pointcloud_normals.ply`` (``TSDFFusion.pcwrite_normals``), without the points that have no valid normal (fewer than
    three neighbours within the distance, or all of them in one place), and the share of valid points is printed; every other file is
    what it is without these flags, byte for byte.

    ``point_mesh_voxel`` (metres) with ``point_mesh_radius`` (metres; None: 2.5 voxels), ``point_mesh_neighbours`` (1 .. 32) and
    ``point_mesh_min_neighbours``, needing ``filter_consistency``, ``save_point_cloud`` and ``point_normals_neighbours``: the cloud that
    ``_pointcloud_normals.ply`` holds is meshed on the device (``dvmvs.implicit.mesh_points_device``: the implicit moving-least-squares
    signed distance of the oriented points on a grid of ``point_mesh_voxel``, with weights that reach zero at ``point_mesh_radius``, then
    marching cubes, without the crossings at the edge of the band around the points) and written ADDITIONALLY as
    ``<mesh name>_pointcloud_mesh.ply`` (``TSDFFusion.meshwrite``; normals and colours are those of the nearest point); with
    ``clean_mesh_*`` that mesh goes through the same component filter.  Every other file is what it is without these flags, byte for
    byte.

    ``sparse_volume`` with ``sparse_volume_bricks`` (the pool's capacity in bricks of 8 x 8 x 8 voxels): the system's predictions are fused
    into a ``SparseTSDFVolume`` on the lattice that starts at the volume bounds' lower corner, which allocates the bricks the predictions
    touch, and then made dense (``SparseTSDFVolume.dense``) over the allocated bricks; frames before a brick's birth are not applied to it
    -- the one stated difference from the dense volume, inherent to every hashed volume.  The ground-truth side and every later stage are
    what they are without the flag; the system's files are written under ``<system_name>+sparse`` (before the other suffixes).

    ``sparse_volume_extract`` (needs ``sparse_volume``): the system's mesh files are written straight from the sparse volume's pool
    (``SparseTSDFVolume.get_mesh``: extract -> clean -> smooth -> simplify on device tensors) and ``evaluate_3d`` scores with the sparse
    volume's ``score_against``; ``dense()`` is called only when another requested stage needs a ``TSDFVolume`` (``render_keyframes``).  The
    surface is the dense one's as a set of welded triangles, listed by brick instead of by voxel; the output folder stays
    ``<system_name>+sparse``.

    ``sparse_volume_render`` (needs ``sparse_volume``): ``render_keyframes`` ray-casts the keyframes straight from the sparse volume's pool
    (``SparseTSDFVolume.render``) instead of from ``dense()``; the files are the same bytes.  With ``sparse_volume_extract`` as well,
    ``dense()`` is never called."""
    settings = _settings(locals())            # (the first statement: locals() is the arguments and nothing else) every refusal without a file
    scene = _load_scene(settings)
    keyframe_images, keyframe_predictions = _load_keyframes(settings, scene)
    groundtruths, volume_bounds = _groundtruth_and_bounds(settings, scene, keyframe_predictions)
    products = _filter_keyframes(settings, scene, keyframe_images, keyframe_predictions)
    os.makedirs(settings.reconstruction_folder, exist_ok=True)
    groundtruth_surface = _groundtruth_surface(settings, scene, groundtruths, volume_bounds)
    sparse = sparse_volume_for(settings, volume_bounds) if settings.sparse_volume else None
    volume, mesh_name = _fuse_system(settings, scene, keyframe_images, products.predictions, volume_bounds, sparse)
    _write_point_clouds(settings, mesh_name, products)
    if settings.evaluate_3d:
        _evaluate_3d(settings, scene, volume, groundtruth_surface, mesh_name)
    if settings.render_keyframes:
        _render_keyframes(settings, scene, sparse if settings.sparse_volume_render else _renderable(volume, volume_bounds), volume_bounds)


# ---- settings: run's arguments, checked ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Settings:
    """``run``'s arguments after ``_settings`` has checked them, with what they imply."""
    reconstruction_folder: str
    prediction_folder: str
    data_folder: str
    dataset_name: str
    scene_name: str
    system_name: str                   # as given: it names the prediction file and the keyframe index
    output_name: str                   # with "+consistent", "+clean", "+smooth", "+simple" where those apply: it names every file that is written
    voxel_size: float
    max_depth: float
    use_groundtruth_to_anchor: bool
    save_progressive: bool
    save_groundtruth: bool
    device: object
    device_preprocess: bool
    render_keyframes: bool
    evaluate_3d: bool
    threshold_3d: float
    filter_consistency: bool
    consistency_sources: int
    consistency: dict                  # filter_depths' thresholds: pixel_threshold, relative_threshold, min_views
    save_point_cloud: bool
    evaluate_3d_density: Optional[float]
    evaluate_3d_voxel: Optional[float]
    groundtruth_mesh: Optional[str]
    groundtruth_transform: Optional[str]
    protocol_3d: bool                  # a density, a voxel or a ground-truth mesh: the evaluation protocol instead of vertex to vertex
    fuse_groundtruth_3d: bool          # the score needs the surface fused from the ground-truth depth maps
    visible_min_views: Optional[int]   # evaluate_3d_visible: the views that must see a ground-truth face; None without it
    align: dict                        # _aligned_score's keywords: align_distance, align_scale, align_plane (None or score_against's keywords)
    clean: object                      # ComponentFilter of clean_mesh_*, or None
    simplify: object                   # SimplifySettings of simplify_mesh_*, or None
    smooth: object                     # SmoothSettings of smooth_mesh_*, or None
    clean_points: object               # OutlierFilter of clean_points_*, or None
    point_normals: Optional[tuple]     # (neighbours, max_distance) of point_normals_*, or None
    point_mesh: Optional[tuple]        # (voxel, radius, neighbours, min_neighbours) of point_mesh_*, or None
    sparse_volume: bool = False        # fuse the system's predictions into a SparseTSDFVolume, then dense()
    sparse_volume_bricks: int = 65536
    sparse_volume_render: bool = False    # render_keyframes ray-casts the sparse volume's pool instead of dense()
    sparse_volume_extract: bool = False   # the system's meshes and score straight from the sparse volume's pool; dense() only for rendering


def _settings(arguments):
    """The ``Settings`` of ``run``'s arguments (a dict by name).  Every refusal that needs no file is made here, and names its flag."""
    a = SimpleNamespace(**arguments)
    clean = _clean_filter(a.clean_mesh_area, a.clean_mesh_faces, a.clean_mesh_largest)
    simplify = _simplify_settings(a.simplify_mesh_voxel, a.simplify_mesh_average)
    smooth = _smooth_settings(a.smooth_mesh_iterations, a.smooth_mesh_laplacian, a.smooth_mesh_lambda, a.smooth_mesh_mu,
                              a.smooth_mesh_fixed_boundary)
    clean_points = _clean_points_filter(a.save_point_cloud, a.clean_points_neighbours, a.clean_points_ratio, a.clean_points_max_distance,
                                        a.clean_points_radius, a.clean_points_min_neighbours)
    point_normals = _point_normals_settings(a.save_point_cloud, a.point_normals_neighbours, a.point_normals_max_distance)
    point_mesh = _point_mesh_settings(a.filter_consistency, a.save_point_cloud, point_normals, a.point_mesh_voxel, a.point_mesh_radius,
                                      a.point_mesh_neighbours, a.point_mesh_min_neighbours)
    if a.save_point_cloud and not a.filter_consistency:
        raise ValueError("save_point_cloud needs filter_consistency: the point cloud is made of the pixels the filter keeps")
    protocol_3d = a.evaluate_3d_density is not None or a.evaluate_3d_voxel is not None or a.groundtruth_mesh is not None
    if protocol_3d and not a.evaluate_3d:
        raise ValueError("evaluate_3d_density, evaluate_3d_voxel and groundtruth_mesh say how evaluate_3d scores: they need evaluate_3d")
    if a.evaluate_3d_visible and not (a.evaluate_3d and a.groundtruth_mesh is not None and a.evaluate_3d_density is not None):
        raise ValueError("evaluate_3d_visible culls a ground-truth mesh whose kept faces are then sampled: it needs evaluate_3d, "
                         "groundtruth_mesh and evaluate_3d_density")
    if int(a.evaluate_3d_min_views) != 1 and not a.evaluate_3d_visible:
        raise ValueError("evaluate_3d_min_views says how evaluate_3d_visible culls: it needs evaluate_3d_visible")
    if int(a.evaluate_3d_min_views) < 1:
        raise ValueError(f"evaluate_3d_min_views must be at least 1, got {a.evaluate_3d_min_views}")
    if a.evaluate_3d_align is not None and not a.evaluate_3d:
        raise ValueError("evaluate_3d_align registers the surface that evaluate_3d scores: it needs evaluate_3d")
    if a.evaluate_3d_align_scale and a.evaluate_3d_align is None:
        raise ValueError("evaluate_3d_align_scale says how evaluate_3d_align registers: it needs evaluate_3d_align")
    if a.evaluate_3d_align_plane and (a.evaluate_3d_align is None or a.evaluate_3d_align_scale):
        raise ValueError("evaluate_3d_align_plane says how evaluate_3d_align registers, a rigid motion: it needs evaluate_3d_align and excludes "
                         "evaluate_3d_align_scale")
    if not a.evaluate_3d_align_plane and (int(a.evaluate_3d_align_neighbours) != 20 or a.evaluate_3d_align_normal_distance is not None):
        raise ValueError("evaluate_3d_align_neighbours and evaluate_3d_align_normal_distance say how evaluate_3d_align_plane estimates normals: "
                         "they need evaluate_3d_align_plane")
    align_plane = None
    if a.evaluate_3d_align_plane:
        align_plane = {"align_plane": True, "align_normal_neighbours": int(a.evaluate_3d_align_neighbours),
                       "align_normal_distance": np.inf if a.evaluate_3d_align_normal_distance is None else float(a.evaluate_3d_align_normal_distance)}
    if a.groundtruth_transform is not None and a.groundtruth_mesh is None:
        raise ValueError("groundtruth_transform moves the mesh of groundtruth_mesh: it needs groundtruth_mesh")
    if a.evaluate_3d_align is not None and not float(a.evaluate_3d_align) > 0.0:
        raise ValueError(f"evaluate_3d_align must be a positive distance, got {a.evaluate_3d_align}")
    if int(a.sparse_volume_bricks) != 65536 and not a.sparse_volume:
        raise ValueError("sparse_volume_bricks sizes the pool of sparse_volume: it needs sparse_volume")
    if int(a.sparse_volume_bricks) < 1:
        raise ValueError(f"sparse_volume_bricks must be at least 1, got {a.sparse_volume_bricks}")
    if a.sparse_volume_extract and not a.sparse_volume:
        raise ValueError("sparse_volume_extract meshes the pool of sparse_volume: it needs sparse_volume")
    if a.sparse_volume_render and not a.sparse_volume:
        raise ValueError("sparse_volume_render ray-casts the pool of sparse_volume: it needs sparse_volume")
    output_name = a.system_name + ("+sparse" if a.sparse_volume else "") + ("+consistent" if a.filter_consistency else "") + ("+clean" if clean is not None else "") + (
        "+smooth" if smooth is not None else "") + ("+simple" if simplify is not None else "")
    return Settings(
        reconstruction_folder=a.reconstruction_folder, prediction_folder=a.prediction_folder, data_folder=a.data_folder,
        dataset_name=a.dataset_name, scene_name=a.scene_name, system_name=a.system_name, output_name=output_name, voxel_size=a.voxel_size,
        max_depth=a.max_depth, use_groundtruth_to_anchor=a.use_groundtruth_to_anchor, save_progressive=a.save_progressive,
        save_groundtruth=a.save_groundtruth, device=a.device, device_preprocess=a.device_preprocess, render_keyframes=a.render_keyframes,
        evaluate_3d=a.evaluate_3d, threshold_3d=a.threshold_3d, filter_consistency=a.filter_consistency,
        consistency_sources=a.consistency_sources,
        consistency=dict(pixel_threshold=a.consistency_pixel, relative_threshold=a.consistency_relative, min_views=a.consistency_views),
        save_point_cloud=a.save_point_cloud, evaluate_3d_density=a.evaluate_3d_density, evaluate_3d_voxel=a.evaluate_3d_voxel,
        groundtruth_mesh=a.groundtruth_mesh, groundtruth_transform=a.groundtruth_transform, protocol_3d=protocol_3d,
        fuse_groundtruth_3d=a.evaluate_3d and a.groundtruth_mesh is None,
        visible_min_views=int(a.evaluate_3d_min_views) if a.evaluate_3d_visible else None,
        align={"align_distance": a.evaluate_3d_align, "align_scale": a.evaluate_3d_align_scale, "align_plane": align_plane},
        clean=clean, simplify=simplify, smooth=smooth, clean_points=clean_points, point_normals=point_normals, point_mesh=point_mesh,
        sparse_volume=bool(a.sparse_volume), sparse_volume_bricks=int(a.sparse_volume_bricks),
        sparse_volume_render=bool(a.sparse_volume_render), sparse_volume_extract=bool(a.sparse_volume_extract))


def _number(value):
    return not isinstance(value, bool) and isinstance(value, (int, float, np.integer, np.floating))


def _clean_filter(clean_mesh_area, clean_mesh_faces, clean_mesh_largest):
    """The ``ComponentFilter`` of ``run``'s three settings, None when none is given; each refusal names its flag."""
    if not isinstance(clean_mesh_largest, bool):
        raise ValueError(f"clean_mesh_largest must be a bool, got {clean_mesh_largest!r}")
    if clean_mesh_area is not None and not float(clean_mesh_area) >= 0.0:
        raise ValueError(f"clean_mesh_area must be an area in square metres, not negative or NaN, got {clean_mesh_area}")
    if clean_mesh_faces is not None and not (float(clean_mesh_faces) >= 0.0 and float(clean_mesh_faces).is_integer()):
        raise ValueError(f"clean_mesh_faces must be a whole number of faces, not negative, got {clean_mesh_faces}")
    if clean_mesh_area is None and clean_mesh_faces is None and not clean_mesh_largest:
        return None
    from dvmvs.components import ComponentFilter, filter_settings
    clean = ComponentFilter(0.0 if clean_mesh_area is None else float(clean_mesh_area), 0 if clean_mesh_faces is None else int(clean_mesh_faces),
                            clean_mesh_largest)
    try:
        filter_settings(clean)
    except ValueError as e:
        raise ValueError(f"clean_mesh_area / clean_mesh_faces: {e}") from None
    return clean


def _simplify_settings(simplify_mesh_voxel, simplify_mesh_average):
    """The ``SimplifySettings`` of ``run``'s two settings, None when no voxel is given; each refusal names its flag."""
    if not isinstance(simplify_mesh_average, bool):
        raise ValueError(f"simplify_mesh_average must be a bool, got {simplify_mesh_average!r}")
    if simplify_mesh_voxel is None:
        if simplify_mesh_average:
            raise ValueError("simplify_mesh_average says how simplify_mesh_voxel places a cell's vertex: it needs simplify_mesh_voxel")
        return None
    if not _number(simplify_mesh_voxel) or not 0.0 < float(simplify_mesh_voxel) < np.inf:
        raise ValueError(f"simplify_mesh_voxel must be a positive, finite cell edge in metres, got {simplify_mesh_voxel!r}")
    from dvmvs.simplify import SimplifySettings
    return SimplifySettings(float(simplify_mesh_voxel), "average" if simplify_mesh_average else "quadric")


def _smooth_settings(iterations, laplacian, lam, mu, fixed_boundary):
    """The ``SmoothSettings`` of ``run``'s five settings, None when no iteration count is given; each refusal names its flag."""
    for flag, value in (("smooth_mesh_laplacian", laplacian), ("smooth_mesh_fixed_boundary", fixed_boundary)):
        if not isinstance(value, bool):
            raise ValueError(f"{flag} must be a bool, got {value!r}")
    if iterations is None:
        if laplacian or lam is not None or mu is not None or fixed_boundary:
            raise ValueError("smooth_mesh_laplacian, smooth_mesh_lambda, smooth_mesh_mu and smooth_mesh_fixed_boundary say how "
                             "smooth_mesh_iterations smooths: they need smooth_mesh_iterations")
        return None
    if not _number(iterations) or not float(iterations).is_integer() or not 0 <= int(iterations) <= 1024:
        raise ValueError(f"smooth_mesh_iterations must be a whole number of iterations in [0, 1024], got {iterations!r}")
    if lam is not None and not (_number(lam) and 0.0 < float(lam) <= 1.0):
        raise ValueError(f"smooth_mesh_lambda must be a factor in (0, 1], got {lam!r}")
    if mu is not None and laplacian:
        raise ValueError("smooth_mesh_mu is the second factor of Taubin's filter: it excludes smooth_mesh_laplacian")
    from dvmvs.smooth import SmoothSettings, smooth_settings
    defaults = SmoothSettings(0)
    lam = defaults.lam if lam is None else float(lam)
    if mu is not None and not (_number(mu) and -1.0 <= float(mu) < -lam):
        raise ValueError(f"smooth_mesh_mu must be a factor in [-1, -smooth_mesh_lambda) = [-1, {-lam}), got {mu!r}")
    smooth = SmoothSettings(int(iterations), "laplacian" if laplacian else "taubin", lam, defaults.mu if mu is None else float(mu),
                            "fixed" if fixed_boundary else "free")
    try:
        smooth_settings(smooth)
    except ValueError as e:
        raise ValueError(f"smooth_mesh_lambda / smooth_mesh_mu: {e}") from None
    return smooth


def _clean_points_filter(save_point_cloud, neighbours, ratio, max_distance, radius, min_neighbours):
    """The ``OutlierFilter`` of ``run``'s five ``clean_points_*`` settings, None when none is given; each refusal names its flag."""
    if not _number(ratio) or not 0.0 <= float(ratio) < np.inf:
        raise ValueError(f"clean_points_ratio must be a finite number of deviations, not negative, got {ratio!r}")
    if neighbours is not None and not (_number(neighbours) and float(neighbours).is_integer() and 1 <= int(neighbours) <= 32):
        raise ValueError(f"clean_points_neighbours must be a whole number of neighbours in [1, 32], got {neighbours!r}")
    if max_distance is not None and not (_number(max_distance) and float(max_distance) > 0.0):
        raise ValueError(f"clean_points_max_distance must be a positive distance in metres, got {max_distance!r}")
    if radius is not None and not (_number(radius) and 0.0 <= float(radius) < np.inf):
        raise ValueError(f"clean_points_radius must be a finite distance in metres, not negative, got {radius!r}")
    if min_neighbours is not None and not (_number(min_neighbours) and float(min_neighbours).is_integer() and 1 <= int(min_neighbours) < 2 ** 31):
        raise ValueError(f"clean_points_min_neighbours must be a whole number of neighbours, at least 1, got {min_neighbours!r}")
    if float(ratio) != 2.0 and neighbours is None:
        raise ValueError("clean_points_ratio says how clean_points_neighbours filters: it needs clean_points_neighbours")
    if max_distance is not None and neighbours is None:
        raise ValueError("clean_points_max_distance bounds the search of clean_points_neighbours: it needs clean_points_neighbours")
    if radius is not None and min_neighbours is None:
        raise ValueError("clean_points_radius needs clean_points_min_neighbours, the neighbours a point must have within it")
    if min_neighbours is not None and radius is None:
        raise ValueError("clean_points_min_neighbours needs clean_points_radius, the distance its neighbours are counted within")
    if neighbours is None and radius is None:
        return None
    if not save_point_cloud:
        raise ValueError("clean_points_neighbours and clean_points_radius filter the cloud of save_point_cloud: they need save_point_cloud")
    from dvmvs.outliers import OutlierFilter, filter_settings
    clean_points = OutlierFilter(None if neighbours is None else int(neighbours), float(ratio), None if max_distance is None else float(max_distance),
                                 None if radius is None else float(radius), None if min_neighbours is None else int(min_neighbours))
    filter_settings(clean_points)
    return clean_points


def _point_normals_settings(save_point_cloud, neighbours, max_distance):
    """``(neighbours, max_distance)`` of ``run``'s two ``point_normals_*`` settings (``max_distance`` inf when not given), None when neither
    is given; each refusal names its flag."""
    if neighbours is not None and not (_number(neighbours) and float(neighbours).is_integer() and 3 <= int(neighbours) <= 32):
        raise ValueError(f"point_normals_neighbours must be a whole number of neighbours in [3, 32], got {neighbours!r}")
    if max_distance is not None and not (_number(max_distance) and float(max_distance) > 0.0):
        raise ValueError(f"point_normals_max_distance must be a positive distance in metres, got {max_distance!r}")
    if max_distance is not None and neighbours is None:
        raise ValueError("point_normals_max_distance bounds the search of point_normals_neighbours: it needs point_normals_neighbours")
    if neighbours is None:
        return None
    if not save_point_cloud:
        raise ValueError("point_normals_neighbours estimates the normals of the cloud of save_point_cloud: it needs save_point_cloud")
    return int(neighbours), np.inf if max_distance is None else float(max_distance)


def _point_mesh_settings(filter_consistency, save_point_cloud, point_normals, voxel, radius, neighbours, min_neighbours):
    """``(voxel, radius, neighbours, min_neighbours)`` of ``run``'s four ``point_mesh_*`` settings (``radius`` 2.5 voxels when not given), None
    when ``point_mesh_voxel`` is not given; each refusal names its flag."""
    if voxel is not None and not (_number(voxel) and 0.0 < float(voxel) < np.inf):
        raise ValueError(f"point_mesh_voxel must be a positive voxel size in metres, got {voxel!r}")
    if radius is not None and not (_number(radius) and 0.0 < float(radius) < np.inf):
        raise ValueError(f"point_mesh_radius must be a positive distance in metres, got {radius!r}")
    if not (_number(neighbours) and float(neighbours).is_integer() and 1 <= int(neighbours) <= 32):
        raise ValueError(f"point_mesh_neighbours must be a whole number of neighbours in [1, 32], got {neighbours!r}")
    if not (_number(min_neighbours) and float(min_neighbours).is_integer() and 1 <= int(min_neighbours) < 2 ** 31):
        raise ValueError(f"point_mesh_min_neighbours must be a whole number of neighbours, at least 1, got {min_neighbours!r}")
    if voxel is None:
        if radius is not None or int(neighbours) != 32 or int(min_neighbours) != 3:
            raise ValueError("point_mesh_radius, point_mesh_neighbours and point_mesh_min_neighbours say how point_mesh_voxel meshes: they need "
                             "point_mesh_voxel")
        return None
    if not (filter_consistency and save_point_cloud and point_normals is not None):
        raise ValueError("point_mesh_voxel meshes the cloud with normals of point_normals_neighbours: it needs filter_consistency, "
                         "save_point_cloud and point_normals_neighbours")
    return float(voxel), 2.5 * float(voxel) if radius is None else float(radius), int(neighbours), int(min_neighbours)


# ---- the stages of run, in its order ------------------------------------------------------------------------------------------------------
class Scene(NamedTuple):
    """What ``_load_scene`` reads of a scene and of its prediction file."""
    folder: str
    original_K: np.ndarray                 # of the images as they are stored
    all_poses: np.ndarray                  # [frames,4,4] camera-to-world
    all_image_filenames: list
    predictions: np.ndarray                # [keyframes,height,width], the file's array: ``_load_keyframes`` masks it in place
    height: int                            # the prediction size
    width: int
    keyframe_poses: list
    keyframe_image_filenames: list
    keyframe_segments: list                # the number of "TRACKING LOST" lines before each keyframe
    preprocessor: object                   # PreprocessImage from the stored size to the prediction size
    scaled_K: np.ndarray                   # the intrinsics at the prediction size


class ConsistencyProducts(NamedTuple):
    """What ``_filter_keyframes`` makes: the predictions to fuse and, where asked for and there are keyframes, host arrays for the
    ``_pointcloud*.ply`` files (None otherwise)."""
    predictions: list                      # the keyframe predictions, filtered where filter_consistency is given
    cloud: Optional[np.ndarray] = None     # [P,6] xyzrgb
    clean_cloud: Optional[np.ndarray] = None
    normals_cloud: Optional[tuple] = None  # (xyzrgb [Q,6], normals [Q,3])
    cloud_mesh: Optional[tuple] = None     # the four arrays of TSDFFusion.meshwrite


def _image_loader(settings):
    """The colour image reader: 8-bit from the decoder on with ``device_preprocess`` (``resize_nearest`` only selects pixels: the uint8
    values are those of the float path's astype)."""
    from dvmvs.dataset_loader import load_image, load_image_u8
    return load_image_u8 if settings.device_preprocess else load_image


def _mesh_name(settings, system):
    return (f"{settings.reconstruction_folder}/reconstruction_voxelsize-{settings.voxel_size}_maxdepth-{settings.max_depth}_"
            f"anchor-{settings.use_groundtruth_to_anchor}_{system}_{settings.dataset_name}_{settings.scene_name}")


def _load_scene(settings):
    """Intrinsics, poses, the prediction file and the keyframe index of the scene, and from them the keyframes' poses, file names and
    segments, the pre-processor to the prediction size and the intrinsics there."""
    from dvmvs.dataset_loader import PreprocessImage
    scene_folder = os.path.join(settings.data_folder, settings.dataset_name, settings.scene_name)
    original_K = np.loadtxt(os.path.join(scene_folder, "K.txt")).astype(np.float32)
    all_poses = np.fromfile(os.path.join(scene_folder, "poses.txt"), dtype=float, sep="\n ").reshape((-1, 4, 4))
    all_image_filenames = sorted(glob.glob(os.path.join(scene_folder, "images", "*.png")))

    pattern = f"keyframe_{settings.dataset_name}_{settings.system_name}_predictions_{settings.scene_name}*"
    prediction_files = glob.glob(os.path.join(settings.prediction_folder, pattern))
    if not prediction_files:
        raise FileNotFoundError(f"no prediction file {pattern} in {settings.prediction_folder}")
    predictions = np.load(prediction_files[0])["arr_0"]
    prediction_height, prediction_width = np.shape(predictions[0])

    nmeas = settings.system_name.split("_")[2]
    index_name = f"keyframe+{settings.dataset_name}+{settings.scene_name}+nmeas+{nmeas}"
    with open(os.path.join(settings.data_folder, "indices", index_name)) as f:
        keyframe_lines = [line.rstrip("\n") for line in f if line.strip()]
    keyframe_poses, keyframe_image_filenames, keyframe_segments = [], [], []
    segment = 0
    for line in keyframe_lines:
        if line == "TRACKING LOST":
            segment += 1
            continue
        keyframe_segments.append(segment)
        image_filename = os.path.join(scene_folder, "images", line.split(" ")[0])
        keyframe_poses.append(all_poses[all_image_filenames.index(image_filename)])
        keyframe_image_filenames.append(image_filename)

    first = _image_loader(settings)(all_image_filenames[0])
    preprocessor = PreprocessImage(K=original_K, old_width=first.shape[1], old_height=first.shape[0], new_width=prediction_width,
                                   new_height=prediction_height, distortion_crop=0, perform_crop=False)
    return Scene(scene_folder, original_K, all_poses, all_image_filenames, predictions, prediction_height, prediction_width, keyframe_poses,
                 keyframe_image_filenames, keyframe_segments, preprocessor, preprocessor.get_updated_intrinsics())


def _load_keyframes(settings, scene):
    """``(images, predictions)`` of the keyframes: the colour images at the prediction size as uint8, and the predictions, views of
    ``scene.predictions`` that are masked IN PLACE: ScanNet's black borders and everything beyond ``max_depth`` become 0."""
    from dvmvs.dataset_loader import resize_nearest
    load_image = _image_loader(settings)
    # ScanNet frames have black, undistorted-away borders: predictions there are masked
    edge = 10
    edge_mask = np.zeros((scene.height, scene.width), dtype=bool)
    edge_mask[:edge, :] = edge_mask[-edge:, :] = True
    edge_mask[:, :edge] = edge_mask[:, -edge:] = True
    keyframe_images, keyframe_predictions = [], []
    for index, image_filename in enumerate(scene.keyframe_image_filenames):
        image = resize_nearest(load_image(image_filename), scene.width, scene.height)
        prediction = scene.predictions[index]
        if "scannet" in settings.dataset_name:
            prediction[np.logical_and(np.mean(image.astype(float), axis=-1) < 10.0, edge_mask)] = 0.0
        prediction[prediction > settings.max_depth] = 0.0
        keyframe_predictions.append(prediction)
        keyframe_images.append(image.astype(np.uint8))
    return keyframe_images, keyframe_predictions


def _groundtruth_and_bounds(settings, scene, keyframe_predictions):
    """``(ground-truth depth maps cut at max_depth, or None when no flag needs them; the volume bounds with their margin)``.  The bounds are
    those of the ground truth with ``use_groundtruth_to_anchor`` and of the (unfiltered) predictions otherwise."""
    from dvmvs.dataset_loader import load_depth_png
    groundtruths = None
    if settings.use_groundtruth_to_anchor or settings.save_groundtruth or settings.fuse_groundtruth_3d:
        groundtruths = []
        for filename in sorted(glob.glob(os.path.join(scene.folder, "depth", "*.png"))):
            depth = load_depth_png(filename)
            depth[depth > settings.max_depth] = 0.0
            groundtruths.append(depth)
    if settings.use_groundtruth_to_anchor:
        volume_bounds = TSDFFusion.calculate_volume_bounds(groundtruths, scene.all_poses, scene.original_K)
    else:
        volume_bounds = TSDFFusion.calculate_volume_bounds(keyframe_predictions, scene.keyframe_poses, scene.scaled_K)
    return groundtruths, volume_bounds * 1.05      # margin for errors in the bounds


def _filter_keyframes(settings, scene, images, predictions):
    """With ``filter_consistency`` the keyframe predictions filtered by consistency (a list of host arrays, as they came) and, with
    ``save_point_cloud``, the fused point cloud [P,6] xyzrgb on the host, with ``clean_points`` (an ``OutlierFilter``) also the rows of it
    that the filter keeps, chosen on the device, with ``point_normals`` (``(neighbours, max_distance)``) also ``(xyzrgb [Q,6], normals
    [Q,3])``: the points of the cleaned cloud (of the fused one without ``clean_points``) that have a valid normal, oriented toward the
    camera centre of their keyframe, and with ``point_mesh`` (``(voxel, radius, neighbours, min_neighbours)``) also the mesh of those
    points and normals (``mesh_points_device``, cleaned by ``settings.clean``) as the four host arrays of ``TSDFFusion.meshwrite``.
    Without the flag, or without a keyframe, the predictions as they came and nothing else."""
    if not (settings.filter_consistency and predictions):
        return ConsistencyProducts(predictions)
    from dvmvs.consistency import filter_depths, fused_point_cloud, fused_point_views, nearest_sources
    device, K = settings.device, scene.scaled_K
    depths = torch.as_tensor(np.stack(predictions).astype(np.float32), device=device)
    cameras = torch.as_tensor(np.stack(scene.keyframe_poses).astype(np.float32), device=device)
    sources = torch.as_tensor(nearest_sources(len(predictions), settings.consistency_sources, scene.keyframe_segments), device=device)
    kept, _, _ = filter_depths(depths, K, cameras, sources, average=False, with_count=False, **settings.consistency)
    valid = torch.isfinite(depths) & (depths > 0)
    print("Consistency filter: kept {:.1f} % of the valid pixels of {} keyframes".format(
        100.0 * float((kept > 0).sum()) / max(int(valid.sum()), 1), len(predictions)))
    cloud = clean_cloud = normals_cloud = cloud_mesh = None
    if settings.save_point_cloud:
        averaged, _, points = filter_depths(depths, K, cameras, sources, average=True, with_count=False, with_points=True, **settings.consistency)
        cloud = fused_point_cloud(averaged, points, np.stack(images))
        oriented = cloud                                                  # the cloud that gets the normals, on the device
        if settings.clean_points is not None:
            from dvmvs.outliers import filter_outliers_device
            oriented, keep = filter_outliers_device(cloud, settings.clean_points, return_mask=True)
            clean_cloud = oriented.cpu().numpy()
            print("Outlier filter: kept {:.1f} % of the {} points of the cloud".format(
                100.0 * len(clean_cloud) / max(int(cloud.shape[0]), 1), int(cloud.shape[0])))
        if settings.point_normals is not None:
            from dvmvs.normals import estimate_normals_device
            views = fused_point_views(averaged)
            if settings.clean_points is not None:
                views = views[keep]
            normals, _, valid = estimate_normals_device(oriented[:, :3], settings.point_normals[0], settings.point_normals[1], cameras[:, :3, 3],
                                                        views)
            normals_cloud = (oriented[valid].cpu().numpy(), normals[valid].cpu().numpy())
            print("Point normals: {:.1f} % of the {} points have a valid normal".format(
                100.0 * len(normals_cloud[0]) / max(int(oriented.shape[0]), 1), int(oriented.shape[0])))
            if settings.point_mesh is not None and len(normals_cloud[0]) > 0:
                from dvmvs.implicit import mesh_points_device
                voxel, radius, neighbours, min_neighbours = settings.point_mesh
                cloud_mesh = tuple(a.cpu().numpy() for a in mesh_points_device(oriented[valid], normals[valid], voxel, radius, neighbours,
                                                                                min_neighbours, clean=settings.clean))
                print("Point mesh: {} vertices and {} faces from {} points".format(len(cloud_mesh[0]), len(cloud_mesh[1]),
                                                                                   len(normals_cloud[0])))
        cloud = cloud.cpu().numpy()
    return ConsistencyProducts(list(kept.cpu().numpy()), cloud, clean_cloud, normals_cloud, cloud_mesh)


def _groundtruth_surface(settings, scene, groundtruths, volume_bounds):
    """What ``evaluate_3d`` scores against, on the device: the vertices (with ``protocol_3d`` the vertices and faces) of the surface fused from
    the ground-truth depth maps, or the ``groundtruth_mesh`` file moved by ``groundtruth_transform``; None without ``evaluate_3d``.  With
    ``save_groundtruth`` the fused ground truth's mesh file is written on the way."""
    surface = None
    if settings.save_groundtruth or settings.fuse_groundtruth_3d:
        volume = TSDFVolume(volume_bounds, voxel_size=settings.voxel_size, device=settings.device)
        load_image = _image_loader(settings)
        images = [load_image(f).astype(np.uint8) for f in scene.all_image_filenames]
        if settings.save_groundtruth:
            TSDFFusion.integrate(volume, images, groundtruths, scene.all_poses, scene.original_K, _mesh_name(settings, "GROUNDTRUTH"),
                                 save_progressive=False)
        else:      # the same fusion, without its mesh file
            for image, depth, pose in zip(images, groundtruths, scene.all_poses):
                volume.integrate(image, depth, scene.original_K, pose, obs_weight=1.0)
        if settings.fuse_groundtruth_3d:       # stay on the device when the volume goes
            surface = volume.mesh_tensors() if settings.protocol_3d else volume.vertices()
        del volume
    if settings.evaluate_3d and settings.groundtruth_mesh is not None:
        mesh_verts, mesh_faces = TSDFFusion.meshread(settings.groundtruth_mesh)
        if settings.groundtruth_transform is not None:
            mesh_verts = apply_transform(mesh_verts, load_transform(settings.groundtruth_transform))
        surface = tuple(torch.as_tensor(a, device=settings.device) for a in (mesh_verts, mesh_faces))
    return surface


def _fuse_system(settings, scene, images, predictions, volume_bounds, sparse=None):
    """Fuses the keyframe predictions and writes the system's meshes (``TSDFFusion.integrate``): ``(the volume, the mesh name)``.  With
    ``sparse_volume`` the frames go into ``sparse`` (``sparse_volume_for``; made here when None), which the caller keeps."""
    mesh_name = _mesh_name(settings, settings.output_name)
    if settings.sparse_volume:
        sparse = sparse_volume_for(settings, volume_bounds) if sparse is None else sparse
        return _fuse_system_sparse(settings, scene, images, predictions, volume_bounds, mesh_name, sparse), mesh_name
    volume = TSDFVolume(volume_bounds, voxel_size=settings.voxel_size, device=settings.device)
    TSDFFusion.integrate(volume, images, predictions, scene.keyframe_poses, scene.scaled_K, mesh_name, settings.save_progressive,
                         simplify=settings.simplify, smooth=settings.smooth, clean=settings.clean)
    return volume, mesh_name


def sparse_volume_for(settings, volume_bounds):
    """The ``SparseTSDFVolume`` of ``sparse_volume``: its lattice starts at the lower corner of the bounds, so its voxels are those of the
    dense volumes of the same run; the extent of the bounds is not used."""
    from dvmvs.tsdf.sparse_volume import SparseTSDFVolume
    return SparseTSDFVolume(settings.voxel_size, origin=np.asarray(volume_bounds, dtype=np.float64)[:, 0], max_bricks=settings.sparse_volume_bricks,
                            device=settings.device)


def _fuse_system_sparse(settings, scene, images, predictions, volume_bounds, mesh_name, sparse):
    """``_fuse_system`` through the ``SparseTSDFVolume`` ``sparse``: every keyframe with weight 1, then ``dense()`` over the allocated bricks (over the
    bounds when nothing was allocated); the meshes are written as ``TSDFFusion.integrate`` writes them.  With ``sparse_volume_extract``
    the meshes come from the pool, nothing is made dense, and the sparse volume itself is returned."""
    stages = dict(simplify=settings.simplify, smooth=settings.smooth, clean=settings.clean)

    def meshed():      # what the meshes are taken from
        return sparse if settings.sparse_volume_extract else _renderable(sparse, volume_bounds)

    for i in range(len(images)):
        print(f"Fusing frame {i + 1}/{len(images)} for {mesh_name}")
        sparse.integrate(images[i], predictions[i], scene.scaled_K, scene.keyframe_poses[i], obs_weight=1.0)
        if settings.save_progressive:
            TSDFFusion.meshwrite(f"{mesh_name}_frame_{i:05d}.ply", *meshed().get_mesh(**stages))
    volume = meshed()
    print(f"{sparse.n_bricks} bricks of {sparse.max_bricks} allocated; saving mesh to", mesh_name)
    TSDFFusion.meshwrite(mesh_name + "_complete.ply", *volume.get_mesh(**stages))
    return volume


def _renderable(volume, volume_bounds):
    """``volume`` as a ``TSDFVolume``: a ``SparseTSDFVolume`` made dense over its allocated bricks (over the bounds when it has none)."""
    if isinstance(volume, TSDFVolume):
        return volume
    return volume.dense() if volume.n_bricks else volume.dense(volume_bounds)


def _write_point_clouds(settings, mesh_name, products):
    """Writes the ``_pointcloud*.ply`` files that the flags ask for; a product that was not made (a scene without keyframes, a cloud without
    a valid normal) is written empty."""
    if not settings.save_point_cloud:
        return

    no_cloud, no_normals = np.zeros((0, 6), np.float32), np.zeros((0, 3), np.float32)
    no_mesh = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    print("Saving point cloud to", mesh_name + "_pointcloud.ply")
    TSDFFusion.pcwrite(mesh_name + "_pointcloud.ply", no_cloud if products.cloud is None else products.cloud)
    if settings.clean_points is not None:
        print("Saving cleaned point cloud to", mesh_name + "_pointcloud_clean.ply")
        TSDFFusion.pcwrite(mesh_name + "_pointcloud_clean.ply", no_cloud if products.clean_cloud is None else products.clean_cloud)
    if settings.point_normals is not None:
        print("Saving point cloud with normals to", mesh_name + "_pointcloud_normals.ply")
        TSDFFusion.pcwrite_normals(mesh_name + "_pointcloud_normals.ply", *(products.normals_cloud or (no_cloud, no_normals)))
    if settings.point_mesh is not None:
        print("Saving mesh of the point cloud to", mesh_name + "_pointcloud_mesh.ply")
        TSDFFusion.meshwrite(mesh_name + "_pointcloud_mesh.ply", *(products.cloud_mesh or no_mesh))


def _clean_entries(volume, clean):
    """What ``_errors3d.npz`` gains with a ``ComponentFilter``: its settings and the kept and all faces of the system's mesh (tensor shapes:
    nothing more is read than the extractions read themselves)."""
    if clean is None:
        return {}
    kept, total = int(volume.mesh_tensors(clean=clean)[1].shape[0]), int(volume.mesh_tensors()[1].shape[0])
    print("Mesh cleaned of small components: {} of {} faces kept".format(kept, total))
    return {"clean_min_area": np.float64(clean.min_area), "clean_min_faces": np.int64(clean.min_faces), "clean_largest": np.bool_(clean.keep_largest),
            "clean_faces": np.array([kept, total], dtype=np.int64)}


def _smooth_entries(smooth):
    """What ``_errors3d.npz`` gains with a ``SmoothSettings``: its settings."""
    if smooth is None:
        return {}
    print("Mesh smoothed by {} iterations of the {} filter (lambda {}, mu {}, boundary {})".format(smooth.iterations, smooth.method, smooth.lam,
                                                                                                  smooth.mu, smooth.boundary))
    return {"smooth_iterations": np.int64(smooth.iterations), "smooth_method": np.array(smooth.method), "smooth_lambda": np.float64(smooth.lam),
            "smooth_mu": np.float64(smooth.mu), "smooth_fixed_boundary": np.bool_(smooth.boundary == "fixed")}


def _simplify_entries(volume, clean, simplify, smooth=None):
    """What ``_errors3d.npz`` gains with a ``SimplifySettings``: its settings and the faces of the system's mesh after and before it."""
    if simplify is None:
        return {}
    kept = int(volume.mesh_tensors(simplify=simplify, smooth=smooth, clean=clean)[1].shape[0])
    total = int(volume.mesh_tensors(clean=clean)[1].shape[0])
    print("Mesh simplified with cells of {} m ({}): {} of {} faces left".format(simplify.voxel, simplify.contraction, kept, total))
    return {"simplify_voxel": np.float64(simplify.voxel), "simplify_average": np.bool_(simplify.contraction == "average"),
            "simplify_faces": np.array([kept, total], dtype=np.int64)}


def _evaluate_3d(settings, scene, volume, groundtruth, mesh_name):
    """Scores the fused surface against the ground truth on the device (``groundtruth``: its vertices; with ``protocol_3d`` a mesh, device
    verts and faces, with face sampling and / or voxel down-sampling of both sides, and with ``visible_min_views`` only the part of the mesh
    that the keyframes' views observed); one row comes down, is printed and saved as ``<mesh_name>_errors3d.npz``."""
    from dvmvs.errors import RECONSTRUCTION_METRICS
    threshold, clean, density, voxel = settings.threshold_3d, settings.clean, settings.evaluate_3d_density, settings.evaluate_3d_voxel
    score = dict(reference=groundtruth, threshold=threshold, return_sizes=True)
    if settings.protocol_3d:
        score.update(sample_density=density, voxel=voxel)
    if clean is not None:
        score["clean"] = clean
    if settings.simplify is not None:
        score["simplify"] = settings.simplify
    if settings.smooth is not None:
        score["smooth"] = settings.smooth
    if settings.visible_min_views is not None:
        if not scene.keyframe_poses:
            raise ValueError("evaluate_3d_visible: the scene has no keyframe to take the visibility from")
        score["visible_from"] = (scene.scaled_K, np.stack(scene.keyframe_poses), scene.height, scene.width, settings.visible_min_views)
    row, points, *kept, aligned = _aligned_score(volume, **settings.align, **score)
    metrics = ", ".join(f"{n} {v:.4f}" for n, v in zip(RECONSTRUCTION_METRICS, row))
    extra = {}
    if kept:
        print("Ground truth restricted to what {} keyframes saw: {} of {} faces".format(len(scene.keyframe_poses), kept[0][0], kept[0][1]))
        extra = {"visible_faces": np.int64(kept[0][0]), "total_faces": np.int64(kept[0][1])}
    if settings.protocol_3d:
        sizes = (int(volume.vertices(simplify=settings.simplify, smooth=settings.smooth, clean=clean).shape[0]), int(groundtruth[0].shape[0]))
        print("3-D metrics at {} m over {} predicted and {} ground-truth points (density {}, voxel {}; {} and {} vertices): {}".format(
            threshold, points[0], points[1], density, voxel, sizes[0], sizes[1], metrics))
        extra = {"sample_density": np.float64(np.nan if density is None else density), "voxel": np.float64(np.nan if voxel is None else voxel),
                 "points": np.array(points, dtype=np.int64), **extra}
    else:
        sizes = points
        print("3-D metrics at {} m over {} predicted and {} ground-truth vertices: {}".format(threshold, sizes[0], sizes[1], metrics))
    np.savez_compressed(mesh_name + "_errors3d.npz", arr_0=row, names=np.array(RECONSTRUCTION_METRICS), counts=np.array(sizes, dtype=np.int64),
                        threshold=np.float32(threshold), **extra, **aligned, **_clean_entries(volume, clean),
                        **_smooth_entries(settings.smooth), **_simplify_entries(volume, clean, settings.simplify, settings.smooth))


def _render_keyframes(settings, scene, volume, volume_bounds=None):
    """The fused depth of every keyframe: rendered, saved like predictions and, where ground truth exists, scored on the device.  A
    ``SparseTSDFVolume`` is ray-cast from its pool over the box of its allocated bricks (over ``volume_bounds`` when it has none): the box
    of ``_renderable``."""
    from dvmvs.dataset_loader import load_depth_png
    from dvmvs.errors import compute_errors_device
    from dvmvs.utils import save_predictions, save_results
    system_name, save_folder = f"keyframe_{settings.dataset_name}_{settings.output_name}+tsdf", settings.reconstruction_folder
    poses = scene.keyframe_poses
    if not poses:
        print("No keyframe to render")
        return
    box = {}
    if not isinstance(volume, TSDFVolume) and volume.brick_extent is None:
        box = {"bounds": volume_bounds}
    depth, _, _ = volume.render(scene.scaled_K, np.stack(poses), scene.height, scene.width, normals=False, colour=False, **box)
    hit = depth > 0
    print("Rendered {} keyframes from the fused volume: {:.1f} % of the pixels hit a surface".format(len(poses), 100.0 * float(hit.float().mean())))
    rendered = depth.cpu().numpy()
    depth_files = [os.path.join(scene.folder, "depth", os.path.basename(f)) for f in scene.keyframe_image_filenames]
    if os.path.isdir(os.path.join(scene.folder, "depth")) and all(os.path.exists(f) for f in depth_files):
        groundtruths = np.stack([scene.preprocessor.apply_depth(load_depth_png(f)) for f in depth_files]).astype(np.float32)
        gt = torch.from_numpy(groundtruths).to(depth.device)
        gt = torch.where(hit, gt, torch.zeros_like(gt))       # a miss takes no part in the metrics
        rows = compute_errors_device(gt, depth).cpu().numpy()
        save_results(rendered, groundtruths, system_name, settings.scene_name, save_folder, errors=rows)
    else:
        save_predictions(rendered, system_name, settings.scene_name, save_folder)


def load_transform(filename):
    """The float64 4x4 of a ``groundtruth_transform`` file: 16 numbers separated by white space, row by row, on any number of lines."""
    with open(filename) as f:
        words = f.read().split()
    try:
        values = np.array([float(w) for w in words], dtype=np.float64)
    except ValueError:
        values = np.zeros(0)
    if values.size != 16 or not np.isfinite(values).all():
        raise ValueError(f"groundtruth_transform: {filename} must hold the 16 finite numbers of a 4x4 matrix")
    return values.reshape(4, 4)


def apply_transform(verts, transform):
    """Mesh vertices [V,3] moved by a float64 4x4 (affine: its last row is not used), evaluated in float64 and rounded to float32 once."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    return (verts @ transform[:3, :3].T + transform[:3, 3]).astype(np.float32)


def build_parser():
    parser = ArgumentParser(description="TSDF reconstruction of a scene from saved keyframe depth predictions (writes .ply meshes)")
    parser.add_argument("--reconstruction_folder", default="./reconstructions", type=str)
    parser.add_argument("--prediction_folder", default="./predictions", type=str)
    parser.add_argument("--data_folder", default=".", type=str)
    parser.add_argument("--dataset_name", default="hololens-dataset", type=str)
    parser.add_argument("--scene_name", default="000", type=str)
    parser.add_argument("--system_name", default="320_256_3_dvmvs_fusionnet_online", type=str)
    parser.add_argument("--voxel_size", default=0.025, type=float)
    parser.add_argument("--max_depth", default=5.0, type=float)
    parser.add_argument("--use_groundtruth_to_anchor", action="store_true",
                        help="compute the volume bounds from the ground-truth depth maps (recommended when they are available)")
    parser.add_argument("--save_progressive", action="store_true", help="also write the mesh after every fused keyframe")
    parser.add_argument("--save_groundtruth", action="store_true", help="also write the reconstruction from the ground-truth depth maps")
    parser.add_argument("--device-preprocess", dest="device_preprocess", action="store_true",
                        help="load the colour images as 8-bit (no float32 round trip); same meshes")
    parser.add_argument("--render_keyframes", action="store_true",
                        help="also ray-cast the fused volume from every keyframe's view and save the fused depth maps (<system>+tsdf)")
    parser.add_argument("--evaluate_3d", action="store_true",
                        help="also fuse the ground-truth depth maps and score the system's mesh against that surface in 3-D on the device "
                             "(accuracy, completeness, chamfer, precision, recall, F-score; saved as <mesh name>_errors3d.npz)")
    parser.add_argument("--threshold_3d", default=0.05, type=float, help="distance threshold of precision / recall / F-score, metres")
    parser.add_argument("--evaluate_3d_density", default=None, type=float,
                        help="with --evaluate_3d: sample both surfaces on their faces, this many points per square metre, instead of taking their vertices")
    parser.add_argument("--evaluate_3d_voxel", default=None, type=float,
                        help="with --evaluate_3d: down-sample both point sets to one point per voxel of this edge, metres")
    parser.add_argument("--groundtruth_mesh", default=None, type=str,
                        help="with --evaluate_3d: score against this .ply mesh (ascii or binary little endian) instead of the fused ground-truth depth maps")
    parser.add_argument("--evaluate_3d_visible", action="store_true",
                        help="with --evaluate_3d, --groundtruth_mesh and --evaluate_3d_density: score against the part of the ground-truth "
                             "mesh that the fused keyframes saw (the mesh is rasterised from their views on the device)")
    parser.add_argument("--evaluate_3d_min_views", default=1, type=int,
                        help="with --evaluate_3d_visible: keyframes that must see each vertex of a ground-truth face for it to be kept")
    parser.add_argument("--evaluate_3d_align", default=None, type=float,
                        help="with --evaluate_3d: register the system's point set to the ground truth's by trimmed ICP with this inlier "
                             "distance, metres, before it is scored (on the device)")
    parser.add_argument("--evaluate_3d_align_scale", action="store_true", help="with --evaluate_3d_align: the registration also finds a scale")
    parser.add_argument("--evaluate_3d_align_plane", action="store_true",
                        help="with --evaluate_3d_align: register point to plane, on normals estimated from the ground truth's points (a rigid "
                             "motion; far fewer iterations on walls and floors)")
    parser.add_argument("--evaluate_3d_align_neighbours", default=20, type=int,
                        help="with --evaluate_3d_align_plane: nearest points a ground-truth normal is estimated from (3 .. 32)")
    parser.add_argument("--evaluate_3d_align_normal_distance", default=None, type=float,
                        help="with --evaluate_3d_align_plane: those points are searched within this distance only, metres")
    parser.add_argument("--groundtruth_transform", default=None, type=str,
                        help="with --groundtruth_mesh: a text file of 16 numbers, the 4x4 that takes the mesh's frame into the dataset's world frame")
    parser.add_argument("--filter_consistency", action="store_true",
                        help="fuse only the pixels that neighbouring keyframes agree on (multi-view geometric consistency, on the device); "
                             "files are written under <system>+consistent")
    parser.add_argument("--consistency_views", default=2, type=int, help="neighbouring keyframes that must agree for a pixel to be kept")
    parser.add_argument("--consistency_sources", default=4, type=int, help="neighbouring keyframes each keyframe is checked against (at most 16)")
    parser.add_argument("--consistency_pixel", default=1.0, type=float, help="largest re-projection error of an agreeing view, pixels")
    parser.add_argument("--consistency_relative", default=0.01, type=float, help="largest relative depth difference of an agreeing view")
    parser.add_argument("--save_point_cloud", action="store_true",
                        help="with --filter_consistency: also write the kept pixels as a coloured point cloud (<mesh name>_pointcloud.ply)")
    parser.add_argument("--point_normals_neighbours", default=None, type=int,
                        help="with --save_point_cloud: oriented normals of the point cloud (the cleaned one with --clean_points_*) on the "
                             "device, from this many nearest neighbours (3 .. 32), turned toward the camera that saw each point; the "
                             "cloud with normals is written additionally as <mesh name>_pointcloud_normals.ply")
    parser.add_argument("--point_normals_max_distance", default=None, type=float,
                        help="with --point_normals_neighbours: neighbours are searched within this distance only, metres (bounds the search; "
                             "a point with fewer than three inside it gets no normal and is left out of the file)")
    parser.add_argument("--point_mesh_voxel", default=None, type=float,
                        help="with --filter_consistency --save_point_cloud --point_normals_neighbours: mesh the point cloud with normals on "
                             "the device (implicit moving-least-squares signed distance on a grid of this voxel size, metres, then marching "
                             "cubes); the mesh is written additionally as <mesh name>_pointcloud_mesh.ply")
    parser.add_argument("--point_mesh_radius", default=None, type=float,
                        help="with --point_mesh_voxel: the distance at which a point's weight reaches zero, metres (default: 2.5 voxels)")
    parser.add_argument("--point_mesh_neighbours", default=32, type=int,
                        help="with --point_mesh_voxel: at most this many nearest points within the radius shape a node (1 .. 32)")
    parser.add_argument("--point_mesh_min_neighbours", default=3, type=int,
                        help="with --point_mesh_voxel: a node with fewer points with a normal within the radius carries no surface")
    parser.add_argument("--simplify_mesh_voxel", default=None, type=float,
                        help="simplify the system's mesh on the device (after --clean_mesh_*): one vertex per occupied cell of this edge, "
                             "metres, placed by the quadrics of the faces around it; files are written under <system>+simple")
    parser.add_argument("--simplify_mesh_average", action="store_true",
                        help="with --simplify_mesh_voxel: a cell's vertex is the mean of its vertices instead of the quadric minimiser")
    parser.add_argument("--smooth_mesh_iterations", default=None, type=int,
                        help="smooth the system's mesh on the device (after --clean_mesh_*, before --simplify_mesh_*): this many "
                             "iterations of Taubin's filter; normals are recomputed; files are written under <system>+smooth")
    parser.add_argument("--smooth_mesh_laplacian", action="store_true",
                        help="with --smooth_mesh_iterations: the plain Laplacian filter (it shrinks the surface) instead of Taubin's")
    parser.add_argument("--smooth_mesh_lambda", default=None, type=float,
                        help="with --smooth_mesh_iterations: the factor of the smoothing step, in (0, 1] (default 0.5)")
    parser.add_argument("--smooth_mesh_mu", default=None, type=float,
                        help="with --smooth_mesh_iterations: the factor of Taubin's second step, in [-1, -lambda) (default -0.53)")
    parser.add_argument("--smooth_mesh_fixed_boundary", action="store_true",
                        help="with --smooth_mesh_iterations: the vertices on an open edge of the mesh do not move")
    parser.add_argument("--clean_points_neighbours", default=None, type=int,
                        help="with --save_point_cloud: statistical outlier removal of the fused cloud on the device, over this many nearest "
                             "neighbours (1 .. 32); the result is written additionally as <mesh name>_pointcloud_clean.ply")
    parser.add_argument("--clean_points_ratio", default=2.0, type=float,
                        help="with --clean_points_neighbours: a point goes when its mean neighbour distance is more than this many sample "
                             "deviations above the cloud's mean")
    parser.add_argument("--clean_points_max_distance", default=None, type=float,
                        help="with --clean_points_neighbours: neighbours are searched within this distance only, metres (bounds the search "
                             "of far outliers; a point without a neighbour inside it goes)")
    parser.add_argument("--clean_points_radius", default=None, type=float,
                        help="with --save_point_cloud and --clean_points_min_neighbours: radius outlier removal of the fused cloud on the "
                             "device, metres (after the statistical filter when both are given)")
    parser.add_argument("--clean_points_min_neighbours", default=None, type=int,
                        help="with --clean_points_radius: a point stays when it has at least this many other points within the radius")
    parser.add_argument("--clean_mesh_area", default=None, type=float,
                        help="remove the connected components of the system's mesh with less area than this, square metres (on the device); "
                             "files are written under <system>+clean")
    parser.add_argument("--clean_mesh_faces", default=None, type=int,
                        help="remove the connected components of the system's mesh with fewer faces than this; files are written under <system>+clean")
    parser.add_argument("--clean_mesh_largest", action="store_true",
                        help="keep only the largest connected component of the system's mesh (by area), if it passes the two thresholds")
    parser.add_argument("--sparse_volume", action="store_true",
                        help="fuse the system's predictions into a brick-hashed volume that allocates what they touch, then make it dense; "
                             "files are written under <system>+sparse")
    parser.add_argument("--sparse_volume_bricks", default=65536, type=int,
                        help="with --sparse_volume: the pool's capacity in bricks of 8 x 8 x 8 voxels")
    parser.add_argument("--sparse_volume_extract", action="store_true",
                        help="with --sparse_volume: write the system's meshes and score them straight from the allocated bricks (marching cubes "
                             "over the pool); the volume is made dense only for --render_keyframes")
    parser.add_argument("--sparse_volume_render", action="store_true",
                        help="with --sparse_volume: --render_keyframes ray-casts the keyframes straight from the allocated bricks, without "
                             "making the volume dense")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    run(**vars(args))
