"""Connected components of a triangle mesh and their removal by size: the step between extracting a surface and everything done with it.
A TSDF fused from predicted depth has floaters, small shells of surface where a few frames agreed on a wrong depth; they are components of
the welded mesh that ``marching_cubes`` extracts, too small to be surface.

This module is the host definition, in numpy, importable without a GPU.  ``mesh_components_device`` and ``filter_components_device`` are the
same on the GPU (``dvmvs.hip.components``, csrc/mesh_components.hip) and give the same bits.  Everything that decides a result is an
integer: areas are ``dvmvs.errors.quantised_face_areas`` (units of 2^-32 m^2) and their sums are exact, so no order of evaluation can show.
"""
import math
from typing import NamedTuple

import numpy as np

from dvmvs.errors import quantised_face_areas

AREA_SCALE = 4294967296.0            # units per square metre
AREA_LIMIT = 1 << 63
MAX_ELEMENTS = 1 << 28               # vertices and faces the kernels take


class ComponentFilter(NamedTuple):
    """Which components ``filter_components`` keeps: those with at least ``min_area`` square metres (compared as
    ``area[r] >= ceil(min_area * 2^32)``, the right side computed once in float64) and at least ``min_faces`` faces; with ``keep_largest``
    only the one with the greatest area (ties: the greater face count, then the smaller label), and it only if it passes the thresholds."""
    min_area: float = 0.0
    min_faces: int = 0
    keep_largest: bool = False


def filter_settings(filter):
    """``(min_area_units, min_faces, keep_largest)`` of a ``ComponentFilter`` as the integers and the bool that are compared; ``ValueError``
    for a negative, NaN or non-integer setting and for an area of 2^31 square metres or more."""
    if not isinstance(filter, ComponentFilter):
        raise ValueError(f"expected a ComponentFilter, got {type(filter).__name__}")
    min_area, min_faces, keep_largest = filter
    if isinstance(min_area, bool) or not isinstance(min_area, (int, float, np.integer, np.floating)):
        raise ValueError(f"ComponentFilter: min_area must be a number of square metres, got {min_area!r}")
    min_area = float(min_area)
    if not min_area >= 0.0:
        raise ValueError(f"ComponentFilter: min_area must not be negative or NaN, got {min_area}")
    scaled = min_area * AREA_SCALE
    if not scaled < 2.0 ** 63:
        raise ValueError(f"ComponentFilter: min_area must be below 2^31 square metres, got {min_area}")
    if isinstance(min_faces, bool) or not isinstance(min_faces, (int, np.integer)):
        if not isinstance(min_faces, (float, np.floating)) or not float(min_faces).is_integer():
            raise ValueError(f"ComponentFilter: min_faces must be an integer, got {min_faces!r}")
    min_faces = int(min_faces)
    if min_faces < 0 or min_faces >= AREA_LIMIT:
        raise ValueError(f"ComponentFilter: min_faces must not be negative, got {min_faces}")
    if not isinstance(keep_largest, (bool, np.bool_)):
        raise ValueError(f"ComponentFilter: keep_largest must be a bool, got {keep_largest!r}")
    return int(math.ceil(scaled)), min_faces, bool(keep_largest)


def _faces(faces):
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be int32 [F,3], got {faces.shape}")
    return faces


def mesh_components(faces, n_verts, verts=None):
    """The connected components of the mesh ``faces`` int32 [F,3] over ``n_verts`` vertices, as a dict:
      ``labels`` int32 [V]: the smallest vertex index reachable from v over the edges of VALID faces, those whose three indices lie in
        [0, V); an invalid face joins nothing, and a vertex that no valid face uses is its own label;
      ``face_labels`` int32 [F]: ``labels[faces[f,0]]``, -1 for an invalid face;
      ``face_count`` int32 [V]: at r, the number of valid faces of the component whose label is r; 0 everywhere else;
      ``area`` int64 [V], only with ``verts`` (float32 [V,3]): at r, the sum of ``quantised_face_areas`` over those faces, exact;
      ``n_components``: the number of r with ``face_count[r] > 0``.
    Raises ``ValueError`` for a face whose area is not finite and for a mesh whose total area reaches 2^63 units, as ``sample_surface``."""
    faces = _faces(faces)
    V, F = int(n_verts), len(faces)
    if V < 0 or V > MAX_ELEMENTS or F > MAX_ELEMENTS:
        raise ValueError(f"mesh_components: {V} vertices and {F} faces are outside what is taken (2^28 at most)")
    valid = np.all((faces >= 0) & (faces < V), axis=1)
    good = faces[valid].astype(np.int64)
    edges = np.concatenate([good[:, [0, 1]], good[:, [1, 2]]])
    labels = np.arange(V, dtype=np.int64)
    while len(edges):
        # hook: the label of either end's label becomes the smaller of the two; then every chain is followed to its end
        la, lb = labels[edges[:, 0]], labels[edges[:, 1]]
        low = np.minimum(la, lb)
        hooked = labels.copy()
        np.minimum.at(hooked, la, low)
        np.minimum.at(hooked, lb, low)
        while True:
            jumped = hooked[hooked]
            if np.array_equal(jumped, hooked):
                break
            hooked = jumped
        if np.array_equal(hooked, labels):
            break
        labels = hooked
    face_labels = np.full(F, -1, dtype=np.int64)
    face_labels[valid] = labels[good[:, 0]]
    face_count = np.bincount(face_labels[valid], minlength=V).astype(np.int32) if V else np.zeros(0, np.int32)
    out = {"labels": labels.astype(np.int32), "face_labels": face_labels.astype(np.int32), "face_count": face_count,
           "n_components": int(np.count_nonzero(face_count))}
    if verts is not None:
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        if len(verts) != V:
            raise ValueError(f"mesh_components: {len(verts)} vertices for n_verts = {V}")
        try:
            areas, _ = quantised_face_areas(verts, faces)
        except ValueError:
            raise ValueError("mesh_components: a face's area is not finite or the mesh is larger than 2^31 square metres") from None
        total = (int((areas >> 32).sum()) << 32) + int((areas & 0xffffffff).sum())
        if total >= AREA_LIMIT:
            raise ValueError("mesh_components: the mesh is larger than 2^31 square metres")
        area = np.zeros(V, dtype=np.int64)
        np.add.at(area, face_labels[valid], areas[valid])
        out["area"] = area
    return out


def kept_components(face_count, area, filter):
    """bool [V]: True at the labels of the components that ``filter`` keeps."""
    min_area, min_faces, keep_largest = filter_settings(filter)
    candidates = face_count > 0
    passes = candidates & (face_count.astype(np.int64) >= min_faces) & (area >= min_area)
    if not keep_largest or not candidates.any():
        return passes
    roots = np.flatnonzero(candidates)
    # the greatest area, then the greater face count, then the smaller label
    best = roots[np.lexsort((roots, -face_count[roots].astype(np.int64), -area[roots]))[0]]
    keep = np.zeros_like(passes)
    keep[best] = passes[best]
    return keep


def filter_components(verts, faces, filter, normals=None, colors=None, return_index=False):
    """The mesh without the components that ``filter`` (a ``ComponentFilter``) does not keep: ``(verts', faces', normals' or None, colors' or
    None)``; with ``return_index`` also ``(vertex_index int32 [V'], face_index int32 [F'])``, the old indices.  Kept faces are the valid
    faces of kept components in their original order, kept vertices those that a kept face uses, in their original order; the faces are
    re-indexed; ``normals`` (float32 [V,3]) and ``colors`` (uint8 [V,3]) are gathered alongside.  Nothing kept gives V' = F' = 0."""
    filter_settings(filter)
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    if verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must be float32 [V,3], got {verts.shape}")
    faces = _faces(faces)
    V = len(verts)
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if normals.shape != verts.shape:
            raise ValueError(f"normals must be float32 [{V},3], got {normals.shape}")
    if colors is not None:
        colors = np.ascontiguousarray(colors, dtype=np.uint8)
        if colors.shape != verts.shape:
            raise ValueError(f"colors must be uint8 [{V},3], got {colors.shape}")
    parts = mesh_components(faces, V, verts)
    keep = kept_components(parts["face_count"], parts["area"], filter)
    face_labels = parts["face_labels"]
    face_kept = (face_labels >= 0) & keep[np.maximum(face_labels, 0)] if V else np.zeros(len(faces), bool)
    vertex_kept = keep[parts["labels"]]          # a component with a face has no vertex outside its faces
    face_index = np.flatnonzero(face_kept).astype(np.int32)
    vertex_index = np.flatnonzero(vertex_kept).astype(np.int32)
    new_index = np.full(V, -1, dtype=np.int32)
    new_index[vertex_index] = np.arange(len(vertex_index), dtype=np.int32)
    new_faces = new_index[faces[face_index]].reshape(-1, 3) if len(face_index) else np.zeros((0, 3), np.int32)
    result = (verts[vertex_index], new_faces, None if normals is None else normals[vertex_index], None if colors is None else colors[vertex_index])
    return result + ((vertex_index, face_index),) if return_index else result


def mesh_components_device(faces, n_verts, verts=None):
    """``mesh_components`` for device tensors (``dvmvs.hip.components.mesh_components``): the same bits, on the GPU, as a dict of DEVICE
    tensors; nothing is read by the host, so an error is the dict's ``status`` and not an exception."""
    from dvmvs.hip import components
    return components.mesh_components(faces, n_verts, verts)


def filter_components_device(verts, faces, filter, normals=None, colors=None, return_index=False):
    """``filter_components`` for device tensors (``dvmvs.hip.components.filter_components``): the same bits, on the GPU."""
    from dvmvs.hip import components
    return components.filter_components(verts, faces, filter, normals, colors, return_index)
