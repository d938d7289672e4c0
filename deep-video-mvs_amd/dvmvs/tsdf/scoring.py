"""3-D scoring of a fused volume against a ground-truth surface: the work of ``TSDFVolume.score_against`` and the one download that the
command-line program makes of a registered score."""
import numpy as np
import torch

from dvmvs.tsdf.mesh_views import visible_mesh
from dvmvs.tsdf.volume import TSDFVolume


def score_volume(volume, reference, threshold, return_sizes, sample_density, voxel, visible_from, align_distance, align_scale,
                 return_transform, clean=None, align_plane=False, align_normal_neighbours=20, align_normal_distance=np.inf, simplify=None,
                 smooth=None):
    """``TSDFVolume.score_against`` of ``volume``: ``(what it returns, the registration's record or None)``; the record is
    ``dvmvs.hip.registration.icp``'s (with ``align_plane``: ``icp_plane``'s) ``info`` (device tensors)."""
    from dvmvs.errors import _check_alignment, _check_plane, _score_device, prepare_points_device
    _check_alignment("score_against", align_distance, align_scale, None, return_transform)
    _check_plane("score_against", align_plane, align_distance, align_scale, None, False, align_normal_neighbours, align_normal_distance)
    gt_normals = None
    prepare = sample_density is not None or voxel is not None
    if visible_from is not None:
        if sample_density is None:
            raise ValueError("score_against: visible_from needs sample_density (the kept faces are sampled; the vertices are not culled)")
        if len(visible_from) not in (4, 5):
            raise ValueError("score_against: visible_from is (cam_intr, cam_poses, height, width[, min_views])")
    gt_faces = None
    if isinstance(reference, TSDFVolume):
        if prepare:
            gt, gt_faces = reference.mesh_tensors()
        elif align_plane:                            # the gradient normals of the reference's marching-cubes mesh come with its vertices
            gt, _, gt_normals = reference._extract(False, None)[:3]
            gt_normals = gt_normals.to(volume.device).contiguous()
        else:
            gt = reference.vertices()
        gt = gt.to(volume.device)
    else:
        if isinstance(reference, (tuple, list)) and len(reference) == 2 and all(len(getattr(part, "shape", ())) == 2 for part in reference):
            reference, gt_faces = reference          # a mesh: two arrays or tensors [V,3] and [F,3]
        gt = torch.as_tensor(reference, dtype=torch.float32, device=volume.device)
        if gt.dim() != 2 or gt.shape[1] != 3:
            raise ValueError(f"score_against: reference points must be [M,3], got {tuple(gt.shape)}")
    face_counts = None
    if visible_from is not None:
        if gt_faces is None:
            raise ValueError("score_against: visible_from restricts a mesh reference; a bare point set has no faces to cull")
        cam_intr, cam_poses, height, width = visible_from[:4]
        all_faces = int(gt_faces.shape[0])
        gt, gt_faces = visible_mesh(gt.contiguous(), torch.as_tensor(gt_faces, device=volume.device).to(torch.int32), cam_intr, cam_poses,
                                    height, width, min_views=visible_from[4] if len(visible_from) == 5 else 1)
        face_counts = (int(gt_faces.shape[0]), all_faces)
    if prepare:
        if gt_faces is not None:
            gt_faces = torch.as_tensor(gt_faces, device=volume.device).to(torch.int32)
        pred = volume.surface_points(sample_density, voxel, clean=clean, simplify=simplify, smooth=smooth)
        gt = prepare_points_device(gt.contiguous(), gt_faces, sample_density, voxel)
    else:
        pred = volume.vertices(clean=clean, simplify=simplify, smooth=smooth)
    if pred.shape[0] == 0 or gt.shape[0] == 0:
        raise ValueError(f"score_against: a surface without a vertex cannot be scored ({pred.shape[0]} predicted, {gt.shape[0]} reference)")
    row, transform, info = _score_device(pred, gt.contiguous(), threshold, None, None, None, None, None, align_distance, align_scale, None,
                                         align_plane, gt_normals, align_normal_neighbours, align_normal_distance)
    result = (row,)
    if return_sizes:
        result += ((int(pred.shape[0]), int(gt.shape[0])),) + (() if face_counts is None else (face_counts,))
    if return_transform:
        result += (transform,)
    return (result[0] if len(result) == 1 else result), info


# The row that ``_aligned_score`` downloads: its parts and their lengths in float64 entries, in the order they are packed in.
# ``rmse_point`` is there with ``align_plane`` only.
_DOWNLOAD = {"row": 6, "transform": 16, "iterations": 1, "status": 1, "fitness": 1, "rmse": 1, "rmse_point": 1}


def _download(parts):
    """``parts`` (name -> device tensor of ``_DOWNLOAD[name]`` entries) as name -> float64 host array: ONE concatenation, ONE download."""
    names = [name for name in _DOWNLOAD if name in parts]
    down = torch.cat([parts[name].reshape(-1) for name in names]).cpu().numpy()
    return dict(zip(names, np.split(down, np.cumsum([_DOWNLOAD[name] for name in names])[:-1])))


def _aligned_score(volume, align_distance, align_scale, align_plane=None, **score):
    """``score_against`` with its row on the host; with ``align_distance`` also the entries ``_errors3d.npz`` gains.  Row, transform and
    record come down as ONE float64 tensor (a float32 row is exact in float64).  ``align_plane``: None, or ``score_against``'s
    point-to-plane keywords; the entries then include the point RMSE and the status name."""
    if align_distance is None:
        result = volume.score_against(**score)
        return (result[0].cpu().numpy(),) + tuple(result[1:]) + ({},)
    score = {"return_sizes": False, "sample_density": None, "voxel": None, "visible_from": None, **score}
    plane = align_plane is not None
    result, info = score_volume(volume, align_distance=align_distance, align_scale=False if plane else align_scale,
                                return_transform=True, **(align_plane or {}), **score)
    last = (info["iterations"] - 1).clamp(min=0).reshape(1)      # (selected on the device: indexing with a 0-d tensor would read it)
    parts = {"row": result[0].double(), "transform": result[-1], "iterations": info["iterations"].double(), "status": info["status"].double()}
    parts.update({key: info[key].index_select(0, last) for key in (("fitness", "rmse", "rmse_point") if plane else ("fitness", "rmse"))})
    down = _download(parts)
    iterations, status, fitness, rmse = (down[key][0] for key in ("iterations", "status", "fitness", "rmse"))
    extra = {"transform": down["transform"].reshape(4, 4), "align_iterations": np.int64(iterations), "align_status": np.int64(status),
             "align_fitness": np.float64(fitness), "align_rmse": np.float64(rmse)}
    from dvmvs.errors import REGISTRATION_PLANE_STATUS, REGISTRATION_STATUS
    name = (REGISTRATION_PLANE_STATUS if plane else REGISTRATION_STATUS)[int(status)]
    if plane:                                                    # with the point RMSE and the status name
        rmse_point = down["rmse_point"][0]
        extra.update(align_rmse_point=np.float64(rmse_point), align_status_name=np.array(name))
        print("Registered the surface to the ground truth within {} m, point to plane: {} after {} iterations, fitness {:.4f}, plane rmse {:.5f} "
              "m, point rmse {:.5f} m".format(align_distance, name, int(iterations), fitness, rmse, rmse_point))
    else:
        print("Registered the surface to the ground truth within {} m{}: {} after {} iterations, fitness {:.4f}, rmse {:.5f} m".format(
            align_distance, " with scale" if align_scale else "", name, int(iterations), fitness, rmse))
    return (down["row"].astype(np.float32),) + tuple(result[1:-1]) + (extra,)
