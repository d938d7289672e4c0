"""Views of a triangle mesh on the device: its depth maps (``render_mesh``) and the part of it that a set of cameras saw
(``visible_mesh``); and ``camera_tensors``, the one place where intrinsics and poses become checked device tensors."""
import numpy as np
import torch


def camera_tensors(cam_intr, cam_poses, device, frames=None):
    """Contiguous float32 DEVICE tensors ``(K [N,3,3], poses [N,4,4])`` of cameras given as numpy arrays or tensors; one intrinsic matrix
    [3,3] serves all N poses.  Without ``frames`` a single pose [4,4] is one view and N is the number of poses (``render_mesh``,
    ``visible_mesh``, ``TSDFVolume.render``); with ``frames``, the number of depth maps of ``TSDFVolume.integrate_frames``, the poses
    must be [frames,4,4].  A tensor that is already there in that type is used in place."""
    def as_dev(a):
        return a.to(device, torch.float32) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float32), device=device)

    if frames is not None:
        K, P = as_dev(cam_intr), as_dev(cam_poses)
        if K.dim() == 2:
            K = K.unsqueeze(0).expand(frames, 3, 3)
        if tuple(K.shape) != (frames, 3, 3) or tuple(P.shape) != (frames, 4, 4):
            raise ValueError(f"expected intrinsics [3,3] or [{frames},3,3] and poses [{frames},4,4], got {tuple(K.shape)} and {tuple(P.shape)}")
        return K.contiguous(), P.contiguous()

    def batch(a, tail):
        t = as_dev(a)
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or tuple(t.shape[1:]) != tail:
            raise ValueError(f"expected [{tail[0]},{tail[1]}] or [N,{tail[0]},{tail[1]}], got {tuple(t.shape)}")
        return t

    P, K = batch(cam_poses, (4, 4)), batch(cam_intr, (3, 3))
    if K.shape[0] == 1 and P.shape[0] > 1:
        K = K.expand(P.shape[0], 3, 3)
    if K.shape[0] != P.shape[0]:
        raise ValueError(f"{K.shape[0]} intrinsics for {P.shape[0]} poses")
    return K.contiguous(), P.contiguous()


def _mesh_and_cameras(verts, faces, cam_intr, cam_poses, device=None):
    """Device tensors (verts float32 [V,3], faces int32 [F,3], K float32 [N,3,3], poses float32 [N,4,4]) of a mesh and its views, given as
    arrays or tensors, the cameras as one matrix or a batch.  ``device``: where arrays go (default: where the vertices are, else "cuda")."""
    if device is None:
        device = verts.device if torch.is_tensor(verts) and verts.device.type == "cuda" else torch.device("cuda")

    def as_dev(a, dtype):
        if torch.is_tensor(a):
            return a.to(device, dtype)
        return torch.as_tensor(np.asarray(a, dtype={torch.float32: np.float32, torch.int32: np.int32}[dtype]), device=device)

    verts, faces = as_dev(verts, torch.float32), as_dev(faces, torch.int32)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"expected vertices [V,3] and faces [F,3], got {tuple(verts.shape)} and {tuple(faces.shape)}")
    return (verts.contiguous(), faces.contiguous()) + camera_tensors(cam_intr, cam_poses, device)


def render_mesh(verts, faces, cam_intr, cam_poses, height, width, near=0.05, far=float("inf"), cull_backfaces=False):
    """Rasterises a triangle mesh from N views in one call (``dvmvs.hip.ops.mesh_raster``, csrc/mesh_raster.hip; definition in
    include/dvmvs_hip.h): ``verts`` [V,3] world space and ``faces`` [F,3], ``cam_poses`` camera-to-world [N,4,4] or one [4,4], ``cam_intr``
    [N,3,3] or one [3,3] for all views; numpy arrays or tensors, as ``TSDFVolume.render`` takes them.  Returns DEVICE tensors ``(depth
    [N,height,width] float32, face [N,height,width] int32)``: the camera depth of the nearest face at every pixel (0 where there is none)
    and its index (-1), at the pixel positions of ``TSDFVolume.render``, so that the depth maps can go to ``compute_errors_device``.
    Reads ONE number per view from the device (a synchronisation): the triangles left out because they project beyond 2^21 pixels, and
    warns when there are any."""
    import warnings
    from dvmvs.hip import ops
    verts, faces, K, P = _mesh_and_cameras(verts, faces, cam_intr, cam_poses)
    depth, face, overflow = ops.mesh_raster(verts, faces, K, P, height, width, near=near, far=far, cull_backfaces=cull_backfaces,
                                            return_overflow=True)
    left_out = int(overflow.sum())                                  # the one host read
    if left_out:
        warnings.warn(f"render_mesh: {left_out} clipped triangles project beyond 2^21 pixels and were left out", RuntimeWarning, stacklevel=2)
    return depth, face


VISIBLE_MESH_CHUNK = 32       # views rasterised per call of visible_mesh: bounds the z-buffer keys (8 bytes per pixel and view)


def visible_mesh(verts, faces, cam_intr, cam_poses, height, width, min_views=1, near=0.05, relative=0.01, absolute=0.0):
    """The part of a mesh that N views observed: the mesh is rasterised from the views (``render_mesh``'s op), every vertex is tested
    against those depth maps (``dvmvs.hip.ops.mesh_visibility``: in front of ``near``, inside the image, not deeper than the rendered
    surface by more than ``relative`` of it plus ``absolute`` metres), and the faces whose three vertices are each seen by at least
    ``min_views`` views are kept.  Arguments as ``render_mesh``.  Returns DEVICE tensors ``(verts, kept_faces)``: the vertices are
    unchanged, so the face indices stay valid.  The views go through in chunks of ``VISIBLE_MESH_CHUNK``, so the memory does not grow
    with the length of the sequence.  No host read but the size of the result (the boolean selection of the kept faces)."""
    from dvmvs.hip import ops
    verts, faces, K, P = _mesh_and_cameras(verts, faces, cam_intr, cam_poses)
    min_views = int(min_views)
    if min_views < 1:
        raise ValueError(f"visible_mesh: min_views must be at least 1, got {min_views}")
    count = torch.zeros(verts.shape[0], dtype=torch.int32, device=verts.device)
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        return verts, faces[:0]
    for first in range(0, P.shape[0], VISIBLE_MESH_CHUNK):
        k, p = K[first:first + VISIBLE_MESH_CHUNK], P[first:first + VISIBLE_MESH_CHUNK]
        depth, _ = ops.mesh_raster(verts, faces, k, p, height, width, near=near)
        count += ops.mesh_visibility(verts, depth, k, p, near=near, relative=relative, absolute=absolute)
    V = verts.shape[0]
    index = faces.long()
    valid = ((index >= 0) & (index < V)).all(dim=1)
    seen = (count[index.clamp(0, V - 1)] >= min_views).all(dim=1) & valid
    return verts, faces[seen]
