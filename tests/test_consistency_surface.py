"""CPU: the public surface of the depth-map consistency filter -- argument checks of the ops and of both C entry points (no device
needed: every error is returned before anything is enqueued), the program's new flags, and ``LiveFusion``'s new arguments."""
import numpy as np
import pytest
import torch


def _inputs(n=3, s=2, h=6, w=8):
    return (torch.ones(n, h, w), torch.eye(3).repeat(n, 1, 1), torch.eye(4).repeat(n, 1, 1), torch.zeros(n, s, dtype=torch.int32))


def test_ops_refuse_cpu_tensors():
    from dvmvs.hip import ops
    depths, K, poses, sources = _inputs()
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.consistency_matrices(K, poses, sources)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.depth_consistency(depths, K, poses, sources)
    assert "consistency_matrices" in ops.__all__ and "depth_consistency" in ops.__all__


def test_ops_refuse_wrong_shapes_and_dtypes():
    from dvmvs.hip import ops
    depths, K, poses, sources = _inputs()
    bad_cameras = [(K[:, :2], poses, sources), (K.double(), poses, sources), (K, poses[:2], sources), (K, poses.double(), sources),
                   (K, poses, sources.long()), (K, poses, sources[:2]), (K, poses, torch.zeros(3, 17, dtype=torch.int32)),
                   (K, poses, sources[:, 0])]
    for args in bad_cameras:
        with pytest.raises(ValueError):
            ops.consistency_matrices(*args)
        with pytest.raises(ValueError):
            ops.depth_consistency(depths, *args)
    with pytest.raises(TypeError):
        ops.consistency_matrices(K.numpy(), poses, sources)
    for bad in (depths[:2], depths.double(), depths[0], depths[:, :0]):
        with pytest.raises(ValueError):
            ops.depth_consistency(bad, K, poses, sources)
    with pytest.raises(TypeError):
        ops.depth_consistency(depths.numpy(), K, poses, sources)
    for kwargs in ({"min_views": -1}, {"pixel_threshold": float("nan")}, {"relative_threshold": float("nan")}):
        with pytest.raises(ValueError):
            ops.depth_consistency(depths, K, poses, sources, **kwargs)


def test_entry_points_validate_without_gpu():
    """Negative return codes are produced before anything is enqueued, so this is safe without a device."""
    import ctypes
    from dvmvs.hip import _capi
    lib = _capi.lib()
    null = None
    buf = (ctypes.c_float * 64)()          # host memory that is never read: only its address is looked at
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)
    nan = float("nan")
    assert lib.dvmvs_consistency_matrices(null, null, null, null, 1, 1, null) == -1
    assert lib.dvmvs_consistency_matrices(p, p, null, p, 2, 1, null) == -1          # S > 0 needs sources
    assert lib.dvmvs_consistency_matrices(p, p, p, p, 0, 1, null) == -1
    assert lib.dvmvs_consistency_matrices(p, p, p, p, 2, -1, null) == -1
    assert lib.dvmvs_consistency_matrices(p, p, p, p, 2, 17, null) == -1
    assert lib.dvmvs_consistency_matrices(p, p, p, p, 65536, 1, null) == -2

    def pixels(depth=p, K=p, pose=p, sources=p, matrices=p, out=p, count=null, points=null, N=2, S=1, H=4, W=4, pix=1.0, rel=0.01,
               min_views=2, average=1):
        return lib.dvmvs_depth_consistency_fwd(depth, K, pose, sources, matrices, out, count, points, N, S, H, W, pix, rel, min_views, average, null)

    assert pixels(depth=null) == -1 and pixels(K=null) == -1 and pixels(pose=null) == -1 and pixels(out=null) == -1
    assert pixels(sources=null) == -1 and pixels(matrices=null) == -1
    assert pixels(N=0) == -1 and pixels(S=-1) == -1 and pixels(S=17) == -1 and pixels(H=0) == -1 and pixels(W=0) == -1
    assert pixels(pix=nan) == -1 and pixels(rel=nan) == -1 and pixels(min_views=-1) == -1 and pixels(average=2) == -1
    assert pixels(out=odd) == -1 and pixels(depth=odd) == -1
    assert pixels(N=65536) == -2 and pixels(H=65536, W=65536) == -2 and pixels(H=30000, W=30000) == -2
    assert _capi.ADDED_WITHIN_ABI_CONSISTENCY == ("dvmvs_consistency_matrices", "dvmvs_depth_consistency_fwd") and _capi.ABI_VERSION == 11


def test_program_flags():
    from dvmvs.tsdf import build_parser, run
    args = build_parser().parse_args([])
    assert args.filter_consistency is False and args.save_point_cloud is False
    assert (args.consistency_views, args.consistency_sources, args.consistency_pixel, args.consistency_relative) == (2, 4, 1.0, 0.01)
    args = build_parser().parse_args(["--filter_consistency", "--consistency_views", "3", "--consistency_sources", "6", "--consistency_pixel",
                                      "0.5", "--consistency_relative", "0.02", "--save_point_cloud"])
    assert args.filter_consistency and args.save_point_cloud
    assert (args.consistency_views, args.consistency_sources, args.consistency_pixel, args.consistency_relative) == (3, 6, 0.5, 0.02)
    import inspect
    defaults = {k: v.default for k, v in inspect.signature(run).parameters.items()}
    for name in ("filter_consistency", "consistency_views", "consistency_sources", "consistency_pixel", "consistency_relative", "save_point_cloud"):
        assert defaults[name] == getattr(build_parser().parse_args([]), name)


def test_point_cloud_needs_the_filter(tmp_path):
    from dvmvs.tsdf import main, run
    with pytest.raises(ValueError, match="filter_consistency"):
        run(str(tmp_path), str(tmp_path), str(tmp_path), "d", "s", "320_256_3_x", 0.05, 5.0, False, False, False, save_point_cloud=True)
    with pytest.raises(ValueError, match="filter_consistency"):
        main(["--reconstruction_folder", str(tmp_path), "--save_point_cloud"])
    assert not list(tmp_path.iterdir())


def test_live_fusion_checks_its_new_arguments():
    from dvmvs.tsdf import LiveFusion
    bounds = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 1.0]])
    with pytest.raises(ValueError, match="min_consistent_views"):
        LiveFusion(bounds, min_consistent_views=-1)
    with pytest.raises(ValueError, match="consistency_sources"):
        LiveFusion(bounds, min_consistent_views=1, consistency_sources=17)
    with pytest.raises(ValueError, match="NaN"):
        LiveFusion(bounds, min_consistent_views=1, pixel_threshold=float("nan"))
    import inspect
    defaults = {k: v.default for k, v in inspect.signature(LiveFusion.__init__).parameters.items()}
    assert (defaults["min_consistent_views"], defaults["consistency_sources"], defaults["pixel_threshold"], defaults["relative_threshold"]) == (0, 4, 1.0, 0.01)


def test_filter_depths_and_point_cloud_argument_checks():
    from dvmvs.consistency import filter_depths, fused_point_cloud
    with pytest.raises(ValueError):
        fused_point_cloud(torch.ones(2, 3, 4), torch.ones(2, 3, 4, 2))
    with pytest.raises(ValueError):
        fused_point_cloud(torch.ones(2, 3, 4), torch.ones(2, 3, 4, 3), np.zeros((2, 3, 4), np.uint8))
    cloud = fused_point_cloud(torch.tensor([[[0.0, 1.0], [2.0, 0.0]]]), torch.arange(12.0).reshape(1, 2, 2, 3),
                              np.arange(12, dtype=np.uint8).reshape(1, 2, 2, 3))
    assert cloud.tolist() == [[3, 4, 5, 3, 4, 5], [6, 7, 8, 6, 7, 8]]        # row-major, xyz then rgb
    with pytest.raises(RuntimeError, match="MI355X"):                         # host data goes where ``device`` says: no CPU route
        filter_depths(np.ones((2, 4, 4), np.float32), np.eye(3), np.stack([np.eye(4)] * 2), device="cpu")
