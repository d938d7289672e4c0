"""CPU: pins the float64 reference of the frame pre-processing (tests/preprocess_reference.py) before tests/test_preprocess_gpu.py
judges the kernels with it -- against the committed fixture rows (torch's interpolate: independent of this repository), against the
host functions on every shape of the GPU tests -- and checks what of the new surface runs without a device: argument validation of the
two C entry points, the binding's "rebuild" message, the uploader's ring logic."""
import ctypes
import os

import numpy as np
import pytest
import torch

import preprocess_reference as ref


@pytest.fixture(scope="module")
def library():
    from dvmvs.hip import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


def test_reference_matches_the_committed_fixture_rows(golden_dir):
    """tests/golden/preprocess_rows.npz: rows of the pre-processed sample frame produced with torch's interpolate; the bound is the one
    tests/test_runner.py holds the host function to on the same fixture."""
    from dvmvs.dataset_loader import load_image_u8
    z = np.load(os.path.join(golden_dir, "preprocess_rows.npz"))
    image = load_image_u8(os.path.join(golden_dir, "sample_scene", "images", "00012.png"))
    assert image.shape == (360, 540, 3) and image.dtype == np.uint8
    for tag, crop_x in (("crop", 45), ("nocrop", 0)):
        out = ref.preprocess_rgb(image, crop_x, 0, 256, 320, *ref.IMAGENET)
        assert out.shape == (3, 256, 320) and out.dtype == np.float64
        np.testing.assert_allclose(np.transpose(out, (1, 2, 0))[z["rows"]], z[f"{tag}_rows"], atol=2e-5)


@pytest.mark.parametrize("case", sorted(ref.CASES))
@pytest.mark.parametrize("kind", ["random", "spikes"])
def test_reference_matches_the_host_functions(case, kind):
    """PreprocessImage.apply_rgb (fp32) against the float64 reference within the derived rounding bound, both normalisations and none;
    apply_depth exactly."""
    H, W, new_h, new_w, crop_x, crop_y = ref.CASES[case]
    frame = (ref.random_frames if kind == "random" else ref.spike_frames)(1, H, W, seed=11)[0]
    pre = ref.preprocessor(H, W, new_h, new_w, crop_x, crop_y)
    for scale, mean, std, normalize in (ref.IMAGENET + (True,), ref.BASELINE + (True,), ref.BASELINE + (False,)):
        host = pre.apply_rgb(frame.astype(np.float32), scale, list(mean), list(std), normalize_colors=normalize)
        want = ref.preprocess_rgb(frame, crop_x, crop_y, new_h, new_w, scale, mean, std, normalize)
        bound = ref.tolerance(scale, mean, std, normalize)
        err = float(np.max(np.abs(np.transpose(host, (2, 0, 1)).astype(np.float64) - want)))
        print(f"{case} {kind} scale {scale} normalize {normalize}: host vs float64 reference {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    depth = ref.random_depths(1, H, W, seed=12)[0]
    assert np.array_equal(pre.apply_depth(depth.astype(np.float64) / 1000.0), ref.preprocess_depth(depth, crop_x, crop_y, new_h, new_w))


def test_identity_size_returns_the_pixels():
    frame = ref.random_frames(1, 240, 320, seed=3)[0]
    out = ref.preprocess_rgb(frame, 0, 0, 240, 320, normalize=False)
    assert np.array_equal(out, np.transpose(frame, (2, 0, 1)).astype(np.float64))


@pytest.mark.parametrize("case", sorted(ref.CASES))
def test_nearest_indices_equal_resize_nearest(case):
    from dvmvs.dataset_loader import resize_nearest
    H, W, new_h, new_w, crop_x, crop_y = ref.CASES[case]
    h, w = H - 2 * crop_y, W - 2 * crop_x
    assert resize_nearest(np.arange(w).reshape(1, w), new_w, 1)[0].tolist() == ref.nearest_indices(new_w, w).tolist()
    assert resize_nearest(np.arange(h).reshape(h, 1), 1, new_h)[:, 0].tolist() == ref.nearest_indices(new_h, h).tolist()


def test_tolerance_formula():
    assert abs(ref.tolerance(*ref.IMAGENET, True) - 6.3e-6) < 1e-7 and abs(ref.tolerance(*ref.BASELINE, True) - 9.2e-6) < 1e-7
    assert ref.tolerance(*ref.BASELINE, False) == 16 * 2.0 ** -24 * 255


def test_argument_validation_without_gpu(library):
    """Negative return codes come before anything is enqueued, so this is safe without a device (the pointers are never read)."""
    lib = library.lib()
    p = ctypes.c_void_p(4096)
    mean, std = library.float_array([0.485, 0.456, 0.406]), library.float_array([0.229, 0.224, 0.225])
    zero_std = library.float_array([0.229, 0.0, 0.225])

    def rgb(src=p, dst=p, N=1, H=360, W=540, row=3 * 540, cx=45, cy=0, nh=256, nw=320, bs=3 * 256 * 320, scale=255.0, mean=mean, std=std,
            normalize=1):
        return lib.dvmvs_preprocess_rgb_fwd(src, dst, N, H, W, row, cx, cy, nh, nw, bs, scale, mean, std, normalize, None)

    assert rgb(src=None) == -1 and rgb(dst=None) == -1
    assert rgb(N=0) == -1 and rgb(H=0) == -1 and rgb(W=-540) == -1 and rgb(nh=0) == -1 and rgb(nw=-1) == -1
    assert rgb(cx=270) == -1 and rgb(cy=180) == -1 and rgb(cx=-1) == -1           # a crop that leaves no pixels; a negative crop
    assert rgb(row=3 * 540 - 1) == -1 and rgb(bs=3 * 256 * 320 - 1) == -1         # strides smaller than a row / an output frame
    assert rgb(std=zero_std) == -1 and rgb(scale=0.0) == -1 and rgb(mean=None) == -1 and rgb(std=None) == -1 and rgb(normalize=2) == -1
    assert rgb(N=65536, bs=3 * 256 * 320) == -2
    assert rgb(H=40000, W=20000, row=60000, cx=0) == -2                            # 2.4e9 source bytes per frame
    assert rgb(row=1 << 62) == -2 and rgb(row=(1 << 63) - 1) == -2 and rgb(row=1 << 31) == -2    # no overflow in H * stride
    assert rgb(bs=1 << 62) == -2 and rgb(N=4, bs=(1 << 63) - 1) == -2 and rgb(bs=1 << 40) == -2
    assert rgb(nh=30000, nw=30000, bs=3 * 30000 * 30000) == -2                     # 2.7e9 output elements per frame

    def depth(src=p, dst=p, N=1, H=360, W=540, cx=45, cy=0, nh=256, nw=320, scaling=1000.0):
        return lib.dvmvs_preprocess_depth_fwd(src, dst, N, H, W, cx, cy, nh, nw, scaling, None)

    assert depth(src=None) == -1 and depth(dst=None) == -1 and depth(N=0) == -1 and depth(H=0) == -1 and depth(nw=0) == -1
    assert depth(cx=270) == -1 and depth(cy=-1) == -1 and depth(scaling=0.0) == -1
    assert depth(N=65536) == -2 and depth(H=50000, W=50000, cx=0) == -2 and depth(nh=50000, nw=50000) == -2


def test_binding_reports_a_library_without_the_new_symbols_as_stale(library, monkeypatch):
    """The ABI number did not change with the addition, so a library built before it passes the version check: the binding names the
    missing symbols and says "rebuild" instead of failing with an AttributeError at first use."""
    assert set(library.ADDED_WITHIN_ABI) == {"dvmvs_preprocess_rgb_fwd", "dvmvs_preprocess_depth_fwd"} and library.ABI_VERSION == 11
    monkeypatch.setattr(library, "_lib", None)
    monkeypatch.setattr(library, "ADDED_WITHIN_ABI", library.ADDED_WITHIN_ABI + ("dvmvs_symbol_of_a_later_build",))
    with pytest.raises(RuntimeError, match="dvmvs_symbol_of_a_later_build.*rebuild"):
        library.lib()


def test_ops_refuse_host_tensors_and_bad_arguments():
    from dvmvs.hip import ops
    frame = torch.zeros((4, 6, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.preprocess_rgb(frame, 0, 0, 2, 3, 255.0, [0.5] * 3, [0.5] * 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.preprocess_depth(torch.zeros((4, 6), dtype=torch.int16), 0, 0, 2, 3)


class _Event:
    log = []

    def __init__(self, slot):
        self.slot = slot

    def synchronize(self):
        _Event.log.append(self.slot)


def test_uploader_ring_on_host_memory():
    """Slots are taken round-robin; a slot's event is waited on exactly when the slot comes round again, not before; buffers are reused and
    grow; the returned tensor does not alias the staging buffer."""
    from dvmvs.dataset_loader import FrameUploader
    up = FrameUploader("cpu", slots=3)
    _Event.log = []
    order = []
    up._record = lambda: _Event(order[-1])
    frames = [ref.random_frames(1, 5, 7, seed=s)[0] for s in range(7)]
    outs = []
    for k, f in enumerate(frames):
        order.append(k % 3)
        outs.append(up.upload_rgb(f))
        assert _Event.log == [j % 3 for j in range(max(0, k - 2))]       # upload k waits for the event of upload k - 3 only
    for f, o in zip(frames, outs):
        assert o.dtype == torch.uint8 and tuple(o.shape) == f.shape and np.array_equal(o.numpy(), f)    # later uploads did not overwrite
    buffers = [b.data_ptr() for b in up._buffers]
    up.upload_rgb(frames[0])
    assert [b.data_ptr() for b in up._buffers] == buffers and all(b.numel() == 5 * 7 * 3 for b in up._buffers)
    big = ref.random_frames(2, 9, 11, seed=9)
    out = up.upload_rgb(big)
    assert tuple(out.shape) == big.shape and np.array_equal(out.numpy(), big) and max(b.numel() for b in up._buffers) == big.size
    depth = ref.random_depths(1, 6, 8, seed=1)[0]
    got = up.upload_depth(depth)
    assert got.dtype == torch.int16 and np.array_equal(got.numpy().view(np.uint16), depth)
    with pytest.raises(TypeError):
        up.upload_rgb(frames[0].astype(np.float32))
    with pytest.raises(ValueError):
        FrameUploader("cpu", slots=0)


def test_u8_loaders_return_the_decoded_files(golden_dir):
    from dvmvs.dataset_loader import load_depth_png, load_depth_png_u16, load_image, load_image_u8
    image = os.path.join(golden_dir, "sample_scene", "images", "00012.png")
    depth = os.path.join(golden_dir, "sample_scene", "depth", "00012.png")
    u8, u16 = load_image_u8(image), load_depth_png_u16(depth)
    assert u8.dtype == np.uint8 and np.array_equal(u8.astype(np.float32), load_image(image))
    assert u16.dtype == np.uint16 and np.array_equal(u16.astype(np.float64) / 1000.0, load_depth_png(depth))
