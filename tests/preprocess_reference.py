"""float64 restatement of the two frame pre-processing operations, for the tests of the device path (tests/test_preprocess_gpu.py),
pinned itself by tests/test_preprocess_reference.py before it judges a kernel.

Written from the definition, not from dvmvs/dataset_loader.py: the sampling positions are exact rationals in integer arithmetic
(output pixel i of n_out samples the input of n_in pixels at ((2 i + 1) n_in - n_out) / (2 n_out), clamped at 0; nearest takes
floor(i n_in / n_out)), the blend is the four-tap sum with weights in float64, and nothing is rounded to float32 anywhere.
"""
import numpy as np

IMAGENET = (255.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))      # dvmvs.runner
BASELINE = (1.0, (81.0, 81.0, 81.0), (35.0, 35.0, 35.0))              # dvmvs.baselines.runner

# (H, W, new_h, new_w, crop_x, crop_y)
CASES = {
    "sample_crop": (360, 540, 256, 320, 45, 0),
    "sample_nocrop": (360, 540, 256, 320, 0, 0),
    "vga": (480, 640, 256, 320, 0, 0),
    "identity": (240, 320, 240, 320, 0, 0),
    "magnify": (120, 160, 256, 320, 0, 0),
    "ragged_odd": (97, 131, 33, 47, 0, 0),
    "ragged_even": (97, 131, 35, 50, 0, 0),
}

EPS = 2.0 ** -24


def tolerance(scale, mean, std, normalize):
    """Elementwise bound on |fp32 path - float64 reference|: at most ~8 roundings in the blends on magnitudes <= 255 and three more in
    the normalisation, doubled: 16 eps (255 / scale + max|mean|) / min(std), or 16 eps 255 without normalisation."""
    if not normalize:
        return 16.0 * EPS * 255.0
    return 16.0 * EPS * (255.0 / scale + max(abs(m) for m in mean)) / min(abs(s) for s in std)


def bilinear_taps(n_out, n_in):
    """(i0, i1, weight of i1 as float64) of every output sample: half-pixel centres, positions left of pixel 0 clamp to it, the
    second tap clamps to the last pixel."""
    i = np.arange(n_out, dtype=np.int64)
    den = 2 * n_out
    num = np.maximum((2 * i + 1) * n_in - n_out, 0)          # position * den, exact
    i0 = np.minimum(num // den, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (num - i0 * den).astype(np.float64) / den


def nearest_indices(n_out, n_in):
    """floor(i * n_in / n_out) in exact integer arithmetic, clamped to the last pixel."""
    i = np.arange(n_out, dtype=np.int64)
    return np.minimum((i * n_in) // n_out, n_in - 1)


def _crop(frames, crop_x, crop_y):
    H, W = frames.shape[1:3]
    return frames[:, crop_y:H - crop_y, crop_x:W - crop_x]


def preprocess_rgb(raw, crop_x, crop_y, new_h, new_w, scale=1.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), normalize=True):
    """uint8 [N,H,W,3] (or [H,W,3]) -> float64 [N,3,new_h,new_w] (or [3,new_h,new_w])."""
    raw = np.asarray(raw)
    single = raw.ndim == 3
    src = _crop(raw[None] if single else raw, crop_x, crop_y).astype(np.float64)
    y0, y1, wy = bilinear_taps(new_h, src.shape[1])
    x0, x1, wx = bilinear_taps(new_w, src.shape[2])
    wy, wx = wy[None, :, None, None], wx[None, None, :, None]
    out = ((1.0 - wy) * (1.0 - wx) * src[:, y0][:, :, x0] + (1.0 - wy) * wx * src[:, y0][:, :, x1]
           + wy * (1.0 - wx) * src[:, y1][:, :, x0] + wy * wx * src[:, y1][:, :, x1])
    if normalize:
        out = (out / float(scale) - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    out = np.ascontiguousarray(np.transpose(out, (0, 3, 1, 2)))
    return out[0] if single else out


def preprocess_depth(raw, crop_x, crop_y, new_h, new_w, scaling=1000.0):
    """uint16 [N,H,W] (or [H,W]) -> float64 metres [N,new_h,new_w] (or [new_h,new_w])."""
    raw = np.asarray(raw)
    single = raw.ndim == 2
    src = _crop(raw[None] if single else raw, crop_x, crop_y)
    ys, xs = nearest_indices(new_h, src.shape[1]), nearest_indices(new_w, src.shape[2])
    out = src[:, ys][:, :, xs].astype(np.float64) / float(scaling)
    return out[0] if single else out


# ----------------------------------------------------------------------------------------------------------------------
# inputs shared by the CPU and the GPU tests
# ----------------------------------------------------------------------------------------------------------------------
def random_frames(N, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)


def spike_frames(N, H, W, seed):
    """Isolated 255 pixels on 0 (and the inverse in odd frames): the largest gradients an 8-bit image has."""
    rng = np.random.RandomState(seed)
    frames = np.where(rng.rand(N, H, W, 3) < 0.08, 255, 0).astype(np.uint8)
    frames[1::2] = 255 - frames[1::2]
    return frames


def random_depths(N, H, W, seed):
    depth = np.random.RandomState(seed).randint(0, 65536, size=(N, H, W)).astype(np.uint16)
    depth[:, 0, 0], depth[:, -1, -1] = 0, 65535
    depth[:, H // 2 - 4:H // 2 + 4, W // 2 - 4:W // 2 + 4] = 65535      # blocks wider than any sampling step of CASES: always sampled
    depth[:, H // 4 - 4:H // 4 + 4, W // 2 - 4:W // 2 + 4] = 0
    return depth


def preprocessor(H, W, new_h, new_w, crop_x, crop_y):
    """A dvmvs PreprocessImage with the given crop and target size (its constructor derives the crop from the aspect ratios; the tests
    set the listed crops directly)."""
    from dvmvs.dataset_loader import PreprocessImage
    pre = PreprocessImage(np.eye(3), W, H, new_w, new_h, distortion_crop=0, perform_crop=False)
    pre.crop_x, pre.crop_y = crop_x, crop_y
    return pre
