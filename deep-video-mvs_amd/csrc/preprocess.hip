// Frame pre-processing on the device (gfx950): the camera's 8-bit frames and 16-bit depth maps as they come, in one launch each.
//   dvmvs_preprocess_rgb_fwd   : uint8 [N,H,W,3] (row stride in bytes) -> float32 [N,3,new_h,new_w]: centre crop, bilinear resampling
//                                with half-pixel centres and clamped edges, optional (v / scale - mean[c]) / std[c], HWC -> CHW
//   dvmvs_preprocess_depth_fwd : uint16 [N,H,W] (millimetres) -> float32 [N,new_h,new_w] (metres): crop, nearest resampling, / scaling
// They restate dvmvs/dataset_loader.py (PreprocessImage.apply_rgb / apply_depth on resize_bilinear / resize_nearest) operation by
// operation, so that the device path is the host path and not a cousin of it:
//   - source coordinates, tap indices and blend weights are evaluated in DOUBLE by the host's expressions (IEEE double gives the same
//     bits on both sides); fp32 coordinates would cost ~1e-4 in the normalised image at 540 columns;
//   - blends and normalisation are fp32 in the host's order with true divisions, and NOTHING in this file is contracted into an FMA:
//     numpy rounds every product, and (x + 0.5) * s - 0.5 as one fma would move the weights themselves.
// At 0.6 MB read and 1 MB written per frame the launches sit at the launch floor like the kernels of frame_ops.hip; what is left to get
// right is the access shape: four output pixels per thread along x with one 16-byte store per channel plane, the per-column and per-row
// tables (tap offsets, weights) computed once per workgroup, N frames per launch, no scratch.
#include "dvmvs_device.h"

#pragma clang fp contract(off)

namespace dvmvs {

constexpr int kPreTileW = 64;   // output columns of a workgroup's tile: 16 threads x 4 pixels
constexpr int kPreTileH = 16;   // output rows of the tile
constexpr int kPreQuad = 4;     // horizontally adjacent outputs per thread

typedef float float4v __attribute__((ext_vector_type(4)));
typedef int int4v __attribute__((ext_vector_type(4)));

struct PreNorm {
  float scale;
  float mean[3];
  float std[3];
};

// One workgroup = one 64 x 16 tile of one frame's output, all three channels.  Threads 0..63 fill the column table, threads 64..79 the
// row table (byte offsets of both taps with the crop folded in, and the fp32 weight of the second tap); then thread (qx, ry) blends the
// four pixels ox = 4 qx .. 4 qx + 3 of row ry for the three channels from byte loads (the 3 channels of a tap are adjacent bytes, the
// two taps of a pixel adjacent or identical pixels: all within one or two 64-byte lines per row) and stores one quad per plane.
// VEC: new_w % 4 == 0 and every plane row is 16-byte aligned (decided by the launcher); otherwise scalar stores with a column guard.
template <bool VEC, bool NORM>
__global__ __launch_bounds__(256) void preprocess_rgb_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst,
                                                             long long src_frame_stride, int row_stride, int crop_x, int crop_y, int h, int w,
                                                             int new_h, int new_w, int tiles_x, double sx, double sy,
                                                             long long dst_batch_stride, PreNorm norm) {
  __shared__ __attribute__((aligned(16))) int s_xa[kPreTileW];
  __shared__ __attribute__((aligned(16))) int s_xb[kPreTileW];
  __shared__ __attribute__((aligned(16))) float s_fx[kPreTileW];
  __shared__ int s_ya[kPreTileH], s_yb[kPreTileH];
  __shared__ float s_fy[kPreTileH];
  const int t = threadIdx.x;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  if (t < kPreTileW) {
    // resize_bilinear: xs = clip((x + 0.5) * (w / new_w) - 0.5, 0);  x0 = min(floor(xs), w - 1);  x1 = min(x0 + 1, w - 1);  fx = float32(xs - x0)
    const int x = min(tile_x * kPreTileW + t, new_w - 1);     // columns past the end repeat the last one: valid loads, never stored
    const double xs = fmax((static_cast<double>(x) + 0.5) * sx - 0.5, 0.0);
    const int x0 = min(static_cast<int>(xs), w - 1);
    const int x1 = min(x0 + 1, w - 1);
    s_xa[t] = (crop_x + x0) * 3;
    s_xb[t] = (crop_x + x1) * 3;
    s_fx[t] = static_cast<float>(xs - static_cast<double>(x0));
  } else if (t < kPreTileW + kPreTileH) {
    const int r = t - kPreTileW;
    const int y = min(tile_y * kPreTileH + r, new_h - 1);
    const double ys = fmax((static_cast<double>(y) + 0.5) * sy - 0.5, 0.0);
    const int y0 = min(static_cast<int>(ys), h - 1);
    const int y1 = min(y0 + 1, h - 1);
    s_ya[r] = (crop_y + y0) * row_stride;
    s_yb[r] = (crop_y + y1) * row_stride;
    s_fy[r] = static_cast<float>(ys - static_cast<double>(y0));
  }
  __syncthreads();
  const int qx = t & 15, ry = t >> 4;
  const int oy = tile_y * kPreTileH + ry, ox = tile_x * kPreTileW + qx * kPreQuad;
  if (oy >= new_h || ox >= new_w) return;
  const unsigned char* frame = src + static_cast<size_t>(blockIdx.y) * src_frame_stride;
  const unsigned char* r0 = frame + s_ya[ry];
  const unsigned char* r1 = frame + s_yb[ry];
  const float fy = s_fy[ry], gy = 1.0f - fy;
  const int4v xa = *reinterpret_cast<const int4v*>(s_xa + qx * kPreQuad);      // one ds_read_b128 per table
  const int4v xb = *reinterpret_cast<const int4v*>(s_xb + qx * kPreQuad);
  const float4v fx = *reinterpret_cast<const float4v*>(s_fx + qx * kPreQuad);
  float4v v[3];
#pragma unroll
  for (int e = 0; e < kPreQuad; ++e) {
    const float gx = 1.0f - fx[e];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = static_cast<float>(r0[xa[e] + c]), b = static_cast<float>(r0[xb[e] + c]);
      const float p = static_cast<float>(r1[xa[e] + c]), q = static_cast<float>(r1[xb[e] + c]);
      // top = a * (1 - fx) + b * fx;  bottom likewise;  top * (1 - fy) + bottom * fy   (every product and sum rounded: no FMA)
      const float top = a * gx + b * fx[e];
      const float bottom = p * gx + q * fx[e];
      float val = top * gy + bottom * fy;
      if (NORM) val = (val / norm.scale - norm.mean[c]) / norm.std[c];
      v[c][e] = val;
    }
  }
  const size_t plane = static_cast<size_t>(new_h) * new_w;
  float* o = dst + static_cast<size_t>(blockIdx.y) * dst_batch_stride + static_cast<size_t>(oy) * new_w + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (VEC) {
      *reinterpret_cast<float4v*>(o + c * plane) = v[c];
    } else {
#pragma unroll
      for (int e = 0; e < kPreQuad; ++e)
        if (ox + e < new_w) o[c * plane + e] = v[c][e];
    }
  }
}

// Four horizontally adjacent outputs per thread; resize_nearest: source index = min(int(dst * (size / new_size)), size - 1) in double,
// value = float32(double(d) / scaling) -- the float32 rounding of what load_depth_png + apply_depth return.
template <bool VEC>
__global__ __launch_bounds__(256) void preprocess_depth_kernel(const unsigned short* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                               int crop_x, int crop_y, int h, int w, int new_h, int new_w, int quads_x,
                                                               double sx, double sy, double scaling) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int oy = q / quads_x, ox = kPreQuad * (q - oy * quads_x);
  if (oy >= new_h) return;
  const int y0 = min(static_cast<int>(static_cast<double>(oy) * sy), h - 1);
  const unsigned short* row = src + static_cast<size_t>(blockIdx.y) * H * W + static_cast<size_t>(crop_y + y0) * W + crop_x;
  float4v v;
#pragma unroll
  for (int e = 0; e < kPreQuad; ++e) {
    const int x = min(ox + e, new_w - 1);
    const int x0 = min(static_cast<int>(static_cast<double>(x) * sx), w - 1);
    v[e] = static_cast<float>(static_cast<double>(row[x0]) / scaling);
  }
  float* o = dst + (static_cast<size_t>(blockIdx.y) * new_h + oy) * new_w + ox;
  if (VEC) {
    *reinterpret_cast<float4v*>(o) = v;
  } else {
#pragma unroll
    for (int e = 0; e < kPreQuad; ++e)
      if (ox + e < new_w) o[e] = v[e];
  }
}

// crop and sizes common to both entry points: DVMVS_EINVAL for a non-positive size, a negative crop or a crop that leaves no pixels
static int check_geometry(int N, int H, int W, int crop_x, int crop_y, int new_h, int new_w) {
  if (N < 1 || H < 1 || W < 1 || new_h < 1 || new_w < 1 || crop_x < 0 || crop_y < 0) return DVMVS_EINVAL;
  if (static_cast<long long>(W) - 2LL * crop_x < 1 || static_cast<long long>(H) - 2LL * crop_y < 1) return DVMVS_EINVAL;
  return 0;
}

}  // namespace dvmvs

extern "C" int dvmvs_preprocess_rgb_fwd(const unsigned char* src, float* dst, int N, int H, int W, long long src_row_stride, int crop_x,
                                        int crop_y, int new_h, int new_w, long long dst_batch_stride, double scale,
                                        const float* mean_host, const float* std_host, int normalize, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!src || !dst || (normalize != 0 && normalize != 1)) return DVMVS_EINVAL;
  if (const int rc = check_geometry(N, H, W, crop_x, crop_y, new_h, new_w)) return rc;
  const long long out_frame = 3LL * new_h * new_w;      // < 2^63: both factors are ints
  if (src_row_stride < 3LL * W || dst_batch_stride < out_frame) return DVMVS_EINVAL;
  // strides are bounded on their own before any product is formed with them (a stride near 2^62 would overflow H * stride)
  if (src_row_stride >= (1LL << 31) || dst_batch_stride >= (1LL << 40)) return DVMVS_EUNSUPPORTED;
  PreNorm norm = {1.0f, {0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}};
  if (normalize) {
    if (!mean_host || !std_host) return DVMVS_EINVAL;
    norm.scale = static_cast<float>(scale);
    if (!(norm.scale != 0.0f)) return DVMVS_EINVAL;       // also refuses NaN
    for (int c = 0; c < 3; ++c) {
      norm.mean[c] = mean_host[c];
      norm.std[c] = std_host[c];
      if (!(norm.std[c] != 0.0f)) return DVMVS_EINVAL;
    }
  }
  // the kernel holds byte offsets inside a source frame and element offsets inside an output frame in 32-bit integers
  if (N > 65535 || static_cast<long long>(H) * src_row_stride >= (1LL << 31) || out_frame >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  const int h = H - 2 * crop_y, w = W - 2 * crop_x;
  const double sx = w / static_cast<double>(new_w), sy = h / static_cast<double>(new_h);
  const int tiles_x = (new_w + kPreTileW - 1) / kPreTileW, tiles_y = (new_h + kPreTileH - 1) / kPreTileH;
  const bool vec = new_w % kPreQuad == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0 && dst_batch_stride % kPreQuad == 0;
  const dim3 grid(tiles_x * tiles_y, N), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long frame_stride = static_cast<long long>(H) * src_row_stride;
  const int rs = static_cast<int>(src_row_stride);
#define DVMVS_PRE_LAUNCH(V, NRM)                                                                                                          \
  hipLaunchKernelGGL((preprocess_rgb_kernel<V, NRM>), grid, block, 0, s, src, dst, frame_stride, rs, crop_x, crop_y, h, w, new_h, new_w, \
                     tiles_x, sx, sy, dst_batch_stride, norm)
  if (vec) {
    if (normalize) DVMVS_PRE_LAUNCH(true, true); else DVMVS_PRE_LAUNCH(true, false);
  } else {
    if (normalize) DVMVS_PRE_LAUNCH(false, true); else DVMVS_PRE_LAUNCH(false, false);
  }
#undef DVMVS_PRE_LAUNCH
  return launch_status();
}

extern "C" int dvmvs_preprocess_depth_fwd(const unsigned short* src, float* dst, int N, int H, int W, int crop_x, int crop_y, int new_h,
                                          int new_w, double scaling, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!src || !dst) return DVMVS_EINVAL;
  if (const int rc = check_geometry(N, H, W, crop_x, crop_y, new_h, new_w)) return rc;
  if (!(scaling != 0.0)) return DVMVS_EINVAL;
  if (N > 65535 || static_cast<long long>(H) * W >= (1LL << 31) || static_cast<long long>(new_h) * new_w >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  const int h = H - 2 * crop_y, w = W - 2 * crop_x;
  const double sx = w / static_cast<double>(new_w), sy = h / static_cast<double>(new_h);
  const int quads_x = (new_w + kPreQuad - 1) / kPreQuad;
  const long long quads = static_cast<long long>(quads_x) * new_h;
  const dim3 grid(static_cast<unsigned>((quads + 255) / 256), N), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (new_w % kPreQuad == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0)
    hipLaunchKernelGGL((preprocess_depth_kernel<true>), grid, block, 0, s, src, dst, H, W, crop_x, crop_y, h, w, new_h, new_w, quads_x, sx, sy, scaling);
  else
    hipLaunchKernelGGL((preprocess_depth_kernel<false>), grid, block, 0, s, src, dst, H, W, crop_x, crop_y, h, w, new_h, new_w, quads_x, sx, sy, scaling);
  return launch_status();
}
