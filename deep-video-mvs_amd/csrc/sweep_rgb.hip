// SAD plane sweep of a 3-channel (RGB) reference image against M <= 8 measurement images, written into a channel slice of a
// caller-owned [B,Cout,H,W] tensor (gfx950).  This is the cost volume of the MVDepthNet and GP-MVS baselines
// (the reference's dvmvs/baselines/mvdepthnet/run-testing.py:141-156): cost_volume_fusion(..., dot_product=False) on the
// full-resolution normalised image, C = 3, followed there by torch.cat((image, cost_volume), 1).  With copy_image the same launch
// also writes the reference image into channels 0..2, so the 67-channel encoder input exists without a separate volume or a cat.
//
// Semantics: the reference's dvmvs/utils.py:45-107 in the generic kernel's order (cost_volume.hip): per plane and measurement frame,
// bilinear taps (grid_sample, align_corners=True, zeros padding), sum_c |ref - warp(meas)| over c in order, a running sum over m
// from zero, divided by M.  Sample positions come from SweepRay / sweep_sample (sweep_sample.h), whose divisions are correctly
// rounded like the generic kernel's '/', and the taps from make_taps: the result is bit-identical to the generic SAD kernel.
//
// Layout: one lane per pixel, a workgroup = 256 consecutive pixels x kRgbPlanes planes.  A wave's store of one plane is 256
// contiguous bytes; the three reference values and the M rays are computed once per lane and reused over the planes.  The floor is
// the output write (D * H * W * 4 bytes per item); the gathers of three 320x256 fp32 planes per measurement frame stay in L2.
#include "sweep_sample.h"

namespace dvmvs {

constexpr int kRgbWaves = 4;
constexpr int kRgbPlanes = 16;   // planes per workgroup: 4 x 64 = 1280 workgroups for 320x256 x 64 planes on 256 CUs

__global__ __launch_bounds__(kWave* kRgbWaves) void rgb_sweep_kernel(CostVolumeArgs a, int Cout, int channel_offset, int copy_image) {
  __shared__ float s_H[DVMVS_MAX_MEASUREMENTS * 9];
  __shared__ float s_kt[DVMVS_MAX_MEASUREMENTS * 3];
  __shared__ float s_ktd[DVMVS_MAX_MEASUREMENTS * kRgbPlanes * 3];

  const int b = blockIdx.z;
  const int d_block = blockIdx.y * kRgbPlanes;
  const int tid = threadIdx.x;
  sweep_setup(a, b, d_block, kRgbPlanes, tid, kWave * kRgbWaves, s_H, s_kt, s_ktd);

  const int HW = a.H * a.W;
  const int pix = blockIdx.x * (kWave * kRgbWaves) + tid;
  if (pix >= HW) return;
  const int y = pix / a.W;
  const int x = pix - y * a.W;
  const float xf = static_cast<float>(x), yf = static_cast<float>(y);
  const SweepScale sc = sweep_scale(a.W, a.H);

  gcfloat_p ref = as_global(a.image1) + static_cast<size_t>(b) * 3 * HW + pix;
  const float r0 = ref[0], r1 = ref[HW], r2 = ref[2 * HW];
  gfloat_p out = as_global(a.out) + static_cast<size_t>(b) * Cout * HW + pix;
  if (copy_image && blockIdx.y == 0) {
    out[0] = r0;
    out[HW] = r1;
    out[2 * HW] = r2;
  }
  out += static_cast<size_t>(channel_offset) * HW;

  const int planes = min(kRgbPlanes, a.D - d_block);
  for (int j = 0; j < planes; ++j) {
    float fused = 0.0f;
    for (int m = 0; m < a.M; ++m) {
      const SweepRay ray = sweep_ray(s_H + m * 9, xf, yf);
      const float* k = s_ktd + (m * kRgbPlanes + j) * 3;
      float ix, iy;
      sweep_sample(ray, k[0], k[1], k[2], sc, &ix, &iy);
      const BilinearTaps t = make_taps(ix, iy, a.W, a.H);
      const int xa = t.in_x0 ? t.x0 : 0, xb = t.in_x1 ? t.x0 + 1 : 0;
      const int ya = t.in_y0 ? t.y0 : 0, yb = t.in_y1 ? t.y0 + 1 : 0;
      const int o0 = ya * a.W + xa, o1 = ya * a.W + xb, o2 = yb * a.W + xa, o3 = yb * a.W + xb;
      const float w0 = (t.in_x0 && t.in_y0) ? t.w_nw : 0.0f;
      const float w1 = (t.in_x1 && t.in_y0) ? t.w_ne : 0.0f;
      const float w2 = (t.in_x0 && t.in_y1) ? t.w_sw : 0.0f;
      const float w3 = (t.in_x1 && t.in_y1) ? t.w_se : 0.0f;
      gcfloat_p meas = as_global(a.image2[m]) + static_cast<size_t>(b) * 3 * HW;
      const float r[3] = {r0, r1, r2};
      float acc = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        gcfloat_p plane = meas + static_cast<size_t>(c) * HW;
        // the generic kernel's expression, statement for statement (same contractions)
        float s = plane[o0] * w0;
        s += plane[o1] * w1;
        s += plane[o2] * w2;
        s += plane[o3] * w3;
        acc += fabsf(r[c] - s);
      }
      fused += acc;
    }
    out[static_cast<size_t>(d_block + j) * HW] = fused / static_cast<float>(a.M);
  }
}

}  // namespace dvmvs

extern "C" int dvmvs_rgb_sweep_fwd(const float* image1, const float* const* image2s, const float* Hm, const float* kt, float* out,
                                   int B, int M, int C, int H, int W, int D, double min_depth, double max_depth, int Cout,
                                   int channel_offset, int copy_image, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (C != 3) return DVMVS_EUNSUPPORTED;
  CostVolumeArgs a;
  const int rc = fill_sweep_args(&a, image1, image2s, Hm, kt, out, B, M, C, H, W, D, min_depth, max_depth, true);
  if (rc != 0) return rc;
  if (copy_image != 0 && copy_image != 1) return DVMVS_EINVAL;
  // the volume occupies channels [channel_offset, channel_offset + D) and must not overlap the copied image (channels 0..2)
  if (channel_offset < (copy_image ? 3 : 0) || Cout <= 0 || static_cast<long long>(channel_offset) + D > Cout) return DVMVS_EINVAL;
  if (static_cast<long long>(Cout) * H * W >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  const int HW = H * W;
  constexpr int kBlock = kWave * kRgbWaves;
  dim3 grid((HW + kBlock - 1) / kBlock, (D + kRgbPlanes - 1) / kRgbPlanes, B);
  hipLaunchKernelGGL(rgb_sweep_kernel, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), a, Cout, channel_offset, copy_image);
  return launch_status();
}
