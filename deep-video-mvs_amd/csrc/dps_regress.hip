// DPSNet's depth regression in one launch (gfx950): up-sampling of the plane costs, softmax over the planes, expectation, depth.
// Semantics (the reference's dvmvs/baselines/dpsnet/dpsnet.py:373-383):
//   c = F.interpolate(costs [B,1,nlabel,h,w], [nlabel,H,W], mode='trilinear', align_corners=False)
//       (the plane axis keeps its size: per plane, a bilinear up-sampling with half-pixel centres and clamped borders)
//   p = softmax(c, planes);   pred = sum_i p_i * i;   depth = mindepth * nlabel / (pred + 1e-16)
// The COSTS are interpolated, not the probabilities.  The reference materialises [B,nlabel,H,W] about six times per call; this kernel
// reads the 1.2 MB of costs (60x80, 64 planes) and writes 0.3 MB.
//
// Layout: a workgroup is 64 output pixels x 4 plane groups (one wave per group, planes interleaved: group g takes planes g, g+4, ...).
// Each lane takes the maximum of its planes, then their sum and index-weighted sum relative to that maximum (the four taps are read
// again: they are L1 hits); the four partial (max, sum, weighted sum) triples of a pixel meet in LDS and wave 0 merges them in a fixed
// order, so results are deterministic.  The per-plane loads of a wave cover ~16 neighbouring source pixels of two rows.
#include "dvmvs_device.h"

namespace dvmvs {

constexpr int kRegGroups = 4;

// ATen's area_pixel_compute_source_index (align_corners=False, linear) + guard_index_and_lambda
__device__ inline void upsample_source(int dst, float scale, int in_size, int* i0, int* i1, float* l0, float* l1) {
  const float src = fmaxf(scale * (static_cast<float>(dst) + 0.5f) - 0.5f, 0.0f);
  const int idx = min(static_cast<int>(src), in_size - 1);
  const float lam = fminf(fmaxf(src - static_cast<float>(idx), 0.0f), 1.0f);
  *i0 = idx;
  *i1 = idx + (idx < in_size - 1 ? 1 : 0);
  *l1 = lam;
  *l0 = 1.0f - lam;
}

__global__ __launch_bounds__(kWave* kRegGroups) void dps_regress_kernel(const float* __restrict__ costs, float* __restrict__ depth,
                                                                        float* __restrict__ pred, int nlabel, int h, int w, int H, int W,
                                                                        float scale_h, float scale_w, float depth_num) {
  __shared__ float s_max[kRegGroups][kWave];
  __shared__ float s_sum[kRegGroups][kWave];
  __shared__ float s_wsum[kRegGroups][kWave];
  const int lane = threadIdx.x & (kWave - 1);
  const int group = threadIdx.x / kWave;
  const int b = blockIdx.y;
  const int HW = H * W, hw = h * w;
  const int pix = blockIdx.x * kWave + lane;
  const int p = min(pix, HW - 1);          // lanes past the end compute a valid pixel and do not store
  const int oy = p / W;
  const int ox = p - oy * W;
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  upsample_source(oy, scale_h, h, &y0, &y1, &ly0, &ly1);
  upsample_source(ox, scale_w, w, &x0, &x1, &lx0, &lx1);
  const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
  gcfloat_p src = as_global(costs) + static_cast<size_t>(b) * nlabel * hw;

  auto sample = [&](int i) {
    gcfloat_p c = src + static_cast<size_t>(i) * hw;
    return ly0 * (lx0 * c[o00] + lx1 * c[o01]) + ly1 * (lx0 * c[o10] + lx1 * c[o11]);
  };

  float m = -INFINITY;
  for (int i = group; i < nlabel; i += kRegGroups) m = fmaxf(m, sample(i));
  float s = 0.0f, ws = 0.0f;
  for (int i = group; i < nlabel; i += kRegGroups) {
    const float e = expf(sample(i) - m);
    s += e;
    ws += e * static_cast<float>(i);
  }
  s_max[group][lane] = m;
  s_sum[group][lane] = s;
  s_wsum[group][lane] = ws;
  __syncthreads();
  if (group != 0 || pix >= HW) return;

  float M = s_max[0][lane];
#pragma unroll
  for (int g = 1; g < kRegGroups; ++g) M = fmaxf(M, s_max[g][lane]);
  float S = 0.0f, WS = 0.0f;
#pragma unroll
  for (int g = 0; g < kRegGroups; ++g) {
    // a group without planes (nlabel < 4) holds max = -inf, sum = 0: its factor is exp(-inf) = 0
    const float f = expf(s_max[g][lane] - M);
    S += s_sum[g][lane] * f;
    WS += s_wsum[g][lane] * f;
  }
  const float e = WS / S;
  const size_t o = static_cast<size_t>(b) * HW + pix;
  if (pred) as_global(pred)[o] = e;
  // the reference's `mindepth * nlabel / (pred + 1e-16)` is Tensor.__rtruediv__: reciprocal, then the product
  as_global(depth)[o] = (1.0f / (e + 1e-16f)) * depth_num;
}

}  // namespace dvmvs

extern "C" int dvmvs_dps_regress_fwd(const float* costs, float* depth, float* pred, int B, int nlabel, int h, int w, int H, int W,
                                     double mindepth, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!costs || !depth) return DVMVS_EINVAL;      // pred may be null: the expectation is not written then
  if (B <= 0 || nlabel <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || !(mindepth > 0.0)) return DVMVS_EINVAL;
  if (nlabel > DVMVS_MAX_DEPTH_LEVELS || B > 65535) return DVMVS_EUNSUPPORTED;
  if (static_cast<long long>(H) * W >= (1LL << 30) || static_cast<long long>(h) * w >= (1LL << 30)) return DVMVS_EUNSUPPORTED;
  const float scale_h = static_cast<float>(h) / static_cast<float>(H);
  const float scale_w = static_cast<float>(w) / static_cast<float>(W);
  const float depth_num = static_cast<float>(mindepth * static_cast<double>(nlabel));
  dim3 grid((H * W + kWave - 1) / kWave, B);
  hipLaunchKernelGGL(dps_regress_kernel, grid, dim3(kWave * kRegGroups), 0, static_cast<hipStream_t>(stream), costs, depth, pred, nlabel,
                     h, w, H, W, scale_h, scale_w, depth_num);
  return launch_status();
}
