// Plane volume of the DPSNet baseline for one measurement frame, in one launch (gfx950).
// Replaces the per-plane loop of the reference's dvmvs/baselines/dpsnet/dpsnet.py:343-351 (inverse_warp + two slice copies, 64 times):
//   out[b, 0..C-1,  i] = reference features                      out[b, C..2C-1, i] = measurement features warped to plane i
// with the depth of plane i = (mindepth * nlabel) / (i + 1e-16) (plane 0 is at ~3.2e17: the reference's behaviour, kept).
//
// Warp convention (dpsnet.py:36-120), which is NOT the one of cost_volume.hip / sweep_*.hip:
//   cam = (Kinv [x, y, 1]) * depth;   p = (K pose)[:, :3] cam + (K pose)[:, 3];   Z = max(p_z, 1e-3)
//   gx = 2 (p_x / Z) / (w - 1) - 1,  gy likewise with h;   gx or gy outside [-1, 1] -> 2 (the sample is fully masked)
//   grid_sample(bilinear, zeros padding, align_corners=True)
// The fp32 operations are taken in the reference's order with contraction off up to the mask, which is a discontinuity; K pose is a
// plain fp32 product in the prologue.  Divisions are correctly rounded (hipcc's default for '/').
//
// Layout: one lane per (plane, pixel): blockIdx.y = plane, 256 consecutive pixels per workgroup.  A lane computes its four taps and
// weights once and walks the C channels; every store of a wave is 256 contiguous bytes.  The launch is bound by its writes
// (2C * nlabel * h * w * 4 bytes per item: 78.6 MB at C = 32, 64 planes, 60x80); both feature maps (614 KB each) stay in L2.
#include "dvmvs_device.h"

namespace dvmvs {

constexpr int kDpsBlock = 256;
constexpr int kDpsMaxChannels = 64;

struct DpsVolumeArgs {
  const float* ref;
  const float* meas;
  const float* pose;   // [B,3,4]
  const float* K;      // [B,3,3]
  const float* Kinv;   // [B,3,3]
  float* out;
  int C, h, w, nlabel;
  float depth_num;     // fp32(fp32(mindepth) * nlabel): the reference's disp2depth
};

#pragma clang fp contract(off)
// entry (r, c) of K pose (fp32, k in order): the reference's intrinsics.bmm(pose)
__device__ inline float dps_proj_entry(gcfloat_p K_row, gcfloat_p pose_col) {
  return (K_row[0] * pose_col[0] + K_row[1] * pose_col[4]) + K_row[2] * pose_col[8];
}

// Normalised sample position of pixel (xf, yf) on the plane at `depth`, masked as cam2pixel(padding_mode='zeros') masks it.
__device__ inline void dps_grid(const float* kinv, const float* proj, float xf, float yf, float depth, int w, int h, float* gx, float* gy) {
  const float c0 = ((kinv[0] * xf + kinv[1] * yf) + kinv[2]) * depth;
  const float c1 = ((kinv[3] * xf + kinv[4] * yf) + kinv[5]) * depth;
  const float c2 = ((kinv[6] * xf + kinv[7] * yf) + kinv[8]) * depth;
  const float X = ((proj[0] * c0 + proj[1] * c1) + proj[2] * c2) + proj[3];
  const float Y = ((proj[4] * c0 + proj[5] * c1) + proj[6] * c2) + proj[7];
  const float Z = fmaxf(((proj[8] * c0 + proj[9] * c1) + proj[10] * c2) + proj[11], 1e-3f);
  float nx = 2.0f * (X / Z) / static_cast<float>(w - 1) - 1.0f;
  float ny = 2.0f * (Y / Z) / static_cast<float>(h - 1) - 1.0f;
  if (nx > 1.0f || nx < -1.0f) nx = 2.0f;
  if (ny > 1.0f || ny < -1.0f) ny = 2.0f;
  *gx = nx;
  *gy = ny;
}
#pragma clang fp contract(fast)

__global__ __launch_bounds__(kDpsBlock) void dps_volume_kernel(DpsVolumeArgs a) {
  __shared__ float s_proj[12];
  __shared__ float s_kinv[9];
  const int b = blockIdx.z;
  const int plane = blockIdx.y;
  const int tid = threadIdx.x;
  if (tid < 12) {
    const int r = tid / 4, c = tid - r * 4;
    s_proj[tid] = dps_proj_entry(as_global(a.K) + b * 9 + r * 3, as_global(a.pose) + b * 12 + c);
  } else if (tid < 21) {
    s_kinv[tid - 12] = as_global(a.Kinv)[b * 9 + (tid - 12)];
  }
  __syncthreads();

  const int HW = a.h * a.w;
  const int pix = blockIdx.x * kDpsBlock + tid;
  if (pix >= HW) return;
  const int y = pix / a.w;
  const int x = pix - y * a.w;

  // i + 1e-16 is taken in double as Python does (it equals i for i >= 1) and rounded to fp32 where it meets the fp32 tensor
  const float depth = a.depth_num / static_cast<float>(static_cast<double>(plane) + 1e-16);
  float gx, gy;
  dps_grid(s_kinv, s_proj, static_cast<float>(x), static_cast<float>(y), depth, a.w, a.h, &gx, &gy);
  const BilinearTaps t = make_taps(unnormalize_ac(gx, a.w), unnormalize_ac(gy, a.h), a.w, a.h);

  // out-of-image taps get weight 0 and a valid address (pixel 0), as in sweep_rgb.hip
  const int xa = t.in_x0 ? t.x0 : 0, xb = t.in_x1 ? t.x0 + 1 : 0;
  const int ya = t.in_y0 ? t.y0 : 0, yb = t.in_y1 ? t.y0 + 1 : 0;
  const int o0 = ya * a.w + xa, o1 = ya * a.w + xb, o2 = yb * a.w + xa, o3 = yb * a.w + xb;
  const float w0 = (t.in_x0 && t.in_y0) ? t.w_nw : 0.0f;
  const float w1 = (t.in_x1 && t.in_y0) ? t.w_ne : 0.0f;
  const float w2 = (t.in_x0 && t.in_y1) ? t.w_sw : 0.0f;
  const float w3 = (t.in_x1 && t.in_y1) ? t.w_se : 0.0f;
  const bool any = (t.in_x0 || t.in_x1) && (t.in_y0 || t.in_y1);

  const size_t plane_stride = static_cast<size_t>(a.nlabel) * HW;    // one channel of the volume
  gcfloat_p ref = as_global(a.ref) + static_cast<size_t>(b) * a.C * HW + pix;
  gcfloat_p meas = as_global(a.meas) + static_cast<size_t>(b) * a.C * HW;
  gfloat_p out_ref = as_global(a.out) + static_cast<size_t>(b) * 2 * a.C * plane_stride + static_cast<size_t>(plane) * HW + pix;
  gfloat_p out_warp = out_ref + static_cast<size_t>(a.C) * plane_stride;

#pragma unroll 4
  for (int c = 0; c < a.C; ++c) {
    out_ref[c * plane_stride] = ref[static_cast<size_t>(c) * HW];
    float s = 0.0f;
    if (any) {
      gcfloat_p m = meas + static_cast<size_t>(c) * HW;
      s = m[o0] * w0;
      s += m[o1] * w1;
      s += m[o2] * w2;
      s += m[o3] * w3;
    }
    out_warp[c * plane_stride] = s;
  }
}

}  // namespace dvmvs

extern "C" int dvmvs_dps_volume_fwd(const float* ref, const float* meas, const float* pose, const float* K, const float* Kinv, float* out,
                                    int B, int C, int h, int w, int nlabel, double mindepth, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!ref || !meas || !pose || !K || !Kinv || !out) return DVMVS_EINVAL;
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || nlabel <= 0 || !(mindepth > 0.0)) return DVMVS_EINVAL;
  if (C > kDpsMaxChannels || nlabel > DVMVS_MAX_DEPTH_LEVELS || B > 65535) return DVMVS_EUNSUPPORTED;
  if (static_cast<long long>(h) * w >= (1LL << 24)) return DVMVS_EUNSUPPORTED;     // pixel indices stay exact in fp32 and int
  DpsVolumeArgs a;
  a.ref = ref, a.meas = meas, a.pose = pose, a.K = K, a.Kinv = Kinv, a.out = out;
  a.C = C, a.h = h, a.w = w, a.nlabel = nlabel;
  a.depth_num = static_cast<float>(mindepth) * static_cast<float>(nlabel);
  dim3 grid((h * w + kDpsBlock - 1) / kDpsBlock, nlabel, B);
  hipLaunchKernelGGL(dps_volume_kernel, grid, dim3(kDpsBlock), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}
