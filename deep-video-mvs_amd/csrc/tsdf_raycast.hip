// Ray-casting of a fused TSDF volume from N camera views (gfx950): depth, world-space normal and colour of the first zero crossing
// along every pixel's ray.  The reference project has no ray-caster; the definition below is this project's own and is restated in
// float32 / float64 by tests/raycast_reference.py.
//
// Definition, per pixel (u, v) of view n (every operation in float32, rounded, contraction off):
//   d_c = ((u - cx) / fx, (v - cy) / fy, 1);  o_g = (t - origin) / voxel_size;  d_g = (R d_c) / voxel_size, R d_c summed left to right.
//   A point of the ray is g(z) = o_g + z d_g in voxel coordinates: z is the camera depth.
//   [z0, z1] = slab intersection of the ray with the box [0, dim - 1]^3 (where trilinear interpolation has its eight corners), cut to
//   [near, far].  A component d_g == 0 contributes (-inf, +inf) when o_g lies inside its slab and nothing otherwise.  A non-finite o_g,
//   d_g, z0 or z1, or z0 > z1, is a miss.
//   dz = step / |d_g|;  n = min(floor((z1 - z0) / dz), n_cap) with n_cap = floor(box diagonal / step) + 2;  z_k = z0 + float(k) dz, k = 0..n.
//   f_k = trilinear tsdf at clamp(g(z_k)) in the cell i0 = min(floor(g), dim - 2): lerp(a, b, w) = a (1 - w) + b w along z, then y, then x.
//   Sample k is valid when the eight corner weights of its cell are > 0.
//   Hit = the first k >= 1 with samples k - 1 and k valid and f_{k-1} > 0 >= f_k;  depth = z_{k-1} + dz (f_{k-1} / (f_{k-1} - f_k)).
//   No hit: depth 0.  Normal: central differences of the same trilinear tsdf at clamp(g* +- 1 voxel) per axis, normalised; zero when one
//   of the six samples is invalid or the gradient vanishes.  Colour: the folded colour voxel at rint(g*), decoded as marching_cubes.hip does.
//
// Mapping: one lane per pixel, a wave covers an 8x8 pixel tile (neighbouring rays gather from neighbouring voxels), four waves a 16x16
// block, blockIdx.z the view.  The march is a divergent per-lane loop: k strictly increases and ends at n <= n_cap.
//
// Empty-space skipping.  tsdf_raycast_mask_kernel flags every 8x8x8 brick of cells that has a corner with weight > 0 && tsdf <= 0.
// A hit at sample k needs f_k <= 0 with the cell valid; lerp(a, b, w) of positive a, b with w in [0, 1] is positive (both products are
// >= 0 and the one with the weight >= 1/2 is > 0), so a sample whose cell lies in an unflagged brick never ends a hit and is not
// evaluated.  Jumps are verified, not predicted: every float32 operation that maps k to the cell index is monotone in k per axis
// (int -> float, * dz, + z0, * d_g, + o_g, clamp, floor, min), so when samples k and k' > k fall into the same brick, every sample
// between them does.  The slab arithmetic only proposes k'; a wrong proposal costs one step, never a sample.  When an evaluated sample
// follows skipped ones, f_{k-1} is evaluated on demand (only when f_k <= 0 makes it matter).  z_k comes from k alone, so both paths
// produce the same bits.
#include "dvmvs_device.h"

#include <math.h>

namespace dvmvs {

constexpr int kRcBrick = 8;       // cells per brick edge
constexpr int kRcBrickShift = 3;
constexpr int kRcMaxSteps = 1 << 20;

struct RcGeom {
  int X, Y, Z;      // voxels
  int bx, by, bz;   // bricks of cells: ceil((dim - 1) / 8)
};

inline int rc_bricks(int dim) { return (dim - 1 + kRcBrick - 1) / kRcBrick; }

#pragma clang fp contract(off)

__device__ inline float rc_lerp(float a, float b, float w) { return a * (1.0f - w) + b * w; }

// clamp(o_g + z d_g) into the box; never NaN for finite inputs (fmaxf / fminf drop a NaN operand anyway)
__device__ inline void rc_point(const float* og, const float* dg, float z, const RcGeom& G, float* g) {
  g[0] = fminf(fmaxf(og[0] + z * dg[0], 0.0f), static_cast<float>(G.X - 1));
  g[1] = fminf(fmaxf(og[1] + z * dg[1], 0.0f), static_cast<float>(G.Y - 1));
  g[2] = fminf(fmaxf(og[2] + z * dg[2], 0.0f), static_cast<float>(G.Z - 1));
}

// cell of a clamped point: i0 = min(floor(g), dim - 2), kept inside [0, dim - 2] whatever g is
__device__ inline void rc_cell(const float* g, const RcGeom& G, int* c) {
  c[0] = max(min(static_cast<int>(floorf(g[0])), G.X - 2), 0);
  c[1] = max(min(static_cast<int>(floorf(g[1])), G.Y - 2), 0);
  c[2] = max(min(static_cast<int>(floorf(g[2])), G.Z - 2), 0);
}

// trilinear tsdf at the clamped point g in cell c; valid <- all eight corner weights > 0
__device__ inline float rc_sample(const float* __restrict__ tsdf, const float* __restrict__ weight, const RcGeom& G, const float* g,
                                  const int* c, bool& valid) {
  const long long sy = G.Z, sx = static_cast<long long>(G.Y) * G.Z;
  const long long base = c[0] * sx + c[1] * sy + c[2];
  const float wx = g[0] - static_cast<float>(c[0]), wy = g[1] - static_cast<float>(c[1]), wz = g[2] - static_cast<float>(c[2]);
  float t[8], w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const long long idx = base + ((i >> 2) & 1) * sx + ((i >> 1) & 1) * sy + (i & 1);
    t[i] = tsdf[idx];
    w[i] = weight[idx];
  }
  valid = w[0] > 0.0f && w[1] > 0.0f && w[2] > 0.0f && w[3] > 0.0f && w[4] > 0.0f && w[5] > 0.0f && w[6] > 0.0f && w[7] > 0.0f;
  const float c00 = rc_lerp(t[0], t[1], wz), c01 = rc_lerp(t[2], t[3], wz), c10 = rc_lerp(t[4], t[5], wz), c11 = rc_lerp(t[6], t[7], wz);
  return rc_lerp(rc_lerp(c00, c01, wy), rc_lerp(c10, c11, wy), wx);
}

__device__ inline float rc_sample_at(const float* __restrict__ tsdf, const float* __restrict__ weight, const RcGeom& G, const float* g,
                                     bool& valid) {
  int c[3];
  rc_cell(g, G, c);
  return rc_sample(tsdf, weight, G, g, c, valid);
}

__device__ inline bool rc_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for NaN and +-inf

__global__ __launch_bounds__(256) void tsdf_raycast_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                            const float* __restrict__ color, RcGeom G, float origin_x, float origin_y,
                                                            float origin_z, float voxel_size, const unsigned char* __restrict__ mask,
                                                            const float* __restrict__ cam_intr, const float* __restrict__ cam_pose, int H,
                                                            int W, float near, float far, float step, int n_cap, float* __restrict__ depth,
                                                            float* __restrict__ normal, unsigned char* __restrict__ rgb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int v = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const int view = blockIdx.z;
  if (u >= W || v >= H) return;
  const long long pixel = (static_cast<long long>(view) * H + v) * W + u;
  const float* Kp = cam_intr + 9 * static_cast<long long>(view);
  const float* Pp = cam_pose + 16 * static_cast<long long>(view);
  const float fx = Kp[0], cx = Kp[2], fy = Kp[4], cy = Kp[5];
  const int dims[3] = {G.X, G.Y, G.Z};

  const float dcx = (static_cast<float>(u) - cx) / fx, dcy = (static_cast<float>(v) - cy) / fy;
  float og[3], dg[3];
  og[0] = (Pp[3] - origin_x) / voxel_size;
  og[1] = (Pp[7] - origin_y) / voxel_size;
  og[2] = (Pp[11] - origin_z) / voxel_size;
#pragma unroll
  for (int a = 0; a < 3; ++a) dg[a] = (Pp[4 * a + 0] * dcx + Pp[4 * a + 1] * dcy + Pp[4 * a + 2]) / voxel_size;

  bool ok = rc_finite(og[0]) && rc_finite(og[1]) && rc_finite(og[2]) && rc_finite(dg[0]) && rc_finite(dg[1]) && rc_finite(dg[2]);
  float tmin = -INFINITY, tmax = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float hi = static_cast<float>(dims[a] - 1);
    if (dg[a] == 0.0f) {
      ok = ok && og[a] >= 0.0f && og[a] <= hi;
    } else {
      const float ta = (0.0f - og[a]) / dg[a], tb = (hi - og[a]) / dg[a];
      tmin = fmaxf(tmin, fminf(ta, tb));
      tmax = fminf(tmax, fmaxf(ta, tb));
    }
  }
  const float z0 = fmaxf(tmin, near), z1 = fminf(tmax, far);
  const float len = sqrtf(dg[0] * dg[0] + dg[1] * dg[1] + dg[2] * dg[2]);
  const float dz = step / len;
  ok = ok && rc_finite(z0) && rc_finite(z1) && z0 <= z1 && rc_finite(dz) && dz > 0.0f;

  float hit_depth = 0.0f;
  if (ok) {
    const int n = static_cast<int>(fminf(floorf((z1 - z0) / dz), static_cast<float>(n_cap)));   // >= 0: z0 <= z1
    int k = 0, prev_k = -1;
    float prev_f = 0.0f;
    bool prev_valid = false;
    while (k <= n) {
      float g[3];
      int c[3];
      rc_point(og, dg, z0 + static_cast<float>(k) * dz, G, g);
      rc_cell(g, G, c);
      if (mask) {
        const int b[3] = {c[0] >> kRcBrickShift, c[1] >> kRcBrickShift, c[2] >> kRcBrickShift};
        if (mask[(static_cast<long long>(b[0]) * G.by + b[1]) * G.bz + b[2]] == 0) {
          // nothing in this brick can end a hit: propose the last sample before the ray leaves it, accept it only if it is in the brick
          float zexit = INFINITY;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            if (dg[a] > 0.0f) zexit = fminf(zexit, (static_cast<float>((b[a] + 1) * kRcBrick) - og[a]) / dg[a]);
            if (dg[a] < 0.0f) zexit = fminf(zexit, (static_cast<float>(b[a] * kRcBrick) - og[a]) / dg[a]);
          }
          const float kf = fminf(floorf((zexit - z0) / dz) - 1.0f, static_cast<float>(n));
          int next = k + 1;
          if (kf > static_cast<float>(k)) {   // false for a NaN proposal
            const int kj = static_cast<int>(kf);
            float gj[3];
            int cj[3];
            rc_point(og, dg, z0 + static_cast<float>(kj) * dz, G, gj);
            rc_cell(gj, G, cj);
            if ((cj[0] >> kRcBrickShift) == b[0] && (cj[1] >> kRcBrickShift) == b[1] && (cj[2] >> kRcBrickShift) == b[2]) next = kj + 1;
          }
          k = next;
          continue;
        }
      }
      bool valid;
      const float f = rc_sample(tsdf, weight, G, g, c, valid);
      if (k >= 1 && valid && f <= 0.0f) {
        if (prev_k != k - 1) {   // the previous sample was skipped: evaluate it now
          float gp[3];
          rc_point(og, dg, z0 + static_cast<float>(k - 1) * dz, G, gp);
          prev_f = rc_sample_at(tsdf, weight, G, gp, prev_valid);
        }
        if (prev_valid && prev_f > 0.0f) {
          hit_depth = (z0 + static_cast<float>(k - 1) * dz) + dz * (prev_f / (prev_f - f));
          break;
        }
      }
      prev_k = k;
      prev_f = f;
      prev_valid = valid;
      ++k;
    }
  }
  depth[pixel] = hit_depth;
  if (!normal && !rgb) return;

  const bool hit = hit_depth != 0.0f;
  float gs[3] = {0.0f, 0.0f, 0.0f};
  if (hit) rc_point(og, dg, hit_depth, G, gs);
  if (normal) {
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    if (hit) {
      bool all_valid = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        float gp[3] = {gs[0], gs[1], gs[2]}, gm[3] = {gs[0], gs[1], gs[2]};
        gp[a] = fminf(gs[a] + 1.0f, static_cast<float>(dims[a] - 1));
        gm[a] = fmaxf(gs[a] - 1.0f, 0.0f);
        bool vp, vm;
        const float fp = rc_sample_at(tsdf, weight, G, gp, vp), fm = rc_sample_at(tsdf, weight, G, gm, vm);
        nrm[a] = fp - fm;
        all_valid = all_valid && vp && vm;
      }
      const float nlen = sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
      const bool keep = all_valid && nlen > 0.0f && rc_finite(nlen);
#pragma unroll
      for (int a = 0; a < 3; ++a) nrm[a] = keep ? nrm[a] / nlen : 0.0f;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) normal[3 * pixel + a] = nrm[a];
  }
  if (rgb) {
    float cr = 0.0f, cg = 0.0f, cb_ = 0.0f;
    if (hit) {
      int q[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) q[a] = min(max(static_cast<int>(rintf(gs[a])), 0), dims[a] - 1);
      const float col = color[(static_cast<long long>(q[0]) * G.Y + q[1]) * G.Z + q[2]];
      cb_ = floorf(col / 65536.0f);
      cg = floorf((col - cb_ * 65536.0f) / 256.0f);
      cr = col - cb_ * 65536.0f - cg * 256.0f;
    }
    rgb[3 * pixel + 0] = static_cast<unsigned char>(floorf(cr));
    rgb[3 * pixel + 1] = static_cast<unsigned char>(floorf(cg));
    rgb[3 * pixel + 2] = static_cast<unsigned char>(floorf(cb_));
  }
}
#pragma clang fp contract(fast)

// One wave per brick: its lanes walk the brick's (up to) 9x9x9 corners, z fastest; one byte per brick, z fastest.
__global__ __launch_bounds__(256) void tsdf_raycast_mask_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, RcGeom G,
                                                                 long long n_bricks, unsigned char* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const long long brick = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (brick >= n_bricks) return;   // whole waves leave
  const int bz = static_cast<int>(brick % G.bz), by = static_cast<int>((brick / G.bz) % G.by);
  const int bx = static_cast<int>(brick / (static_cast<long long>(G.bz) * G.by));
  const int x0 = bx * kRcBrick, y0 = by * kRcBrick, z0 = bz * kRcBrick;
  const int nx = min(x0 + kRcBrick, G.X - 1) - x0 + 1, ny = min(y0 + kRcBrick, G.Y - 1) - y0 + 1, nz = min(z0 + kRcBrick, G.Z - 1) - z0 + 1;
  const int total = nx * ny * nz;
  bool any = false;
  for (int i = lane; i < total; i += 64) {
    const int cz = i % nz, cy = (i / nz) % ny, cx = i / (nz * ny);
    const long long idx = (static_cast<long long>(x0 + cx) * G.Y + (y0 + cy)) * G.Z + (z0 + cz);
    any = any || (weight[idx] > 0.0f && tsdf[idx] <= 0.0f);
  }
  const unsigned long long votes = __ballot(any);
  if (lane == 0) mask[brick] = votes != 0ull ? 1 : 0;
}

static int rc_check_dims(int X, int Y, int Z) {
  if (X < 2 || Y < 2 || Z < 2) return DVMVS_EINVAL;
  if (static_cast<long long>(Y) * Z >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  const long long n_bricks = static_cast<long long>(rc_bricks(X)) * rc_bricks(Y) * rc_bricks(Z);
  if (n_bricks >= (1LL << 26)) return DVMVS_EUNSUPPORTED;   // one wave per brick in a 1-D grid
  return 0;
}

}  // namespace dvmvs

extern "C" size_t dvmvs_tsdf_raycast_mask_bytes(int dim_x, int dim_y, int dim_z) {
  using namespace dvmvs;
  if (rc_check_dims(dim_x, dim_y, dim_z) != 0) return 0;
  return static_cast<size_t>(rc_bricks(dim_x)) * rc_bricks(dim_y) * rc_bricks(dim_z);
}

extern "C" int dvmvs_tsdf_raycast_mask(const float* tsdf_vol, const float* weight_vol, int dim_x, int dim_y, int dim_z, unsigned char* mask,
                                       dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!tsdf_vol || !weight_vol || !mask) return DVMVS_EINVAL;
  const int rc = rc_check_dims(dim_x, dim_y, dim_z);
  if (rc != 0) return rc;
  const RcGeom G{dim_x, dim_y, dim_z, rc_bricks(dim_x), rc_bricks(dim_y), rc_bricks(dim_z)};
  const long long n_bricks = static_cast<long long>(G.bx) * G.by * G.bz;
  hipLaunchKernelGGL(tsdf_raycast_mask_kernel, dim3(static_cast<unsigned>((n_bricks + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     tsdf_vol, weight_vol, G, n_bricks, mask);
  return launch_status();
}

extern "C" int dvmvs_tsdf_raycast_fwd(const float* tsdf_vol, const float* weight_vol, const float* color_vol, int dim_x, int dim_y, int dim_z,
                                      float origin_x, float origin_y, float origin_z, float voxel_size, const unsigned char* mask,
                                      const float* cam_intr, const float* cam_pose, int n_views, int im_h, int im_w, float near, float far,
                                      float step, float* depth, float* normal, unsigned char* rgb, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!tsdf_vol || !weight_vol || !cam_intr || !cam_pose || !depth || (rgb && !color_vol)) return DVMVS_EINVAL;
  if (n_views <= 0 || im_h <= 0 || im_w <= 0) return DVMVS_EINVAL;
  if (!(voxel_size > 0.0f) || !(step > 0.0f) || !(step <= 5.0f) || !(near >= 0.0f) || far != far || !(near < INFINITY)) return DVMVS_EINVAL;
  const int rc = rc_check_dims(dim_x, dim_y, dim_z);
  if (rc != 0) return rc;
  if (static_cast<long long>(im_h) * im_w >= (1LL << 31) || n_views > 65535) return DVMVS_EUNSUPPORTED;
  // the longest march: the box diagonal in steps (+ 2 for rounding); float(k) must stay exact and the loop short
  const double dx = dim_x - 1, dy = dim_y - 1, dzv = dim_z - 1;
  const double steps = floor(sqrt(dx * dx + dy * dy + dzv * dzv) / static_cast<double>(step)) + 2.0;
  if (steps >= static_cast<double>(kRcMaxSteps)) return DVMVS_EUNSUPPORTED;
  const RcGeom G{dim_x, dim_y, dim_z, rc_bricks(dim_x), rc_bricks(dim_y), rc_bricks(dim_z)};
  const dim3 grid(static_cast<unsigned>((im_w + 15) / 16), static_cast<unsigned>((im_h + 15) / 16), static_cast<unsigned>(n_views));
  if (grid.y > 65535u) return DVMVS_EUNSUPPORTED;
  // a launch holds fewer than 2^32 threads in all
  if (static_cast<unsigned long long>(grid.x) * grid.y * grid.z * 256ull >= (1ull << 32)) return DVMVS_EUNSUPPORTED;
  hipLaunchKernelGGL(tsdf_raycast_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), tsdf_vol, weight_vol, color_vol, G, origin_x,
                     origin_y, origin_z, voxel_size, mask, cam_intr, cam_pose, im_h, im_w, near, far, step, static_cast<int>(steps), depth,
                     normal, rgb);
  return launch_status();
}
