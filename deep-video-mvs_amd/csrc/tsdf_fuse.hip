// TSDF fusion of a BATCH of RGB-D frames into a voxel volume in one launch (gfx950): what dvmvs_tsdf_integrate (tsdf.hip) does when it is
// called once per frame, for the use where depth maps arrive in a stream (dvmvs.tsdf.LiveFusion) -- DESIGN.md section 4.8d.
//
// Why the result is BIT-IDENTICAL to N dense launches.  tsdf_integrate_kernel updates a voxel from that voxel's own three values and the
// frame's images and matrices only: no voxel reads another voxel.  N launches in frame order therefore apply, to each voxel, a fixed sequence
// of float32 operations: frame 0's statements, then frame 1's on the values frame 0 left, and so on.  Here a thread OWNS its voxels for the
// whole launch: it loads tsdf / weight / colour once, applies the frames in index order 0..N-1 in registers with the dense kernel's
// statements copied one by one (contraction off, the same roundf / floorf / fminf, the same comparisons in the same order, the same
// colour mix), and stores once.  Memory is a place to keep a float between two launches; a register keeps the same float.  The world
// position of a voxel (origin + float(v) * voxel_size) does not depend on the frame and is evaluated once: the same two operations give the
// same float every time.  A voxel that no frame updates is not stored (the dense kernel does not store it either).
//
// Depth clamp: a depth > max_depth counts as 0 (prediction[prediction > max_depth] = 0 of dvmvs.tsdf.run); +inf switches it off and a NaN
// stays a NaN.  Colour comes folded (b * 65536 + g * 256 + r in a float, as the dense kernel takes it) or as 8-bit RGB that is folded
// here: three integers below 2^8 scaled by powers of two sum exactly in float32, which is fold_color's value.
//
// Culling.  The volume is cut into tiles of TX x TY x TZ voxels (z fastest in memory), one 256-thread workgroup per tile.  Lane f of the
// first wave decides, for frame f of the launch (at most 64), whether ANY voxel of the tile can pass the per-voxel tests of that frame
// (fuse_keep below, with the derivation of its margins); a ballot makes the frame bit-mask, LDS hands it to the other waves.  A tile
// with an empty mask returns before it touches the volume; any other tile loops over the set bits only.  The far plane needs the
// frame's largest depth after the clamp: tsdf_fuse_zmax_kernel writes it into the workspace first, on the same stream.
//
// No float atomics, no scratch; the only atomics are the two optional integer tile counters, added once per workgroup by one thread.
#include "dvmvs_device.h"

#include <math.h>
#include <stdlib.h>

namespace dvmvs {

constexpr int kFuseMaxFrames = 64;    // frames per launch: one bit of the mask each
constexpr int kFuseThreads = 256;
constexpr int kFuseZmaxParts = 8;     // partial maxima per frame in the workspace

// read-only for the whole launch and addressed wave-uniformly: constant address space, so the loads are scalar
typedef const float __attribute__((address_space(4)))* fuse_const_p;
typedef const unsigned char DVMVS_GLOBAL* fuse_u8_p;

struct FuseParams {
  float* tsdf;
  float* weight;
  float* color;
  int dim_x, dim_y, dim_z;
  int tiles_y, tiles_z;
  float origin_x, origin_y, origin_z, voxel_size;
  const float* cam_intr;          // [n,3,3] of this launch
  const float* cam_pose;          // [n,4,4]
  const unsigned char* rgb;       // [n,h,w,3] or NULL
  const float* folded;            // [n,h,w] or NULL
  const float* depth;             // [n,h,w]
  const float* zmax;              // [n,kFuseZmaxParts]
  int n_frames, im_h, im_w;
  float trunc_margin, max_depth;
  unsigned long long* stats;      // [2] or NULL
  float obs_weight[kFuseMaxFrames];
};

// Largest depth of a frame after the clamp, over the pixels that can update a voxel (depth != 0); -inf when there is none (the far plane
// then drops the frame everywhere) and +inf when a pixel is NaN or infinite (no far plane: the dense kernel integrates dist = 1 for a NaN
// depth, because every comparison with NaN is false).  blockIdx.y = frame, blockIdx.x = one of kFuseZmaxParts strided parts.
__global__ __launch_bounds__(kFuseThreads) void tsdf_fuse_zmax_kernel(const float* __restrict__ depth, long long pixels, float max_depth,
                                                                       float* __restrict__ zmax) {
  __shared__ float partial[kFuseThreads / kWave];
  const float* d = depth + static_cast<long long>(blockIdx.y) * pixels;
  float m = -INFINITY;
  for (long long i = static_cast<long long>(blockIdx.x) * kFuseThreads + threadIdx.x; i < pixels; i += kFuseZmaxParts * kFuseThreads) {
    float v = d[i];
    if (v > max_depth) v = 0.0f;
    if (v != 0.0f) {                                   // true for NaN
      if (!(fabsf(v) <= 3.402823466e+38f)) v = INFINITY;
      m = fmaxf(m, v);
    }
  }
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) partial[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = partial[0];
#pragma unroll
    for (int w = 1; w < kFuseThreads / kWave; ++w) r = fmaxf(r, partial[w]);
    zmax[blockIdx.y * kFuseZmaxParts + blockIdx.x] = r;
  }
}

// Can a voxel of the tile [v0, v0 + n) pass frame f's per-voxel tests?  Returns false only when it is PROVABLE that none can; every
// "drop" below is a comparison that is false for NaN, so a non-finite pose or intrinsic keeps the frame.  Evaluated in float64 from the
// float32 arguments: its own rounding (2^-53 per operation) is far inside the slack of the margins, which use eps = 2^-23, twice the
// unit round-off u = 2^-24 of the float32 operations they bound.
//
// Exact quantities.  With the float arguments taken as real numbers, voxel v has world position P_a = o_a + v_a s and camera coordinate
// k (x, y, z) X_k(v) = sum_a R[a][k] (P_a - t_a): LINEAR in v.  Over the tile's box of indices a linear function takes exactly the
// values centre +- sum_a |coefficient_a| h_a, h_a = (n_a - 1) s / 2 -- a tighter bound than a sphere around the tile.
//
// Per-voxel error E_k.  The kernel computes p = fl(o + fl(v s)), d = fl(p - t) (three roundings, every intermediate at most
// B_a = |o_a| + dim_a s + |t_a| in magnitude: |error of d_a| <= 3u(1 + u)^2 B_a) and x~_k = fl(fl(fl(R0 d0) + fl(R1 d1)) + fl(R2 d2))
// (three products, two sums: <= 3u(1 + 3u) sum_a |R_a| |d_a|), so |x~_k - X_k| <= 6.01 u sum_a |R[a][k]| B_a.  E_k takes 8 eps = 16 u
// of that sum, plus 1e-37 for products that underflow.  (If an intermediate overflows, the voxel fails its tests whatever we decide.)
//
// Tests a voxel must pass, and what each implies for the exact coordinates:
//  * not (z~ < 0)                       =>  Z >= -E_z.                    Behind: drop when  max Z < -E_z.
//  * not (fl(d - z~) < -trunc), d the pixel's finite, non-zero depth: fl(d - z~) = (d - z~)(1 + delta)  =>  z~ <= d + trunc (1 + 2u)
//                                       =>  Z <= zmax + trunc (1 + 2u) + E_z.   Far: drop when  min Z - E_z > zmax + trunc (1 + 4 eps).
//    There is no near plane: a voxel in front of the surface is updated with dist = 1.
//  * round(u~) in [0, W): roundf rounds halves away from zero, so -0.5 <= u~ <= W - 0.5, where u~ = fl(fl(fx fl(x~ / z~)) + cx).  z~ = 0
//    gives inf or NaN, which fails, so z~ > 0.  Undoing the three roundings, with S = W + |cx| + 1 >= |fl(fx q)|:
//    -0.5 - cx - mu <= fx x~ / z~ <= W - 0.5 - cx + mu, mu = 2uW + 2.01uS <= 4.01 u S; mu takes 6 eps S plus (|fx| + 1) 1e-37 for a quotient or
//    product that underflows.  Times z~ > 0 and with x~ = X + e_x, z~ = Z + e_z:
//        fx X - a_hi Z <= |fx| E_x + |a_hi| E_z,  a_hi = W - 0.5 - cx + mu      Right: drop when the minimum over the tile exceeds that.
//        fx X - a_lo Z >= -(|fx| E_x + |a_lo| E_z),  a_lo = -0.5 - cx - mu       Left: drop when the maximum is below that.
//    Both left sides are linear in v again, so their extrema over the tile are centre -+ sum_a |fx R[a][x] - a R[a][z]| h_a.  The same
//    holds for v~ with fy, cy, H and the y row.  The implication only needs z~ > 0 of the voxel that passes, not of the tile; still the
//    side planes are applied only to a tile that lies wholly in front of the camera (min Z > E_z): one that the plane cam_z = 0 cuts
//    is never dropped by a side plane.
__device__ inline bool fuse_keep(const FuseParams& p, int f, int x0, int y0, int z0, int nx, int ny, int nz) {
  const double eps = 1.1920928955078125e-07;   // 2^-23
  const gcfloat_p Kf = as_global(p.cam_intr) + 9 * f;
  const gcfloat_p Pf = as_global(p.cam_pose) + 16 * f;
  const gcfloat_p zparts = as_global(p.zmax) + f * kFuseZmaxParts;
  const double fx = Kf[0], cx = Kf[2], fy = Kf[4], cy = Kf[5];
  double zmax = -INFINITY;
#pragma unroll
  for (int i = 0; i < kFuseZmaxParts; ++i) zmax = fmax(zmax, static_cast<double>(zparts[i]));   // never NaN
  const double s = p.voxel_size;
  const double o[3] = {p.origin_x, p.origin_y, p.origin_z};
  const int v0[3] = {x0, y0, z0}, n[3] = {nx, ny, nz}, dims[3] = {p.dim_x, p.dim_y, p.dim_z};
  double R[3][3], c[3], h[3], B[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double t = Pf[4 * a + 3];
    h[a] = 0.5 * static_cast<double>(n[a] - 1) * s;
    c[a] = (o[a] + static_cast<double>(v0[a]) * s + h[a]) - t;
    B[a] = fabs(o[a]) + static_cast<double>(dims[a]) * s + fabs(t);
#pragma unroll
    for (int k = 0; k < 3; ++k) R[a][k] = Pf[4 * a + k];
  }
  double C[3], H[3], E[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    C[k] = R[0][k] * c[0] + R[1][k] * c[1] + R[2][k] * c[2];
    H[k] = fabs(R[0][k]) * h[0] + fabs(R[1][k]) * h[1] + fabs(R[2][k]) * h[2];
    E[k] = 8.0 * eps * (fabs(R[0][k]) * B[0] + fabs(R[1][k]) * B[1] + fabs(R[2][k]) * B[2]) + 1e-37;
  }
  if (C[2] + H[2] < -E[2]) return false;                                                                  // behind the camera
  if (C[2] - H[2] - E[2] > zmax + static_cast<double>(p.trunc_margin) * (1.0 + 4.0 * eps)) return false;   // beyond zmax + truncation
  if (C[2] - H[2] > E[2]) {   // wholly in front: the four image sides
    const double focal[2] = {fx, fy}, centre[2] = {cx, cy}, size[2] = {static_cast<double>(p.im_w), static_cast<double>(p.im_h)};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double S = size[k] + fabs(centre[k]) + 1.0;
      const double mu = 6.0 * eps * S + (fabs(focal[k]) + 1.0) * 1e-37;
      const double a_hi = size[k] - 0.5 - centre[k] + mu, a_lo = -0.5 - centre[k] - mu;
      const double hi_c = focal[k] * C[k] - a_hi * C[2], lo_c = focal[k] * C[k] - a_lo * C[2];
      const double hi_h = fabs(focal[k] * R[0][k] - a_hi * R[0][2]) * h[0] + fabs(focal[k] * R[1][k] - a_hi * R[1][2]) * h[1] +
                          fabs(focal[k] * R[2][k] - a_hi * R[2][2]) * h[2];
      const double lo_h = fabs(focal[k] * R[0][k] - a_lo * R[0][2]) * h[0] + fabs(focal[k] * R[1][k] - a_lo * R[1][2]) * h[1] +
                          fabs(focal[k] * R[2][k] - a_lo * R[2][2]) * h[2];
      if (hi_c - hi_h > fabs(focal[k]) * E[k] + fabs(a_hi) * E[2]) return false;       // past the right / bottom side
      if (lo_c + lo_h < -(fabs(focal[k]) * E[k] + fabs(a_lo) * E[2])) return false;    // past the left / top side
    }
  }
  return true;
}

#pragma clang fp contract(off)
template <int TX, int TY, int TZ>
__global__ __launch_bounds__(kFuseThreads) void tsdf_fuse_kernel(const FuseParams p) {
  constexpr int VPT = TX * TY * TZ / kFuseThreads;   // voxels a thread owns
  static_assert(TX * TY * TZ % kFuseThreads == 0 && VPT >= 1, "a tile is a whole number of voxels per thread");
  __shared__ unsigned long long s_mask;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int bz = b % p.tiles_z, by = (b / p.tiles_z) % p.tiles_y, bx = b / (p.tiles_z * p.tiles_y);
  const int x0 = bx * TX, y0 = by * TY, z0 = bz * TZ;

  if (tid < kWave) {
    bool keep = false;
    if (tid < p.n_frames) keep = fuse_keep(p, tid, x0, y0, z0, min(TX, p.dim_x - x0), min(TY, p.dim_y - y0), min(TZ, p.dim_z - z0));
    const unsigned long long kept = __ballot(keep);
    if (tid == 0) {
      s_mask = kept;
      if (p.stats) {
        if (kept) {
          atomicAdd(p.stats, static_cast<unsigned long long>(__popcll(kept)));   // (tile, frame) pairs kept
          atomicAdd(p.stats + 1, 1ull);                                          // tiles that load the volume
        }
      }
    }
  }
  __syncthreads();
  const unsigned long long shared_mask = s_mask;
  unsigned long long mask = (static_cast<unsigned long long>(__builtin_amdgcn_readfirstlane(static_cast<int>(shared_mask >> 32))) << 32) |
                            static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(shared_mask & 0xffffffffull)));
  if (mask == 0ull) return;   // no frame of the batch can touch this tile: no volume access

  const gfloat_p tsdf_vol = as_global(p.tsdf), weight_vol = as_global(p.weight), color_vol = as_global(p.color);
  float tsdf[VPT], weight[VPT], color[VPT], wx[VPT], wy[VPT], wz[VPT];
  long long idx[VPT];
  bool valid[VPT], touched[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int local = j * kFuseThreads + tid;
    const int vz = z0 + local % TZ, vy = y0 + (local / TZ) % TY, vx = x0 + local / (TZ * TY);
    valid[j] = vx < p.dim_x && vy < p.dim_y && vz < p.dim_z;
    touched[j] = false;
    idx[j] = (static_cast<long long>(vx) * p.dim_y + vy) * p.dim_z + vz;
    wx[j] = p.origin_x + static_cast<float>(vx) * p.voxel_size;
    wy[j] = p.origin_y + static_cast<float>(vy) * p.voxel_size;
    wz[j] = p.origin_z + static_cast<float>(vz) * p.voxel_size;
    tsdf[j] = weight[j] = color[j] = 0.0f;
    if (valid[j]) {
      tsdf[j] = tsdf_vol[idx[j]];
      weight[j] = weight_vol[idx[j]];
      color[j] = color_vol[idx[j]];
    }
  }

  const long long pixels = static_cast<long long>(p.im_h) * p.im_w;
  while (mask != 0ull) {
    const int f = __builtin_ctzll(mask);   // wave-uniform: the matrices below come through scalar loads
    mask &= mask - 1ull;
    const fuse_const_p Kf = (fuse_const_p)p.cam_intr + 9 * f;
    const fuse_const_p Pf = (fuse_const_p)p.cam_pose + 16 * f;
    const float fx = Kf[0], cx = Kf[2], fy = Kf[4], cy = Kf[5];
    float R[9], t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) R[r * 3 + c] = Pf[r * 4 + c];
      t[r] = Pf[r * 4 + 3];
    }
    const float obs_weight = p.obs_weight[f];
    const gcfloat_p depth_im = as_global(p.depth) + f * pixels;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      if (!valid[j]) continue;
      // tsdf_integrate_kernel, statement by statement
      const float tx = wx[j] - t[0];
      const float ty = wy[j] - t[1];
      const float tz = wz[j] - t[2];
      const float cam_x = R[0] * tx + R[3] * ty + R[6] * tz;
      const float cam_y = R[1] * tx + R[4] * ty + R[7] * tz;
      const float cam_z = R[2] * tx + R[5] * ty + R[8] * tz;
      const float u = roundf(fx * (cam_x / cam_z) + cx), v = roundf(fy * (cam_y / cam_z) + cy);
      if (!(u >= 0.0f && u < static_cast<float>(p.im_w) && v >= 0.0f && v < static_cast<float>(p.im_h)) || cam_z < 0.0f) continue;
      const int pixel = static_cast<int>(v) * p.im_w + static_cast<int>(u);
      float depth_value = depth_im[pixel];
      if (depth_value > p.max_depth) depth_value = 0.0f;
      if (depth_value == 0.0f) continue;
      const float depth_diff = depth_value - cam_z;
      if (depth_diff < -p.trunc_margin) continue;
      const float dist = fminf(1.0f, depth_diff / p.trunc_margin);
      const float w_old = weight[j];
      const float w_new = w_old + obs_weight;
      weight[j] = w_new;
      tsdf[j] = (tsdf[j] * w_old + obs_weight * dist) / w_new;
      const float old_color = color[j];
      const float old_b = floorf(old_color / 65536.0f);
      const float old_g = floorf((old_color - old_b * 65536.0f) / 256.0f);
      const float old_r = old_color - old_b * 65536.0f - old_g * 256.0f;
      float new_color;
      if (p.rgb) {
        const fuse_u8_p c8 = (fuse_u8_p)p.rgb + 3 * (f * pixels + pixel);
        new_color = static_cast<float>(c8[2]) * 65536.0f + static_cast<float>(c8[1]) * 256.0f + static_cast<float>(c8[0]);   // exact
      } else {
        new_color = as_global(p.folded)[f * pixels + pixel];
      }
      float new_b = floorf(new_color / 65536.0f);
      float new_g = floorf((new_color - new_b * 65536.0f) / 256.0f);
      float new_r = new_color - new_b * 65536.0f - new_g * 256.0f;
      new_b = fminf(roundf((old_b * w_old + obs_weight * new_b) / w_new), 255.0f);
      new_g = fminf(roundf((old_g * w_old + obs_weight * new_g) / w_new), 255.0f);
      new_r = fminf(roundf((old_r * w_old + obs_weight * new_r) / w_new), 255.0f);
      color[j] = new_b * 65536.0f + new_g * 256.0f + new_r;
      touched[j] = true;
    }
  }

#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    if (touched[j]) {
      weight_vol[idx[j]] = weight[j];
      tsdf_vol[idx[j]] = tsdf[j];
      color_vol[idx[j]] = color[j];
    }
  }
}
#pragma clang fp contract(fast)

// The tile: 4 x 4 x 32 voxels, the fastest of the six shapes measured (tools/tsdf_fuse_bench.py, profiles/tsdf_fuse_bench.json): 128-byte
// runs along z and a tight bound.  dvmvs.hip.ops.TSDF_FUSE_TILE states the same three numbers (tests/test_tsdf_fuse.py compares them).
constexpr int kFuseTX = 4, kFuseTY = 4, kFuseTZ = 32;

struct FuseTile {
  int tx, ty, tz;
  void (*kernel)(const FuseParams);
};
#ifdef DVMVS_TSDF_FUSE_TUNING
// Tools-only build (`make tuning`, not the product): every shape that was measured, the product's first.  The environment variable
// DVMVS_TSDF_FUSE_TILE picks one by number and dvmvs_tsdf_fuse_tuning_tiles lists them, for tools/tsdf_fuse_bench.py; every shape gives
// the same bits.
static const FuseTile kFuseTiles[] = {
    {kFuseTX, kFuseTY, kFuseTZ, tsdf_fuse_kernel<kFuseTX, kFuseTY, kFuseTZ>}, {8, 8, 8, tsdf_fuse_kernel<8, 8, 8>},
    {2, 2, 64, tsdf_fuse_kernel<2, 2, 64>},                                   {4, 4, 16, tsdf_fuse_kernel<4, 4, 16>},
    {2, 4, 32, tsdf_fuse_kernel<2, 4, 32>},                                   {8, 8, 16, tsdf_fuse_kernel<8, 8, 16>},
};
constexpr int kFuseTileCount = static_cast<int>(sizeof(kFuseTiles) / sizeof(kFuseTiles[0]));
static const FuseTile* fuse_tile() {
  int choice = 0;
  if (const char* env = getenv("DVMVS_TSDF_FUSE_TILE")) choice = atoi(env);
  return choice >= 0 && choice < kFuseTileCount ? &kFuseTiles[choice] : nullptr;
}
#else
static const FuseTile kFuseTileInUse = {kFuseTX, kFuseTY, kFuseTZ, tsdf_fuse_kernel<kFuseTX, kFuseTY, kFuseTZ>};
static const FuseTile* fuse_tile() { return &kFuseTileInUse; }
#endif

}  // namespace dvmvs

extern "C" size_t dvmvs_tsdf_integrate_frames_workspace_bytes(int n_frames) {
  if (n_frames <= 0) return 0;
  return static_cast<size_t>(n_frames) * dvmvs::kFuseZmaxParts * sizeof(float);
}

extern "C" int dvmvs_tsdf_integrate_frames(float* tsdf_vol, float* weight_vol, float* color_vol, int dim_x, int dim_y, int dim_z, float origin_x,
                                           float origin_y, float origin_z, float voxel_size, const float* cam_intr, const float* cam_pose,
                                           const unsigned char* rgb_u8, const float* folded, const float* depth, int n_frames, int im_h,
                                           int im_w, float trunc_margin, const float* obs_weight_host, float max_depth, void* workspace,
                                           long long* tile_stats, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!tsdf_vol || !weight_vol || !color_vol || !cam_intr || !cam_pose || !depth || !obs_weight_host || !workspace) return DVMVS_EINVAL;
  if ((rgb_u8 != nullptr) == (folded != nullptr)) return DVMVS_EINVAL;   // exactly one colour form
  if (dim_x <= 0 || dim_y <= 0 || dim_z <= 0 || im_h <= 0 || im_w <= 0 || n_frames <= 0) return DVMVS_EINVAL;
  if (!(voxel_size > 0.0f) || !(trunc_margin > 0.0f) || max_depth != max_depth) return DVMVS_EINVAL;
  if (static_cast<long long>(dim_y) * dim_z >= (1LL << 31) || static_cast<long long>(im_h) * im_w >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  if (n_frames > 65535) return DVMVS_EUNSUPPORTED;   // one grid row of the reduction per frame
  const FuseTile* chosen = fuse_tile();
  if (!chosen) return DVMVS_EINVAL;
  const FuseTile& tile = *chosen;
  const long long tiles_x = (dim_x + tile.tx - 1) / tile.tx, tiles_y = (dim_y + tile.ty - 1) / tile.ty, tiles_z = (dim_z + tile.tz - 1) / tile.tz;
  if (tiles_y * tiles_z >= (1LL << 31) || tiles_x * tiles_y * tiles_z >= (1LL << 31)) return DVMVS_EUNSUPPORTED;   // a 1-D grid of tiles
  const long long pixels = static_cast<long long>(im_h) * im_w;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* zmax = static_cast<float*>(workspace);
  hipLaunchKernelGGL(tsdf_fuse_zmax_kernel, dim3(kFuseZmaxParts, static_cast<unsigned>(n_frames)), dim3(kFuseThreads), 0, s, depth, pixels,
                     max_depth, zmax);
  int rc = launch_status();
  if (rc != 0) return rc;
  FuseParams p;
  p.tsdf = tsdf_vol;
  p.weight = weight_vol;
  p.color = color_vol;
  p.dim_x = dim_x;
  p.dim_y = dim_y;
  p.dim_z = dim_z;
  p.tiles_y = static_cast<int>(tiles_y);
  p.tiles_z = static_cast<int>(tiles_z);
  p.origin_x = origin_x;
  p.origin_y = origin_y;
  p.origin_z = origin_z;
  p.voxel_size = voxel_size;
  p.im_h = im_h;
  p.im_w = im_w;
  p.trunc_margin = trunc_margin;
  p.max_depth = max_depth;
  p.stats = reinterpret_cast<unsigned long long*>(tile_stats);
  // more than 64 frames: consecutive launches in frame order (each voxel still sees the frames in index order)
  for (int first = 0; first < n_frames; first += kFuseMaxFrames) {
    const int n = n_frames - first < kFuseMaxFrames ? n_frames - first : kFuseMaxFrames;
    p.cam_intr = cam_intr + 9LL * first;
    p.cam_pose = cam_pose + 16LL * first;
    p.rgb = rgb_u8 ? rgb_u8 + 3LL * first * pixels : nullptr;
    p.folded = folded ? folded + first * pixels : nullptr;
    p.depth = depth + first * pixels;
    p.zmax = zmax + static_cast<long long>(first) * kFuseZmaxParts;
    p.n_frames = n;
    for (int i = 0; i < kFuseMaxFrames; ++i) p.obs_weight[i] = i < n ? obs_weight_host[first + i] : 0.0f;
    hipLaunchKernelGGL(tile.kernel, dim3(static_cast<unsigned>(tiles_x * tiles_y * tiles_z)), dim3(kFuseThreads), 0, s, p);
    rc = launch_status();
    if (rc != 0) return rc;
  }
  return 0;
}

#ifdef DVMVS_TSDF_FUSE_TUNING
// tools-only: writes up to `capacity` shapes as x, y, z triples into `xyz`, in the order DVMVS_TSDF_FUSE_TILE numbers them; returns their number
extern "C" int dvmvs_tsdf_fuse_tuning_tiles(int* xyz, int capacity) {
  using namespace dvmvs;
  for (int i = 0; i < kFuseTileCount && i < capacity; ++i) {
    xyz[3 * i] = kFuseTiles[i].tx;
    xyz[3 * i + 1] = kFuseTiles[i].ty;
    xyz[3 * i + 2] = kFuseTiles[i].tz;
  }
  return kFuseTileCount;
}
#endif
