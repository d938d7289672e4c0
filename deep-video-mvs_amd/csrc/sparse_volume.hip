// A TSDF volume that needs no bounds (gfx950): space is the unbounded lattice of 8 x 8 x 8-voxel bricks of sparse_grid.h, a hash table
// maps brick keys to existence and birth, a pool of fixed capacity holds the voxels of the allocated bricks -- DESIGN.md section 4.8r,
// contract in include/dvmvs_hip.h, host definition of the marking in dvmvs/sparse.py.
//
// One flush of N frames is four steps on one stream, nothing read by the host:
//   mark       one pixel per lane over the N frames: the bricks its truncation band can touch go into the table (compare-and-swap on the
//              64-bit key; a slot is READ before it is swapped, so the common case -- the brick exists -- is one load), the brick's birth
//              becomes the smallest frame number that marks it (integer atomicMin, after a read that usually makes it unnecessary), and the
//              key of every brick this flush inserted is appended to a scratch list.
//   sort       the scratch list (filled with the empty key behind its entries), by the caller: any device sort, no host read.
//   assign     rank r of the sorted list -> pool slot n_bricks + r, in ascending key order whatever the schedule did to the table; ranks at or
//              beyond the capacity are dropped and counted; then one thread commits the new n_bricks.
//   integrate  one workgroup per pool slot, z fastest: the voxels of a brick in registers, the frames in index order with the statements of
//              tsdf_integrate_kernel / tsdf_fuse.hip copied one by one, one load and one store per voxel; frame g is applied iff
//              g >= birth.  Workgroups of slots >= n_bricks (read from the device) return at once.  There is no per-brick frame cull: a
//              brick is 512 voxels, two per lane, and a frame costs a brick that it misses one projection per voxel (measured as part of
//              the integrate time in profiles/sparse_fuse_bench.json, not separately).
//
// Margin of the marking.  A voxel that frame f gives a tsdf < 1 projects (roundf) to a pixel (u, v) with depth d and has camera depth
// Z in (d - trunc, d + trunc], Z >= 0.  The pixel's ray is sampled at depths z_i, delta apart, from max(d - trunc, 0) to d + trunc, so some
// |Z - z_i| <= delta / 2.  With a = (u - cx) / fx, b = (v - cy) / fy the voxel's camera position (X, Y, Z) has |X / Z - a| <= 0.5 / fx
// and |Y / Z - b| <= 0.5 / fy, so (X, Y, Z) - z_i (a, b, 1) = (X - a Z, Y - b Z, 0) + (Z - z_i)(a, b, 1) is at most
// 0.5 Z sqrt(1/fx^2 + 1/fy^2) + (delta / 2) sqrt(1 + a^2 + b^2) long, with Z <= z_i + delta / 2; a rigid pose keeps lengths, and the
// axis-aligned box sample +- m contains the ball of radius m.
// Slack for float32 (u = 2^-24), in the manner of fuse_keep: every float the dense kernel forms on the way from a voxel index to its
// camera position, and every float formed here on the way from a pixel to a brick index, is at most 2 W in magnitude,
// W = sum |origin| + sum |t| + z1 (1 + |a| + |b|); each chain has fewer than 10 roundings, so the two positions are each within 20 u W of
// their exact values, the quotient by the brick size adds 2 u W, the truncation test's own rounding 2 u trunc <= 2 u W: 64 u W = 2^-18 W
// covers them with room.  The projection u~ = fl(fl(fx fl(x / z)) + cx) is within 4.01 u (w + |cx| + 1) of exact, under 2^-9 pixel for
// images up to 8192 wide, so "half a pixel" is taken as 0.5 (1 + 2^-8).  1e-4 voxel is added on top.
//
// Atomics: compare-and-swap and add on 64-bit integers, min on 32-bit integers, all vector atomics on global memory; no float atomics.
#include "dvmvs_device.h"
#include "sparse_grid.h"

#include <math.h>

namespace dvmvs {

constexpr int kSparseThreads = 256;
constexpr int kSparseMaxFrames = 64;     // frames per integrate launch (their weights travel by value)
constexpr int kMarkMaxIntervals = 16;
constexpr int kMarkMaxSpan = 4;
// status words (int64): bricks allocated; bricks dropped because the pool was full; marks dropped because the table was full; pixels that
// marked nothing (range or span); keys the current flush inserted (zero between flushes)
enum { kStatBricks = 0, kStatDroppedPool = 1, kStatDroppedTable = 2, kStatRejected = 3, kStatFresh = 4, kStatWords = 8 };

typedef const float __attribute__((address_space(4)))* sparse_const_p;
typedef const unsigned char DVMVS_GLOBAL* sparse_u8_p;

struct MarkParams {
  long long* table_keys;
  int* table_birth;
  long long table_slots;   // a power of two
  long long* fresh;        // [table_slots]
  unsigned long long* status;
  const float* depth;      // [n,h,w]
  const float* cam_intr;   // [n,3,3]
  const float* cam_pose;   // [n,4,4]
  long long total;         // n * h * w
  int im_h, im_w;
  float origin[3];
  float voxel_size, trunc, max_depth;
  int first_frame;
};

// Puts `key` into the table unless it is there, and lowers its birth to g.  At most table_slots attempts.
__device__ inline void mark_brick(const MarkParams& p, long long key, int g) {
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(p.table_keys);
  const uint64_t mask = static_cast<uint64_t>(p.table_slots) - 1;
  const uint64_t hash = sg_hash(key);
  const unsigned long long want = static_cast<unsigned long long>(key), empty = static_cast<unsigned long long>(kBrickEmpty);
  for (uint64_t i = 0; i <= mask; ++i) {
    const uint64_t slot = sg_probe(hash, i, mask);
    unsigned long long cur = __atomic_load_n(keys + slot, __ATOMIC_RELAXED);
    if (cur == empty) {
      cur = atomicCAS(keys + slot, empty, want);
      if (cur == empty) {            // this lane inserted the key
        const unsigned long long n = atomicAdd(p.status + kStatFresh, 1ull);
        if (n < static_cast<unsigned long long>(p.table_slots)) p.fresh[n] = key;   // (always: every insert takes a table slot of its own)
        cur = want;
      }
    }
    if (cur == want) {
      if (__atomic_load_n(p.table_birth + slot, __ATOMIC_RELAXED) > g) atomicMin(p.table_birth + slot, g);
      return;
    }
  }
  atomicAdd(p.status + kStatDroppedTable, 1ull);
}

#pragma clang fp contract(off)
// dvmvs/sparse.py::mark_bricks, operation by operation
__global__ __launch_bounds__(kSparseThreads) void sparse_mark_kernel(const MarkParams p) {
  const long long idx = static_cast<long long>(blockIdx.x) * kSparseThreads + threadIdx.x;
  if (idx >= p.total) return;
  const long long pixels = static_cast<long long>(p.im_h) * p.im_w;
  const int f = static_cast<int>(idx / pixels);
  const int pix = static_cast<int>(idx - f * pixels);
  const int pv = pix / p.im_w, pu = pix - pv * p.im_w;
  float d = as_global(p.depth)[idx];
  if (d > p.max_depth) d = 0.0f;
  if (!(d > 0.0f && d <= 3.402823466e+38f)) return;
  const gcfloat_p Kf = as_global(p.cam_intr) + 9 * f;
  const gcfloat_p Pf = as_global(p.cam_pose) + 16 * f;
  const float fx = Kf[0], cx = Kf[2], fy = Kf[4], cy = Kf[5];
  const float s = p.voxel_size;
  const float z0 = fmaxf(d - p.trunc, 0.0f);
  const float z1 = d + p.trunc;
  const float span = z1 - z0;
  const float kf = fminf(fmaxf(ceilf(span / (2.0f * s)), 1.0f), static_cast<float>(kMarkMaxIntervals));
  const float delta = span / kf;
  const int k = static_cast<int>(kf);
  const float a = (static_cast<float>(pu) - cx) / fx;
  const float b = (static_cast<float>(pv) - cy) / fy;
  const float ifx = 1.0f / fx, ify = 1.0f / fy;
  const float r_pix = sqrtf(ifx * ifx + ify * ify);
  const float r_ray = sqrtf((1.0f + a * a) + b * b);
  const float hd = 0.5f * delta;
  float R[9], t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = Pf[r * 4 + c];
    t[r] = Pf[r * 4 + 3];
  }
  const float W = (((fabsf(p.origin[0]) + fabsf(p.origin[1])) + fabsf(p.origin[2])) + ((fabsf(t[0]) + fabsf(t[1])) + fabsf(t[2]))) +
                  z1 * ((1.0f + fabsf(a)) + fabsf(b));
  const float slack = 1e-4f * s + 3.814697265625e-06f * W;   // 2^-18
  const float brick = 8.0f * s;
  const int g = p.first_frame + f;
  long long last = kBrickEmpty;
  // pass 0 checks every sample (a pixel with one bad sample marks nothing), pass 1 marks
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = 0; i <= k; ++i) {
      const float z = z0 + static_cast<float>(i) * delta;
      const float m = ((0.501953125f * (z + hd)) * r_pix + hd * r_ray) + slack;
      const float x = a * z, y = b * z;
      int lo[3], hi[3];
      bool ok = true;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float S = ((R[c * 3] * x + R[c * 3 + 1] * y) + R[c * 3 + 2] * z) + t[c];
        const float qlo = floorf(((S - m) - p.origin[c]) / brick);
        const float qhi = floorf(((S + m) - p.origin[c]) / brick);
        const bool in = qlo >= -static_cast<float>(kBrickLimit) && qhi <= static_cast<float>(kBrickLimit) &&
                        qhi - qlo <= static_cast<float>(kMarkMaxSpan - 1);   // false for NaN
        ok = ok && in;
        lo[c] = in ? static_cast<int>(qlo) : 0;
        hi[c] = in ? static_cast<int>(qhi) : 0;
      }
      if (pass == 0) {
        if (!ok) {
          atomicAdd(p.status + kStatRejected, 1ull);
          return;
        }
        continue;
      }
      for (int bx = lo[0]; bx <= hi[0]; ++bx)
        for (int by = lo[1]; by <= hi[1]; ++by)
          for (int bz = lo[2]; bz <= hi[2]; ++bz) {
            const long long key = sg_pack(bx, by, bz);
            if (key == last) continue;    // consecutive samples mostly stay in one brick
            last = key;
            mark_brick(p, key, g);
          }
    }
  }
}
#pragma clang fp contract(fast)

// rank r of the sorted fresh keys -> pool slot n_bricks + r; the scratch list is refilled with the empty key for the next flush
__global__ __launch_bounds__(kSparseThreads) void sparse_assign_kernel(const long long* __restrict__ table_keys, const int* __restrict__ table_birth,
                                                                       long long table_slots, const long long* __restrict__ sorted,
                                                                       long long* __restrict__ fresh, const unsigned long long* __restrict__ status,
                                                                       long long* __restrict__ pool_key, int* __restrict__ pool_birth,
                                                                       long long max_bricks) {
  const long long r = static_cast<long long>(blockIdx.x) * kSparseThreads + threadIdx.x;
  if (r >= table_slots) return;
  fresh[r] = kBrickEmpty;
  const long long key = sorted[r];
  if (key == kBrickEmpty) return;
  const long long slot = static_cast<long long>(status[kStatBricks]) + r;
  if (slot >= max_bricks) return;          // dropped; counted by the commit
  const uint64_t mask = static_cast<uint64_t>(table_slots) - 1;
  const uint64_t hash = sg_hash(key);
  int birth = 0x7fffffff;
  for (uint64_t i = 0; i <= mask; ++i) {
    const uint64_t at = sg_probe(hash, i, mask);
    const long long cur = table_keys[at];
    if (cur == key) {
      birth = table_birth[at];
      break;
    }
    if (cur == kBrickEmpty) break;         // (cannot happen: the key was inserted)
  }
  pool_key[slot] = key;
  pool_birth[slot] = birth;
}

__global__ void sparse_commit_kernel(unsigned long long* status, long long table_slots, long long max_bricks) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long old = static_cast<long long>(status[kStatBricks]);
  long long fresh = static_cast<long long>(status[kStatFresh]);
  if (fresh > table_slots) fresh = table_slots;
  long long now = old + fresh;
  if (now > max_bricks) now = max_bricks;
  status[kStatDroppedPool] += static_cast<unsigned long long>(old + fresh - now);
  status[kStatBricks] = static_cast<unsigned long long>(now);
  status[kStatFresh] = 0ull;
}

struct SparseFuseParams {
  float* tsdf;
  float* weight;
  float* color;
  const long long* pool_key;
  const int* pool_birth;
  const unsigned long long* status;
  float origin_x, origin_y, origin_z, voxel_size;
  const float* cam_intr;
  const float* cam_pose;
  const unsigned char* rgb;
  const float* folded;
  const float* depth;
  int n_frames, im_h, im_w, first_frame;
  float trunc_margin, max_depth;
  float obs_weight[kSparseMaxFrames];
};

#pragma clang fp contract(off)
__global__ __launch_bounds__(kSparseThreads) void sparse_integrate_kernel(const SparseFuseParams p) {
  constexpr int VPT = kBrickVoxels / kSparseThreads;
  const long long slot = blockIdx.x;
  if (slot >= static_cast<long long>(p.status[kStatBricks])) return;
  const int tid = threadIdx.x;
  int bx, by, bz;
  sg_unpack(p.pool_key[slot], bx, by, bz);
  const int birth = p.pool_birth[slot];
  const gfloat_p tsdf_vol = as_global(p.tsdf) + slot * kBrickVoxels, weight_vol = as_global(p.weight) + slot * kBrickVoxels,
                 color_vol = as_global(p.color) + slot * kBrickVoxels;
  float tsdf[VPT], weight[VPT], color[VPT], wx[VPT], wy[VPT], wz[VPT];
  bool touched[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int local = j * kSparseThreads + tid;      // x * 64 + y * 8 + z
    const int vx = bx * kBrick + (local >> 6), vy = by * kBrick + ((local >> 3) & 7), vz = bz * kBrick + (local & 7);
    wx[j] = p.origin_x + static_cast<float>(vx) * p.voxel_size;
    wy[j] = p.origin_y + static_cast<float>(vy) * p.voxel_size;
    wz[j] = p.origin_z + static_cast<float>(vz) * p.voxel_size;
    tsdf[j] = tsdf_vol[local];
    weight[j] = weight_vol[local];
    color[j] = color_vol[local];
    touched[j] = false;
  }
  const long long pixels = static_cast<long long>(p.im_h) * p.im_w;
  for (int f = 0; f < p.n_frames; ++f) {
    if (p.first_frame + f < birth) continue;        // the birth rule (wave-uniform)
    const sparse_const_p Kf = (sparse_const_p)p.cam_intr + 9 * f;
    const sparse_const_p Pf = (sparse_const_p)p.cam_pose + 16 * f;
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
        const sparse_u8_p c8 = (sparse_u8_p)p.rgb + 3 * (f * pixels + pixel);
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
      const int local = j * kSparseThreads + tid;
      weight_vol[local] = weight[j];
      tsdf_vol[local] = tsdf[j];
      color_vol[local] = color[j];
    }
  }
}
#pragma clang fp contract(fast)

// pool slot -> its place in dense [X,Y,Z] arrays whose voxel (0,0,0) is the first voxel of brick (b0x, b0y, b0z); bricks outside stay out
__global__ __launch_bounds__(kSparseThreads) void sparse_gather_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                       const float* __restrict__ color, const long long* __restrict__ pool_key,
                                                                       float* __restrict__ out_tsdf, float* __restrict__ out_weight,
                                                                       float* __restrict__ out_color, int bricks_x, int bricks_y, int bricks_z,
                                                                       int b0x, int b0y, int b0z) {
  const long long slot = blockIdx.x;
  int bx, by, bz;
  sg_unpack(pool_key[slot], bx, by, bz);
  const long long rx = static_cast<long long>(bx) - b0x, ry = static_cast<long long>(by) - b0y, rz = static_cast<long long>(bz) - b0z;
  if (rx < 0 || rx >= bricks_x || ry < 0 || ry >= bricks_y || rz < 0 || rz >= bricks_z) return;
  const long long Y = static_cast<long long>(bricks_y) * kBrick, Z = static_cast<long long>(bricks_z) * kBrick;
#pragma unroll
  for (int j = 0; j < kBrickVoxels / kSparseThreads; ++j) {
    const int local = j * kSparseThreads + threadIdx.x;
    const long long x = rx * kBrick + (local >> 6), y = ry * kBrick + ((local >> 3) & 7), z = rz * kBrick + (local & 7);
    const long long at = (x * Y + y) * Z + z;
    const long long from = slot * kBrickVoxels + local;
    out_tsdf[at] = tsdf[from];
    out_weight[at] = weight[from];
    out_color[at] = color[from];
  }
}

static bool power_of_two(long long n) { return n > 0 && (n & (n - 1)) == 0; }
static bool finite3(float a, float b, float c) { return a - a == 0.0f && b - b == 0.0f && c - c == 0.0f; }

}  // namespace dvmvs

extern "C" int dvmvs_sparse_mark(long long* table_keys, int* table_birth, long long table_slots, long long* fresh, long long* status,
                                 const float* depth, const float* cam_intr, const float* cam_pose, int n_frames, int im_h, int im_w,
                                 float origin_x, float origin_y, float origin_z, float voxel_size, float trunc_margin, float max_depth,
                                 int first_frame, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!table_keys || !table_birth || !fresh || !status || !depth || !cam_intr || !cam_pose) return DVMVS_EINVAL;
  if (!power_of_two(table_slots) || n_frames <= 0 || im_h <= 0 || im_w <= 0 || first_frame < 0) return DVMVS_EINVAL;
  if (!(voxel_size > 0.0f) || !(trunc_margin > 0.0f) || max_depth != max_depth || !finite3(origin_x, origin_y, origin_z) ||
      !finite3(voxel_size, trunc_margin, 0.0f))
    return DVMVS_EINVAL;
  const long long pixels = static_cast<long long>(im_h) * im_w;
  if (pixels >= (1LL << 31) || table_slots > (1LL << 30) || static_cast<long long>(first_frame) + n_frames >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  const long long total = pixels * n_frames;
  const long long groups = (total + kSparseThreads - 1) / kSparseThreads;
  if (groups >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  MarkParams p;
  p.table_keys = table_keys;
  p.table_birth = table_birth;
  p.table_slots = table_slots;
  p.fresh = fresh;
  p.status = reinterpret_cast<unsigned long long*>(status);
  p.depth = depth;
  p.cam_intr = cam_intr;
  p.cam_pose = cam_pose;
  p.total = total;
  p.im_h = im_h;
  p.im_w = im_w;
  p.origin[0] = origin_x;
  p.origin[1] = origin_y;
  p.origin[2] = origin_z;
  p.voxel_size = voxel_size;
  p.trunc = trunc_margin;
  p.max_depth = max_depth;
  p.first_frame = first_frame;
  hipLaunchKernelGGL(sparse_mark_kernel, dim3(static_cast<unsigned>(groups)), dim3(kSparseThreads), 0, static_cast<hipStream_t>(stream), p);
  return launch_status();
}

extern "C" int dvmvs_sparse_assign(const long long* table_keys, const int* table_birth, long long table_slots, const long long* sorted,
                                   long long* fresh, long long* status, long long* pool_key, int* pool_birth, long long max_bricks,
                                   dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!table_keys || !table_birth || !sorted || !fresh || !status || !pool_key || !pool_birth) return DVMVS_EINVAL;
  if (!power_of_two(table_slots) || max_bricks < 1) return DVMVS_EINVAL;
  if (table_slots > (1LL << 30) || max_bricks >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
  const unsigned groups = static_cast<unsigned>((table_slots + kSparseThreads - 1) / kSparseThreads);
  hipLaunchKernelGGL(sparse_assign_kernel, dim3(groups), dim3(kSparseThreads), 0, s, table_keys, table_birth, table_slots, sorted, fresh, st,
                     pool_key, pool_birth, max_bricks);
  int rc = launch_status();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(sparse_commit_kernel, dim3(1), dim3(64), 0, s, st, table_slots, max_bricks);
  return launch_status();
}

extern "C" int dvmvs_sparse_integrate(float* pool_tsdf, float* pool_weight, float* pool_color, const long long* pool_key, const int* pool_birth,
                                      const long long* status, long long max_bricks, float origin_x, float origin_y, float origin_z,
                                      float voxel_size, const float* cam_intr, const float* cam_pose, const unsigned char* rgb_u8,
                                      const float* folded, const float* depth, int n_frames, int im_h, int im_w, float trunc_margin,
                                      const float* obs_weight_host, float max_depth, int first_frame, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!pool_tsdf || !pool_weight || !pool_color || !pool_key || !pool_birth || !status || !cam_intr || !cam_pose || !depth || !obs_weight_host)
    return DVMVS_EINVAL;
  if ((rgb_u8 != nullptr) == (folded != nullptr)) return DVMVS_EINVAL;
  if (max_bricks < 1 || n_frames <= 0 || im_h <= 0 || im_w <= 0 || first_frame < 0) return DVMVS_EINVAL;
  if (!(voxel_size > 0.0f) || !(trunc_margin > 0.0f) || max_depth != max_depth) return DVMVS_EINVAL;
  const long long pixels = static_cast<long long>(im_h) * im_w;
  if (pixels >= (1LL << 31) || max_bricks >= (1LL << 31) || static_cast<long long>(first_frame) + n_frames >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  SparseFuseParams p;
  p.tsdf = pool_tsdf;
  p.weight = pool_weight;
  p.color = pool_color;
  p.pool_key = pool_key;
  p.pool_birth = pool_birth;
  p.status = reinterpret_cast<const unsigned long long*>(status);
  p.origin_x = origin_x;
  p.origin_y = origin_y;
  p.origin_z = origin_z;
  p.voxel_size = voxel_size;
  p.im_h = im_h;
  p.im_w = im_w;
  p.trunc_margin = trunc_margin;
  p.max_depth = max_depth;
  for (int first = 0; first < n_frames; first += kSparseMaxFrames) {
    const int n = n_frames - first < kSparseMaxFrames ? n_frames - first : kSparseMaxFrames;
    p.cam_intr = cam_intr + 9LL * first;
    p.cam_pose = cam_pose + 16LL * first;
    p.rgb = rgb_u8 ? rgb_u8 + 3LL * first * pixels : nullptr;
    p.folded = folded ? folded + first * pixels : nullptr;
    p.depth = depth + first * pixels;
    p.n_frames = n;
    p.first_frame = first_frame + first;
    for (int i = 0; i < kSparseMaxFrames; ++i) p.obs_weight[i] = i < n ? obs_weight_host[first + i] : 0.0f;
    hipLaunchKernelGGL(sparse_integrate_kernel, dim3(static_cast<unsigned>(max_bricks)), dim3(kSparseThreads), 0, static_cast<hipStream_t>(stream), p);
    const int rc = launch_status();
    if (rc != 0) return rc;
  }
  return 0;
}

extern "C" int dvmvs_sparse_gather(const float* pool_tsdf, const float* pool_weight, const float* pool_color, const long long* pool_key,
                                   long long n_bricks, float* tsdf_vol, float* weight_vol, float* color_vol, int bricks_x, int bricks_y,
                                   int bricks_z, int first_x, int first_y, int first_z, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!pool_tsdf || !pool_weight || !pool_color || !pool_key || !tsdf_vol || !weight_vol || !color_vol) return DVMVS_EINVAL;
  if (n_bricks < 0 || bricks_x < 1 || bricks_y < 1 || bricks_z < 1) return DVMVS_EINVAL;
  if (n_bricks >= (1LL << 31) || static_cast<long long>(bricks_x) * bricks_y * bricks_z >= (1LL << 40)) return DVMVS_EUNSUPPORTED;
  if (n_bricks == 0) return 0;
  hipLaunchKernelGGL(sparse_gather_kernel, dim3(static_cast<unsigned>(n_bricks)), dim3(kSparseThreads), 0, static_cast<hipStream_t>(stream),
                     pool_tsdf, pool_weight, pool_color, pool_key, tsdf_vol, weight_vol, color_vol, bricks_x, bricks_y, bricks_z, first_x,
                     first_y, first_z);
  return launch_status();
}
