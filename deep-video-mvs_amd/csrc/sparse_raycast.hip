// Ray-casting of the sparse TSDF volume straight from its pool (gfx950): depth, world-space normal and colour of the first zero crossing
// along every pixel's ray, without the dense copy -- DESIGN.md section 4.8t, contract in include/dvmvs_hip.h, index, corner arithmetic
// and flag rule in sparse_raycast_grid.h.
//
// Definition.  For a brick-aligned box (first brick, count bricks per axis) the outputs equal, bit for bit, those of tsdf_raycast_kernel
// (csrc/tsdf_raycast.hip) on the dense volume of 8 * count voxels whose voxel w holds the pool's voxel of brick first + (w >> 3) at local
// (w & 7) (x * 64 + y * 8 + z) and (tsdf 1, weight 0, colour 0) where that brick is not allocated.  The per-pixel statements of that kernel
// are RESTATED here one by one (float32, contraction off, the same order): o_g, d_g, the slab test against [0, dim - 1], z0, dz, n, n_cap,
// z_k from k alone, the clamp, the cell min(floor(g), dim - 2), the z, y, x lerps, the hit rule, the on-demand f_{k-1}, the six-sample
// normal and the colour at rint(g*).  Only where a voxel is read from differs.  The duplication is deliberate; the equality tests of
// tests/test_sparse_raycast_gpu.py hold the two together.
//
// Three facts make the sparse march cheap.
// 1. A sample whose cell lies in an UNALLOCATED brick is invalid: the cell's own lowest corner c is a voxel of that brick and reads
//    weight 0.  A hit needs samples k - 1 and k valid, the normal is kept only when its six samples are valid, and no other statement
//    reads a sample's value: the value of an invalid sample never reaches an output.  So such a brick can neither end a hit nor serve as
//    f_{k-1} of one, the sampler returns at once for it, and the march skips it with the dense kernel's VERIFIED jump: the slab
//    arithmetic proposes the last sample k' before the ray leaves the brick, and k' is accepted only if the cell of sample k' lies in the
//    same brick -- every float32 operation from k to the cell index is monotone in k per axis, so every sample between k and k' does too.
// 2. An ALLOCATED brick without a crossing corner is skipped the same way.  A hit at sample k needs f_k <= 0 with the cell valid, and
//    lerp(a, b, w) of positive a, b with w in [0, 1] is positive, so one of the cell's eight corners has weight > 0 && tsdf <= 0.  The
//    flag (sparse_raycast_flags_kernel) looks at all 9^3 corners of the brick's cells, those of the seven forward neighbours included,
//    whether or not they lie in the box: a superset of the dense kernel's mask.  Only "unflagged => no hit can end here" is used, and a
//    skipped sample that turns out to be f_{k-1} of a hit is evaluated on demand, so the bits do not depend on the flags.
// 3. step <= 5 < 8 voxels, so the cells of consecutive evaluated samples differ by at most one brick per axis.  From an allocated brick
//    the next brick's slot is one load from the row neighbour[slot][27] of dvmvs_sparse_neighbours (and one from flags[]); a lookup in
//    the render index is needed only at ray entry, after a jump, and when leaving an unallocated brick.
//
// Mapping: one lane per pixel, a wave covers an 8x8 pixel tile, four waves a 16x16 block, blockIdx.z the view -- as the dense kernel.  The
// march is a divergent per-lane loop (k strictly increases and ends at n <= n_cap < 2^20); every probe loop is bounded by the index
// size.  No float atomics, no LDS; the only atomics are the 64-bit compare-and-swaps of the index build.  Every pool slot that is
// dereferenced comes from an index value or a neighbour entry checked against [0, n_bricks), n_bricks read on the device and clamped
// to max_bricks; every voxel index is slot * 512 + a local index < 512.
#include "dvmvs_device.h"
#include "sparse_raycast_grid.h"
#ifdef DVMVS_SPARSE_RAYCAST_TUNING
#include "sparse_extract_grid.h"      // se_find: the binary-search lookup that tools/sparse_raycast_bench.py measures against the index
#endif

#include <math.h>

namespace dvmvs {

namespace {

constexpr int kSrThreads = 256;
constexpr int kSrMaxSteps = 1 << 20;
constexpr int kSrMaxCount = 1 << 21;      // bricks per axis: 8 * count <= 2^24, so float(dim - 1) is exact
enum { kSrStatBricks = 0 };

struct SrParams {
  const float* tsdf;
  const float* weight;
  const float* color;
  const unsigned long long* status;
  long long max_bricks;
  const long long* index;
  unsigned long long index_slots;
  const int* neighbour;
  const unsigned char* flags;
#ifdef DVMVS_SPARSE_RAYCAST_TUNING
  const long long* sorted;       // the sorted keys and the slots they came from, as dvmvs_sparse_neighbours takes them; null: the index
  const long long* sort_index;
#endif
  int first[3];     // the box's first brick
  int dims[3];      // voxels: 8 * count
  float origin[3];
  float voxel_size;
  int skip_empty;
  const float* cam_intr;
  const float* cam_pose;
  int H, W;
  float near, far, step;
  int n_cap;
  float* depth;
  float* normal;
  unsigned char* rgb;
};

__device__ inline long long sr_bricks_on_device(const unsigned long long* status, long long max_bricks) {
  const long long n = static_cast<long long>(status[kSrStatBricks]);
  return n < 0 ? 0 : (n > max_bricks ? max_bricks : n);
}

// ---- index build ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSrThreads) void sparse_raycast_clear_kernel(long long* __restrict__ index, long long index_slots) {
  const long long e = static_cast<long long>(blockIdx.x) * kSrThreads + threadIdx.x;
  if (e >= index_slots) return;
  index[2 * e] = kBrickEmpty;
  index[2 * e + 1] = -1;
}

// One thread per pool slot < n_bricks: its key takes the first free entry on its probe path (64-bit compare-and-swap, as mark_brick);
// the value is written by the thread that owns the key.  At most index_slots attempts.
__global__ __launch_bounds__(kSrThreads) void sparse_raycast_index_kernel(const long long* __restrict__ pool_key,
                                                                           const unsigned long long* __restrict__ status, long long max_bricks,
                                                                           long long* __restrict__ index, unsigned long long index_slots) {
  const long long slot = static_cast<long long>(blockIdx.x) * kSrThreads + threadIdx.x;
  if (slot >= sr_bricks_on_device(status, max_bricks)) return;
  const long long key = pool_key[slot];
  if (key < 0 || key == kBrickEmpty) return;      // no brick
  unsigned long long* words = reinterpret_cast<unsigned long long*>(index);
  const unsigned long long want = static_cast<unsigned long long>(key), empty = static_cast<unsigned long long>(kBrickEmpty);
  const uint64_t mask = index_slots - 1, hash = sg_hash(key);
  for (uint64_t i = 0; i <= mask; ++i) {
    const uint64_t e = sg_probe(hash, i, mask);
    unsigned long long cur = __atomic_load_n(words + 2 * e, __ATOMIC_RELAXED);
    if (cur == empty) {
      cur = atomicCAS(words + 2 * e, empty, want);
      if (cur == empty) cur = want;
    }
    if (cur == want) {
      index[2 * e + 1] = sr_value(slot, false);
      return;
    }
  }
}

// The checked entry `entry` of the row of `slot`.
__device__ inline int sr_row(const int* __restrict__ neighbour, long long slot, int entry, long long n) {
  const int s = neighbour[slot * kRaycastRow + entry];
  return (s >= 0 && s < n) ? s : -1;
}

// One wave per pool slot: its lanes walk the brick's 9^3 corners; flags[slot] and the flag bit of the brick's index entry.
__global__ __launch_bounds__(kSrThreads) void sparse_raycast_flags_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                           const long long* __restrict__ pool_key,
                                                                           const int* __restrict__ neighbour,
                                                                           const unsigned long long* __restrict__ status, long long max_bricks,
                                                                           long long* __restrict__ index, unsigned long long index_slots,
                                                                           unsigned char* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const long long slot = static_cast<long long>(blockIdx.x) * (kSrThreads / 64) + (threadIdx.x >> 6);
  const long long n = sr_bricks_on_device(status, max_bricks);
  if (slot >= n) return;   // whole waves leave
  bool any = false;
  for (int i = lane; i < kRaycastCorners; i += 64) {
    int entry, local;
    sr_lattice_corner(i, entry, local);
    const long long s = entry == kRaycastOwn ? slot : sr_row(neighbour, slot, entry, n);
    if (s >= 0) any = any || sr_crossing(tsdf[s * kBrickVoxels + local], weight[s * kBrickVoxels + local]);
  }
  const unsigned long long votes = __ballot(any);
  if (lane == 0) {
    const bool flag = votes != 0ull;
    flags[slot] = flag ? 1 : 0;
    const long long e = sr_find(index, index_slots, pool_key[slot]);
    if (e >= 0 && sr_slot(index[2 * e + 1]) == slot) index[2 * e + 1] = sr_value(slot, flag);
  }
}

// ---- the march --------------------------------------------------------------------------------------------------------------------------
// The brick the march stands in: box-relative coordinates, pool slot (-1: not allocated) and crossing flag.
struct SrCursor {
  int b[3];
  int slot;
  bool flag;
};

// Slot and flag of the box-relative brick (bx, by, bz), from the cursor's row where it is a neighbour of an allocated brick, else from
// the index.  (The tuning library alone also carries the fallback design that lost, for tools/sparse_raycast_bench.py: se_find's binary
// search of 32 dependent loads over the sorted keys in place of the index lookup, chosen per launch by a wave-uniform pointer test.)
__device__ inline void sr_resolve(const SrParams& p, long long n, const SrCursor& cur, int bx, int by, int bz, int& slot, bool& flag) {
  const int dx = bx - cur.b[0], dy = by - cur.b[1], dz = bz - cur.b[2];
  if (dx == 0 && dy == 0 && dz == 0) {
    slot = cur.slot;
    flag = cur.flag;
    return;
  }
  if (cur.slot >= 0 && dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && dz >= -1 && dz <= 1) {
    slot = sr_row(p.neighbour, cur.slot, sr_row_entry(dx, dy, dz), n);
    flag = slot >= 0 && p.flags[slot] != 0;
    return;
  }
  slot = -1;
  flag = false;
  const int x = p.first[0] + bx, y = p.first[1] + by, z = p.first[2] + bz;
  if (!sg_in_range(x, y, z)) return;
#ifdef DVMVS_SPARSE_RAYCAST_TUNING
  if (p.sorted) {
    const long long at = se_find(p.sorted, n, sg_pack(x, y, z));
    if (at < 0) return;
    const long long s = p.sort_index[at];
    if (s < 0 || s >= n) return;
    slot = static_cast<int>(s);
    flag = p.flags[s] != 0;
    return;
  }
#endif
  const long long v = sr_lookup(p.index, p.index_slots, sg_pack(x, y, z));
  if (v < 0 || sr_slot(v) >= n) return;
  slot = sr_slot(v);
  flag = sr_flag(v);
}

#pragma clang fp contract(off)

__device__ inline float sr_lerp(float a, float b, float w) { return a * (1.0f - w) + b * w; }

// clamp(o_g + z d_g) into the box; never NaN for finite inputs (fmaxf / fminf drop a NaN operand anyway)
__device__ inline void sr_point(const float* og, const float* dg, float z, const int* dims, float* g) {
  g[0] = fminf(fmaxf(og[0] + z * dg[0], 0.0f), static_cast<float>(dims[0] - 1));
  g[1] = fminf(fmaxf(og[1] + z * dg[1], 0.0f), static_cast<float>(dims[1] - 1));
  g[2] = fminf(fmaxf(og[2] + z * dg[2], 0.0f), static_cast<float>(dims[2] - 1));
}

// cell of a clamped point: i0 = min(floor(g), dim - 2), kept inside [0, dim - 2] whatever g is
__device__ inline void sr_cell(const float* g, const int* dims, int* c) {
  c[0] = max(min(static_cast<int>(floorf(g[0])), dims[0] - 2), 0);
  c[1] = max(min(static_cast<int>(floorf(g[1])), dims[1] - 2), 0);
  c[2] = max(min(static_cast<int>(floorf(g[2])), dims[2] - 2), 0);
}

// trilinear tsdf at the clamped point g in cell c, whose brick has pool slot `slot` (-1: not allocated -- the sample is invalid and its
// value is never used); valid <- all eight corner weights > 0
__device__ inline float sr_sample(const SrParams& p, long long n, int slot, const float* g, const int* c, bool& valid) {
  valid = false;
  if (slot < 0) return 0.0f;
  const float wx = g[0] - static_cast<float>(c[0]), wy = g[1] - static_cast<float>(c[1]), wz = g[2] - static_cast<float>(c[2]);
  const int lx = c[0] & 7, ly = c[1] & 7, lz = c[2] & 7;
  float t[8], w[8];
  if (sr_interior(lx, ly, lz)) {
    const long long base = static_cast<long long>(slot) * kBrickVoxels + (lx * 64 + ly * 8 + lz);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long long idx = base + ((i >> 2) & 1) * 64 + ((i >> 1) & 1) * 8 + (i & 1);
      t[i] = p.tsdf[idx];
      w[i] = p.weight[idx];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int entry, local;
      sr_corner(lx, ly, lz, i, entry, local);
      const int s = entry == kRaycastOwn ? slot : sr_row(p.neighbour, slot, entry, n);
      t[i] = 1.0f;
      w[i] = 0.0f;
      if (s >= 0) {
        const long long idx = static_cast<long long>(s) * kBrickVoxels + local;
        t[i] = p.tsdf[idx];
        w[i] = p.weight[idx];
      }
    }
  }
  valid = w[0] > 0.0f && w[1] > 0.0f && w[2] > 0.0f && w[3] > 0.0f && w[4] > 0.0f && w[5] > 0.0f && w[6] > 0.0f && w[7] > 0.0f;
  const float c00 = sr_lerp(t[0], t[1], wz), c01 = sr_lerp(t[2], t[3], wz), c10 = sr_lerp(t[4], t[5], wz), c11 = sr_lerp(t[6], t[7], wz);
  return sr_lerp(sr_lerp(c00, c01, wy), sr_lerp(c10, c11, wy), wx);
}

__device__ inline float sr_sample_at(const SrParams& p, long long n, const SrCursor& cur, const float* g, bool& valid) {
  int c[3], slot;
  bool flag;
  sr_cell(g, p.dims, c);
  sr_resolve(p, n, cur, c[0] >> 3, c[1] >> 3, c[2] >> 3, slot, flag);
  return sr_sample(p, n, slot, g, c, valid);
}

__device__ inline bool sr_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for NaN and +-inf

__global__ __launch_bounds__(kSrThreads) void sparse_raycast_kernel(const SrParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int v = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const int view = blockIdx.z;
  const int H = p.H, W = p.W;
  if (u >= W || v >= H) return;
  const long long n_bricks = sr_bricks_on_device(p.status, p.max_bricks);
  const long long pixel = (static_cast<long long>(view) * H + v) * W + u;
  const float* Kp = p.cam_intr + 9 * static_cast<long long>(view);
  const float* Pp = p.cam_pose + 16 * static_cast<long long>(view);
  const float fx = Kp[0], cx = Kp[2], fy = Kp[4], cy = Kp[5];
  const int dims[3] = {p.dims[0], p.dims[1], p.dims[2]};
  const float voxel_size = p.voxel_size, near = p.near, far = p.far, step = p.step;

  const float dcx = (static_cast<float>(u) - cx) / fx, dcy = (static_cast<float>(v) - cy) / fy;
  float og[3], dg[3];
  og[0] = (Pp[3] - p.origin[0]) / voxel_size;
  og[1] = (Pp[7] - p.origin[1]) / voxel_size;
  og[2] = (Pp[11] - p.origin[2]) / voxel_size;
#pragma unroll
  for (int a = 0; a < 3; ++a) dg[a] = (Pp[4 * a + 0] * dcx + Pp[4 * a + 1] * dcy + Pp[4 * a + 2]) / voxel_size;

  bool ok = sr_finite(og[0]) && sr_finite(og[1]) && sr_finite(og[2]) && sr_finite(dg[0]) && sr_finite(dg[1]) && sr_finite(dg[2]);
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
  ok = ok && sr_finite(z0) && sr_finite(z1) && z0 <= z1 && sr_finite(dz) && dz > 0.0f;

  SrCursor cur = {{-4, -4, -4}, -1, false};      // no brick yet: the first sample looks its brick up in the index
  float hit_depth = 0.0f;
  if (ok) {
    const int n = static_cast<int>(fminf(floorf((z1 - z0) / dz), static_cast<float>(p.n_cap)));   // >= 0: z0 <= z1
    int k = 0, prev_k = -1;
    float prev_f = 0.0f;
    bool prev_valid = false;
    while (k <= n) {
      float g[3];
      int c[3];
      sr_point(og, dg, z0 + static_cast<float>(k) * dz, dims, g);
      sr_cell(g, dims, c);
      const int b[3] = {c[0] >> 3, c[1] >> 3, c[2] >> 3};
      {
        int slot;
        bool flag;
        sr_resolve(p, n_bricks, cur, b[0], b[1], b[2], slot, flag);
        cur.b[0] = b[0];
        cur.b[1] = b[1];
        cur.b[2] = b[2];
        cur.slot = slot;
        cur.flag = flag;
      }
      if (p.skip_empty && !cur.flag) {
        // nothing in this brick can end a hit: propose the last sample before the ray leaves it, accept it only if it is in the brick
        float zexit = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          if (dg[a] > 0.0f) zexit = fminf(zexit, (static_cast<float>((b[a] + 1) * kBrick) - og[a]) / dg[a]);
          if (dg[a] < 0.0f) zexit = fminf(zexit, (static_cast<float>(b[a] * kBrick) - og[a]) / dg[a]);
        }
        const float kf = fminf(floorf((zexit - z0) / dz) - 1.0f, static_cast<float>(n));
        int next = k + 1;
        if (kf > static_cast<float>(k)) {   // false for a NaN proposal
          const int kj = static_cast<int>(kf);
          float gj[3];
          int cj[3];
          sr_point(og, dg, z0 + static_cast<float>(kj) * dz, dims, gj);
          sr_cell(gj, dims, cj);
          if ((cj[0] >> 3) == b[0] && (cj[1] >> 3) == b[1] && (cj[2] >> 3) == b[2]) next = kj + 1;
        }
        k = next;
        continue;
      }
      bool valid;
      const float f = sr_sample(p, n_bricks, cur.slot, g, c, valid);
      if (k >= 1 && valid && f <= 0.0f) {
        if (prev_k != k - 1) {   // the previous sample was skipped: evaluate it now
          float gp[3];
          sr_point(og, dg, z0 + static_cast<float>(k - 1) * dz, dims, gp);
          prev_f = sr_sample_at(p, n_bricks, cur, gp, prev_valid);
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
  p.depth[pixel] = hit_depth;
  if (!p.normal && !p.rgb) return;

  const bool hit = hit_depth != 0.0f;
  float gs[3] = {0.0f, 0.0f, 0.0f};
  if (hit) sr_point(og, dg, hit_depth, dims, gs);
  if (p.normal) {
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    if (hit) {
      bool all_valid = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        float gp[3] = {gs[0], gs[1], gs[2]}, gm[3] = {gs[0], gs[1], gs[2]};
        gp[a] = fminf(gs[a] + 1.0f, static_cast<float>(dims[a] - 1));
        gm[a] = fmaxf(gs[a] - 1.0f, 0.0f);
        bool vp, vm;
        const float fp = sr_sample_at(p, n_bricks, cur, gp, vp), fm = sr_sample_at(p, n_bricks, cur, gm, vm);
        nrm[a] = fp - fm;
        all_valid = all_valid && vp && vm;
      }
      const float nlen = sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
      const bool keep = all_valid && nlen > 0.0f && sr_finite(nlen);
#pragma unroll
      for (int a = 0; a < 3; ++a) nrm[a] = keep ? nrm[a] / nlen : 0.0f;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) p.normal[3 * pixel + a] = nrm[a];
  }
  if (p.rgb) {
    float cr = 0.0f, cg = 0.0f, cb_ = 0.0f;
    if (hit) {
      int q[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) q[a] = min(max(static_cast<int>(rintf(gs[a])), 0), dims[a] - 1);
      int slot;
      bool flag;
      sr_resolve(p, n_bricks, cur, q[0] >> 3, q[1] >> 3, q[2] >> 3, slot, flag);
      float col = 0.0f;      // the colour of a voxel of an unallocated brick
      if (slot >= 0) col = p.color[static_cast<long long>(slot) * kBrickVoxels + ((q[0] & 7) * 64 + (q[1] & 7) * 8 + (q[2] & 7))];
      cb_ = floorf(col / 65536.0f);
      cg = floorf((col - cb_ * 65536.0f) / 256.0f);
      cr = col - cb_ * 65536.0f - cg * 256.0f;
    }
    p.rgb[3 * pixel + 0] = static_cast<unsigned char>(floorf(cr));
    p.rgb[3 * pixel + 1] = static_cast<unsigned char>(floorf(cg));
    p.rgb[3 * pixel + 2] = static_cast<unsigned char>(floorf(cb_));
  }
}
#pragma clang fp contract(fast)

int sr_check_index(long long max_bricks, long long index_slots) {
  if (max_bricks < 1 || index_slots < 1) return DVMVS_EINVAL;
  if (max_bricks >= (1LL << 31) || index_slots > (1LL << 32)) return DVMVS_EUNSUPPORTED;
  if ((index_slots & (index_slots - 1)) != 0 || index_slots < 2 * max_bricks) return DVMVS_EINVAL;
  return 0;
}

}  // namespace

}  // namespace dvmvs

extern "C" int dvmvs_sparse_raycast_index(const long long* pool_key, const long long* status, long long max_bricks, long long* index,
                                          long long index_slots, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!pool_key || !status || !index) return DVMVS_EINVAL;
  const int rc = sr_check_index(max_bricks, index_slots);
  if (rc != 0) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sparse_raycast_clear_kernel, dim3(static_cast<unsigned>((index_slots + kSrThreads - 1) / kSrThreads)), dim3(kSrThreads), 0, s,
                     index, index_slots);
  hipLaunchKernelGGL(sparse_raycast_index_kernel, dim3(static_cast<unsigned>((max_bricks + kSrThreads - 1) / kSrThreads)), dim3(kSrThreads), 0, s,
                     pool_key, reinterpret_cast<const unsigned long long*>(status), max_bricks, index,
                     static_cast<unsigned long long>(index_slots));
  return launch_status();
}

extern "C" int dvmvs_sparse_raycast_flags(const float* pool_tsdf, const float* pool_weight, const long long* pool_key, const int* neighbour,
                                          const long long* status, long long max_bricks, long long* index, long long index_slots,
                                          unsigned char* flags, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!pool_tsdf || !pool_weight || !pool_key || !neighbour || !status || !index || !flags) return DVMVS_EINVAL;
  const int rc = sr_check_index(max_bricks, index_slots);
  if (rc != 0) return rc;
  const long long groups = (max_bricks + kSrThreads / 64 - 1) / (kSrThreads / 64);
  hipLaunchKernelGGL(sparse_raycast_flags_kernel, dim3(static_cast<unsigned>(groups)), dim3(kSrThreads), 0, static_cast<hipStream_t>(stream),
                     pool_tsdf, pool_weight, pool_key, neighbour, reinterpret_cast<const unsigned long long*>(status), max_bricks, index,
                     static_cast<unsigned long long>(index_slots), flags);
  return launch_status();
}

namespace dvmvs {
namespace {

// The checks and the launch of dvmvs_sparse_raycast_fwd; sorted / sort_index non-null (the tuning library): the binary-search lookup.
int sr_forward(const float* pool_tsdf, const float* pool_weight, const float* pool_color, const long long* status, long long max_bricks,
               const long long* index, long long index_slots, const int* neighbour, const unsigned char* flags, const long long* sorted,
               const long long* sort_index, int first_x, int first_y, int first_z, int count_x, int count_y, int count_z, float origin_x,
               float origin_y, float origin_z, float voxel_size, int skip_empty, const float* cam_intr, const float* cam_pose, int n_views,
               int im_h, int im_w, float near, float far, float step, float* depth, float* normal, unsigned char* rgb, dvmvs_stream_t stream) {
  if (!pool_tsdf || !pool_weight || !status || !index || !neighbour || !flags || !cam_intr || !cam_pose || !depth || (rgb && !pool_color))
    return DVMVS_EINVAL;
  if (n_views <= 0 || im_h <= 0 || im_w <= 0) return DVMVS_EINVAL;
  if (!(voxel_size > 0.0f) || !(step > 0.0f) || !(step <= 5.0f) || !(near >= 0.0f) || far != far || !(near < INFINITY)) return DVMVS_EINVAL;
  const int rc = sr_check_index(max_bricks, index_slots);
  if (rc != 0) return rc;
  const int first[3] = {first_x, first_y, first_z}, count[3] = {count_x, count_y, count_z};
  for (int a = 0; a < 3; ++a) {
    if (count[a] < 1) return DVMVS_EINVAL;
    if (count[a] > kSrMaxCount) return DVMVS_EUNSUPPORTED;
    // the box stays within one brick of the lattice's coordinate range (as dense() asks)
    if (first[a] < -(1 << 20) || static_cast<long long>(first[a]) + count[a] - 1 > (1 << 20)) return DVMVS_EINVAL;
  }
  if (static_cast<long long>(im_h) * im_w >= (1LL << 31) || n_views > 65535) return DVMVS_EUNSUPPORTED;
  // the longest march: the box diagonal in steps (+ 2 for rounding); float(k) must stay exact and the loop short
  const double dx = 8.0 * count_x - 1, dy = 8.0 * count_y - 1, dzv = 8.0 * count_z - 1;
  const double steps = floor(sqrt(dx * dx + dy * dy + dzv * dzv) / static_cast<double>(step)) + 2.0;
  if (steps >= static_cast<double>(kSrMaxSteps)) return DVMVS_EUNSUPPORTED;
  const dim3 grid(static_cast<unsigned>((im_w + 15) / 16), static_cast<unsigned>((im_h + 15) / 16), static_cast<unsigned>(n_views));
  if (grid.y > 65535u) return DVMVS_EUNSUPPORTED;
  // a launch holds fewer than 2^32 threads in all
  if (static_cast<unsigned long long>(grid.x) * grid.y * grid.z * 256ull >= (1ull << 32)) return DVMVS_EUNSUPPORTED;
  SrParams p;
  p.tsdf = pool_tsdf;
  p.weight = pool_weight;
  p.color = pool_color;
  p.status = reinterpret_cast<const unsigned long long*>(status);
  p.max_bricks = max_bricks;
  p.index = index;
  p.index_slots = static_cast<unsigned long long>(index_slots);
  p.neighbour = neighbour;
  p.flags = flags;
#ifdef DVMVS_SPARSE_RAYCAST_TUNING
  p.sorted = (sorted && sort_index) ? sorted : nullptr;
  p.sort_index = sort_index;
#endif
  for (int a = 0; a < 3; ++a) {
    p.first[a] = first[a];
    p.dims[a] = 8 * count[a];
  }
  p.origin[0] = origin_x;
  p.origin[1] = origin_y;
  p.origin[2] = origin_z;
  p.voxel_size = voxel_size;
  p.skip_empty = skip_empty ? 1 : 0;
  p.cam_intr = cam_intr;
  p.cam_pose = cam_pose;
  p.H = im_h;
  p.W = im_w;
  p.near = near;
  p.far = far;
  p.step = step;
  p.n_cap = static_cast<int>(steps);
  p.depth = depth;
  p.normal = normal;
  p.rgb = rgb;
  hipLaunchKernelGGL(sparse_raycast_kernel, grid, dim3(kSrThreads), 0, static_cast<hipStream_t>(stream), p);
  return launch_status();
}

}  // namespace
}  // namespace dvmvs

extern "C" int dvmvs_sparse_raycast_fwd(const float* pool_tsdf, const float* pool_weight, const float* pool_color, const long long* status,
                                        long long max_bricks, const long long* index, long long index_slots, const int* neighbour,
                                        const unsigned char* flags, int first_x, int first_y, int first_z, int count_x, int count_y,
                                        int count_z, float origin_x, float origin_y, float origin_z, float voxel_size, int skip_empty,
                                        const float* cam_intr, const float* cam_pose, int n_views, int im_h, int im_w, float near, float far,
                                        float step, float* depth, float* normal, unsigned char* rgb, dvmvs_stream_t stream) {
  return dvmvs::sr_forward(pool_tsdf, pool_weight, pool_color, status, max_bricks, index, index_slots, neighbour, flags, nullptr, nullptr, first_x,
                           first_y, first_z, count_x, count_y, count_z, origin_x, origin_y, origin_z, voxel_size, skip_empty, cam_intr, cam_pose,
                           n_views, im_h, im_w, near, far, step, depth, normal, rgb, stream);
}

#ifdef DVMVS_SPARSE_RAYCAST_TUNING
// tools-only (the tuning library; not in the header): the same render with the binary-search lookup, for tools/sparse_raycast_bench.py
extern "C" int dvmvs_sparse_raycast_fwd_search(const float* pool_tsdf, const float* pool_weight, const float* pool_color, const long long* status,
                                               long long max_bricks, const long long* index, long long index_slots, const int* neighbour,
                                               const unsigned char* flags, const long long* sorted, const long long* sort_index, int first_x,
                                               int first_y, int first_z, int count_x, int count_y, int count_z, float origin_x, float origin_y,
                                               float origin_z, float voxel_size, int skip_empty, const float* cam_intr, const float* cam_pose,
                                               int n_views, int im_h, int im_w, float near, float far, float step, float* depth, float* normal,
                                               unsigned char* rgb, dvmvs_stream_t stream) {
  if (!sorted || !sort_index) return DVMVS_EINVAL;
  return dvmvs::sr_forward(pool_tsdf, pool_weight, pool_color, status, max_bricks, index, index_slots, neighbour, flags, sorted, sort_index, first_x,
                           first_y, first_z, count_x, count_y, count_z, origin_x, origin_y, origin_z, voxel_size, skip_empty, cam_intr, cam_pose,
                           n_views, im_h, im_w, near, far, step, depth, normal, rgb, stream);
}
#endif
