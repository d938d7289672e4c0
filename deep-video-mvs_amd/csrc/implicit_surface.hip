// Implicit moving-least-squares (IMLS) signed distance of an oriented point cloud on a voxel grid (gfx950): what turns the point path's
// cloud with normals into a volume that csrc/marching_cubes.hip meshes.  dvmvs/implicit.py is the host form; include/dvmvs_hip.h states
// the contract.
//   dvmvs_implicit_band_fwd   : points fp32 [M,3], grid, radius -> mask uint8 [X,Y,Z], 1 at every node that can have a candidate
//   dvmvs_implicit_nodes_fwd  : linear node indices int64 [A], grid -> node positions fp32 [A,3]
//   dvmvs_implicit_values_fwd : positions, points, normals, index rows int32 [A,k] of dvmvs_knn_fwd -> volume fp32 and valid uint8, scattered
//   dvmvs_implicit_trim_fwd   : marching-cubes vertices in index space, faces, valid -> keep_vertex uint8 [V], keep_face uint8 [F]
//
// Arithmetic contract of the values: fp64 from the fp32 inputs with +, -, *, / only, every operation correctly rounded, nothing contracted
// into an FMA (contract(off) for the whole file; fp64 division is the correctly rounded one).  The node positions are fp32:
// x = fl(fl(fl(i) * voxel) + origin), the multiply and the add rounded separately (contract(off) again).  Per node, over its row in slot
// order, for every USED slot (0 <= j < M and normals[j] != 0): e = x - points[j] (exact), d2 = (ex ex + ey ey) + ez ez,
// t = 1 - d2 / h2 with h2 = fp64(radius) fp64(radius), t < 0 -> 0, w = (t t) t, s = (nx ex + ny ey) + nz ez, num += w s, den += w from 0.0.
// Valid when at least min_neighbours slots were used and den > 0: value = fp32(num / den).  Other nodes are not written: the caller
// pre-fills the volume with fp32(radius) and valid with 0.
//
// The band is a SUPERSET of the nodes with a candidate.  A node x is a candidate of point p under the search's fp32 test when
// fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) <= fl(r r) with dx = fl(x_x - p_x) and so on.  With u = 2^-24:
//   a. Adding a non-negative fp32 number never gives less than the other operand (rounding is monotone and the operand is a float), so
//      fl(dx dx) <= fl(r r) on every axis.
//   b. fl(r r) <= r r (1 + u) and fl(dx dx) >= dx dx (1 - u) unless the square is below the normal range (2^-126, or flushed to zero);
//      so |dx| <= r sqrt((1 + u) / (1 - u)) <= r (1 + 2u), or |dx| < 2^-63.  dx = (x_x - p_x)(1 + d), |d| <= u, so
//      |x_x - p_x| <= r (1 + 4u) + 2^-62.
//   c. The node's coordinate is x_x = (i v (1 + d1) + o)(1 + d2), |d1|, |d2| <= u, so |x_x - (i v + o)| <= u |i v| + u |x_x| (1 + 2u) and,
//      with |i v| <= (|x_x| + |o|)(1 + 5u) and |x_x| <= |p_x| + r (1 + 4u) + 2^-62, it is at most 2^-23 (|o| + |p_x| + r)(1 + 8u): half
//      of the 2^-22 that is used.  (An index above 2^24 is itself rounded, fl(i) = i (1 + d0): one more u |i v|, three quarters of it.)
//   So |i - g| <= (r (1 + 4u) + 2^-62 + 2^-23 (|o| + |p_x| + r)) / v with g = (p_x - o) / v.  The kernel marks the whole numbers i with
//   |i - g| <= reach = (r (1 + 2^-20) + 2^-22 (|o| + |p_x| + r) + 2^-62) / v + 2^-20 on every axis, in fp64: the factor 2^-20 against 4u =
//   2^-22, the doubled coordinate term and the absolute 2^-20 are far above the fp64 roundings of g and reach themselves (2^-52 relative,
//   of numbers below 2^31 in index units).  It marks the CUBE of those i, which holds the ball: more nodes than have a candidate, which
//   costs a search that finds nothing and changes no result.
// One point per lane; the z run of a cube row is consecutive bytes.  Lanes of many points store the constant 1 into the same bytes: a
// benign race of plain vector byte stores.  The cube is clamped to [0, dim) on every axis BEFORE any address is formed, in fp64 and then
// as ints, so a point outside the grid (or with a coordinate that is not finite: it marks nothing) writes only inside it.
//
// The values: one node per lane, nothing crosses lanes after the staging barrier, so the result does not depend on the schedule.  A slot
// outside [0, M) never becomes an address: its gather reads points[0] and normals[0] (M >= 1) and its sums are not taken.  The gathers
// of a slot do not depend on the slots before it, so the loop keeps several in flight.  num, den and the count are named scalars: no
// array indexed at run time, no scratch.  The index rows go through LDS at the odd pitch k | 1, as in csrc/point_normals.hip, which
// measured the direct read of a lane's own row 3.4 times slower at k = 32 (profiles/point_normals_index_read.json): the workgroup copies
// its 256 rows, one contiguous piece, with coalesced 4-byte loads, and every lane reads its row back on 32 different banks.
#include "dvmvs_device.h"

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

constexpr int kImBlock = 256;
constexpr int kImMinK = 1, kImMaxK = 32;
constexpr long long kImMaxPoints = 1ll << 28;
constexpr long long kImMaxNodes = 1ll << 31;
constexpr long long kImMaxMesh = 0x7fffffffll;

// The whole numbers i of one axis with |i - g| <= reach, clamped to [0, dim): false when there is none (or p is not finite).
__device__ inline bool im_axis_range(float p32, float o32, double v, double r, int dim, int& lo, int& hi) {
  const double p = static_cast<double>(p32), o = static_cast<double>(o32);
  const double g = (p - o) / v;
  const double reach = (r * (1.0 + 0x1p-20) + 0x1p-22 * ((fabs(o) + fabs(p)) + r) + 0x1p-62) / v + 0x1p-20;
  const double a = g - reach, b = g + reach;
  if (!(a <= b)) return false;                               // NaN or inf - inf
  const double top = static_cast<double>(dim - 1);
  const double first = a < 0.0 ? 0.0 : ceil(a), last = b > top ? top : floor(b);
  if (!(first <= last)) return false;                        // wholly outside the grid: first and last are then never converted
  lo = static_cast<int>(first);
  hi = static_cast<int>(last);
  return true;
}

__global__ __launch_bounds__(kImBlock) void im_band_kernel(const float* __restrict__ points, int m, float ox, float oy, float oz, float voxel,
                                                           int X, int Y, int Z, float radius, unsigned char* __restrict__ mask) {
  const long long i = static_cast<long long>(blockIdx.x) * kImBlock + threadIdx.x;
  if (i >= m) return;
  const float* p = points + 3 * static_cast<size_t>(i);
  const double v = static_cast<double>(voxel), r = static_cast<double>(radius);
  int x0, x1, y0, y1, z0, z1;
  if (!im_axis_range(p[0], ox, v, r, X, x0, x1) || !im_axis_range(p[1], oy, v, r, Y, y0, y1) || !im_axis_range(p[2], oz, v, r, Z, z0, z1))
    return;
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y) {
      unsigned char* row = mask + (static_cast<size_t>(x) * Y + y) * Z;
      for (int z = z0; z <= z1; ++z) row[z] = 1;
    }
}

__global__ __launch_bounds__(kImBlock) void im_nodes_kernel(const long long* __restrict__ linear, long long n, float ox, float oy, float oz,
                                                            float voxel, int Y, int Z, float* __restrict__ nodes) {
  const long long a = static_cast<long long>(blockIdx.x) * kImBlock + threadIdx.x;
  if (a >= n) return;
  const long long l = linear[a];
  const long long xy = l / Z;
  const int k = static_cast<int>(l - xy * Z), i = static_cast<int>(xy / Y), j = static_cast<int>(xy - static_cast<long long>(i) * Y);
  const float sx = static_cast<float>(i) * voxel, sy = static_cast<float>(j) * voxel, sz = static_cast<float>(k) * voxel;
  nodes[3 * static_cast<size_t>(a) + 0] = sx + ox;
  nodes[3 * static_cast<size_t>(a) + 1] = sy + oy;
  nodes[3 * static_cast<size_t>(a) + 2] = sz + oz;
}

__global__ __launch_bounds__(kImBlock) void im_values_kernel(const float* __restrict__ nodes, long long n_nodes, const float* __restrict__ points,
                                                             const float* __restrict__ normals, int m, const int* __restrict__ index, int k,
                                                             float radius, int min_neighbours, const long long* __restrict__ linear,
                                                             long long total, float* __restrict__ volume, unsigned char* __restrict__ valid) {
  extern __shared__ int s_index[];                           // [row][k | 1]
  const int lane = threadIdx.x;
  const long long first = static_cast<long long>(blockIdx.x) * kImBlock;
  const int rows = static_cast<int>(min(static_cast<long long>(kImBlock), n_nodes - first));
  const int pitch = k | 1;
  {
    const int* __restrict__ src = index + first * k;
    const int total_slots = rows * k, step_row = kImBlock / k, step_slot = kImBlock % k;
    int r = lane / k, s = lane % k;
    for (int e = lane; e < total_slots; e += kImBlock) {     // e = r * k + s
      s_index[r * pitch + s] = src[e];
      r += step_row;
      s += step_slot;
      if (s >= k) {
        s -= k;
        ++r;
      }
    }
  }
  __syncthreads();
  if (lane >= rows) return;
  const long long a = first + lane;
  const int* row = s_index + lane * pitch;
  const float* q = nodes + 3 * static_cast<size_t>(a);
  const double x = static_cast<double>(q[0]), y = static_cast<double>(q[1]), z = static_cast<double>(q[2]);
  const double h2 = static_cast<double>(radius) * static_cast<double>(radius);

  int used = 0;
  double num = 0.0, den = 0.0;
#pragma unroll 4
  for (int slot = 0; slot < k; ++slot) {
    const int j = row[slot];
    const bool inside = static_cast<unsigned int>(j) < static_cast<unsigned int>(m);
    const size_t at = 3 * static_cast<size_t>(inside ? j : 0);
    const float px = points[at], py = points[at + 1], pz = points[at + 2];
    const float nx = normals[at], ny = normals[at + 1], nz = normals[at + 2];
    const bool ok = inside && (nx != 0.0f || ny != 0.0f || nz != 0.0f);
    const double ex = x - static_cast<double>(px), ey = y - static_cast<double>(py), ez = z - static_cast<double>(pz);
    const double d2 = (ex * ex + ey * ey) + ez * ez;
    double t = 1.0 - d2 / h2;
    if (t < 0.0) t = 0.0;
    const double w = (t * t) * t;
    const double s = (static_cast<double>(nx) * ex + static_cast<double>(ny) * ey) + static_cast<double>(nz) * ez;
    if (ok) {
      ++used;
      num += w * s;
      den += w;
    }
  }
  if (used < min_neighbours || !(den > 0.0)) return;
  const long long l = linear[a];
  if (l < 0 || l >= total) return;                           // an index outside the grid never becomes an address
  volume[l] = static_cast<float>(num / den);
  valid[l] = 1;
}

__global__ __launch_bounds__(kImBlock) void im_trim_vertices_kernel(const float* __restrict__ verts, long long n_verts,
                                                                    const unsigned char* __restrict__ valid, int X, int Y, int Z,
                                                                    unsigned char* __restrict__ keep) {
  const long long v = static_cast<long long>(blockIdx.x) * kImBlock + threadIdx.x;
  if (v >= n_verts) return;
  const float* p = verts + 3 * static_cast<size_t>(v);
  const float fx = floorf(p[0]), fy = floorf(p[1]), fz = floorf(p[2]);
  const float cx = ceilf(p[0]), cy = ceilf(p[1]), cz = ceilf(p[2]);
  unsigned char good = 0;
  // floor >= 0 and ceil < 2^31 make the conversions exact (a NaN fails both); ceil < dim, compared as whole numbers, then puts both nodes
  // inside the grid, and only then are they addressed
  if (fx >= 0.0f && fy >= 0.0f && fz >= 0.0f && cx < 0x1p31f && cy < 0x1p31f && cz < 0x1p31f) {
    const int x0 = static_cast<int>(fx), y0 = static_cast<int>(fy), z0 = static_cast<int>(fz);
    const int x1 = static_cast<int>(cx), y1 = static_cast<int>(cy), z1 = static_cast<int>(cz);
    if (x1 < X && y1 < Y && z1 < Z) {
      const size_t lo = (static_cast<size_t>(x0) * Y + y0) * Z + z0;
      const size_t hi = (static_cast<size_t>(x1) * Y + y1) * Z + z1;
      good = (valid[lo] != 0 && valid[hi] != 0) ? 1 : 0;
    }
  }
  keep[v] = good;
}

__global__ __launch_bounds__(kImBlock) void im_trim_faces_kernel(const int* __restrict__ faces, long long n_faces, long long n_verts,
                                                                 const unsigned char* __restrict__ keep_vertex,
                                                                 unsigned char* __restrict__ keep_face) {
  const long long f = static_cast<long long>(blockIdx.x) * kImBlock + threadIdx.x;
  if (f >= n_faces) return;
  const int* c = faces + 3 * static_cast<size_t>(f);
  const int a = c[0], b = c[1], d = c[2];
  unsigned char good = 0;
  if (a >= 0 && a < n_verts && b >= 0 && b < n_verts && d >= 0 && d < n_verts)
    good = (keep_vertex[a] != 0 && keep_vertex[b] != 0 && keep_vertex[d] != 0) ? 1 : 0;
  keep_face[f] = good;
}

// host side: x - x is 0 for a finite number and NaN otherwise
inline bool im_finite(float v) { return v - v == 0.0f; }

inline bool im_aligned(const void* p, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// 0 for a grid the kernels take, else the error: voxel finite and > 0, a finite origin, every dimension >= 1, at most 2^31 nodes
inline int im_grid_status(float ox, float oy, float oz, float voxel, int X, int Y, int Z) {
  if (!(voxel > 0.0f) || !im_finite(voxel) || !im_finite(ox) || !im_finite(oy) || !im_finite(oz) || X < 1 || Y < 1 || Z < 1) return DVMVS_EINVAL;
  if (static_cast<long long>(X) * Y > kImMaxNodes || static_cast<long long>(X) * Y * Z > kImMaxNodes) return DVMVS_EUNSUPPORTED;
  return 0;
}

inline dim3 im_blocks(long long n) { return dim3(static_cast<unsigned int>((n + kImBlock - 1) / kImBlock)); }

}  // namespace

}  // namespace dvmvs

extern "C" int dvmvs_implicit_band_fwd(const float* points, long long M, float origin_x, float origin_y, float origin_z, float voxel, int X,
                                       int Y, int Z, float radius, unsigned char* mask, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (M < 0 || !(radius > 0.0f) || !im_finite(radius) || !mask || (M > 0 && !points) || !im_aligned(points, 4)) return DVMVS_EINVAL;
  if (const int status = im_grid_status(origin_x, origin_y, origin_z, voxel, X, Y, Z)) return status;
  if (M > kImMaxPoints) return DVMVS_EUNSUPPORTED;
  if (M == 0) return 0;
  hipLaunchKernelGGL(im_band_kernel, im_blocks(M), dim3(kImBlock), 0, static_cast<hipStream_t>(stream), points, static_cast<int>(M), origin_x,
                     origin_y, origin_z, voxel, X, Y, Z, radius, mask);
  return launch_status();
}

extern "C" int dvmvs_implicit_nodes_fwd(const long long* linear, long long A, float origin_x, float origin_y, float origin_z, float voxel,
                                        int X, int Y, int Z, float* nodes, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (A < 0 || (A > 0 && (!linear || !nodes)) || !im_aligned(linear, 8) || !im_aligned(nodes, 4)) return DVMVS_EINVAL;
  if (const int status = im_grid_status(origin_x, origin_y, origin_z, voxel, X, Y, Z)) return status;
  if (A > kImMaxPoints) return DVMVS_EUNSUPPORTED;
  if (A == 0) return 0;
  hipLaunchKernelGGL(im_nodes_kernel, im_blocks(A), dim3(kImBlock), 0, static_cast<hipStream_t>(stream), linear, A, origin_x, origin_y,
                     origin_z, voxel, Y, Z, nodes);
  return launch_status();
}

extern "C" int dvmvs_implicit_values_fwd(const float* nodes, long long A, const float* points, const float* normals, long long M,
                                         const int* index, int k, float radius, int min_neighbours, const long long* linear,
                                         long long total, float* volume, unsigned char* valid, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (A < 0 || M < 1 || k < kImMinK || k > kImMaxK || min_neighbours < 1 || !(radius > 0.0f) || !im_finite(radius) || total < 1)
    return DVMVS_EINVAL;
  if (!points || !normals || !volume || !valid || (A > 0 && (!nodes || !index || !linear))) return DVMVS_EINVAL;
  if (!im_aligned(nodes, 4) || !im_aligned(points, 4) || !im_aligned(normals, 4) || !im_aligned(index, 4) || !im_aligned(linear, 8) ||
      !im_aligned(volume, 4)) return DVMVS_EINVAL;
  if (A > kImMaxPoints || M > kImMaxPoints || total > kImMaxNodes) return DVMVS_EUNSUPPORTED;
  if (A == 0) return 0;
  hipLaunchKernelGGL(im_values_kernel, im_blocks(A), dim3(kImBlock), static_cast<size_t>(kImBlock) * (k | 1) * sizeof(int),
                     static_cast<hipStream_t>(stream), nodes, A, points, normals, static_cast<int>(M), index, k, radius, min_neighbours, linear,
                     total, volume, valid);
  return launch_status();
}

extern "C" int dvmvs_implicit_trim_fwd(const float* verts, long long V, const int* faces, long long F, const unsigned char* valid, int X,
                                       int Y, int Z, unsigned char* keep_vertex, unsigned char* keep_face, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (V < 0 || F < 0 || X < 1 || Y < 1 || Z < 1 || !valid || (V > 0 && (!verts || !keep_vertex)) || (F > 0 && (!faces || !keep_face || !keep_vertex)))
    return DVMVS_EINVAL;
  if (!im_aligned(verts, 4) || !im_aligned(faces, 4)) return DVMVS_EINVAL;
  if (static_cast<long long>(X) * Y > kImMaxNodes || static_cast<long long>(X) * Y * Z > kImMaxNodes || V > kImMaxMesh || F > kImMaxMesh)
    return DVMVS_EUNSUPPORTED;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (V > 0) {
    hipLaunchKernelGGL(im_trim_vertices_kernel, im_blocks(V), dim3(kImBlock), 0, s, verts, V, valid, X, Y, Z, keep_vertex);
    if (const int status = launch_status()) return status;
  }
  if (F > 0) {
    hipLaunchKernelGGL(im_trim_faces_kernel, im_blocks(F), dim3(kImBlock), 0, s, faces, F, V, keep_vertex, keep_face);
    return launch_status();
  }
  return 0;
}
