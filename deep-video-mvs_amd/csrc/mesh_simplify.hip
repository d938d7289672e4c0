// Simplifying a triangle mesh by vertex clustering with quadric error representatives (gfx950).  It reproduces its host definition bit
// for bit (dvmvs/simplify.py::simplify_mesh; include/dvmvs_hip.h).
//   dvmvs_mesh_simplify_keys      : the cluster of every vertex; per face its mapped corners, three incidence keys and the two sort keys of
//                                   its rotation-canonical triple
//   dvmvs_mesh_simplify_pair_keys : the second sort key in the order of the first sort
//   dvmvs_mesh_simplify_count     : every cluster's vertex and attributes, the surviving faces, the clusters they use -> counts int64 [3] =
//                                   {V', F', status}
//   dvmvs_mesh_simplify_emit      : the compacted, re-indexed mesh with its optional attributes and the two index arrays
//
// The clusters are the voxels of dvmvs_voxel_keys / dvmvs_voxel_downsample_count (csrc/surface_sample.hip), which the caller runs on the
// vertices first, with a stable sort of the keys between them; their run starts and the vertices in sorted order
// (dvmvs_voxel_downsample_runs), the number of voxels and the status (the count entry's `counts`) are read where those entries left them.
// The caller also sorts, stably: the incidence keys (cluster of corner j of face f at 3 f + j; a face with an index outside [0, V) has
// the key INT_MAX and sorts behind every cluster), and for the duplicate faces the canonical triples, third corner first, then the first
// two corners packed into 56 bits (clusters < 2^28).
//
// Arithmetic contract: fp64 from the fp32 inputs with +, -, *, / and sqrt only, every operation correctly rounded, nothing contracted into
// an FMA (contract(off) for the whole file).  No float atomics and no float value crosses threads: one thread owns a cluster and walks
// its members (sorted order: sequential memory) and its incidences (gathered faces) serially, in the order of the definition, so the
// result does not depend on the schedule.  A cluster with a long run is therefore one long serial walk; there is no second path for it.
// The nine sums of the quadric, the six entries of A and the nine of V are named scalars and the three rotations are written out
// (ms_rotate, point_normals.hip's pn_rotate restated): nothing is indexed at run time, nothing lives in scratch.
//
// Everything else is integers.  Flags are plain stores of one value (ref[c] = 1 from any number of threads); counts come from
// block_exclusive_scan and scan_totals of dvmvs_device.h.  No index read from memory becomes an address before it is checked against its
// array's size, so a sort order that is no permutation (never, from a sort) gives wrong values and no access out of bounds.
//
// Launches.  keys: ms_cluster_kernel (sorted slot j -> cluster[sorted_index[j]] by a binary search of the run starts; clears ref) ->
// ms_face_map_kernel.  pair_keys: ms_gather_kernel.  count: ms_run_start_kernel (inc_start[c] = the first sorted incidence whose key is >= c,
// c = 0 .. M) -> ms_solve_kernel (one thread per cluster) -> ms_face_head_kernel (a valid face is kept when it begins a run of equal
// triples: the smallest face index of the run, by the stability of the sorts) -> ms_keep_kernel (ref[c] = 1 for the corners of kept faces)
// -> ms_flag_count_kernel -> ms_scan_blocks_kernel.  emit: ms_emit_verts_kernel -> ms_emit_faces_kernel, ms_emit_index_kernel.
#include "dvmvs_device.h"

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

constexpr int kMsBlock = 256;
constexpr int kMsPerThread = 4;
constexpr int kMsChunk = kMsBlock * kMsPerThread;      // elements per workgroup of a count or a scan
constexpr int kMsScanThreads = 1024;
constexpr long long kMsMaxElements = 1LL << 28;        // V and F
constexpr int kMsSweeps = 16;
constexpr int kMsBatch = 4;                          // incidences whose loads a cluster's thread keeps in flight
constexpr int kMsNone = 0x7fffffff;                    // the key of what takes no part: sorts behind every cluster
constexpr long long kMsNonePair = 0x7fffffffffffffffLL;
constexpr double kMsRankThreshold = 1e-3;

// M of the voxel count step, clipped to what the arrays hold
__device__ inline long long ms_clusters(const long long* __restrict__ voxel_counts, long long V) {
  const long long m = voxel_counts[0];
  return m < 0 ? 0 : m > V ? V : m;
}

// i clamped into [0, last]
__device__ inline long long ms_clamp(long long i, long long last) { return i < 0 ? 0 : i > last ? last : i; }

__device__ inline bool ms_valid(int ia, int ib, int ic, long long V) { return ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V; }

// sorted slot j belongs to run m: the last m with starts[m] <= j.  cluster[sorted_index[j]] = m; ref[j] = 0.
__global__ __launch_bounds__(kMsBlock) void ms_cluster_kernel(const long long* __restrict__ sorted_index, const int* __restrict__ starts,
                                                              const long long* __restrict__ voxel_counts, long long V, int* __restrict__ cluster,
                                                              int* __restrict__ ref) {
  const long long j = static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x;
  if (j >= V) return;
  ref[j] = 0;
  const long long M = ms_clusters(voxel_counts, V);
  long long lo = 0, hi = M;                            // the first m with starts[m] > j
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (starts[mid] > j) hi = mid; else lo = mid + 1;
  }
  const long long i = sorted_index[j];
  if (i >= 0 && i < V) cluster[i] = static_cast<int>(lo > 0 ? lo - 1 : 0);
}

__global__ __launch_bounds__(kMsBlock) void ms_face_map_kernel(const int* __restrict__ faces, long long F, long long V, const int* __restrict__ cluster,
                                                               int* __restrict__ mapped, int* __restrict__ keep, int* __restrict__ inc_key,
                                                               int* __restrict__ third, long long* __restrict__ pair) {
  const long long f = static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x;
  if (f >= F) return;
  const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
  const bool valid = ms_valid(ia, ib, ic, V);
  const int a = valid ? cluster[ia] : -1, b = valid ? cluster[ib] : -1, c = valid ? cluster[ic] : -1;
  mapped[f * 3] = a;
  mapped[f * 3 + 1] = b;
  mapped[f * 3 + 2] = c;
  inc_key[f * 3] = valid ? a : kMsNone;
  inc_key[f * 3 + 1] = valid ? b : kMsNone;
  inc_key[f * 3 + 2] = valid ? c : kMsNone;
  keep[f] = 0;
  const bool proper = valid && a != b && b != c && a != c && a >= 0 && b >= 0 && c >= 0;
  // the rotation that puts the smallest corner first
  const bool first_a = a <= b && a <= c, first_b = b <= a && b <= c;
  const int x = first_a ? a : first_b ? b : c, y = first_a ? b : first_b ? c : a, z = first_a ? c : first_b ? a : b;
  third[f] = proper ? z : kMsNone;
  pair[f] = proper ? (static_cast<long long>(x) << 28) | static_cast<long long>(y) : kMsNonePair;
}

__global__ __launch_bounds__(kMsBlock) void ms_gather_kernel(const long long* __restrict__ pair, const long long* __restrict__ order, long long F,
                                                             long long* __restrict__ out) {
  const long long s = static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x;
  if (s >= F) return;
  const long long f = order[s];
  out[s] = f >= 0 && f < F ? pair[f] : kMsNonePair;
}

// inc_start[c] = the first slot s with inc_sorted[s] >= c, for c = 0 .. M
__global__ __launch_bounds__(kMsBlock) void ms_run_start_kernel(const int* __restrict__ inc_sorted, long long n, const long long* __restrict__ voxel_counts,
                                                                long long V, int* __restrict__ inc_start) {
  const long long c = static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x;
  if (c > ms_clusters(voxel_counts, V)) return;
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (inc_sorted[mid] >= c) hi = mid; else lo = mid + 1;
  }
  inc_start[c] = static_cast<int>(lo);                // n <= 3 * 2^28 < 2^31
}

// One Jacobi rotation of the pair (p, q) on the symmetric 3x3 with r the third index (pn_rotate of point_normals.hip, the same operations
// in the same order): the columns p, q, then the rows, old values on the right, on the upper triangle.
__device__ inline void ms_rotate(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p, double& v0q, double& v1p,
                                 double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double pp = c * app - s * apq, pq = s * app + c * apq;
  const double qp = c * apq - s * aqq, qq = s * apq + c * aqq;
  app = c * pp - s * qp;
  aqq = s * pq + c * qq;
  apq = 0.0;
  const double pr = apr, qr = aqr;
  apr = c * pr - s * qr;
  aqr = s * pr + c * qr;
  double o;
  o = v0p, v0p = c * o - s * v0q, v0q = s * o + c * v0q;
  o = v1p, v1p = c * o - s * v1q, v1q = s * o + c * v1q;
  o = v2p, v2p = c * o - s * v2q, v2q = s * o + c * v2q;
}

// x += (-(((v0 b0 + v1 b1) + v2 b2) / l)) * v for a kept column
__device__ inline void ms_add_column(double l, double threshold, double v0, double v1, double v2, double bx, double by, double bz, double& x,
                                     double& y, double& z) {
  if (!(l > threshold)) return;
  const double coef = -(((v0 * bx + v1 * by) + v2 * bz) / l);
  x += coef * v0;
  y += coef * v1;
  z += coef * v2;
}

// step 2 for one incidence: the plane of the face with the corners p[0..2], p[3..5], p[6..8] about o, added to the nine sums
__device__ inline void ms_add_plane(const float (&p)[9], double ox, double oy, double oz, double& a00, double& a01, double& a02, double& a11,
                                    double& a12, double& a22, double& bx, double& by, double& bz) {
  const double p0x = static_cast<double>(p[0]) - ox, p0y = static_cast<double>(p[1]) - oy, p0z = static_cast<double>(p[2]) - oz;
  const double p1x = static_cast<double>(p[3]) - ox, p1y = static_cast<double>(p[4]) - oy, p1z = static_cast<double>(p[5]) - oz;
  const double p2x = static_cast<double>(p[6]) - ox, p2y = static_cast<double>(p[7]) - oy, p2z = static_cast<double>(p[8]) - oz;
  const double e1x = p1x - p0x, e1y = p1y - p0y, e1z = p1z - p0z;
  const double e2x = p2x - p0x, e2y = p2y - p0y, e2z = p2z - p0z;
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const double d = -((nx * p0x + ny * p0y) + nz * p0z);
  a00 += nx * nx, a01 += nx * ny, a02 += nx * nz;
  a11 += ny * ny, a12 += ny * nz, a22 += nz * nz;
  bx += d * nx, by += d * ny, bz += d * nz;
}

// One thread per cluster: steps 1 (the mean), 2, 3 and 4 of the definition -> pos, nrm, col at the cluster's number
__global__ __launch_bounds__(kMsBlock) void ms_solve_kernel(const float* __restrict__ verts, const float* __restrict__ normals,
                                                            const unsigned char* __restrict__ colors, long long V, const int* __restrict__ faces,
                                                            long long F, const float* __restrict__ sorted_pts, const long long* __restrict__ sorted_index,
                                                            const int* __restrict__ starts, const long long* __restrict__ voxel_counts,
                                                            const int* __restrict__ inc_start, const long long* __restrict__ inc_order, long long n_inc,
                                                            double limit, int average, float* __restrict__ pos, float* __restrict__ nrm,
                                                            unsigned char* __restrict__ col) {
  const long long c = static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x;
  const long long M = ms_clusters(voxel_counts, V);
  if (c >= M) return;
  long long begin = starts[c], end = c + 1 < M ? starts[c + 1] : V;
  begin = begin < 0 ? 0 : begin;
  end = end > V ? V : end;
  double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll 4
  for (long long j = begin; j < end; ++j) {
    sx += static_cast<double>(sorted_pts[j * 3]);
    sy += static_cast<double>(sorted_pts[j * 3 + 1]);
    sz += static_cast<double>(sorted_pts[j * 3 + 2]);
  }
  const double cnt = static_cast<double>(end - begin);
  float px = static_cast<float>(sx / cnt), py = static_cast<float>(sy / cnt), pz = static_cast<float>(sz / cnt);

  if (normals || colors) {
    double tx = 0.0, ty = 0.0, tz = 0.0;
    unsigned long long r = 0, g = 0, b = 0;
#pragma unroll 4
    for (long long j = begin; j < end; ++j) {
      const long long i = ms_clamp(sorted_index[j], V - 1);      // (a no-op for the indices of a sort of V keys)
      if (normals) {
        tx += static_cast<double>(normals[i * 3]);
        ty += static_cast<double>(normals[i * 3 + 1]);
        tz += static_cast<double>(normals[i * 3 + 2]);
      }
      if (colors) {
        r += colors[i * 3];
        g += colors[i * 3 + 1];
        b += colors[i * 3 + 2];
      }
    }
    if (normals) {
      const double len = sqrt((tx * tx + ty * ty) + tz * tz);
      const bool ok = len > 0.0 && len < __builtin_inf();
      nrm[c * 3] = ok ? static_cast<float>(tx / len) : 0.0f;
      nrm[c * 3 + 1] = ok ? static_cast<float>(ty / len) : 0.0f;
      nrm[c * 3 + 2] = ok ? static_cast<float>(tz / len) : 0.0f;
    }
    if (colors) {
      col[c * 3] = static_cast<unsigned char>(rint(static_cast<double>(r) / cnt));
      col[c * 3 + 1] = static_cast<unsigned char>(rint(static_cast<double>(g) / cnt));
      col[c * 3 + 2] = static_cast<unsigned char>(rint(static_cast<double>(b) / cnt));
    }
  }

  if (!average) {
    const double ox = static_cast<double>(px), oy = static_cast<double>(py), oz = static_cast<double>(pz);
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
    long long s0 = inc_start[c], s1 = inc_start[c + 1];
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 > n_inc ? n_inc : s1;
    // An incidence's loads (its id, its face, nine coordinates) do not depend on the incidences before it.  Every index is clamped into
    // its array (a no-op for the order of a sort and the faces it lists: an invalid face's keys sort behind every cluster), so there is no
    // branch around a load, and the loads of kMsBatch incidences are issued level by level before their sums run, in the order of the
    // definition: three memory latencies per batch instead of three per incidence.  The arrays are indexed by unrolled constants only.
    const long long last_vertex = V - 1, last_incidence = n_inc - 1;
    long long s = s0;
    for (; s + kMsBatch <= s1; s += kMsBatch) {
      long long f[kMsBatch], corner[kMsBatch][3];
      float p[kMsBatch][9];
#pragma unroll
      for (int k = 0; k < kMsBatch; ++k) f[k] = ms_clamp(inc_order[s + k], last_incidence) / 3;
#pragma unroll
      for (int k = 0; k < kMsBatch; ++k) {
#pragma unroll
        for (int j = 0; j < 3; ++j) corner[k][j] = ms_clamp(faces[f[k] * 3 + j], last_vertex);
      }
#pragma unroll
      for (int k = 0; k < kMsBatch; ++k) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
          for (int d = 0; d < 3; ++d) p[k][j * 3 + d] = verts[corner[k][j] * 3 + d];
        }
      }
#pragma unroll
      for (int k = 0; k < kMsBatch; ++k) ms_add_plane(p[k], ox, oy, oz, a00, a01, a02, a11, a12, a22, bx, by, bz);
    }
    for (; s < s1; ++s) {
      const long long f = ms_clamp(inc_order[s], last_incidence) / 3;
      float p[9];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const long long corner = ms_clamp(faces[f * 3 + j], last_vertex);
#pragma unroll
        for (int d = 0; d < 3; ++d) p[j * 3 + d] = verts[corner * 3 + d];
      }
      ms_add_plane(p, ox, oy, oz, a00, a01, a02, a11, a12, a22, bx, by, bz);
    }
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < kMsSweeps; ++sweep) {
      if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
      ms_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0,1), r = 2
      ms_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0,2), r = 1
      ms_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1,2), r = 0
    }
    double lmax = a00;
    if (a11 > lmax) lmax = a11;
    if (a22 > lmax) lmax = a22;
    const double threshold = kMsRankThreshold * lmax;
    double x = 0.0, y = 0.0, z = 0.0;
    ms_add_column(a00, threshold, v00, v10, v20, bx, by, bz, x, y, z);
    ms_add_column(a11, threshold, v01, v11, v21, bx, by, bz, x, y, z);
    ms_add_column(a22, threshold, v02, v12, v22, bx, by, bz, x, y, z);
    if (lmax > 0.0 && fabs(x) <= limit && fabs(y) <= limit && fabs(z) <= limit) {      // (false for a NaN)
      px = static_cast<float>(ox + x);
      py = static_cast<float>(oy + y);
      pz = static_cast<float>(oz + z);
    }
  }
  pos[c * 3] = px;
  pos[c * 3 + 1] = py;
  pos[c * 3 + 2] = pz;
}

// the face at sorted slot s: third_order[pair_order[s]], -1 where an order holds what no sort gives
__device__ inline long long ms_sorted_face(const long long* __restrict__ third_order, const long long* __restrict__ pair_order, long long F,
                                           long long s) {
  const long long k = pair_order[s];
  if (k < 0 || k >= F) return -1;
  const long long f = third_order[k];
  return f >= 0 && f < F ? f : -1;
}

__global__ __launch_bounds__(kMsBlock) void ms_face_head_kernel(const int* __restrict__ third, const long long* __restrict__ third_order,
                                                                const long long* __restrict__ pair_sorted, const long long* __restrict__ pair_order,
                                                                long long F, int* __restrict__ keep) {
  const long long s = static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x;
  if (s >= F) return;
  const long long f = ms_sorted_face(third_order, pair_order, F, s);
  if (f < 0 || third[f] == kMsNone) return;            // (keep[f] is 0 from the map kernel)
  bool head = s == 0 || pair_sorted[s] != pair_sorted[s - 1];
  if (!head) {
    const long long before = ms_sorted_face(third_order, pair_order, F, s - 1);
    head = before < 0 || third[before] != third[f];
  }
  if (head) keep[f] = 1;
}

__global__ __launch_bounds__(kMsBlock) void ms_keep_kernel(const int* __restrict__ mapped, const int* __restrict__ keep, long long F, long long V,
                                                           int* __restrict__ ref) {
  const long long f = static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x;
  if (f >= F || !keep[f]) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = mapped[f * 3 + k];
    if (c >= 0 && c < V) ref[c] = 1;
  }
}

// Workgroups [0, fblocks): kept faces per 1024 faces -> ftotals[b]; workgroups [fblocks, fblocks + vblocks): used clusters per 1024.
__global__ __launch_bounds__(kMsBlock) void ms_flag_count_kernel(const int* __restrict__ keep, long long F, const int* __restrict__ ref, long long V,
                                                                 int fblocks, int* __restrict__ ftotals, int* __restrict__ vtotals) {
  __shared__ int lds[kMsBlock / 64];
  const bool is_face = static_cast<int>(blockIdx.x) < fblocks;
  const int b = is_face ? blockIdx.x : blockIdx.x - fblocks;
  const long long n = is_face ? F : V;
  const int* __restrict__ flags = is_face ? keep : ref;
  const long long first = (static_cast<long long>(b) * kMsBlock + threadIdx.x) * kMsPerThread;
  int v = 0;
  for (int e = 0; e < kMsPerThread; ++e)
    if (first + e < n && flags[first + e]) ++v;
  int total;
  block_exclusive_scan<kMsBlock>(v, lds, total);
  if (threadIdx.x == 0) (is_face ? ftotals : vtotals)[b] = total;
}

__global__ __launch_bounds__(kMsScanThreads) void ms_scan_blocks_kernel(int* __restrict__ ftotals, int fblocks, int* __restrict__ vtotals, int vblocks,
                                                                        const long long* __restrict__ voxel_counts, long long* __restrict__ counts) {
  __shared__ int s[kMsScanThreads];
  const int kept_faces = scan_totals<kMsScanThreads>(ftotals, fblocks, s);
  const int kept_verts = scan_totals<kMsScanThreads>(vtotals, vblocks, s);
  if (threadIdx.x == 0) {
    const long long status = voxel_counts[1] ? 1 : 0;
    counts[0] = status ? 0 : kept_verts;
    counts[1] = status ? 0 : kept_faces;
    counts[2] = status;
  }
}

// used cluster c -> slot new_index[c] of the outputs (order-preserving); new_index[c] = -1 for the others
__global__ __launch_bounds__(kMsBlock) void ms_emit_verts_kernel(const float* __restrict__ pos, const float* __restrict__ nrm,
                                                                 const unsigned char* __restrict__ col, const int* __restrict__ ref, long long V,
                                                                 const int* __restrict__ offsets, long long V_out, int* __restrict__ new_index,
                                                                 float* __restrict__ verts_out, float* __restrict__ normals_out,
                                                                 unsigned char* __restrict__ colors_out) {
  __shared__ int lds[kMsBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x) * kMsPerThread;
  bool used[kMsPerThread];
  int n = 0;
#pragma unroll
  for (int e = 0; e < kMsPerThread; ++e) {
    used[e] = first + e < V && ref[first + e] != 0;
    n += used[e] ? 1 : 0;
  }
  int total;
  long long slot = offsets[blockIdx.x] + block_exclusive_scan<kMsBlock>(n, lds, total);
#pragma unroll
  for (int e = 0; e < kMsPerThread; ++e) {
    const long long c = first + e;
    if (c >= V) break;
    const bool ok = used[e] && slot >= 0 && slot < V_out;      // always, when V_out comes from the count step of the same mesh
    new_index[c] = ok ? static_cast<int>(slot) : -1;
    if (!ok) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      verts_out[slot * 3 + d] = pos[c * 3 + d];
      if (normals_out) normals_out[slot * 3 + d] = nrm[c * 3 + d];
      if (colors_out) colors_out[slot * 3 + d] = col[c * 3 + d];
    }
    ++slot;
  }
}

__global__ __launch_bounds__(kMsBlock) void ms_emit_faces_kernel(const int* __restrict__ mapped, const int* __restrict__ keep, long long F, long long V,
                                                                 const int* __restrict__ offsets, const int* __restrict__ new_index, long long F_out,
                                                                 int* __restrict__ faces_out, int* __restrict__ face_index) {
  __shared__ int lds[kMsBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x) * kMsPerThread;
  bool kept[kMsPerThread];
  int n = 0;
#pragma unroll
  for (int e = 0; e < kMsPerThread; ++e) {
    kept[e] = first + e < F && keep[first + e] != 0;
    n += kept[e] ? 1 : 0;
  }
  int total;
  long long slot = offsets[blockIdx.x] + block_exclusive_scan<kMsBlock>(n, lds, total);
#pragma unroll
  for (int e = 0; e < kMsPerThread; ++e) {
    const long long f = first + e;
    if (f >= F) break;
    if (!kept[e] || slot < 0 || slot >= F_out) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int c = mapped[f * 3 + d];
      faces_out[slot * 3 + d] = c >= 0 && c < V ? new_index[c] : -1;      // (a kept face is valid and its clusters are used)
    }
    if (face_index) face_index[slot] = static_cast<int>(f);
    ++slot;
  }
}

__global__ __launch_bounds__(kMsBlock) void ms_emit_index_kernel(const int* __restrict__ cluster, const int* __restrict__ new_index, long long V,
                                                                 int* __restrict__ vertex_cluster) {
  const long long i = static_cast<long long>(blockIdx.x) * kMsBlock + threadIdx.x;
  if (i >= V) return;
  const int c = cluster[i];
  vertex_cluster[i] = c >= 0 && c < V ? new_index[c] : -1;
}

size_t ms_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

int ms_blocks(long long n) { return static_cast<int>((n + kMsChunk - 1) / kMsChunk); }      // <= 2^18

unsigned int ms_grid(long long n) { return static_cast<unsigned int>((n + kMsBlock - 1) / kMsBlock); }

// workspace: cluster [V] int | ref [V] int | new_index [V] int | inc_start [V + 1] int | pos [V,3] fp32 | nrm [V,3] fp32 | col [V,3] uint8 |
// mapped [F,3] int | keep [F] int | face block totals [blocks of F] int | cluster block totals [blocks of V] int
struct MsLayout {
  size_t ref_off, index_off, start_off, pos_off, nrm_off, col_off, mapped_off, keep_off, ftotals_off, vtotals_off, total;
};

MsLayout ms_layout(long long V, long long F) {
  MsLayout l;
  const size_t v = static_cast<size_t>(V), f = static_cast<size_t>(F);
  l.ref_off = ms_align(v * sizeof(int));
  l.index_off = l.ref_off + ms_align(v * sizeof(int));
  l.start_off = l.index_off + ms_align(v * sizeof(int));
  l.pos_off = l.start_off + ms_align((v + 1) * sizeof(int));
  l.nrm_off = l.pos_off + ms_align(v * 3 * sizeof(float));
  l.col_off = l.nrm_off + ms_align(v * 3 * sizeof(float));
  l.mapped_off = l.col_off + ms_align(v * 3);
  l.keep_off = l.mapped_off + ms_align(f * 3 * sizeof(int));
  l.ftotals_off = l.keep_off + ms_align(f * sizeof(int));
  l.vtotals_off = l.ftotals_off + ms_align(static_cast<size_t>(ms_blocks(F)) * sizeof(int));
  l.total = l.vtotals_off + ms_align(static_cast<size_t>(ms_blocks(V)) * sizeof(int));
  return l;
}

bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

bool out_of_range(long long V, long long F) { return V > kMsMaxElements || F > kMsMaxElements; }

}  // namespace

}  // namespace dvmvs

extern "C" size_t dvmvs_mesh_simplify_workspace_bytes(long long V, long long F) {
  if (V < 0 || F < 0 || dvmvs::out_of_range(V, F)) return 0;
  return dvmvs::ms_layout(V, F).total;
}

extern "C" int dvmvs_mesh_simplify_keys(const int* faces, long long V, long long F, const long long* sorted_index, const void* voxel_workspace,
                                        const long long* voxel_counts, void* workspace, size_t workspace_bytes, int* incidence_keys, int* third,
                                        long long* pair, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!sorted_index || !voxel_workspace || !voxel_counts || !workspace || V < 1 || F < 0) return DVMVS_EINVAL;
  if (F > 0 && (!faces || !incidence_keys || !third || !pair)) return DVMVS_EINVAL;
  if (misaligned(faces, 4) || misaligned(sorted_index, 8) || misaligned(voxel_counts, 8) || misaligned(workspace, 16) ||
      misaligned(incidence_keys, 4) || misaligned(third, 4) || misaligned(pair, 8))
    return DVMVS_EINVAL;
  if (out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  const MsLayout l = ms_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  const int* starts = nullptr;
  const float* sorted_pts = nullptr;
  const int rc = dvmvs_voxel_downsample_runs(V, voxel_workspace, &starts, &sorted_pts);
  if (rc != 0) return rc;
  char* ws = static_cast<char*>(workspace);
  int* cluster = reinterpret_cast<int*>(ws);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ms_cluster_kernel, dim3(ms_grid(V)), dim3(kMsBlock), 0, s, sorted_index, starts, voxel_counts, V, cluster,
                     reinterpret_cast<int*>(ws + l.ref_off));
  if (F > 0)
    hipLaunchKernelGGL(ms_face_map_kernel, dim3(ms_grid(F)), dim3(kMsBlock), 0, s, faces, F, V, cluster, reinterpret_cast<int*>(ws + l.mapped_off),
                       reinterpret_cast<int*>(ws + l.keep_off), incidence_keys, third, pair);
  return launch_status();
}

extern "C" int dvmvs_mesh_simplify_pair_keys(const long long* pair, const long long* third_order, long long F, long long* out,
                                             dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (F < 0 || (F > 0 && (!pair || !third_order || !out))) return DVMVS_EINVAL;
  if (misaligned(pair, 8) || misaligned(third_order, 8) || misaligned(out, 8)) return DVMVS_EINVAL;
  if (F > kMsMaxElements) return DVMVS_EUNSUPPORTED;
  if (F == 0) return 0;
  hipLaunchKernelGGL(ms_gather_kernel, dim3(ms_grid(F)), dim3(kMsBlock), 0, static_cast<hipStream_t>(stream), pair, third_order, F, out);
  return launch_status();
}

extern "C" int dvmvs_mesh_simplify_count(const float* verts, const float* normals, const unsigned char* colors, long long V, const int* faces,
                                         long long F, double voxel, int average, const long long* sorted_index, const void* voxel_workspace,
                                         const long long* voxel_counts, const int* incidence_sorted, const long long* incidence_order,
                                         const int* third, const long long* third_order, const long long* pair_sorted,
                                         const long long* pair_order, void* workspace, size_t workspace_bytes, long long* counts,
                                         dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!verts || !sorted_index || !voxel_workspace || !voxel_counts || !workspace || !counts || V < 1 || F < 0) return DVMVS_EINVAL;
  if (F > 0 && (!faces || !incidence_sorted || !incidence_order || !third || !third_order || !pair_sorted || !pair_order)) return DVMVS_EINVAL;
  if (!(voxel > 0.0) || voxel == __builtin_inf() || (average != 0 && average != 1)) return DVMVS_EINVAL;
  if (misaligned(verts, 4) || misaligned(normals, 4) || misaligned(faces, 4) || misaligned(sorted_index, 8) || misaligned(voxel_counts, 8) ||
      misaligned(incidence_sorted, 4) || misaligned(incidence_order, 8) || misaligned(third, 4) || misaligned(third_order, 8) ||
      misaligned(pair_sorted, 8) || misaligned(pair_order, 8) || misaligned(workspace, 16) || misaligned(counts, 8))
    return DVMVS_EINVAL;
  if (out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  const MsLayout l = ms_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  const int* starts = nullptr;
  const float* sorted_pts = nullptr;
  const int rc = dvmvs_voxel_downsample_runs(V, voxel_workspace, &starts, &sorted_pts);
  if (rc != 0) return rc;
  char* ws = static_cast<char*>(workspace);
  int* ref = reinterpret_cast<int*>(ws + l.ref_off);
  int* inc_start = reinterpret_cast<int*>(ws + l.start_off);
  int* mapped = reinterpret_cast<int*>(ws + l.mapped_off);
  int* keep = reinterpret_cast<int*>(ws + l.keep_off);
  int* ftotals = reinterpret_cast<int*>(ws + l.ftotals_off);
  int* vtotals = reinterpret_cast<int*>(ws + l.vtotals_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const long long n_inc = 3 * F;
  // (one more thread than clusters: inc_start has M + 1 entries; incidence_sorted is not read when n_inc = 0)
  hipLaunchKernelGGL(ms_run_start_kernel, dim3(ms_grid(V + 1)), dim3(kMsBlock), 0, s, incidence_sorted, n_inc, voxel_counts, V, inc_start);
  hipLaunchKernelGGL(ms_solve_kernel, dim3(ms_grid(V)), dim3(kMsBlock), 0, s, verts, normals, colors, V, faces, F, sorted_pts, sorted_index, starts,
                     voxel_counts, inc_start, incidence_order, n_inc, voxel, average, reinterpret_cast<float*>(ws + l.pos_off),
                     reinterpret_cast<float*>(ws + l.nrm_off), reinterpret_cast<unsigned char*>(ws + l.col_off));
  if (F > 0) {
    hipLaunchKernelGGL(ms_face_head_kernel, dim3(ms_grid(F)), dim3(kMsBlock), 0, s, third, third_order, pair_sorted, pair_order, F, keep);
    hipLaunchKernelGGL(ms_keep_kernel, dim3(ms_grid(F)), dim3(kMsBlock), 0, s, mapped, keep, F, V, ref);
  }
  const int fblocks = ms_blocks(F), vblocks = ms_blocks(V);
  hipLaunchKernelGGL(ms_flag_count_kernel, dim3(fblocks + vblocks), dim3(kMsBlock), 0, s, keep, F, ref, V, fblocks, ftotals, vtotals);
  hipLaunchKernelGGL(ms_scan_blocks_kernel, dim3(1), dim3(kMsScanThreads), 0, s, ftotals, fblocks, vtotals, vblocks, voxel_counts, counts);
  return launch_status();
}

extern "C" int dvmvs_mesh_simplify_emit(long long V, long long F, void* workspace, size_t workspace_bytes, long long V_out, long long F_out,
                                        float* verts_out, int* faces_out, float* normals_out, unsigned char* colors_out, int* vertex_cluster,
                                        int* face_index, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!workspace || V < 1 || F < 0) return DVMVS_EINVAL;
  if (V_out < 0 || F_out < 0 || V_out > V || F_out > F || (V_out > 0 && !verts_out) || (F_out > 0 && !faces_out)) return DVMVS_EINVAL;
  if (misaligned(workspace, 16) || misaligned(verts_out, 4) || misaligned(faces_out, 4) || misaligned(normals_out, 4) ||
      misaligned(vertex_cluster, 4) || misaligned(face_index, 4))
    return DVMVS_EINVAL;
  if (out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  const MsLayout l = ms_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  const int* cluster = reinterpret_cast<const int*>(ws);
  int* new_index = reinterpret_cast<int*>(ws + l.index_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ms_emit_verts_kernel, dim3(ms_blocks(V)), dim3(kMsBlock), 0, s, reinterpret_cast<const float*>(ws + l.pos_off),
                     reinterpret_cast<const float*>(ws + l.nrm_off), reinterpret_cast<const unsigned char*>(ws + l.col_off),
                     reinterpret_cast<const int*>(ws + l.ref_off), V, reinterpret_cast<const int*>(ws + l.vtotals_off), V_out, new_index, verts_out,
                     V_out > 0 ? normals_out : nullptr, V_out > 0 ? colors_out : nullptr);
  if (F_out > 0)
    hipLaunchKernelGGL(ms_emit_faces_kernel, dim3(ms_blocks(F)), dim3(kMsBlock), 0, s, reinterpret_cast<const int*>(ws + l.mapped_off),
                       reinterpret_cast<const int*>(ws + l.keep_off), F, V, reinterpret_cast<const int*>(ws + l.ftotals_off), new_index, F_out,
                       faces_out, face_index);
  if (vertex_cluster) hipLaunchKernelGGL(ms_emit_index_kernel, dim3(ms_grid(V)), dim3(kMsBlock), 0, s, cluster, new_index, V, vertex_cluster);
  return launch_status();
}
