// Exact nearest-point distances between two point clouds (gfx950), and the six reconstruction metrics that reduce to them
// (accuracy, completeness, chamfer, precision, recall, F-score: dvmvs/errors.py::compute_reconstruction_errors).
//   dvmvs_nearest_build         : target fp32 [M,3] -> a uniform grid over its bounding box, in the workspace
//   dvmvs_nearest_distance_fwd  : query fp32 [N,3] -> dist fp32 [N] (and index int32 [N]) against a built grid
//   dvmvs_distance_metrics_fwd  : two distance arrays and a threshold -> the row of six metrics and two counts
//
// Arithmetic contract (restated by tests/nearest_reference.py):  d2(q, t) = (dx*dx + dy*dy) + dz*dz with dx = q.x - t.x, ...; every
// operation rounded to fp32, nothing contracted into an FMA (contract(off) for the whole file);  dist[i] = sqrt(min_j d2(q_i, t_j)),
// correctly rounded;  index[i] = the smallest j that attains the minimum.  A minimum (with the smallest index among equals) does not
// depend on the order of evaluation, so the result is the brute force's, bit for bit; the grid only decides which j are SKIPPED, and a
// j is skipped only when its d2 is provably larger than the minimum found (search bound below).
//
// Build (8 enqueues, no host read; every size the host needs follows from M):
//   1. nn_bbox_kernel     per-workgroup min / max of the coordinates (min and max do not depend on the order either)
//   2. nn_header_kernel   one workgroup: the box, the cell edge h and the grid dimensions -> NnHeader at the workspace's start
//   3. memset + nn_count_kernel   points per cell (integer atomics)
//   4. nn_scan_*          exclusive scan of the cell counts over three launches (1024 cells per workgroup, one workgroup for the totals; block_exclusive_scan and scan_totals of dvmvs_device.h)
//   5. nn_scatter_kernel  point -> slot atomicAdd(cell's cursor): sorted copy {x, y, z, original index}; the cursors end as the cells' ENDS
// The order of the points inside a cell depends on the order the atomics arrive in; the results do not (minimum, smallest index).
//
// The grid.  cell_a(x) = int((clamp(x, mn_a, mx_a) - mn_a) * inv_h), the SAME fp32 statements for targets, for queries and for the box's
// far corner, which defines dim_a = cell_a(mx_a) + 1: the function is monotone in x, so every point's cell is inside the grid without a
// clamp of the index.  h is chosen on the device so that dim_x dim_y dim_z <= the capacity 4 M (at most 2^22) and every dim_a <= 1024;
// an axis without extent has one layer of cells; a box without extent, or with a longest extent outside [1e-12, 1e12], has ONE cell
// (inv_h = 0: the search is then the brute force).
//
// Search bound.  A query q is searched around the cell of p = its clamp onto the box, ring by ring in Chebyshev cell distance.  After
// ring r every unvisited target t has |cell_a(t) - cell_a(p)| >= r + 1 on some axis a, so with s(x) = fl(fl(x - mn) inv_h):
// s(t) - s(p) > r.  Both subtractions and both products carry a relative error <= 2^-24, the operands are <= E_a (the extent), so
// |t_a - p_a| > r / inv_h - 4.0002 * 2^-24 * E_a >= r h (1 - 2^-24) - 2^-22 * 1024 h  (dim_a <= 1024 gives E_a < 1024 h (1 + 2^-22)),
// i.e. |t_a - p_a| > r h (1 - 2^-11) for r >= 1; and |q - t| >= |p - t| because projection onto a convex box is non-expansive and t is
// in the box.  The computed d2(q, t) is below the exact square by at most 4 roundings, a factor (1 - 2^-21).  The kernel stops after
// ring r when best <= fl(r h_lo)^2 * 0.998 with h_lo = fl(h (1 - 2^-10)): the right side is below r^2 h^2 (1 - 2^-10) (1 - 2^-21) by
// more than its own three roundings (h >= 1e-15 keeps the squares normal numbers), so every unvisited d2 is STRICTLY larger than the
// best one (ties, and so the index, are decided among visited points only).  A product that underflows only postpones the stop.
// There is no stop after ring 0, where the bound is 0: a computed d2 of 0 (equal points, or differences that underflow) could tie with
// an unvisited one, so ring 1 is always searched unless the grid ends first.  Otherwise the search goes on until the rings have covered
// the grid: it never gives up.
//
// Queries are binned with the target's grid by the same count / scan / scatter kernels and processed in cell order, so a wave's
// lanes sit in neighbouring cells: they load the same target runs (a ring's cells along z are contiguous in the sorted copy) and make
// about the same number of rings.  Results are stored through the original index.
//
// Preconditions, not checked on the device: finite coordinates.  (A NaN cannot make an access go out of bounds: fmin / fmax drop it and
// the cell index is clamped; the distances are then meaningless.)
#include "dvmvs_device.h"
#include "nearest_grid.h"      // NnHeader, nn_cell, the workspace layouts: shared with point_neighbours.hip

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

// partials [gridDim.x, 6]: min x, y, z, max x, y, z of the points i = global thread, + threads, ...
__global__ __launch_bounds__(kNnBlock) void nn_bbox_kernel(const float* __restrict__ pts, int n, float* __restrict__ partials) {
  __shared__ float s[kNnBlock / kWave][6];
  const float inf = __builtin_inff();
  float v[6] = {inf, inf, inf, -inf, -inf, -inf};
  for (int i = blockIdx.x * kNnBlock + threadIdx.x; i < n; i += gridDim.x * kNnBlock) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = pts[static_cast<size_t>(i) * 3 + a];
      v[a] = fminf(v[a], x);
      v[3 + a] = fmaxf(v[3 + a], x);
    }
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = fminf(v[a], __shfl_xor(v[a], m, kWave));
      v[3 + a] = fmaxf(v[3 + a], __shfl_xor(v[3 + a], m, kWave));
    }
  }
  const int wave = threadIdx.x / kWave;
  if (threadIdx.x % kWave == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) s[wave][a] = v[a];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float r = s[0][a];
    for (int w = 1; w < kNnBlock / kWave; ++w) r = a < 3 ? fminf(r, s[w][a]) : fmaxf(r, s[w][a]);
    partials[blockIdx.x * 6 + a] = r;
  }
}

// One workgroup of 64 threads: the box of the partial boxes, then (thread 0) the cell edge and the grid dimensions.
__global__ __launch_bounds__(kWave) void nn_header_kernel(const float* __restrict__ partials, int groups, int capacity, NnHeader* __restrict__ hdr) {
  const float inf = __builtin_inff();
  float v[6] = {inf, inf, inf, -inf, -inf, -inf};
  for (int g = threadIdx.x; g < groups; g += kWave) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = fminf(v[a], partials[g * 6 + a]);
      v[3 + a] = fmaxf(v[3 + a], partials[g * 6 + 3 + a]);
    }
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = fminf(v[a], __shfl_xor(v[a], m, kWave));
      v[3 + a] = fmaxf(v[3 + a], __shfl_xor(v[3 + a], m, kWave));
    }
  }
  if (threadIdx.x != 0) return;
  NnHeader h;
  float ext[3], emax = 0.0f;
  double volume = 1.0;
  int axes = 0;
  bool finite = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    h.mn[a] = v[a];
    h.mx[a] = v[3 + a];
    ext[a] = v[3 + a] - v[a];
    finite = finite && ext[a] >= 0.0f && ext[a] < inf;
    emax = fmaxf(emax, ext[a]);
    if (ext[a] > 0.0f) {
      volume *= static_cast<double>(ext[a]);
      ++axes;
    }
    h.dim[a] = 1;
  }
  h.inv_h = 0.0f;       // one cell: the search is the brute force
  h.h_lo = 0.0f;
  if (finite && emax >= 1e-12f && emax <= 1e12f) {
    // the edge at which the occupied axes give `capacity` cells, not below the one that gives ~1000 cells on the longest axis; then
    // grown until the dimensions, computed with the cell function itself, fit (a thin axis collapses to one layer on the way)
    const double per_cell = volume / static_cast<double>(capacity);
    const double h0 = axes == 1 ? per_cell : (axes == 2 ? sqrt(per_cell) : cbrt(per_cell));
    float edge = fmaxf(static_cast<float>(h0), emax / 1000.0f);
    for (int it = 0; it < 128; ++it, edge *= 1.125f) {
      const float inv = 1.0f / edge;
      int d[3];
      long long cells = 1;
      bool fits = inv > 0.0f && inv < inf;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float s = ext[a] * inv;                     // the cell function at the box's far corner: (mx - mn) * inv_h
        fits = fits && s < static_cast<float>(kNnMaxDim);
        d[a] = fits ? static_cast<int>(s) + 1 : 1;
        cells *= d[a];
      }
      if (fits && cells <= capacity) {
        h.inv_h = inv;
        h.h_lo = edge * 0.9990234375f;                    // h (1 - 2^-10)
#pragma unroll
        for (int a = 0; a < 3; ++a) h.dim[a] = d[a];
        break;
      }
    }
  }
  h.ncells = h.dim[0] * h.dim[1] * h.dim[2];
  *hdr = h;
}

__global__ __launch_bounds__(kNnBlock) void nn_count_kernel(const float* __restrict__ pts, int n, const NnHeader* __restrict__ hdr, int* cells) {
  const int i = blockIdx.x * kNnBlock + threadIdx.x;
  if (i >= n) return;
  const NnHeader h = *hdr;
  int cx, cy, cz;
  const size_t o = static_cast<size_t>(i) * 3;
  const int c = nn_cell(h, pts[o], pts[o + 1], pts[o + 2], cx, cy, cz);
  atomicAdd(cells + c, 1);
}

__global__ __launch_bounds__(kNnBlock) void nn_scan_totals_kernel(const int* __restrict__ cells, int capacity, int* __restrict__ totals) {
  __shared__ int lds[kNnBlock / 64];
  const int first = (blockIdx.x * kNnBlock + threadIdx.x) * 4;
  int v = 0;
  for (int e = 0; e < 4 && first + e < capacity; ++e) v += cells[first + e];
  int total;
  block_exclusive_scan<kNnBlock>(v, lds, total);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// One workgroup: totals[b] <- the sum of the totals before b.
__global__ __launch_bounds__(kNnScanThreads) void nn_scan_blocks_kernel(int* __restrict__ totals, int nblocks) {
  __shared__ int s[kNnScanThreads];
  scan_totals<kNnScanThreads>(totals, nblocks, s);
}

// cells[c] <- the number of points in the cells before c (the cell's first slot, and the scatter's cursor)
__global__ __launch_bounds__(kNnBlock) void nn_scan_apply_kernel(int* __restrict__ cells, int capacity, const int* __restrict__ offsets) {
  __shared__ int lds[kNnBlock / 64];
  const int first = (blockIdx.x * kNnBlock + threadIdx.x) * 4;
  int c[4], v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    c[e] = first + e < capacity ? cells[first + e] : 0;
    v += c[e];
  }
  int total;
  int o = offsets[blockIdx.x] + block_exclusive_scan<kNnBlock>(v, lds, total);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (first + e < capacity) cells[first + e] = o;
    o += c[e];
  }
}

__global__ __launch_bounds__(kNnBlock) void nn_scatter_kernel(const float* __restrict__ pts, int n, const NnHeader* __restrict__ hdr, int* cells,
                                                              uint4v* __restrict__ sorted) {
  const int i = blockIdx.x * kNnBlock + threadIdx.x;
  if (i >= n) return;
  const NnHeader h = *hdr;
  int cx, cy, cz;
  const size_t o = static_cast<size_t>(i) * 3;
  const float x = pts[o], y = pts[o + 1], z = pts[o + 2];
  const int c = nn_cell(h, x, y, z, cx, cy, cz);
  const int slot = atomicAdd(cells + c, 1);
  if (slot < 0 || slot >= n) return;          // cannot happen after a count of the same points; keeps a stale workspace in bounds
  uint4v p;
  p[0] = __float_as_uint(x);
  p[1] = __float_as_uint(y);
  p[2] = __float_as_uint(z);
  p[3] = static_cast<unsigned int>(i);
  sorted[slot] = p;
}

struct NnBest {
  float d2;
  int j;
};

// targets of the cells c0..c1 (consecutive along z: one run of the sorted copy)
__device__ inline void nn_scan_run(const uint4v* __restrict__ sorted_t, const int* __restrict__ cell_end, int m, int c0, int c1, float qx,
                                   float qy, float qz, NnBest& best) {
  const int begin = c0 > 0 ? cell_end[c0 - 1] : 0;
  const int end = min(cell_end[c1], m);
  for (int k = max(begin, 0); k < end; ++k) {
    const uint4v t = sorted_t[k];
    const float dx = qx - __uint_as_float(t[0]), dy = qy - __uint_as_float(t[1]), dz = qz - __uint_as_float(t[2]);
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const int j = static_cast<int>(t[3]);
    if (d2 < best.d2 || (d2 == best.d2 && j < best.j)) {
      best.d2 = d2;
      best.j = j;
    }
  }
}

__global__ __launch_bounds__(kNnBlock) void nn_query_kernel(const uint4v* __restrict__ sorted_q, int n, const uint4v* __restrict__ sorted_t, int m,
                                                            const int* __restrict__ cell_end, const NnHeader* __restrict__ hdr,
                                                            float* __restrict__ dist, int* __restrict__ index) {
  const int i = blockIdx.x * kNnBlock + threadIdx.x;
  if (i >= n) return;
  const NnHeader h = *hdr;
  const uint4v q = sorted_q[i];
  const float qx = __uint_as_float(q[0]), qy = __uint_as_float(q[1]), qz = __uint_as_float(q[2]);
  const unsigned int qi = q[3];
  if (qi >= static_cast<unsigned int>(n)) return;
  int cx, cy, cz;
  nn_cell(h, qx, qy, qz, cx, cy, cz);
  const int X = h.dim[0], Y = h.dim[1], Z = h.dim[2];
  const int rmax = max(max(max(cx, X - 1 - cx), max(cy, Y - 1 - cy)), max(cz, Z - 1 - cz));     // the ring that reaches the last cell
  NnBest best = {__builtin_inff(), 0x7fffffff};
  for (int r = 0;; ++r) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, X - 1), y0 = max(cy - r, 0), y1 = min(cy + r, Y - 1);
    const int zlo = max(cz - r, 0), zhi = min(cz + r, Z - 1);
    for (int x = x0; x <= x1; ++x) {
      for (int y = y0; y <= y1; ++y) {
        const int base = (x * Y + y) * Z;
        if (abs(x - cx) == r || abs(y - cy) == r) {          // a column on the ring's side faces: its whole z range
          nn_scan_run(sorted_t, cell_end, m, base + zlo, base + zhi, qx, qy, qz, best);
        } else {                                             // inside them: the ring's two caps
          if (cz - r >= 0) nn_scan_run(sorted_t, cell_end, m, base + cz - r, base + cz - r, qx, qy, qz, best);
          if (cz + r <= Z - 1) nn_scan_run(sorted_t, cell_end, m, base + cz + r, base + cz + r, qx, qy, qz, best);
        }
      }
    }
    if (r >= rmax) break;                                    // every cell has been visited
    const float rb = static_cast<float>(r) * h.h_lo;
    if (r >= 1 && best.d2 <= rb * rb * 0.998f) break;        // every unvisited d2 is strictly larger (file comment); never after ring 0
  }
  dist[qi] = sqrtf(best.d2);
  if (index) index[qi] = best.j;
}

// ONE workgroup, so the order of the additions is a function of (na, nb) alone: thread t adds the elements t, t + 1024, ... of an array in
// fp64, the 64 lanes of a wave are combined by the butterfly, the 16 waves in order by thread 0.
__global__ __launch_bounds__(kNnMetricThreads) void nn_metrics_kernel(const float* __restrict__ dist_a, long long na, const float* __restrict__ dist_b,
                                                                     long long nb, float threshold, float* __restrict__ row,
                                                                     long long* __restrict__ counts) {
  __shared__ double s_sum[2][kNnMetricThreads / kWave];
  __shared__ unsigned long long s_cnt[2][kNnMetricThreads / kWave];
  const int t = threadIdx.x;
  for (int side = 0; side < 2; ++side) {
    const float* d = side == 0 ? dist_a : dist_b;
    const long long n = side == 0 ? na : nb;
    double s = 0.0;
    unsigned long long c = 0;
    for (long long i = t; i < n; i += kNnMetricThreads) {
      const float v = d[i];
      s += static_cast<double>(v);
      c += v < threshold ? 1u : 0u;
    }
    s = wave_sum(s);
    c = wave_sum(c);
    if (t % kWave == 0) {
      s_sum[side][t / kWave] = s;
      s_cnt[side][t / kWave] = c;
    }
  }
  __syncthreads();
  if (t != 0) return;
  double mean[2], share[2];
  for (int side = 0; side < 2; ++side) {
    double s = s_sum[side][0];
    unsigned long long c = s_cnt[side][0];
    for (int w = 1; w < kNnMetricThreads / kWave; ++w) {
      s += s_sum[side][w];
      c += s_cnt[side][w];
    }
    const double n = static_cast<double>(side == 0 ? na : nb);
    mean[side] = s / n;
    share[side] = static_cast<double>(c) / n;
    if (counts) counts[side] = static_cast<long long>(c);
  }
  row[0] = static_cast<float>(mean[0]);
  row[1] = static_cast<float>(mean[1]);
  row[2] = static_cast<float>((mean[0] + mean[1]) / 2.0);
  row[3] = static_cast<float>(share[0]);
  row[4] = static_cast<float>(share[1]);
  const double pr = share[0] + share[1];
  row[5] = pr > 0.0 ? static_cast<float>(2.0 * share[0] * share[1] / pr) : 0.0f;
}

int nn_scan_blocks(int capacity) { return (capacity + kNnScanCells - 1) / kNnScanCells; }      // <= 4096

int nn_bbox_groups(long long m) {
  const long long g = (m + kNnBlock - 1) / kNnBlock;
  return static_cast<int>(g < kNnBboxGroups ? g : kNnBboxGroups);
}

}  // namespace

// count -> scan -> scatter of `n` points into the grid of `hdr`: `cells` ends as the cells' ends, `sorted` as the binned copy
int nn_bin(const float* pts, int n, const NnHeader* hdr, int capacity, int* cells, int* totals, uint4v* sorted, hipStream_t s) {
  DVMVS_RETURN_IF_HIP(hipMemsetAsync(cells, 0, static_cast<size_t>(capacity) * sizeof(int), s));
  const dim3 points((n + kNnBlock - 1) / kNnBlock), block(kNnBlock), scan(nn_scan_blocks(capacity));
  hipLaunchKernelGGL(nn_count_kernel, points, block, 0, s, pts, n, hdr, cells);
  hipLaunchKernelGGL(nn_scan_totals_kernel, scan, block, 0, s, cells, capacity, totals);
  hipLaunchKernelGGL(nn_scan_blocks_kernel, dim3(1), dim3(kNnScanThreads), 0, s, totals, static_cast<int>(scan.x));
  hipLaunchKernelGGL(nn_scan_apply_kernel, scan, block, 0, s, cells, capacity, totals);
  hipLaunchKernelGGL(nn_scatter_kernel, points, block, 0, s, pts, n, hdr, cells, sorted);
  return launch_status();
}

}  // namespace dvmvs

extern "C" size_t dvmvs_nearest_workspace_bytes(long long M) {
  if (M <= 0 || M > dvmvs::kNnMaxPoints) return 0;
  return dvmvs::nn_layout(M).total;
}

extern "C" size_t dvmvs_nearest_query_workspace_bytes(long long N, long long M) {
  if (N <= 0 || M <= 0 || N > dvmvs::kNnMaxPoints || M > dvmvs::kNnMaxPoints) return 0;
  return dvmvs::nn_query_layout(N, M).total;
}

extern "C" int dvmvs_nearest_build(const float* target, long long M, void* workspace, size_t workspace_bytes, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!target || !workspace || M < 1) return DVMVS_EINVAL;
  if (reinterpret_cast<uintptr_t>(target) % 4 != 0 || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return DVMVS_EINVAL;
  if (M > kNnMaxPoints) return DVMVS_EUNSUPPORTED;
  const NnLayout l = nn_layout(M);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  NnHeader* hdr = reinterpret_cast<NnHeader*>(ws);
  float* partials = reinterpret_cast<float*>(ws + l.partials_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int m = static_cast<int>(M), groups = nn_bbox_groups(M);
  hipLaunchKernelGGL(nn_bbox_kernel, dim3(groups), dim3(kNnBlock), 0, s, target, m, partials);
  hipLaunchKernelGGL(nn_header_kernel, dim3(1), dim3(kWave), 0, s, partials, groups, l.capacity, hdr);
  return nn_bin(target, m, hdr, l.capacity, reinterpret_cast<int*>(ws + l.cells_off), reinterpret_cast<int*>(ws + l.totals_off),
                reinterpret_cast<uint4v*>(ws + l.sorted_off), s);
}

extern "C" int dvmvs_nearest_distance_fwd(const float* query, long long N, const float* target, long long M, const void* workspace,
                                          void* query_workspace, size_t query_workspace_bytes, float* dist, int* index,
                                          dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (N < 0 || M < 1 || !target || !workspace) return DVMVS_EINVAL;
  if (N > 0 && (!query || !query_workspace || !dist)) return DVMVS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(dist) | reinterpret_cast<uintptr_t>(index)) % 4 != 0 ||
      (reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(query_workspace)) % 16 != 0) return DVMVS_EINVAL;
  if (N > kNnMaxPoints || M > kNnMaxPoints) return DVMVS_EUNSUPPORTED;
  if (N == 0) return 0;
  const NnLayout l = nn_layout(M);
  const NnQueryLayout ql = nn_query_layout(N, M);
  if (query_workspace_bytes < ql.total) return DVMVS_EINVAL;
  const char* ws = static_cast<const char*>(workspace);
  char* qws = static_cast<char*>(query_workspace);
  const NnHeader* hdr = reinterpret_cast<const NnHeader*>(ws);
  uint4v* sorted_q = reinterpret_cast<uint4v*>(qws + ql.sorted_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = static_cast<int>(N);
  const int rc = nn_bin(query, n, hdr, l.capacity, reinterpret_cast<int*>(qws + ql.cells_off), reinterpret_cast<int*>(qws), sorted_q, s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(nn_query_kernel, dim3((n + kNnBlock - 1) / kNnBlock), dim3(kNnBlock), 0, s, sorted_q, n,
                     reinterpret_cast<const uint4v*>(ws + l.sorted_off), static_cast<int>(M), reinterpret_cast<const int*>(ws + l.cells_off), hdr,
                     dist, index);
  return launch_status();
}

extern "C" int dvmvs_distance_metrics_fwd(const float* dist_a, long long Na, const float* dist_b, long long Nb, float threshold, float* row,
                                          long long* counts, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!dist_a || !dist_b || !row || Na < 1 || Nb < 1 || threshold != threshold) return DVMVS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(dist_a) | reinterpret_cast<uintptr_t>(dist_b) | reinterpret_cast<uintptr_t>(row)) % 4 != 0 ||
      reinterpret_cast<uintptr_t>(counts) % 8 != 0) return DVMVS_EINVAL;
  hipLaunchKernelGGL(nn_metrics_kernel, dim3(1), dim3(kNnMetricThreads), 0, static_cast<hipStream_t>(stream), dist_a, Na, dist_b, Nb, threshold,
                     row, counts);
  return launch_status();
}
