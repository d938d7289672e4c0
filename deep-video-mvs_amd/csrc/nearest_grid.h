// The uniform grid over a point cloud that csrc/nearest_points.hip builds, for the files that search it (nearest_points.hip: the nearest
// target; point_neighbours.hip: the k nearest and the targets within a radius).  Here: the header the build leaves at the workspace's
// start, the cell function (the SAME fp32 statements for targets, queries and the box's far corner), the layouts of the two workspaces,
// and the binning of a query cloud (defined in nearest_points.hip with its kernels).  The ordered wave sum of the one-workgroup reductions
// is dvmvs_device.h's wave_sum.
// The grid, its search bound and their fp32 margins are described at the head of nearest_points.hip.
#pragma once
#include "dvmvs_device.h"

namespace dvmvs {

constexpr int kNnBlock = 256;
constexpr int kNnBboxGroups = 256;          // workgroups of the box reduction at most
constexpr int kNnScanCells = 4 * kNnBlock;  // cells per workgroup of the scan
constexpr int kNnScanThreads = 1024;        // the one workgroup that scans the workgroup totals
constexpr long long kNnMaxPoints = 1LL << 28;
constexpr int kNnMaxCells = 1 << 22;
constexpr int kNnMaxDim = 1024;
constexpr int kNnMetricThreads = 1024;

struct NnHeader {
  float mn[3], mx[3];
  float inv_h, h_lo;
  int dim[3];
  int ncells;
};

typedef unsigned int uint4v __attribute__((ext_vector_type(4)));      // a sorted point: the bits of x, y, z and the original index

__device__ inline int nn_cell_axis(float x, float mn, float mx, float inv_h, int dim) {
  const float c = fminf(fmaxf(x, mn), mx);                 // the projection onto the box (exact)
  const int k = static_cast<int>((c - mn) * inv_h);        // >= 0: truncation is floor
  return min(max(k, 0), dim - 1);                          // no effect on finite input (nearest_points.hip)
}

__device__ inline int nn_cell(const NnHeader& h, float x, float y, float z, int& cx, int& cy, int& cz) {
  cx = nn_cell_axis(x, h.mn[0], h.mx[0], h.inv_h, h.dim[0]);
  cy = nn_cell_axis(y, h.mn[1], h.mx[1], h.inv_h, h.dim[1]);
  cz = nn_cell_axis(z, h.mn[2], h.mx[2], h.inv_h, h.dim[2]);
  return (cx * h.dim[1] + cy) * h.dim[2] + cz;
}

inline size_t nn_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

inline int nn_capacity(long long m) {
  const long long c = 4 * m < 64 ? 64 : 4 * m;
  return static_cast<int>(c < kNnMaxCells ? c : kNnMaxCells);
}

// Target workspace: header | box partials [256, 6] | scan totals [4096] | cells [capacity] | sorted [M] x 16 bytes.
struct NnLayout {
  size_t partials_off, totals_off, cells_off, sorted_off, total;
  int capacity;
};

inline NnLayout nn_layout(long long m) {
  NnLayout l;
  l.capacity = nn_capacity(m);
  l.partials_off = nn_align(sizeof(NnHeader));
  l.totals_off = l.partials_off + nn_align(kNnBboxGroups * 6 * sizeof(float));
  l.cells_off = l.totals_off + nn_align(static_cast<size_t>(kNnMaxCells / kNnScanCells) * sizeof(int));
  l.sorted_off = l.cells_off + nn_align(static_cast<size_t>(l.capacity) * sizeof(int));
  l.total = l.sorted_off + nn_align(static_cast<size_t>(m) * 16);
  return l;
}

// Query workspace: scan totals [4096] | cells [capacity of M] | sorted [N] x 16 bytes.
struct NnQueryLayout {
  size_t cells_off, sorted_off, total;
};

inline NnQueryLayout nn_query_layout(long long n, long long m) {
  NnQueryLayout l;
  l.cells_off = nn_align(static_cast<size_t>(kNnMaxCells / kNnScanCells) * sizeof(int));
  l.sorted_off = l.cells_off + nn_align(static_cast<size_t>(nn_capacity(m)) * sizeof(int));
  l.total = l.sorted_off + nn_align(static_cast<size_t>(n) * 16);
  return l;
}

// count -> scan -> scatter of `n` points into the grid of `hdr`: `cells` ends as the cells' ends, `sorted` as the binned copy
// (nearest_points.hip; five launches and a memset on `s`, integer atomics only)
int nn_bin(const float* pts, int n, const NnHeader* hdr, int capacity, int* cells, int* totals, uint4v* sorted, hipStream_t s);

}  // namespace dvmvs
