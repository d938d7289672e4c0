// Exact k-nearest-neighbour search, radius counts and statistical outlier scores of point clouds (gfx950), on the uniform grid that
// csrc/nearest_points.hip builds (dvmvs_nearest_build; csrc/nearest_grid.h is what the two files share).  dvmvs/outliers.py is the host form.
//   dvmvs_knn_fwd                 : query fp32 [N,3] -> dist fp32 [N,k], index int32 [N,k]: the k nearest targets of every query
//   dvmvs_radius_count_fwd        : query fp32 [N,3] -> count int32 [N]: min(targets within the radius, cap)
//   dvmvs_outlier_statistics_fwd  : dist / index [N,k] -> mean fp32 [N], keep uint8 [N], stats fp64 [4] (statistical outlier removal)
//
// Arithmetic contract, that of nearest_points.hip:  d2(q, t) = (dx*dx + dy*dy) + dz*dz, every operation rounded to fp32, nothing contracted
// into an FMA (contract(off) for the whole file); distances are sqrt(d2), correctly rounded.  The CANDIDATES of query i are the targets j
// with d2 <= cap2 = fl(max_distance * max_distance) (inf stays inf) and, with exclude_same_index, j != i (by index: a duplicate point at
// distance 0 is a neighbour).  Row i holds the k smallest candidates in ascending lexicographic order of (d2, j); missing slots are
// (inf, -1).  The set of the k smallest pairs (d2, j) of a set does not depend on the order in which the set is run through, so the rows
// are the brute force's, bit for bit; the grid only decides which j are SKIPPED, and a j is skipped only when it provably is no
// candidate or its pair is larger than the k-th pair found.
//
// k-NN kernel.  One query per lane, in cell order (the queries are binned by the target's grid: nn_bin), rings of cells in growing
// Chebyshev distance around the cell of the query's clamp onto the box, exactly as nn_query_kernel walks them.  A lane keeps its list of
// at most k pairs sorted in LDS, laid out [slot][lane] so that the lanes of a wave touch consecutive banks whatever slots they are at
// (the list is indexed by a run-time slot: as a register array it would live in scratch), and the k-th pair in two registers: the
// admission test  count < k || (d2, j) < (kd2, kj)  fails for most candidates once the list is full.  An admitted pair is inserted
// by shifting the larger entries one slot up from the end.  The kernel is instantiated for lists of 4, 8, 16 and 32 slots (8 KB .. 64 KB of
// LDS for the 256 lanes of a workgroup); a call runs the smallest that holds its k.
//
// Stop rule: the bound of nearest_points.hip, applied to the k-th best.  After ring r >= 1 every unvisited target t has a computed
// d2(q, t) STRICTLY larger than B = fl(fl(r h_lo)^2 * 0.998) (that file's head comment: the cell function's roundings, the non-expansive
// projection of q onto the box, the four roundings of d2 and the three of B itself are all inside the margins of h_lo and 0.998; h >=
// 1e-15 keeps B a normal number, so B > 0).  The walk stops after ring r >= 1
//   (a) when B >= cap2: every unvisited d2 > B >= cap2, so no unvisited target is a candidate; or
//   (b) when the list is full and kd2 <= B: every unvisited pair has d2 > B >= kd2, so it is lexicographically larger than the k-th
//       pair whatever its index, and could not enter.
// In both cases ties, and therefore indices, are decided among visited targets only.  It never stops after ring 0, where the bound is 0:
// a computed d2 of 0 (equal points, differences that underflow) could tie with an unvisited one.  Otherwise it goes on until the rings
// have covered the grid (r = rmax), so a list that cannot be filled (k > candidates) costs a walk over the whole grid unless
// max_distance ends it by (a): max_distance is what bounds the work for the far outliers.  A one-cell grid (h_lo = 0) has rmax = 0:
// the brute force.
//
// Radius count: the same walk with an integer that saturates at `cap`; it leaves the walk once saturated (the result is min(count,
// cap), so nothing more can change it, after any ring) or by (a) with cap2 = fl(radius * radius).
//
// Statistics (three launches, no host read; dvmvs/outliers.py::statistical_outliers):
//   1. pn_mean_kernel   m_i = fp32(fp64 sum of the found distances of row i in slot order / their number); inf for a row without one
//   2. pn_stats_kernel  ONE workgroup of 1024 threads, so the order of the additions is a function of N alone, the order of
//                       nn_metrics_kernel: thread t adds the elements t, t + 1024, ... in fp64 (an invalid one, m_i not finite, adds 0),
//                       the 64 lanes of a wave are combined by the xor butterfly, the 16 waves in order.  First n and mu = sum / n, then
//                       in a second pass sum (m_i - mu)^2, sigma = sqrt(that / (n - 1)) (0 for n < 2), threshold = mu + ratio * sigma;
//                       fp64 division and square root are the correctly rounded ones.  n == 0 gives mu = sigma = threshold = 0.
//   3. pn_keep_kernel   keep_i = m_i finite and fp64(m_i) <= threshold
// No float atomics anywhere; the only atomics are the integer ones of the binning.
//
// Preconditions, not checked on the device: finite coordinates (a NaN d2 fails every comparison and is never admitted; no access
// depends on it).
#include "dvmvs_device.h"
#include "nearest_grid.h"

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

constexpr int kPnMaxK = 32;
constexpr int kPnStatThreads = kNnMetricThreads;

// The ring walk of nn_query_kernel around the cell of (qx, qy, qz).  run(begin, end): the sorted targets of one run of cells along z,
// returns true to leave the walk at once;  stop(B): asked after every ring r >= 1 that is not the last, with the bound B of the file
// comment.
template <class Run, class Stop>
__device__ inline void pn_walk(const NnHeader& h, const int* __restrict__ cell_end, int m, float qx, float qy, float qz, Run run, Stop stop) {
  int cx, cy, cz;
  nn_cell(h, qx, qy, qz, cx, cy, cz);
  const int X = h.dim[0], Y = h.dim[1], Z = h.dim[2];
  const int rmax = max(max(max(cx, X - 1 - cx), max(cy, Y - 1 - cy)), max(cz, Z - 1 - cz));     // the ring that reaches the last cell
  auto cells = [&](int c0, int c1) {
    const int begin = c0 > 0 ? cell_end[c0 - 1] : 0;
    return run(max(begin, 0), min(cell_end[c1], m));
  };
  for (int r = 0;; ++r) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, X - 1), y0 = max(cy - r, 0), y1 = min(cy + r, Y - 1);
    const int zlo = max(cz - r, 0), zhi = min(cz + r, Z - 1);
    for (int x = x0; x <= x1; ++x) {
      for (int y = y0; y <= y1; ++y) {
        const int base = (x * Y + y) * Z;
        if (abs(x - cx) == r || abs(y - cy) == r) {          // a column on the ring's side faces: its whole z range
          if (cells(base + zlo, base + zhi)) return;
        } else {                                             // inside them: the ring's two caps
          if (cz - r >= 0 && cells(base + cz - r, base + cz - r)) return;
          if (cz + r <= Z - 1 && cells(base + cz + r, base + cz + r)) return;
        }
      }
    }
    if (r >= rmax) return;                                   // every cell has been visited
    const float rb = static_cast<float>(r) * h.h_lo;
    if (r >= 1 && stop(rb * rb * 0.998f)) return;            // never after ring 0
  }
}

template <int KCAP>
__global__ __launch_bounds__(kNnBlock) void pn_knn_kernel(const uint4v* __restrict__ sorted_q, int n, const uint4v* __restrict__ sorted_t, int m,
                                                          const int* __restrict__ cell_end, const NnHeader* __restrict__ hdr, int k, float cap2,
                                                          int exclude, float* __restrict__ dist, int* __restrict__ index) {
  __shared__ float s_d2[KCAP * kNnBlock];                    // [slot][lane]
  __shared__ int s_j[KCAP * kNnBlock];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * kNnBlock + lane;
  if (i >= n || k > KCAP) return;
  const NnHeader h = *hdr;
  const uint4v q = sorted_q[i];
  const float qx = __uint_as_float(q[0]), qy = __uint_as_float(q[1]), qz = __uint_as_float(q[2]);
  const unsigned int qi = q[3];
  if (qi >= static_cast<unsigned int>(n)) return;
  const int self = exclude ? static_cast<int>(qi) : -1;
  int count = 0;
  float kd2 = __builtin_inff();                              // the k-th pair, valid once count == k
  int kj = 0x7fffffff;
  pn_walk(h, cell_end, m, qx, qy, qz,
          [&](int begin, int end) {
            for (int e = begin; e < end; ++e) {
              const uint4v t = sorted_t[e];
              const float dx = qx - __uint_as_float(t[0]), dy = qy - __uint_as_float(t[1]), dz = qz - __uint_as_float(t[2]);
              const float d2 = (dx * dx + dy * dy) + dz * dz;
              const int j = static_cast<int>(t[3]);
              if (!(d2 <= cap2) || j == self) continue;
              if (count == k && !(d2 < kd2 || (d2 == kd2 && j < kj))) continue;
              int p = count < k ? count : k - 1;             // the slot that is free, or the k-th, which goes
              while (p > 0) {
                const float pd = s_d2[(p - 1) * kNnBlock + lane];
                const int pj = s_j[(p - 1) * kNnBlock + lane];
                if (pd < d2 || (pd == d2 && pj < j)) break;
                s_d2[p * kNnBlock + lane] = pd;
                s_j[p * kNnBlock + lane] = pj;
                --p;
              }
              s_d2[p * kNnBlock + lane] = d2;
              s_j[p * kNnBlock + lane] = j;
              if (count < k) ++count;
              if (count == k) {
                kd2 = s_d2[(k - 1) * kNnBlock + lane];
                kj = s_j[(k - 1) * kNnBlock + lane];
              }
            }
            return false;
          },
          [&](float bound) { return bound >= cap2 || (count == k && kd2 <= bound); });
  const size_t row = static_cast<size_t>(qi) * k;
  for (int s = 0; s < k; ++s) {
    const bool found = s < count;
    dist[row + s] = found ? sqrtf(s_d2[s * kNnBlock + lane]) : __builtin_inff();
    index[row + s] = found ? s_j[s * kNnBlock + lane] : -1;
  }
}

__global__ __launch_bounds__(kNnBlock) void pn_radius_kernel(const uint4v* __restrict__ sorted_q, int n, const uint4v* __restrict__ sorted_t, int m,
                                                             const int* __restrict__ cell_end, const NnHeader* __restrict__ hdr, float r2, int cap,
                                                             int exclude, int* __restrict__ count_out) {
  const int i = blockIdx.x * kNnBlock + threadIdx.x;
  if (i >= n) return;
  const NnHeader h = *hdr;
  const uint4v q = sorted_q[i];
  const float qx = __uint_as_float(q[0]), qy = __uint_as_float(q[1]), qz = __uint_as_float(q[2]);
  const unsigned int qi = q[3];
  if (qi >= static_cast<unsigned int>(n)) return;
  const int self = exclude ? static_cast<int>(qi) : -1;
  int count = 0;
  pn_walk(h, cell_end, m, qx, qy, qz,
          [&](int begin, int end) {
            for (int e = begin; e < end; ++e) {
              const uint4v t = sorted_t[e];
              const float dx = qx - __uint_as_float(t[0]), dy = qy - __uint_as_float(t[1]), dz = qz - __uint_as_float(t[2]);
              const float d2 = (dx * dx + dy * dy) + dz * dz;
              if (d2 <= r2 && static_cast<int>(t[3]) != self && ++count >= cap) return true;      // saturated
            }
            return false;
          },
          [&](float bound) { return bound >= r2; });
  count_out[qi] = count;
}

__device__ inline bool pn_finite(float v) { return fabsf(v) < __builtin_inff(); }      // false for a NaN

__global__ __launch_bounds__(kNnBlock) void pn_mean_kernel(const float* __restrict__ dist, const int* __restrict__ index, long long n, int k,
                                                           float* __restrict__ mean) {
  const long long i = static_cast<long long>(blockIdx.x) * kNnBlock + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  int c = 0;
  for (int slot = 0; slot < k; ++slot) {
    if (index[i * k + slot] >= 0) {
      s += static_cast<double>(dist[i * k + slot]);
      ++c;
    }
  }
  mean[i] = c > 0 ? static_cast<float>(s / static_cast<double>(c)) : __builtin_inff();
}

// the sum over the workgroup in the fixed order, in every thread (each adds the 16 wave sums in order itself: the same bits everywhere)
__device__ inline void pn_block_sum(double& s, unsigned long long& c, double* s_sum, unsigned long long* s_cnt) {
  const int t = threadIdx.x;
  s = wave_sum(s);
  c = wave_sum(c);
  __syncthreads();                                           // the previous use of the arrays is over
  if (t % kWave == 0) {
    s_sum[t / kWave] = s;
    s_cnt[t / kWave] = c;
  }
  __syncthreads();
  s = s_sum[0];
  c = s_cnt[0];
  for (int w = 1; w < kPnStatThreads / kWave; ++w) {
    s += s_sum[w];
    c += s_cnt[w];
  }
}

__global__ __launch_bounds__(kPnStatThreads) void pn_stats_kernel(const float* __restrict__ mean, long long n, double ratio,
                                                                  double* __restrict__ stats) {
  __shared__ double s_sum[kPnStatThreads / kWave];
  __shared__ unsigned long long s_cnt[kPnStatThreads / kWave];
  const int t = threadIdx.x;
  double s = 0.0;
  unsigned long long c = 0;
  for (long long i = t; i < n; i += kPnStatThreads) {
    const float v = mean[i];
    const bool valid = pn_finite(v);
    s += valid ? static_cast<double>(v) : 0.0;
    c += valid ? 1u : 0u;
  }
  pn_block_sum(s, c, s_sum, s_cnt);
  const double count = static_cast<double>(c);
  const double mu = c > 0 ? s / count : 0.0;
  double ss = 0.0;
  unsigned long long unused = 0;
  for (long long i = t; i < n; i += kPnStatThreads) {
    const float v = mean[i];
    const double d = static_cast<double>(v) - mu;
    ss += pn_finite(v) ? d * d : 0.0;
  }
  pn_block_sum(ss, unused, s_sum, s_cnt);
  if (t != 0) return;
  const double sigma = c >= 2 ? sqrt(ss / (count - 1.0)) : 0.0;
  stats[0] = count;
  stats[1] = mu;
  stats[2] = sigma;
  stats[3] = mu + ratio * sigma;
}

__global__ __launch_bounds__(kNnBlock) void pn_keep_kernel(const float* __restrict__ mean, long long n, const double* __restrict__ stats,
                                                           unsigned char* __restrict__ keep) {
  const long long i = static_cast<long long>(blockIdx.x) * kNnBlock + threadIdx.x;
  if (i >= n) return;
  const float v = mean[i];
  keep[i] = pn_finite(v) && static_cast<double>(v) <= stats[3] ? 1 : 0;
}

// the checks the two searches share; 1: nothing to do
int pn_check(const float* query, long long N, const float* target, long long M, const void* workspace, void* query_workspace,
             size_t query_workspace_bytes, int exclude, const void* out_a, const void* out_b) {
  if (N < 0 || M < 1 || !target || !workspace || (exclude != 0 && exclude != 1)) return DVMVS_EINVAL;
  if (N > 0 && (!query || !query_workspace || !out_a || !out_b)) return DVMVS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(out_a) |
       reinterpret_cast<uintptr_t>(out_b)) % 4 != 0 ||
      (reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(query_workspace)) % 16 != 0) return DVMVS_EINVAL;
  if (N > kNnMaxPoints || M > kNnMaxPoints) return DVMVS_EUNSUPPORTED;
  if (N == 0) return 1;
  if (query_workspace_bytes < nn_query_layout(N, M).total) return DVMVS_EINVAL;
  return 0;
}

struct PnGrid {
  const NnHeader* hdr;
  const uint4v* sorted_t;
  const int* cell_end;
  uint4v* sorted_q;
};

// bins the queries with the target's grid; the pointers the search kernels take
int pn_bin(const float* query, int n, long long M, const void* workspace, void* query_workspace, hipStream_t s, PnGrid& g) {
  const NnLayout l = nn_layout(M);
  const NnQueryLayout ql = nn_query_layout(n, M);
  const char* ws = static_cast<const char*>(workspace);
  char* qws = static_cast<char*>(query_workspace);
  g.hdr = reinterpret_cast<const NnHeader*>(ws);
  g.sorted_t = reinterpret_cast<const uint4v*>(ws + l.sorted_off);
  g.cell_end = reinterpret_cast<const int*>(ws + l.cells_off);
  g.sorted_q = reinterpret_cast<uint4v*>(qws + ql.sorted_off);
  return nn_bin(query, n, g.hdr, l.capacity, reinterpret_cast<int*>(qws + ql.cells_off), reinterpret_cast<int*>(qws), g.sorted_q, s);
}

}  // namespace

}  // namespace dvmvs

extern "C" int dvmvs_knn_fwd(const float* query, long long N, const float* target, long long M, const void* workspace, void* query_workspace,
                             size_t query_workspace_bytes, int k, float max_distance, int exclude_same_index, float* dist, int* index,
                             dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (k < 1 || k > kPnMaxK || !(max_distance >= 0.0f)) return DVMVS_EINVAL;
  const int rc = pn_check(query, N, target, M, workspace, query_workspace, query_workspace_bytes, exclude_same_index, dist, index);
  if (rc != 0) return rc < 0 ? rc : 0;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = static_cast<int>(N), m = static_cast<int>(M);
  PnGrid g;
  const int bin = pn_bin(query, n, M, workspace, query_workspace, s, g);
  if (bin != 0) return bin;
  const float cap2 = max_distance * max_distance;
  const dim3 grid((n + kNnBlock - 1) / kNnBlock), block(kNnBlock);
  if (k <= 4)
    hipLaunchKernelGGL(pn_knn_kernel<4>, grid, block, 0, s, g.sorted_q, n, g.sorted_t, m, g.cell_end, g.hdr, k, cap2, exclude_same_index, dist, index);
  else if (k <= 8)
    hipLaunchKernelGGL(pn_knn_kernel<8>, grid, block, 0, s, g.sorted_q, n, g.sorted_t, m, g.cell_end, g.hdr, k, cap2, exclude_same_index, dist, index);
  else if (k <= 16)
    hipLaunchKernelGGL(pn_knn_kernel<16>, grid, block, 0, s, g.sorted_q, n, g.sorted_t, m, g.cell_end, g.hdr, k, cap2, exclude_same_index, dist, index);
  else
    hipLaunchKernelGGL(pn_knn_kernel<32>, grid, block, 0, s, g.sorted_q, n, g.sorted_t, m, g.cell_end, g.hdr, k, cap2, exclude_same_index, dist, index);
  return launch_status();
}

extern "C" int dvmvs_radius_count_fwd(const float* query, long long N, const float* target, long long M, const void* workspace,
                                      void* query_workspace, size_t query_workspace_bytes, float radius, int cap, int exclude_same_index,
                                      int* count, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (cap < 1 || !(radius >= 0.0f)) return DVMVS_EINVAL;
  const int rc = pn_check(query, N, target, M, workspace, query_workspace, query_workspace_bytes, exclude_same_index, count, count);
  if (rc != 0) return rc < 0 ? rc : 0;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = static_cast<int>(N);
  PnGrid g;
  const int bin = pn_bin(query, n, M, workspace, query_workspace, s, g);
  if (bin != 0) return bin;
  hipLaunchKernelGGL(pn_radius_kernel, dim3((n + kNnBlock - 1) / kNnBlock), dim3(kNnBlock), 0, s, g.sorted_q, n, g.sorted_t, static_cast<int>(M),
                     g.cell_end, g.hdr, radius * radius, cap, exclude_same_index, count);
  return launch_status();
}

extern "C" int dvmvs_outlier_statistics_fwd(const float* dist, const int* index, long long N, int k, double ratio, float* mean,
                                            unsigned char* keep, double* stats, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (N < 0 || k < 1 || k > kPnMaxK || !(ratio >= 0.0 && ratio < __builtin_inf())) return DVMVS_EINVAL;
  if (N > 0 && (!dist || !index || !mean || !keep || !stats)) return DVMVS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(dist) | reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(mean)) % 4 != 0 ||
      reinterpret_cast<uintptr_t>(stats) % 8 != 0) return DVMVS_EINVAL;
  if (N > kNnMaxPoints) return DVMVS_EUNSUPPORTED;
  if (N == 0) return 0;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 points(static_cast<unsigned int>((N + kNnBlock - 1) / kNnBlock)), block(kNnBlock);
  hipLaunchKernelGGL(pn_mean_kernel, points, block, 0, s, dist, index, N, k, mean);
  hipLaunchKernelGGL(pn_stats_kernel, dim3(1), dim3(kPnStatThreads), 0, s, mean, N, ratio, stats);
  hipLaunchKernelGGL(pn_keep_kernel, points, block, 0, s, mean, N, stats, keep);
  return launch_status();
}
