// Oriented normals of point clouds from rows of k nearest neighbours (gfx950): the step after csrc/point_neighbours.hip's k-NN search.
// dvmvs/normals.py is the host form; include/dvmvs_hip.h states the contract.
//   dvmvs_point_normals_fwd : points fp32 [N,3], target fp32 [M,3], index int32 [N,k] -> normals fp32 [N,3], curvature fp32 [N], valid uint8 [N]
//
// Arithmetic contract: fp64 from the fp32 inputs with +, -, *, / and sqrt only, every operation correctly rounded, nothing contracted
// into an FMA (contract(off) for the whole file; fp64 division and sqrt are the correctly rounded ones).  Per point, in this order:
//   1. the valid slots of its row, those with 0 <= j < M, in slot order; fewer than 3: zeros, invalid
//   2. moments about the anchor a = target[j0] in ONE pass: e = target[j] - a, s_c += e_c, S_cd += e_c e_d (six of them), from 0.0;
//      m_c = s_c / n, C_cd = S_cd / n - m_c m_d
//   3. cyclic Jacobi on the 3x3 (the registration's rule): pairs (0,1), (0,2), (1,2), a zero A_pq skipped, at most 16 sweeps, stop before
//      a sweep when the three off-diagonals are exactly zero
//   4. lambda = the smallest diagonal entry (lowest index on a tie), trace = (A00 + A11) + A22; trace not > 0: zeros, invalid; otherwise
//      curvature = fp32(max(lambda, 0) / trace)
//   5. the normal = that column of V / sqrt((xx + yy) + zz), negated when the first non-zero of (z, y, x) is negative
//   6. with viewpoints: negated when d = (nx (vx - px) + ny (vy - py)) + nz (vz - pz) < 0; a view outside [0, V) keeps the sign
//
// One point per lane, nothing crosses lanes after the staging barrier, so the result does not depend on the schedule.  Every neighbour is
// gathered once (the one-pass moments exist for that); the anchored differences are small and nearly exact wherever the cloud lies, so
// the one pass loses nothing to cancellation.  A slot outside [0, M) never becomes an address: the gather of such a slot reads target[0]
// (M >= 1) and its sums are not taken.  The gathers of a slot do not depend on the slots before it, so the loop keeps several in flight.
//
// The 9 moment sums, the 6 entries of A and the 9 of V are named scalars and the three rotations are written out (pn_rotate, inlined
// with compile-time p, q): an array indexed by a run-time (p, q) would live in scratch, as point_neighbours.hip says of its list.
//
// The index rows.  Row i is k consecutive ints, so lanes that read their own rows directly run k loads of stride 4k bytes, each
// touching up to 64 lines.  Instead the workgroup copies its 256 rows, one contiguous piece of 1024 k bytes, into LDS with coalesced
// 4-byte loads (the tensor is only 4-byte aligned) and every lane reads its row back from there.  The LDS rows are k | 1 ints apart: an
// odd stride puts the 32 lanes of a half wave on 32 different banks at every slot (k = 8, 16, 32 would be 8-, 16- and 32-way conflicts),
// and the copy's writes stay consecutive but for one gap per row.  (256 * 33 * 4 = 33 KB at k = 32: four workgroups on a CU.)
// pn_normals_kernel<false> is the direct read, instantiated in the tools-only tuning build alone, for the comparison of
// tools/point_normals_bench.py (0.209 against 0.061 ms at k = 32, no difference at k = 8: DESIGN.md section 4.8l).
#include "dvmvs_device.h"

#include <stdlib.h>

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

constexpr int kPnBlock = 256;
constexpr int kPnMinK = 3, kPnMaxK = 32;
constexpr int kPnSweeps = 16;
constexpr long long kPnMaxPoints = 1ll << 28;

// One Jacobi rotation of the pair (p, q) on the symmetric 3x3 with r the third index: the columns p, q, then the rows, old values on the
// right.  Written on the upper triangle: with A symmetric, the rows' step at k = r computes what the columns' step left at (r, p) and
// (r, q), bit for bit, so the triangle is the matrix.
__device__ inline void pn_rotate(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p, double& v0q, double& v1p,
                                 double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double pp = c * app - s * apq, pq = s * app + c * apq;       // the columns' step, rows p and q
  const double qp = c * apq - s * aqq, qq = s * apq + c * aqq;
  app = c * pp - s * qp;                                             // the rows' step at k = p and k = q
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

template <bool kStage>
__global__ __launch_bounds__(kPnBlock) void pn_normals_kernel(const float* __restrict__ points, int n_points, const float* __restrict__ target,
                                                              int m, const int* __restrict__ index, int k, const float* __restrict__ viewpoints,
                                                              int n_views, const int* __restrict__ view, float* __restrict__ normals,
                                                              float* __restrict__ curvature, unsigned char* __restrict__ valid) {
  extern __shared__ int s_index[];                           // [row][k | 1]
  const int lane = threadIdx.x;
  const long long first = static_cast<long long>(blockIdx.x) * kPnBlock;
  const int rows = static_cast<int>(min(static_cast<long long>(kPnBlock), n_points - first));
  const int pitch = k | 1;
  const int* row;
  if (kStage) {
    const int* __restrict__ src = index + first * k;
    const int total = rows * k, step_row = kPnBlock / k, step_slot = kPnBlock % k;
    int r = lane / k, s = lane % k;
    for (int e = lane; e < total; e += kPnBlock) {           // e = r * k + s
      s_index[r * pitch + s] = src[e];
      r += step_row;
      s += step_slot;
      if (s >= k) {
        s -= k;
        ++r;
      }
    }
    __syncthreads();
    row = s_index + lane * pitch;
  } else {
    row = index + (first + lane) * k;
  }
  if (lane >= rows) return;
  const long long i = first + lane;

  int n = 0;
  double ax = 0.0, ay = 0.0, az = 0.0;
  double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
#pragma unroll 4
  for (int slot = 0; slot < k; ++slot) {
    const int j = row[slot];
    const bool ok = static_cast<unsigned int>(j) < static_cast<unsigned int>(m);
    const float* t = target + 3 * static_cast<size_t>(ok ? j : 0);
    const double tx = static_cast<double>(t[0]), ty = static_cast<double>(t[1]), tz = static_cast<double>(t[2]);
    if (ok && n == 0) ax = tx, ay = ty, az = tz;
    const double ex = tx - ax, ey = ty - ay, ez = tz - az;
    if (ok) {
      ++n;
      sx += ex, sy += ey, sz += ez;
      sxx += ex * ex, sxy += ex * ey, sxz += ex * ez;
      syy += ey * ey, syz += ey * ez, szz += ez * ez;
    }
  }

  float nx = 0.0f, ny = 0.0f, nz = 0.0f, curv = 0.0f;
  unsigned char good = 0;
  if (n >= kPnMinK) {
    const double count = static_cast<double>(n);
    const double mx = sx / count, my = sy / count, mz = sz / count;
    double a00 = sxx / count - mx * mx, a01 = sxy / count - mx * my, a02 = sxz / count - mx * mz;
    double a11 = syy / count - my * my, a12 = syz / count - my * mz, a22 = szz / count - mz * mz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < kPnSweeps; ++sweep) {
      if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
      pn_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0,1), r = 2
      pn_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0,2), r = 1
      pn_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1,2), r = 0
    }
    int best = 0;
    double lambda = a00;
    if (a11 < lambda) best = 1, lambda = a11;
    if (a22 < lambda) best = 2, lambda = a22;
    const double trace = (a00 + a11) + a22;
    if (trace > 0.0) {
      double x = best == 0 ? v00 : best == 1 ? v01 : v02;
      double y = best == 0 ? v10 : best == 1 ? v11 : v12;
      double z = best == 0 ? v20 : best == 1 ? v21 : v22;
      const double norm = sqrt((x * x + y * y) + z * z);
      x = x / norm, y = y / norm, z = z / norm;
      if (z < 0.0 || (z == 0.0 && (y < 0.0 || (y == 0.0 && x < 0.0)))) x = -x, y = -y, z = -z;
      if (viewpoints) {
        const int which = view ? view[i] : 0;
        if (static_cast<unsigned int>(which) < static_cast<unsigned int>(n_views)) {
          const float* v = viewpoints + 3 * static_cast<size_t>(which);
          const float* p = points + 3 * static_cast<size_t>(i);
          const double dx = static_cast<double>(v[0]) - static_cast<double>(p[0]);
          const double dy = static_cast<double>(v[1]) - static_cast<double>(p[1]);
          const double dz = static_cast<double>(v[2]) - static_cast<double>(p[2]);
          if ((x * dx + y * dy) + z * dz < 0.0) x = -x, y = -y, z = -z;
        }
      }
      nx = static_cast<float>(x), ny = static_cast<float>(y), nz = static_cast<float>(z);
      curv = static_cast<float>((lambda > 0.0 ? lambda : 0.0) / trace);
      good = 1;
    }
  }
  normals[3 * static_cast<size_t>(i) + 0] = nx;
  normals[3 * static_cast<size_t>(i) + 1] = ny;
  normals[3 * static_cast<size_t>(i) + 2] = nz;
  curvature[i] = curv;
  valid[i] = good;
}

inline bool pn_aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace

}  // namespace dvmvs

extern "C" int dvmvs_point_normals_fwd(const float* points, long long N, const float* target, long long M, const int* index, int k,
                                       const float* viewpoints, long long V, const int* view, float* normals, float* curvature,
                                       unsigned char* valid, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (N < 0 || M < 1 || k < kPnMinK || k > kPnMaxK || V < 0) return DVMVS_EINVAL;
  if (!target || (N > 0 && (!points || !index || !normals || !curvature || !valid))) return DVMVS_EINVAL;
  if ((V > 0) != (viewpoints != nullptr) || (view && !viewpoints) || (!view && V > 1)) return DVMVS_EINVAL;
  if (!pn_aligned4(points) || !pn_aligned4(target) || !pn_aligned4(index) || !pn_aligned4(viewpoints) || !pn_aligned4(view) ||
      !pn_aligned4(normals) || !pn_aligned4(curvature)) return DVMVS_EINVAL;
  if (N > kPnMaxPoints || M > kPnMaxPoints || V > kPnMaxPoints) return DVMVS_EUNSUPPORTED;
  if (N == 0) return 0;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = static_cast<int>(N), m = static_cast<int>(M), views = static_cast<int>(V);
  const dim3 grid((n + kPnBlock - 1) / kPnBlock), block(kPnBlock);
#ifdef DVMVS_SWEEP_TUNING          // tools-only build: DVMVS_POINT_NORMALS_INDEX=direct reads the index rows without the LDS stage
  const char* choice = getenv("DVMVS_POINT_NORMALS_INDEX");
  if (choice && choice[0] == 'd') {
    hipLaunchKernelGGL(pn_normals_kernel<false>, grid, block, 0, s, points, n, target, m, index, k, viewpoints, views, view, normals,
                       curvature, valid);
    return launch_status();
  }
#endif
  hipLaunchKernelGGL(pn_normals_kernel<true>, grid, block, static_cast<size_t>(kPnBlock) * (k | 1) * sizeof(int), s, points, n, target, m,
                     index, k, viewpoints, views, view, normals, curvature, valid);
  return launch_status();
}
