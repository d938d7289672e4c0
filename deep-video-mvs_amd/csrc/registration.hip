// Trimmed ICP on the device (gfx950): registers a source cloud to a target cloud, the whole loop enqueued at once and no host read inside
// it (definition: include/dvmvs_hip.h).  Two variants of ONE loop, each described by a traits struct below:
//   IcpPoint : point to point, a rigid or similarity transform by Horn's closed form (restated by tests/registration_reference.py and
//              dvmvs/errors.py::register_points)
//   IcpPlane : point to plane on the target's normals, a rigid transform from the 6x6 normal equations of the linearised residual
//              (dvmvs/errors.py::register_points_plane)
//   dvmvs_icp_workspace_bytes, dvmvs_icp_plane_workspace_bytes : the size of a registration's state block (host arithmetic)
//   dvmvs_icp_fwd, dvmvs_icp_plane_fwd : enqueue max_iterations iterations; the state block ends with T, the status and the per-iteration
//                                        record
//   dvmvs_transform_points_fwd         : p' = fp32(T[:3,:4]) p for a cloud
//
// One iteration is four steps on the stream; the three kernels of an iteration begin by reading the status word and do nothing unless
// it says "running" (icp_init_kernel, which sets it, and the stand-alone transform, which has none, do not), so the iterations enqueued
// after the loop has stopped change nothing:
//   1. icp_transform_kernel   p' = A p with A = fp32(T[:3,:4]); ((A0 x + A1 y) + A2 z) + A3, every operation rounded to fp32, no FMA
//   2. dvmvs_nearest_distance_fwd (csrc/nearest_points.hip, unchanged)   (d_i, j_i) of p'_i in the target's grid
//   3. icp_moments_kernel<V>  the variant's fp64 moments (18 or 30) of the inliers (d_i <= max_distance; for IcpPlane also: the target has
//                             a normal), one partial row per 1024 consecutive points
//   4. icp_solve_kernel<V>    ONE wave: adds the partial rows, records the iteration, decides convergence, solves, updates T
// (Step 2 is the existing launcher and cannot read the status: after the loop has stopped it repeats the last query, whose results
// nothing reads.)
//
// Order of the additions, a function of N alone, the same for both variants.  Workgroup g of step 3 takes the points [1024 g, 1024 g +
// 1024): thread t adds, in fp64 and starting from 0.0, the terms of the points 1024 g + t, + 256, + 512, + 768 that exist and are inliers;
// the 64 lanes of a wave are combined by the xor butterfly (wave_sum of dvmvs_device.h, masks 32, 16, .., 1: a + b and b + a are the same
// bits), the 4 waves in order by thread t < the number of moments.  In step 4 lane l adds the partial rows l, l + 64, ... in that order
// starting from 0.0, then the same butterfly.  A trimmed point is skipped; adding an exact +0.0 instead gives the same bits (no sum that
// starts from +0.0 is ever -0.0).
//
// The solve uses fp64 +, -, *, / and sqrt only, nothing contracted (contract(off) for the whole file), in the order written below.
#include "dvmvs_device.h"

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

constexpr int kIcpBlock = 256;
constexpr int kIcpRows = 4;                              // points per thread of the moments kernel
constexpr int kIcpGroupPoints = kIcpBlock * kIcpRows;    // 1024
constexpr long long kIcpMaxPoints = 1LL << 28;
constexpr int kIcpMaxIterations = 1024;
constexpr int kIcpSweeps = 16;
constexpr double kIcpPlanePivot = 0x1p-30;

enum IcpStatus : long long { kIcpRunning = 0, kIcpConverged = 1, kIcpTooFew = 2, kIcpLimit = 3, kIcpDegenerate = 4 };

// The head of the state block, in 8-byte words: T, the two counters, then the variant's moments up to its kHeadWords; the per-iteration
// arrays follow it (include/dvmvs_hip.h).
constexpr int kIcpWordT = 0, kIcpWordIterations = 16, kIcpWordStatus = 17, kIcpWordMoments = 18;

struct IcpInit {
  double t[16];
};

// records [kRecords][max_iterations] of 8 bytes (inliers, fitness, rmse, then IcpPlane's rmse_point) | moved source | dist | index |
// partial rows
struct IcpLayout {
  size_t records_off, points_off, dist_off, index_off, partials_off, total;
  int groups;
};

size_t icp_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

template <typename V>
IcpLayout icp_layout(long long n, int max_iterations) {
  IcpLayout l;
  const size_t it = static_cast<size_t>(max_iterations);
  l.groups = static_cast<int>((n + kIcpGroupPoints - 1) / kIcpGroupPoints);
  l.records_off = V::kHeadWords * 8;
  l.points_off = icp_align(l.records_off + V::kRecords * it * 8);
  l.dist_off = l.points_off + icp_align(static_cast<size_t>(n) * 12);
  l.index_off = l.dist_off + icp_align(static_cast<size_t>(n) * 4);
  l.partials_off = l.index_off + icp_align(static_cast<size_t>(n) * 4);
  l.total = l.partials_off + icp_align(static_cast<size_t>(l.groups) * V::kMoments * 8);
  return l;
}

template <typename V>
size_t icp_workspace_bytes(long long N, int max_iterations) {
  if (N <= 0 || N > kIcpMaxPoints || max_iterations < 1 || max_iterations > kIcpMaxIterations) return 0;
  return icp_layout<V>(N, max_iterations).total;
}

__device__ inline void icp_load_affine(const double* __restrict__ T, float* A) {
#pragma unroll
  for (int i = 0; i < 12; ++i) A[i] = static_cast<float>(T[i]);
}

__device__ inline void icp_apply(const float* A, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((A[0] * x + A[1] * y) + A[2] * z) + A[3];
  oy = ((A[4] * x + A[5] * y) + A[6] * z) + A[7];
  oz = ((A[8] * x + A[9] * y) + A[10] * z) + A[11];
}

// `head_words`: the variant's kHeadWords (at most the 64 threads of the launch)
__global__ void icp_init_kernel(IcpInit init, int head_words, double* __restrict__ state) {
  const int t = threadIdx.x;
  if (t < 16) state[kIcpWordT + t] = init.t[t];
  if (t >= kIcpWordMoments && t < head_words) state[t] = 0.0;
  if (t == 0) {
    long long* words = reinterpret_cast<long long*>(state);
    words[kIcpWordIterations] = 0;
    words[kIcpWordStatus] = kIcpRunning;
  }
}

// `status`: the state's status word, or NULL for the stand-alone transform
__global__ __launch_bounds__(kIcpBlock) void icp_transform_kernel(const float* points, int n, const double* __restrict__ T,
                                                                  const long long* __restrict__ status, float* out) {
  if (status && *status != kIcpRunning) return;
  const int i = blockIdx.x * kIcpBlock + threadIdx.x;
  if (i >= n) return;
  float A[12];
  icp_load_affine(T, A);
  const size_t o = static_cast<size_t>(i) * 3;
  const float x = points[o], y = points[o + 1], z = points[o + 2];
  float px, py, pz;
  icp_apply(A, x, y, z, px, py, pz);
  out[o] = px;
  out[o + 1] = py;
  out[o + 2] = pz;
}

// The rotation matrix of the unit quaternion (w, x, y, z)
__device__ inline void icp_rotation(double w, double x, double y, double z, double* R) {
  R[0] = 1.0 - 2.0 * (y * y + z * z);
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = 1.0 - 2.0 * (x * x + z * z);
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// Horn's closed form: the unit quaternion (w, x, y, z), w >= 0, of the rotation that best takes the centred p' onto the centred q,
// as the eigenvector of the largest eigenvalue of Horn's symmetric 4x4 matrix of S, by cyclic Jacobi sweeps.
__device__ inline void icp_horn(const double* S, double* quat) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  double A[4][4], V[4][4];
  A[0][0] = (Sxx + Syy) + Szz;
  A[1][1] = (Sxx - Syy) - Szz;
  A[2][2] = (Syy - Sxx) - Szz;
  A[3][3] = (Szz - Sxx) - Syy;
  A[0][1] = A[1][0] = Syz - Szy;
  A[0][2] = A[2][0] = Szx - Sxz;
  A[0][3] = A[3][0] = Sxy - Syx;
  A[1][2] = A[2][1] = Sxy + Syx;
  A[1][3] = A[3][1] = Szx + Sxz;
  A[2][3] = A[3][2] = Syz + Szy;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kIcpSweeps; ++sweep) {
    bool diagonal = true;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) diagonal = diagonal && A[p][q] == 0.0;
    if (diagonal) break;
    for (int p = 0; p < 3; ++p) {
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double mag = fabs(theta) + sqrt(theta * theta + 1.0);
        const double tn = theta < 0.0 ? -1.0 / mag : 1.0 / mag;
        const double c = 1.0 / sqrt(tn * tn + 1.0);
        const double s = tn * c;
        for (int k = 0; k < 4; ++k) {                        // columns p and q
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {                        // rows p and q
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = 0.0;
        A[q][p] = 0.0;
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
    }
  }
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > A[best][best]) best = k;                   // the lowest index on a tie
  double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
  const double norm = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / norm;
  x = x / norm;
  y = y / norm;
  z = z / norm;
  if (w < 0.0) {
    w = -w;
    x = -x;
    y = -y;
    z = -z;
  }
  quat[0] = w;
  quat[1] = x;
  quat[2] = y;
  quat[3] = z;
}

// ---- the variants ----------------------------------------------------------------------------------------------------------------------
// A variant gives the sizes of its state block, and two device functions:
//   add    : adds the terms of one pair to the moments v: p' = the moved point at pf, q = target[qo..], its nearest target, with the normal
//            normals[qo..], d = their distance, o = the first moved point; a pair that does not count adds nothing
//   update : from the summed moments v (n = v[0] >= kMinInliers) the step x -> M x + shift that is composed with T, or the status that
//            stops the loop (kIcpRunning: go on)
struct IcpPoint {
  static constexpr int kMoments = 18;                    // n | sum p' [3] | sum q [3] | sum p' q^T [9] | sum |p'|^2 | sum d^2
  static constexpr int kHeadWords = 36;
  static constexpr int kRecords = 3;                     // inliers, fitness, rmse
  static constexpr int kMinInliers = 3;
  static constexpr int kRmseMoment = 17;

  __device__ static void add(double* v, const float* __restrict__ pf, const float* __restrict__ target, const float* __restrict__, size_t qo,
                             const double*, float d) {
    const double p[3] = {static_cast<double>(pf[0]), static_cast<double>(pf[1]), static_cast<double>(pf[2])};
    const double q[3] = {static_cast<double>(target[qo]), static_cast<double>(target[qo + 1]), static_cast<double>(target[qo + 2])};
    const double dd = static_cast<double>(d);
    v[0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[1 + a] += p[a];
      v[4 + a] += q[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) v[7 + a * 3 + b] += p[a] * q[b];
    }
    v[16] += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
    v[17] += dd * dd;
  }

  // Horn: the rotation of the centred sums, the optional scale, and the shift that takes the moved centroid onto the target's
  __device__ static IcpStatus update(const double* v, double n, int with_scale, const float* __restrict__, double* M, double* shift) {
    double pbar[3], qbar[3], S[9];
    for (int a = 0; a < 3; ++a) {
      pbar[a] = v[1 + a] / n;
      qbar[a] = v[4 + a] / n;
    }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) S[a * 3 + b] = v[7 + a * 3 + b] - (v[1 + a] * v[4 + b]) / n;
    double quat[4], R[9];
    icp_horn(S, quat);
    icp_rotation(quat[0], quat[1], quat[2], quat[3], R);
    double scale = 1.0;
    if (with_scale) {
      const double denominator = v[16] - ((v[1] * v[1] + v[2] * v[2]) + v[3] * v[3]) / n;
      if (!(denominator > 0.0)) return kIcpTooFew;
      double trace = 0.0;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) trace += R[a * 3 + b] * S[b * 3 + a];
      scale = trace / denominator;
    }
    for (int i = 0; i < 9; ++i) M[i] = scale * R[i];
    for (int a = 0; a < 3; ++a) shift[a] = qbar[a] - ((M[a * 3] * pbar[0] + M[a * 3 + 1] * pbar[1]) + M[a * 3 + 2] * pbar[2]);
    return kIcpRunning;
  }
};

struct IcpPlane {
  static constexpr int kMoments = 30;                    // n | sum J_a J_b, a <= b [21] | sum J_a r [6] | sum r^2 | sum d^2
  static constexpr int kHeadWords = 48;
  static constexpr int kRecords = 4;                     // inliers, fitness, rmse (of the plane residual), rmse_point
  static constexpr int kMinInliers = 6;
  static constexpr int kRmseMoment = 28;

  __device__ static bool has_normal(float x, float y, float z) {
    return x - x == 0.0f && y - y == 0.0f && z - z == 0.0f && (x != 0.0f || y != 0.0f || z != 0.0f);
  }

  __device__ static void add(double* v, const float* __restrict__ pf, const float* __restrict__ target, const float* __restrict__ normals,
                             size_t qo, const double* o, float d) {
    const float nx = normals[qo], ny = normals[qo + 1], nz = normals[qo + 2];
    if (!has_normal(nx, ny, nz)) return;                             // a target without a normal pairs with nothing
    const double p[3] = {static_cast<double>(pf[0]), static_cast<double>(pf[1]), static_cast<double>(pf[2])};
    const double q[3] = {static_cast<double>(target[qo]), static_cast<double>(target[qo + 1]), static_cast<double>(target[qo + 2])};
    const double nn[3] = {static_cast<double>(nx), static_cast<double>(ny), static_cast<double>(nz)};
    const double e[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
    const double res = ((p[0] - q[0]) * nn[0] + (p[1] - q[1]) * nn[1]) + (p[2] - q[2]) * nn[2];
    const double J[6] = {e[1] * nn[2] - e[2] * nn[1], e[2] * nn[0] - e[0] * nn[2], e[0] * nn[1] - e[1] * nn[0], nn[0], nn[1], nn[2]};
    const double dd = static_cast<double>(d);
    v[0] += 1.0;
    int c = 1;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = a; b < 6; ++b) v[c++] += J[a] * J[b];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) v[22 + a] += J[a] * res;
    v[28] += res * res;
    v[29] += dd * dd;
  }

  // A x = -b by LDL^T without pivoting: A = sum J J^T (the lower triangle is read), b = sum J r; x = (rotation vector about o, shift).
  // `moved`: the moved source of this iteration; its first point is the origin o of the rotation
  __device__ static IcpStatus update(const double* v, double, int, const float* __restrict__ moved, double* R, double* shift) {
    double A[6][6], L[6][6], D[6], x[6];
    {
      int c = 1;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = a; b < 6; ++b) A[b][a] = v[c++];
      }
    }
    bool degenerate = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double d = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) d = d - (L[j][k] * L[j][k]) * D[k];
      if (!(d > kIcpPlanePivot * A[j][j])) degenerate = true;      // (what follows a failed pivot is not used)
      D[j] = d;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double s = A[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - (L[i][k] * L[j][k]) * D[k];
        L[i][j] = s / d;
      }
    }
    if (degenerate) return kIcpDegenerate;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = -v[22 + i];
#pragma unroll
      for (int k = 0; k < i; ++k) s = s - L[i][k] * x[k];
      x[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = x[i] / D[i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double s = x[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
      x[i] = s;
    }
    double qx = x[0] / 2.0, qy = x[1] / 2.0, qz = x[2] / 2.0;
    const double norm = sqrt(((1.0 + qx * qx) + qy * qy) + qz * qz);
    const double w = 1.0 / norm;
    qx = qx / norm;
    qy = qy / norm;
    qz = qz / norm;
    icp_rotation(w, qx, qy, qz, R);
    const double o[3] = {static_cast<double>(moved[0]), static_cast<double>(moved[1]), static_cast<double>(moved[2])};
#pragma unroll
    for (int a = 0; a < 3; ++a) shift[a] = (o[a] - ((R[a * 3] * o[0] + R[a * 3 + 1] * o[1]) + R[a * 3 + 2] * o[2])) + x[3 + a];
    return kIcpRunning;
  }
};

// ---- the loop --------------------------------------------------------------------------------------------------------------------------
// `normals`: the target's, for IcpPlane; IcpPoint does not read them
template <typename V>
__global__ __launch_bounds__(kIcpBlock) void icp_moments_kernel(const float* __restrict__ moved, int n, const float* __restrict__ target,
                                                                const float* __restrict__ normals, int m, const float* __restrict__ dist,
                                                                const int* __restrict__ index, float max_distance,
                                                                const long long* __restrict__ status, double* __restrict__ partials) {
  __shared__ double s_wave[kIcpBlock / kWave][V::kMoments];
  if (*status != kIcpRunning) return;
  const int t = threadIdx.x;
  double v[V::kMoments];
#pragma unroll
  for (int k = 0; k < V::kMoments; ++k) v[k] = 0.0;
  const double o[3] = {static_cast<double>(moved[0]), static_cast<double>(moved[1]), static_cast<double>(moved[2])};     // IcpPlane's origin (n >= 1)
  const long long first = static_cast<long long>(blockIdx.x) * kIcpGroupPoints;
#pragma unroll
  for (int r = 0; r < kIcpRows; ++r) {
    const long long i = first + r * kIcpBlock + t;
    if (i >= n) break;
    const float d = dist[i];
    const int j = index[i];
    if (!(d <= max_distance) || j < 0 || j >= m) continue;         // trimmed (the index test cannot fail after a query; it keeps the reads in bounds)
    const size_t po = static_cast<size_t>(i) * 3, qo = static_cast<size_t>(j) * 3;
    V::add(v, moved + po, target, normals, qo, o, d);
  }
  wave_sum(v);
  if (t % kWave == 0) {
#pragma unroll
    for (int k = 0; k < V::kMoments; ++k) s_wave[t / kWave][k] = v[k];
  }
  __syncthreads();
  if (t < V::kMoments) {
    double s = s_wave[0][t];
    for (int w = 1; w < kIcpBlock / kWave; ++w) s += s_wave[w][t];
    partials[static_cast<size_t>(blockIdx.x) * V::kMoments + t] = s;
  }
}

// `records`: the V::kRecords per-iteration arrays of max_iterations entries each; `moved`: the moved source of this iteration
template <typename V>
__global__ __launch_bounds__(kWave) void icp_solve_kernel(const double* __restrict__ partials, int groups, long long n_points, int iteration,
                                                          int max_iterations, int with_scale, double tolerance, const float* __restrict__ moved,
                                                          double* __restrict__ state, double* __restrict__ records) {
  long long* words = reinterpret_cast<long long*>(state);
  if (words[kIcpWordStatus] != kIcpRunning) return;
  double v[V::kMoments];
#pragma unroll
  for (int k = 0; k < V::kMoments; ++k) v[k] = 0.0;
  for (int g = threadIdx.x; g < groups; g += kWave) {
#pragma unroll
    for (int k = 0; k < V::kMoments; ++k) v[k] += partials[static_cast<size_t>(g) * V::kMoments + k];
  }
  wave_sum(v);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < V::kMoments; ++k) state[kIcpWordMoments + k] = v[k];
  long long* inliers = reinterpret_cast<long long*>(records);
  double* fitness = records + max_iterations;
  double* rmse = fitness + max_iterations;
  const double n = v[0];
  const double rmse_k = n > 0.0 ? sqrt(v[V::kRmseMoment] / n) : 0.0;
  const double fitness_k = n / static_cast<double>(n_points);
  inliers[iteration] = static_cast<long long>(n);
  fitness[iteration] = fitness_k;
  rmse[iteration] = rmse_k;
  if (V::kRecords == 4) rmse[max_iterations + iteration] = n > 0.0 ? sqrt(v[V::kMoments - 1] / n) : 0.0;      // rmse_point, of sum d^2
  words[kIcpWordIterations] = iteration + 1;
  if (n < static_cast<double>(V::kMinInliers)) {
    words[kIcpWordStatus] = kIcpTooFew;
    return;
  }
  if (iteration >= 1 && fabs(rmse_k - rmse[iteration - 1]) < tolerance && fabs(fitness_k - fitness[iteration - 1]) < tolerance) {
    words[kIcpWordStatus] = kIcpConverged;
    return;
  }
  double M[9], shift[3], next[12];
  const IcpStatus stop = V::update(v, n, with_scale, moved, M, shift);
  if (stop != kIcpRunning) {
    words[kIcpWordStatus] = stop;
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      next[a * 4 + c] = ((M[a * 3] * state[c] + M[a * 3 + 1] * state[4 + c]) + M[a * 3 + 2] * state[8 + c]) + shift[a] * state[12 + c];
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) state[kIcpWordT + i] = next[i];
  if (iteration + 1 >= max_iterations) words[kIcpWordStatus] = kIcpLimit;
}

bool icp_finite(double x) { return x - x == 0.0; }

// Checks the arguments, lays out the state block and enqueues the loop.  `normals`: the target's (IcpPlane; its launcher has refused NULL)
// or NULL; `with_scale`: IcpPoint's option, 0 for IcpPlane.
template <typename V>
int icp_enqueue(const float* source, long long N, const float* target, const float* normals, long long M, const void* grid_workspace,
                void* query_workspace, size_t query_workspace_bytes, float max_distance, int with_scale, int max_iterations, double tolerance,
                const double* init_host, void* state, size_t state_bytes, dvmvs_stream_t stream) {
  if (!source || !target || !grid_workspace || !query_workspace || !state) return DVMVS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(source) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(normals)) % 4 != 0 ||
      (reinterpret_cast<uintptr_t>(grid_workspace) | reinterpret_cast<uintptr_t>(query_workspace) | reinterpret_cast<uintptr_t>(state)) % 16 != 0)
    return DVMVS_EINVAL;
  if (N < 1 || M < 1 || max_iterations < 1 || (with_scale != 0 && with_scale != 1)) return DVMVS_EINVAL;
  if (!(max_distance > 0.0f) || !(tolerance >= 0.0)) return DVMVS_EINVAL;            // NaN fails both
  IcpInit init;
  for (int i = 0; i < 16; ++i) {
    init.t[i] = init_host ? init_host[i] : (i % 5 == 0 ? 1.0 : 0.0);
    if (!icp_finite(init.t[i])) return DVMVS_EINVAL;
  }
  if (N > kIcpMaxPoints || M > kIcpMaxPoints || max_iterations > kIcpMaxIterations) return DVMVS_EUNSUPPORTED;
  const IcpLayout l = icp_layout<V>(N, max_iterations);
  if (state_bytes < l.total || query_workspace_bytes < dvmvs_nearest_query_workspace_bytes(N, M)) return DVMVS_EINVAL;
  char* base = static_cast<char*>(state);
  double* head = reinterpret_cast<double*>(base);
  long long* status = reinterpret_cast<long long*>(base) + kIcpWordStatus;
  double* records = reinterpret_cast<double*>(base + l.records_off);
  float* moved = reinterpret_cast<float*>(base + l.points_off);
  float* dist = reinterpret_cast<float*>(base + l.dist_off);
  int* index = reinterpret_cast<int*>(base + l.index_off);
  double* partials = reinterpret_cast<double*>(base + l.partials_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = static_cast<int>(N), m = static_cast<int>(M);
  const dim3 points((n + kIcpBlock - 1) / kIcpBlock), block(kIcpBlock);
  hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(kWave), 0, s, init, V::kHeadWords, head);
  for (int k = 0; k < max_iterations; ++k) {
    hipLaunchKernelGGL(icp_transform_kernel, points, block, 0, s, source, n, head, status, moved);
    const int rc = dvmvs_nearest_distance_fwd(moved, N, target, M, grid_workspace, query_workspace, query_workspace_bytes, dist, index, stream);
    if (rc != 0) return rc;                                  // a HIP error only: every argument the launcher refuses was checked above
    hipLaunchKernelGGL(icp_moments_kernel<V>, dim3(l.groups), block, 0, s, moved, n, target, normals, m, dist, index, max_distance, status,
                       partials);
    hipLaunchKernelGGL(icp_solve_kernel<V>, dim3(1), dim3(kWave), 0, s, partials, l.groups, N, k, max_iterations, with_scale, tolerance, moved,
                       head, records);
  }
  return launch_status();
}

}  // namespace

}  // namespace dvmvs

extern "C" size_t dvmvs_icp_workspace_bytes(long long N, int max_iterations) {
  return dvmvs::icp_workspace_bytes<dvmvs::IcpPoint>(N, max_iterations);
}

extern "C" int dvmvs_icp_fwd(const float* source, long long N, const float* target, long long M, const void* grid_workspace,
                             void* query_workspace, size_t query_workspace_bytes, float max_distance, int with_scale, int max_iterations,
                             double tolerance, const double* init_host, void* state, size_t state_bytes, dvmvs_stream_t stream) {
  return dvmvs::icp_enqueue<dvmvs::IcpPoint>(source, N, target, nullptr, M, grid_workspace, query_workspace, query_workspace_bytes, max_distance,
                                             with_scale, max_iterations, tolerance, init_host, state, state_bytes, stream);
}

extern "C" size_t dvmvs_icp_plane_workspace_bytes(long long N, int max_iterations) {
  return dvmvs::icp_workspace_bytes<dvmvs::IcpPlane>(N, max_iterations);
}

extern "C" int dvmvs_icp_plane_fwd(const float* source, long long N, const float* target, const float* target_normals, long long M,
                                   const void* grid_workspace, void* query_workspace, size_t query_workspace_bytes, float max_distance,
                                   int max_iterations, double tolerance, const double* init_host, void* state, size_t state_bytes,
                                   dvmvs_stream_t stream) {
  if (!target_normals) return DVMVS_EINVAL;
  return dvmvs::icp_enqueue<dvmvs::IcpPlane>(source, N, target, target_normals, M, grid_workspace, query_workspace, query_workspace_bytes,
                                             max_distance, 0, max_iterations, tolerance, init_host, state, state_bytes, stream);
}

extern "C" int dvmvs_transform_points_fwd(const float* points, long long N, const double* T, float* out, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!points || !T || !out || N < 1) return DVMVS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(out)) % 4 != 0 || reinterpret_cast<uintptr_t>(T) % 8 != 0) return DVMVS_EINVAL;
  if (N > kIcpMaxPoints) return DVMVS_EUNSUPPORTED;
  const int n = static_cast<int>(N);
  hipLaunchKernelGGL(icp_transform_kernel, dim3((n + kIcpBlock - 1) / kIcpBlock), dim3(kIcpBlock), 0, static_cast<hipStream_t>(stream), points, n,
                     T, static_cast<const long long*>(nullptr), out);
  return launch_status();
}
