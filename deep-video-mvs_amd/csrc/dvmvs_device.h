// Shared device helpers for the gfx950 plane-sweep kernels: small fp64 matrix algebra for the pose set-up,
// the bilinear tap decomposition used by every warp kernel, and launch plumbing; and what the point-cloud and mesh kernels share:
// the block scans, the scan of per-workgroup totals, the ordered sum over a wave and the quantised area of a face.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvmvs_hip.h"

namespace dvmvs {

constexpr int kWave = 64;  // gfx950 wavefront

// Pointers that reach a kernel inside a by-value argument struct are generic ("flat") to the compiler: every access
// becomes a flat_load / flat_store, which is counted on BOTH vmcnt and lgkmcnt and therefore serialises against the
// ds_read waits of the LDS-bound sweep kernels.  Hot paths re-type them as global (address space 1) once, at the top.
#define DVMVS_GLOBAL __attribute__((address_space(1)))
typedef const float DVMVS_GLOBAL* gcfloat_p;
typedef float DVMVS_GLOBAL* gfloat_p;
typedef unsigned int DVMVS_GLOBAL* guint_p;
__device__ inline gcfloat_p as_global(const float* p) { return (gcfloat_p)p; }
__device__ inline gfloat_p as_global(float* p) { return (gfloat_p)p; }
__device__ inline guint_p as_global(unsigned int* p) { return (guint_p)p; }

#define DVMVS_RETURN_IF_HIP(expr)                      \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return static_cast<int>(_e); \
  } while (0)

inline int launch_status() { return static_cast<int>(hipGetLastError()); }

// ---- fp64 small-matrix algebra (row-major) -------------------------------------------------------------------
// The reference evaluates inverse(pose)/inverse(K) with an fp32 LU (torch.inverse); evaluating the same algebra
// in fp64 and rounding once lands within the reference's own fp32 round-off of it, needs no library call and
// no host round trip.

__device__ inline double det3(double a, double b, double c, double d, double e, double f, double g, double h, double i) {
  return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
}

__device__ inline void inverse3(const double* m, double* o) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double inv_det = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
  o[0] = c00 * inv_det;
  o[1] = (m[2] * m[7] - m[1] * m[8]) * inv_det;
  o[2] = (m[1] * m[5] - m[2] * m[4]) * inv_det;
  o[3] = c01 * inv_det;
  o[4] = (m[0] * m[8] - m[2] * m[6]) * inv_det;
  o[5] = (m[2] * m[3] - m[0] * m[5]) * inv_det;
  o[6] = c02 * inv_det;
  o[7] = (m[1] * m[6] - m[0] * m[7]) * inv_det;
  o[8] = (m[0] * m[4] - m[1] * m[3]) * inv_det;
}

// General 4x4 inverse by cofactors (poses are rigid, but the reference does not assume it).
__device__ inline void inverse4(const double* m, double* o) {
  double cof[16];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int r0 = (r + 1) & 3, r1 = (r + 2) & 3, r2 = (r + 3) & 3;
      const int c0 = (c + 1) & 3, c1 = (c + 2) & 3, c2 = (c + 3) & 3;
      // remaining rows/cols taken in cyclic order: a rotation of three indices is an even permutation, so the
      // 3x3 determinant equals the standard minor and the cofactor sign is the usual (-1)^(r+c)
      const double minor = det3(m[r0 * 4 + c0], m[r0 * 4 + c1], m[r0 * 4 + c2],
                                m[r1 * 4 + c0], m[r1 * 4 + c1], m[r1 * 4 + c2],
                                m[r2 * 4 + c0], m[r2 * 4 + c1], m[r2 * 4 + c2]);
      cof[r * 4 + c] = ((r + c) & 1) ? -minor : minor;
    }
  }
  const double det = m[0] * cof[0] + m[1] * cof[1] + m[2] * cof[2] + m[3] * cof[3];
  const double inv_det = 1.0 / det;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) o[r * 4 + c] = cof[c * 4 + r] * inv_det;
}

__device__ inline void matmul4(const double* a, const double* b, double* o) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) s += a[r * 4 + k] * b[k * 4 + c];
      o[r * 4 + c] = s;
    }
}

__device__ inline void matmul3(const double* a, const double* b, double* o) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r * 3 + 0] * b[0 * 3 + c] + a[r * 3 + 1] * b[1 * 3 + c] + a[r * 3 + 2] * b[2 * 3 + c];
}

// out = inverse(a) * c for fp32 4x4 inputs, result in fp64.
__device__ inline void relative_pose_f64(const float* a, const float* c, double* out) {
  double A[16], C[16], Ai[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    A[i] = static_cast<double>(a[i]);
    C[i] = static_cast<double>(c[i]);
  }
  inverse4(A, Ai);
  matmul4(Ai, C, out);
}

// ---- bilinear taps ---------------------------------------------------------------------------------------------
// grid_sample(bilinear, zeros padding, align_corners=True) at pixel position (ix, iy): four taps around
// floor(ix), floor(iy); a tap contributes only if it lies inside the image; non-finite positions contribute 0.
struct BilinearTaps {
  int x0, y0;             // north-west tap (may be outside the image)
  float w_nw, w_ne, w_sw, w_se;
  bool in_x0, in_x1, in_y0, in_y1;
};

__device__ inline BilinearTaps make_taps(float ix, float iy, int W, int H) {
  BilinearTaps t;
  // Anything this far out (or NaN/Inf) has no tap inside; clamp before the int conversion so it is well defined.
  const bool sane = (ix > -2.0f) && (ix < static_cast<float>(W) + 1.0f) && (iy > -2.0f) && (iy < static_cast<float>(H) + 1.0f);
  const float fx = sane ? floorf(ix) : -2.0f;
  const float fy = sane ? floorf(iy) : -2.0f;
  const float ax = sane ? ix : -2.0f;
  const float ay = sane ? iy : -2.0f;
  t.x0 = static_cast<int>(fx);
  t.y0 = static_cast<int>(fy);
  const float ex = (fx + 1.0f) - ax;  // ix_se - ix
  const float wx = ax - fx;           // ix - ix_nw
  const float ey = (fy + 1.0f) - ay;
  const float wy = ay - fy;
  t.w_nw = ex * ey;
  t.w_ne = wx * ey;
  t.w_sw = ex * wy;
  t.w_se = wx * wy;
  t.in_x0 = (t.x0 >= 0) && (t.x0 < W);
  t.in_x1 = (t.x0 + 1 >= 0) && (t.x0 + 1 < W);
  t.in_y0 = (t.y0 >= 0) && (t.y0 < H);
  t.in_y1 = (t.y0 + 1 >= 0) && (t.y0 + 1 < H);
  return t;
}

// grid_sample's align_corners=True un-normalisation, in the op order ATen uses: ((g + 1) / 2) * (size - 1)
__device__ inline float unnormalize_ac(float g, int size) { return ((g + 1.0f) * 0.5f) * static_cast<float>(size - 1); }

// ---- scans ------------------------------------------------------------------------------------------------------
__device__ inline int wave_inclusive_scan(int x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

// Exclusive scan of one int per thread over a block of kBlock threads (a multiple of 64); `total` = the block's sum.  `lds` holds
// kBlock / 64 ints.
template <int kBlock = 256>
__device__ inline int block_exclusive_scan(int v, int* lds, int& total) {
  const int incl = wave_inclusive_scan(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) lds[wave] = incl;
  __syncthreads();
  int prefix = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) {
    const int t = lds[w];
    if (w < wave) prefix += t;
    total += t;
  }
  return prefix + incl - v;
}

// The same for 64-bit values (sums wrap like the 32-bit ones): `lds` holds kBlock / 64 long longs.
__device__ inline long long wave_inclusive_scan(long long x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

template <int kBlock = 256>
__device__ inline long long block_exclusive_scan(long long v, long long* lds, long long& total) {
  const long long incl = wave_inclusive_scan(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) lds[wave] = incl;
  __syncthreads();
  long long prefix = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) {
    const long long t = lds[w];
    if (w < wave) prefix += t;
    total += t;
  }
  return prefix + incl - v;
}

// The scan of per-workgroup totals, by ONE workgroup of kThreads threads: totals[b] <- the sum of the totals before b, in place; every
// thread returns the sum of all.  Thread t takes the chunk of ceil(nblocks / kThreads) consecutive totals from t * chunk, clipped to
// nblocks (the last threads' chunks are short or empty).  `s` holds kThreads values in LDS and may be used again after the return.
// Integer sums: any association gives the same result.
template <int kThreads, typename T>
__device__ inline T scan_totals(T* __restrict__ totals, int nblocks, T* s) {
  const int t = threadIdx.x;
  const int chunk = (nblocks + kThreads - 1) / kThreads;
  const int begin = min(t * chunk, nblocks), end = min(begin + chunk, nblocks);
  T v = 0;
  for (int b = begin; b < end; ++b) v += totals[b];
  s[t] = v;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {       // Hillis-Steele inclusive scan
    const T a = t >= off ? s[t - off] : 0;
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  T o = s[t] - v;
  for (int b = begin; b < end; ++b) {
    const T c = totals[b];
    totals[b] = o;
    o += c;
  }
  const T all = s[kThreads - 1];
  __syncthreads();                                     // (s is used again)
  return all;
}

// ---- sums over a wave -------------------------------------------------------------------------------------------
// xor butterfly over the 64 lanes, masks 32, 16, .., 1: every lane ends with the same value (a + b and b + a are the same bits).  The
// order of the masks is part of the definition of every fp64 sum that uses it.
template <typename T>
__device__ inline T wave_sum(T x) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, kWave);
  return x;
}

// The same for every element of an array, in place.
template <typename T, int kCount>
__device__ inline void wave_sum(T (&v)[kCount]) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
#pragma unroll
    for (int k = 0; k < kCount; ++k) v[k] += __shfl_xor(v[k], m, kWave);
  }
}

// ---- the quantised area of a face ---------------------------------------------------------------------------------
// A_f of dvmvs/errors.py::quantised_face_areas for a face whose vertex indices are known to be valid: the fp64 area in units of
// 2^-32 m^2, rounded to nearest even; -1 for an area that is not finite or does not fit (an error).  Nothing is contracted into an FMA.
__device__ inline long long quantised_face_area(const float* __restrict__ verts, int ia, int ib, int ic) {
#pragma clang fp contract(off)
  double a[3], e1[3], e2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    a[d] = static_cast<double>(verts[static_cast<size_t>(ia) * 3 + d]);
    e1[d] = static_cast<double>(verts[static_cast<size_t>(ib) * 3 + d]) - a[d];
    e2[d] = static_cast<double>(verts[static_cast<size_t>(ic) * 3 + d]) - a[d];
  }
  const double cx = e1[1] * e2[2] - e1[2] * e2[1];
  const double cy = e1[2] * e2[0] - e1[0] * e2[2];
  const double cz = e1[0] * e2[1] - e1[1] * e2[0];
  const double n2 = (cx * cx + cy * cy) + cz * cz;
  const double area = sqrt(n2) * 0.5 * 4294967296.0;
  if (!(area < 9223372036854775808.0)) return -1;      // NaN, infinite or 2^63 and more
  return static_cast<long long>(rint(area));
}

}  // namespace dvmvs
