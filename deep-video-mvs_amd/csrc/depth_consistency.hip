// Multi-view geometric consistency filter for depth maps, gfx950 (contract: include/dvmvs_hip.h, "Depth-map consistency").
//
// A pixel of frame r with depth d is projected into a source frame s, the source's depth map is sampled there (bilinear, four
// valid taps), the sample is projected back into r, and the source counts as consistent when the pixel comes back within
// pixel_threshold pixels and within relative_threshold of its own depth.  The reference project has nothing for this; the
// definition is this project's own (the check of the MVSNet family's fusion step, without the square root).
//
// Two launches.  consistency_matrices_kernel: one thread per (frame, slot), float64, each 3x4 matrix rounded once to float32 --
// 24 words per slot, so that the per-pixel kernel's contract is pure float32.  depth_consistency_kernel: one launch for all N
// frames, blockIdx.y = frame.  The frame index being a grid dimension makes sources[r][j], the slot's 24 matrix words and the
// source map's base wave-uniform: they are scalar loads into SGPRs, and a skipped slot is a scalar branch around the whole
// per-pixel body.  A thread owns kPix = 4 consecutive pixels of a row: their 16 taps are gathered with unconditional loads from
// clamped addresses (validity is applied by selects afterwards), so all 16 are in flight before the first use.  Where W is a
// multiple of 4 and the maps are 16-byte aligned (count: 4-byte) the launch takes the kVec instantiation: the own depths arrive
// as one 16-byte load, out_depth leaves as one 16-byte store, count as one 4-byte store and points as three 16-byte stores;
// otherwise (an odd width, a view that starts off a 16-byte boundary) the launch takes the instantiation with single-element
// accesses and a ragged last thread per row.  The choice is the host's, per launch; the values are the same either way.
// Every output element has one writer; there are no atomics and no cross-thread reductions, so the bits depend on the inputs only.
//
// Algorithmic bytes: N * H * W * (4 read + 4 written + 1 count [+ 12 points]) plus the gathered taps (16 bytes per pixel and
// non-skipped slot, served by L2: one 256x320 map is 320 KB).  Measured on an MI355X (profiles/depth_consistency_bench.json, 256x320,
// S = 4, depth and count out, medians of HIP-event timings): the pixel launch takes 34 us for N = 8 and 92 us for N = 64 (8 % of
// the HBM bandwidth a copy reaches: the kernel is bound by its arithmetic -- 5 correctly rounded divisions per pixel and slot --
// and by the L2 gathers, not by HBM); with the matrices launch 61 / 116 us.  The points output was not measured.
#include "dvmvs_device.h"

namespace dvmvs {

constexpr int kConsistencyMaxSources = 16;
constexpr int kPix = 4;   // consecutive pixels of a row per thread

__device__ inline bool source_slot_skipped(int s, int r, int N) { return s < 0 || s >= N || s == r; }

// [R|t] = inv_rigid(pose_b) * pose_a, A = K_b R K_a^-1, b = K_b t: the map from (pixel, depth) of frame a to frame b.
// Operation order (float64, no contraction; part of the contract and restated in tests/consistency_reference.py):
//   R[i][j] = (Rb[0][i] Ra[0][j] + Rb[1][i] Ra[1][j]) + Rb[2][i] Ra[2][j]
//   ti[i]   = -((Rb[0][i] tb[0] + Rb[1][i] tb[1]) + Rb[2][i] tb[2])
//   t[i]    = ((Rb[0][i] ta[0] + Rb[1][i] ta[1]) + Rb[2][i] ta[2]) + ti[i]
//   M       = K_b R: M[0][j] = fx_b R[0][j] + cx_b R[2][j], M[1][j] = fy_b R[1][j] + cy_b R[2][j], M[2][j] = R[2][j]
//   A[i][0] = M[i][0] (1 / fx_a), A[i][1] = M[i][1] (1 / fy_a), A[i][2] = (M[i][0] (-(cx_a / fx_a)) + M[i][1] (-(cy_a / fy_a))) + M[i][2]
//   b[0]    = fx_b t[0] + cx_b t[2], b[1] = fy_b t[1] + cy_b t[2], b[2] = t[2]
__device__ inline void consistency_pair(const float* Ka, const float* Pa, const float* Kb, const float* Pb, float* out) {
#pragma clang fp contract(off)
  double Ra[9], Rb[9], ta[3], tb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Ra[i * 3 + j] = static_cast<double>(Pa[i * 4 + j]);
      Rb[i * 3 + j] = static_cast<double>(Pb[i * 4 + j]);
    }
    ta[i] = static_cast<double>(Pa[i * 4 + 3]);
    tb[i] = static_cast<double>(Pb[i * 4 + 3]);
  }
  const double fxa = Ka[0], fya = Ka[4], cxa = Ka[2], cya = Ka[5];
  const double fxb = Kb[0], fyb = Kb[4], cxb = Kb[2], cyb = Kb[5];
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (Rb[0 + i] * Ra[0 + j] + Rb[3 + i] * Ra[3 + j]) + Rb[6 + i] * Ra[6 + j];
    const double ti = -((Rb[0 + i] * tb[0] + Rb[3 + i] * tb[1]) + Rb[6 + i] * tb[2]);
    t[i] = ((Rb[0 + i] * ta[0] + Rb[3 + i] * ta[1]) + Rb[6 + i] * ta[2]) + ti;
  }
  const double ifx = 1.0 / fxa, ify = 1.0 / fya, k02 = -(cxa / fxa), k12 = -(cya / fya);
  double M[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    M[0 + j] = fxb * R[0 + j] + cxb * R[6 + j];
    M[3 + j] = fyb * R[3 + j] + cyb * R[6 + j];
    M[6 + j] = R[6 + j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    out[i * 3 + 0] = static_cast<float>(M[i * 3 + 0] * ifx);
    out[i * 3 + 1] = static_cast<float>(M[i * 3 + 1] * ify);
    out[i * 3 + 2] = static_cast<float>((M[i * 3 + 0] * k02 + M[i * 3 + 1] * k12) + M[i * 3 + 2]);
  }
  out[9] = static_cast<float>(fxb * t[0] + cxb * t[2]);
  out[10] = static_cast<float>(fyb * t[1] + cyb * t[2]);
  out[11] = static_cast<float>(t[2]);
}

__global__ __launch_bounds__(64) void consistency_matrices_kernel(const float* __restrict__ K, const float* __restrict__ pose,
                                                                  const int* __restrict__ sources, float* __restrict__ out, int N,
                                                                  int S) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * S) return;
  const int r = i / S;
  const int s = sources[i];
  float* o = out + static_cast<size_t>(i) * 24;
  if (source_slot_skipped(s, r, N)) {
#pragma unroll
    for (int k = 0; k < 24; ++k) o[k] = 0.0f;
    return;
  }
  float m[24];
  consistency_pair(K + r * 9, pose + r * 16, K + s * 9, pose + s * 16, m);        // r -> s: A, b
  consistency_pair(K + s * 9, pose + s * 16, K + r * 9, pose + r * 16, m + 12);   // s -> r: A', b'
#pragma unroll
  for (int k = 0; k < 24; ++k) o[k] = m[k];
}

__device__ inline bool valid_depth(float d) { return d > 0.0f && d <= 3.402823466e+38f; }   // finite and positive; false for NaN

template <bool kVec, bool kCount, bool kPoints>
__global__ __launch_bounds__(256) void depth_consistency_kernel(const float* __restrict__ depth, const float* __restrict__ K,
                                                                const float* __restrict__ pose, const int* __restrict__ sources,
                                                                const float* __restrict__ matrices, float* __restrict__ out_depth,
                                                                unsigned char* __restrict__ out_count, float* __restrict__ out_points,
                                                                int N, int S, int H, int W, float threshold2, float relative_threshold,
                                                                int min_views, int average) {
#pragma clang fp contract(off)
  const int r = blockIdx.y;
  const int groups_per_row = (W + kPix - 1) / kPix;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= H * groups_per_row) return;
  const int y = g / groups_per_row;
  const int x = (g - y * groups_per_row) * kPix;
  const int HW = H * W;
  const int first = y * W + x;                         // element of the frame this thread starts at
  const int n_own = kVec ? kPix : (W - x < kPix ? W - x : kPix);   // pixels of the row this thread has (a ragged tail has fewer)
  const size_t frame = static_cast<size_t>(r) * HW;

  const float* own = depth + frame + first;
  float d[kPix];
  if (kVec) {
    const float4 v4 = *reinterpret_cast<const float4*>(own);
    d[0] = v4.x, d[1] = v4.y, d[2] = v4.z, d[3] = v4.w;
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k) d[k] = k < n_own ? own[k] : 0.0f;
  }
  const float v = static_cast<float>(y);
  float sum[kPix];
  int count[kPix];
  bool valid[kPix];
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    valid[k] = valid_depth(d[k]);
    sum[k] = d[k];
    count[k] = 0;
  }

  if (H >= 2 && W >= 2) {
    const float wmax = static_cast<float>(W - 1), hmax = static_cast<float>(H - 1);
    const float xcap = static_cast<float>(W - 2), ycap = static_cast<float>(H - 2);
    for (int j = 0; j < S; ++j) {
      const int s = sources[r * S + j];                         // wave-uniform: a scalar load
      if (source_slot_skipped(s, r, N)) continue;               // ... and a scalar branch
      const float* m = matrices + (static_cast<size_t>(r) * S + j) * 24;   // 24 scalar loads
      const float* src = depth + static_cast<size_t>(s) * HW;
      float us[kPix], vs[kPix], wx[kPix], wy[kPix], t00[kPix], t01[kPix], t10[kPix], t11[kPix];
      bool ok[kPix];
#pragma unroll
      for (int k = 0; k < kPix; ++k) {
        const float u = static_cast<float>(x + k);
        const float px = d[k] * ((m[0] * u + m[1] * v) + m[2]) + m[9];
        const float py = d[k] * ((m[3] * u + m[4] * v) + m[5]) + m[10];
        const float pz = d[k] * ((m[6] * u + m[7] * v) + m[8]) + m[11];
        us[k] = px / pz;
        vs[k] = py / pz;
        ok[k] = valid[k] && pz > 0.0f && us[k] >= 0.0f && us[k] <= wmax && vs[k] >= 0.0f && vs[k] <= hmax;
        const float fx = ok[k] ? fminf(floorf(us[k]), xcap) : 0.0f;   // a pixel that is out keeps a legal address: the loads are unconditional
        const float fy = ok[k] ? fminf(floorf(vs[k]), ycap) : 0.0f;
        wx[k] = us[k] - fx;
        wy[k] = vs[k] - fy;
        const float* tap = src + (static_cast<int>(fy) * W + static_cast<int>(fx));
        t00[k] = tap[0];
        t01[k] = tap[1];
        t10[k] = tap[W];
        t11[k] = tap[W + 1];
      }
#pragma unroll
      for (int k = 0; k < kPix; ++k) {
        const bool taps = valid_depth(t00[k]) && valid_depth(t01[k]) && valid_depth(t10[k]) && valid_depth(t11[k]);
        const float top = t00[k] + wx[k] * (t01[k] - t00[k]);
        const float bot = t10[k] + wx[k] * (t11[k] - t10[k]);
        const float ds = top + wy[k] * (bot - top);
        const float qx = ds * ((m[12] * us[k] + m[13] * vs[k]) + m[14]) + m[21];
        const float qy = ds * ((m[15] * us[k] + m[16] * vs[k]) + m[17]) + m[22];
        const float qz = ds * ((m[18] * us[k] + m[19] * vs[k]) + m[20]) + m[23];
        const float du = qx / qz - static_cast<float>(x + k);
        const float dv = qy / qz - v;
        const float err2 = du * du + dv * dv;
        const float rel = fabsf(qz - d[k]) / d[k];
        const bool consistent = ok[k] && taps && qz > 0.0f && err2 < threshold2 && rel < relative_threshold;
        sum[k] = consistent ? sum[k] + qz : sum[k];
        count[k] += consistent ? 1 : 0;
      }
    }
  }

  float z[kPix];
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    const float fused = sum[k] / static_cast<float>(count[k] + 1);
    z[k] = (valid[k] && count[k] >= min_views) ? (average ? fused : d[k]) : 0.0f;
    if (!valid[k]) count[k] = 0;
  }
  float* od = out_depth + frame + first;
  if (kVec) {
    *reinterpret_cast<float4*>(od) = make_float4(z[0], z[1], z[2], z[3]);
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k)
      if (k < n_own) od[k] = z[k];
  }
  if (kCount) {
    unsigned char* oc = out_count + frame + first;
    if (kVec) {
      *reinterpret_cast<uchar4*>(oc) = make_uchar4(static_cast<unsigned char>(count[0]), static_cast<unsigned char>(count[1]),
                                                   static_cast<unsigned char>(count[2]), static_cast<unsigned char>(count[3]));
    } else {
#pragma unroll
      for (int k = 0; k < kPix; ++k)
        if (k < n_own) oc[k] = static_cast<unsigned char>(count[k]);
    }
  }
  if (kPoints) {
    // world = pose_r * (z * K_r^-1 [u, v, 1]): xn = (u - cx) / fx, yn = (v - cy) / fy, X = z xn, Y = z yn, Z = z,
    // world[i] = ((P[i][0] X + P[i][1] Y) + P[i][2] Z) + P[i][3]; zeros where z == 0
    const float* Kr = K + r * 9;
    const float* P = pose + r * 16;
    const float fx = Kr[0], fy = Kr[4], cx = Kr[2], cy = Kr[5];
    const float yn = (v - cy) / fy;
    float w[kPix * 3];
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      const float xn = (static_cast<float>(x + k) - cx) / fx;
      const float X = z[k] * xn, Y = z[k] * yn, Z = z[k];
      const bool kept = z[k] > 0.0f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float c = ((P[i * 4 + 0] * X + P[i * 4 + 1] * Y) + P[i * 4 + 2] * Z) + P[i * 4 + 3];
        w[k * 3 + i] = kept ? c : 0.0f;
      }
    }
    float* op = out_points + (frame + first) * 3;
    if (kVec) {
      float4* op4 = reinterpret_cast<float4*>(op);
      op4[0] = make_float4(w[0], w[1], w[2], w[3]);
      op4[1] = make_float4(w[4], w[5], w[6], w[7]);
      op4[2] = make_float4(w[8], w[9], w[10], w[11]);
    } else {
#pragma unroll
      for (int k = 0; k < kPix; ++k)
        if (k < n_own) {
          op[k * 3 + 0] = w[k * 3 + 0];
          op[k * 3 + 1] = w[k * 3 + 1];
          op[k * 3 + 2] = w[k * 3 + 2];
        }
    }
  }
}

inline int consistency_sizes_status(int N, int S, int H, int W) {
  if (N < 1 || S < 0 || S > kConsistencyMaxSources || H < 1 || W < 1) return DVMVS_EINVAL;
  if (N > 65535) return DVMVS_EUNSUPPORTED;
  // offsets inside a frame are 32-bit (the largest: 3 H W floats of points, and H * ceil(W / 4) + 255 thread indices); frame bases are 64-bit
  if (static_cast<long long>(H) * W * 3 >= (1LL << 31) || static_cast<long long>(H) * ((W + kPix - 1) / kPix) + 256 >= (1LL << 31))
    return DVMVS_EUNSUPPORTED;
  return 0;
}

}  // namespace dvmvs

extern "C" int dvmvs_consistency_matrices(const float* K, const float* pose, const int* sources, float* matrices, int N, int S,
                                          dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!K || !pose || !matrices || (S > 0 && !sources)) return DVMVS_EINVAL;
  const int rc = consistency_sizes_status(N, S, 1, 1);
  if (rc != 0) return rc;
  if (S == 0) return 0;   // nothing to write
  const int n = N * S;
  hipLaunchKernelGGL(consistency_matrices_kernel, dim3((n + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), K, pose, sources,
                     matrices, N, S);
  return launch_status();
}

extern "C" int dvmvs_depth_consistency_fwd(const float* depth, const float* K, const float* pose, const int* sources, const float* matrices,
                                           float* out_depth, unsigned char* count, float* points, int N, int S, int H, int W,
                                           float pixel_threshold, float relative_threshold, int min_views, int average,
                                           dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!depth || !K || !pose || !out_depth || (S > 0 && (!sources || !matrices))) return DVMVS_EINVAL;
  if (pixel_threshold != pixel_threshold || relative_threshold != relative_threshold || min_views < 0 || (average != 0 && average != 1))
    return DVMVS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(out_depth) | reinterpret_cast<uintptr_t>(points) |
       reinterpret_cast<uintptr_t>(matrices) | reinterpret_cast<uintptr_t>(sources)) & 3)
    return DVMVS_EINVAL;
  const int rc = consistency_sizes_status(N, S, H, W);
  if (rc != 0) return rc;
  const float threshold2 = pixel_threshold * pixel_threshold;   // squared once, in fp32
  const int groups = H * ((W + kPix - 1) / kPix);
  const dim3 grid((groups + 255) / 256, N), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 16-byte accesses need every row of every map to start on a 16-byte boundary (count: 4-byte)
  const bool vec = W % kPix == 0 && ((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(out_depth) |
                                      reinterpret_cast<uintptr_t>(points)) & 15) == 0 && (reinterpret_cast<uintptr_t>(count) & 3) == 0;
#define DVMVS_CONSISTENCY_LAUNCH(V, C, P)                                                                                                 \
  hipLaunchKernelGGL((depth_consistency_kernel<V, C, P>), grid, block, 0, s, depth, K, pose, sources, matrices, out_depth, count, points, \
                     N, S, H, W, threshold2, relative_threshold, min_views, average)
#define DVMVS_CONSISTENCY_OUTPUTS(V)                       \
  do {                                                     \
    if (count && points) DVMVS_CONSISTENCY_LAUNCH(V, true, true);        \
    else if (count) DVMVS_CONSISTENCY_LAUNCH(V, true, false);            \
    else if (points) DVMVS_CONSISTENCY_LAUNCH(V, false, true);           \
    else DVMVS_CONSISTENCY_LAUNCH(V, false, false);                      \
  } while (0)
  if (vec) DVMVS_CONSISTENCY_OUTPUTS(true);
  else DVMVS_CONSISTENCY_OUTPUTS(false);
#undef DVMVS_CONSISTENCY_OUTPUTS
#undef DVMVS_CONSISTENCY_LAUNCH
  return launch_status();
}
