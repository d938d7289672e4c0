// One step of GP-MVS's Gaussian-process Kalman filter over the encoder bottleneck, on the device (gfx950).
// Semantics: the reference's dvmvs/baselines/gpmvs/run-testing.py:179-193 for the state mean M [2,N] (float64, as the reference's numpy):
//   M <- A M;  v = y - M[0];  M <- M + k v;  Z = relu(float32(M[0]))
// The 2x2 algebra (A = expm(F dt), Q, P, s, k) depends on the poses only and is evaluated on the host by the caller; A and k arrive by
// value.  y is the encoder's fp32 conv5 read in place, Z the decoder's fp32 input.  Columns are independent: one lane per column, a
// streaming pass over 16 + 4 + 4 bytes per column (N = 512 * 8 * 10: 0.98 MB in all).
#include "dvmvs_device.h"

namespace dvmvs {

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void gp_filter_step_kernel(double* __restrict__ state, const float* __restrict__ y, float* __restrict__ z, int N,
                                                             double a00, double a01, double a10, double a11, double k0, double k1, int reset) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double m0 = 0.0, m1 = 0.0;      // reset: the reference's M = np.zeros(...) at a scene's first frame
  if (!reset) {
    m0 = state[i];
    m1 = state[N + i];
  }
  const double p0 = a00 * m0 + a01 * m1;     // A.dot(M)
  const double p1 = a10 * m0 + a11 * m1;
  const double v = static_cast<double>(y[i]) - p0;
  m0 = p0 + k0 * v;                          // M += k.dot(v)
  m1 = p1 + k1 * v;
  state[i] = m0;
  state[N + i] = m1;
  z[i] = fmaxf(static_cast<float>(m0), 0.0f);
}
#pragma clang fp contract(fast)

}  // namespace dvmvs

extern "C" int dvmvs_gp_filter_step(double* state, const float* y, float* z, int N, double a00, double a01, double a10, double a11,
                                    double k0, double k1, int reset, dvmvs_stream_t stream) {
  if (!state || !y || !z || N <= 0 || (reset != 0 && reset != 1)) return DVMVS_EINVAL;
  if (N > (1 << 30)) return DVMVS_EUNSUPPORTED;
  hipLaunchKernelGGL(dvmvs::gp_filter_step_kernel, dim3((N + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), state, y, z, N,
                     a00, a01, a10, a11, k0, k1, reset);
  return dvmvs::launch_status();
}
