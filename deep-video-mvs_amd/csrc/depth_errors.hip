// Depth evaluation on the device (gfx950): the eight error metrics of dvmvs/errors.py::compute_errors for N frames in one launch.
//   dvmvs_depth_errors_fwd : gt, pred fp32 [N, pixels] -> metrics fp32 [N, 8] (and counts int [N, 4])
// The per-pixel terms are compute_errors' elementwise fp32 operations, operation by operation (every one rounded, true divisions,
// nothing contracted into an FMA, np.maximum's NaN rule); what differs from the host function is the SUMMATION: numpy adds the fp32
// terms pairwise in fp32, this file adds them in fp64, so a result is the fp32 rounding of the exact mean to ~1e-13 and does not depend
// on the order of the additions beyond that.  The order is fixed all the same, as a function of `pixels` alone:
//   - a frame is cut into quads of four consecutive pixels counted from the frame's first pixel, and into chunks of 256 quads;
//   - workgroup g of the frame's G = min(chunks, 256) takes chunks g, g + G, ...; thread t of it takes quad t of each, elements 0..3 in
//     order, into its own five fp64 sums and four integer counts;
//   - the 64 lanes of a wave are combined by an xor butterfly (32, 16, ... 1), the four waves in order by thread 0, which stores the
//     workgroup's partial sums in the workspace;
//   - the workgroup that arrives last at the frame's integer ticket (no floating-point atomics anywhere) adds the G partial sums BY
//     INDEX -- lane l of its first wave takes g = l, l + 64, ..., then the same butterfly -- writes the frame's row and clears the ticket.
// Which workgroup is last changes nothing: it performs the same additions on the same stored values.  Neither does the load width: a
// frame whose gt and pred rows are both 16-byte aligned is read with one 16-byte load per quad, any other frame (and the ragged last
// quad) with scalar loads of the same pixels into the same slots; and the grid's first dimension depends on `pixels` only, so a frame
// evaluated alone and inside a batch goes through identical additions.
// Measured: 7.2 us for a single 256x320 frame (80 workgroups), 135 us for N = 64 (42 MB): neither the launch
// floor nor the memory roof is reached yet; the per-workgroup release fence and ticket are the first suspects.
#include "dvmvs_device.h"

#pragma clang fp contract(off)

namespace dvmvs {

constexpr int kErrThreads = 256;                 // one quad per thread and chunk
constexpr int kErrChunk = 4 * kErrThreads;       // pixels of a chunk
constexpr int kErrMaxGroups = 256;               // workgroups per frame at most (one per CU)
constexpr int kErrSlab = 8;                      // doubles of one workgroup's partial sums: 5 sums, 4 counts in the space of 2, 1 unused
constexpr int kErrSums = 5;

typedef float float4v __attribute__((ext_vector_type(4)));

struct ErrAcc {
  double s[kErrSums];      // sum |d|, sum |d| / gt, sum |1/gt - 1/pred|, sum d d / gt, sum d d
  unsigned int c[4];       // n, ratio < 1.25, < 1.25^2, < 1.25^3
};

__device__ inline void err_clear(ErrAcc& a) {
#pragma unroll
  for (int k = 0; k < kErrSums; ++k) a.s[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) a.c[k] = 0u;
}

// compute_errors on one pixel: keep = gt >= 0.5 and gt <= max_depth (a NaN gt fails both); pred is not filtered
__device__ inline void err_pixel(ErrAcc& a, float gt, float pred, float max_depth) {
  if (!(gt >= 0.5f && gt <= max_depth)) return;
  const float d = gt - pred;
  const float ad = fabsf(d);
  const float sq = d * d;
  const float inv = fabsf(1.0f / gt - 1.0f / pred);
  const float r0 = gt / pred, r1 = pred / gt;
  const float ratio = (r0 >= r1 || r0 != r0) ? r0 : r1;      // np.maximum: a NaN operand gives NaN (fmaxf would drop it)
  a.s[0] += static_cast<double>(ad);
  a.s[1] += static_cast<double>(ad / gt);
  a.s[2] += static_cast<double>(inv);
  a.s[3] += static_cast<double>(sq / gt);
  a.s[4] += static_cast<double>(sq);
  a.c[0] += 1u;
  a.c[1] += ratio < 1.25f ? 1u : 0u;                          // a NaN ratio compares false: never an inlier
  a.c[2] += ratio < 1.5625f ? 1u : 0u;
  a.c[3] += ratio < 1.953125f ? 1u : 0u;
}

// the sums and the counts of the wave in every lane (wave_sum of dvmvs_device.h: the xor butterfly, masks 32, 16, .., 1)
__device__ inline void err_wave_sum(ErrAcc& a) {
  wave_sum(a.s);
  wave_sum(a.c);
}

// grid (G, n_frames), 256 threads.  workspace: n_frames ticket words (zero between calls), padded to 64 bytes; then per (frame, g) one
// slab of 8 doubles.
__global__ __launch_bounds__(kErrThreads) void depth_errors_kernel(const float* __restrict__ gt_all, const float* __restrict__ pred_all,
                                                                   int pixels, int chunks, float max_depth, float* __restrict__ metrics,
                                                                   int* __restrict__ counts, unsigned int* tickets, double* slabs) {
  __shared__ double s_sums[kErrThreads / kWave][kErrSums];
  __shared__ unsigned int s_counts[kErrThreads / kWave][4];
  __shared__ unsigned int s_last;
  const int t = threadIdx.x, frame = blockIdx.y, G = gridDim.x;
  const float* gt = gt_all + static_cast<size_t>(frame) * pixels;
  const float* pred = pred_all + static_cast<size_t>(frame) * pixels;
  const bool vec = ((reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(pred)) & 15u) == 0;    // per frame, uniform in the workgroup
  ErrAcc a;
  err_clear(a);
  for (int c = blockIdx.x; c < chunks; c += G) {
    const int p = c * kErrChunk + t * 4;           // < pixels + kErrChunk <= 2^24 + 1024
    if (p + 4 <= pixels) {
      float g[4], q[4];
      if (vec) {
        const float4v gv = *reinterpret_cast<const float4v*>(gt + p);
        const float4v qv = *reinterpret_cast<const float4v*>(pred + p);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          g[e] = gv[e];
          q[e] = qv[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          g[e] = gt[p + e];
          q[e] = pred[p + e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) err_pixel(a, g[e], q[e], max_depth);
    } else {
      for (int e = 0; e < 4 && p + e < pixels; ++e) err_pixel(a, gt[p + e], pred[p + e], max_depth);      // the frame's ragged last quad
    }
  }
  err_wave_sum(a);
  const int wave = t / kWave, lane = t % kWave;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kErrSums; ++k) s_sums[wave][k] = a.s[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) s_counts[wave][k] = a.c[k];
  }
  __syncthreads();
  if (t == 0) {
    double* slab = slabs + (static_cast<size_t>(frame) * G + blockIdx.x) * kErrSlab;
#pragma unroll
    for (int k = 0; k < kErrSums; ++k) {
      double s = s_sums[0][k];
      for (int w = 1; w < kErrThreads / kWave; ++w) s += s_sums[w][k];
      slab[k] = s;
    }
    unsigned int* slab_counts = reinterpret_cast<unsigned int*>(slab + kErrSums);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned int n = s_counts[0][k];
      for (int w = 1; w < kErrThreads / kWave; ++w) n += s_counts[w][k];
      slab_counts[k] = n;
    }
    // publish the slab, then take the frame's ticket: release at device scope, the stores drained before the atomic is issued (the
    // fence normally drains them itself; the explicit wait costs nothing and does not depend on the compiler emitting the fence's own)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int ticket = __hip_atomic_fetch_add(tickets + frame, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = ticket == static_cast<unsigned int>(G) - 1u ? 1u : 0u;
  }
  __syncthreads();
  if (s_last == 0u || t >= kWave) return;
  // the last workgroup of the frame: every slab of the frame has been published before its ticket was taken
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  err_clear(a);
  for (int g = t; g < G; g += kWave) {
    const double* slab = slabs + (static_cast<size_t>(frame) * G + g) * kErrSlab;
#pragma unroll
    for (int k = 0; k < kErrSums; ++k) a.s[k] += slab[k];
    const unsigned int* slab_counts = reinterpret_cast<const unsigned int*>(slab + kErrSums);
#pragma unroll
    for (int k = 0; k < 4; ++k) a.c[k] += slab_counts[k];
  }
  err_wave_sum(a);
  if (t != 0) return;
  __hip_atomic_store(tickets + frame, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // as the next call expects it
  float* row = metrics + static_cast<size_t>(frame) * 8;
  if (counts) {
#pragma unroll
    for (int k = 0; k < 4; ++k) counts[static_cast<size_t>(frame) * 4 + k] = static_cast<int>(a.c[k]);
  }
  if (a.c[0] == 0u) {
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = nan;
    return;
  }
  const double n = static_cast<double>(a.c[0]);
#pragma unroll
  for (int k = 0; k < 4; ++k) row[k] = static_cast<float>(a.s[k] / n);
  row[4] = static_cast<float>(sqrt(a.s[4] / n));
  const float nf = static_cast<float>(a.c[0]);     // exact: n < 2^24
#pragma unroll
  for (int k = 1; k < 4; ++k) row[4 + k] = static_cast<float>(a.c[k]) / nf;
}

static int err_chunks(long long pixels) { return static_cast<int>((pixels + kErrChunk - 1) / kErrChunk); }
static int err_groups(long long pixels) { return err_chunks(pixels) < kErrMaxGroups ? err_chunks(pixels) : kErrMaxGroups; }
static size_t err_ticket_bytes(int n_frames) { return (static_cast<size_t>(n_frames) * sizeof(unsigned int) + 63) / 64 * 64; }

}  // namespace dvmvs

extern "C" size_t dvmvs_depth_errors_workspace_bytes(int n_frames, long long pixels) {
  using namespace dvmvs;
  if (n_frames < 1 || n_frames > 65535 || pixels < 1 || pixels >= (1LL << 24)) return 0;
  return err_ticket_bytes(n_frames) + static_cast<size_t>(n_frames) * err_groups(pixels) * kErrSlab * sizeof(double);
}

extern "C" int dvmvs_depth_errors_fwd(const float* gt, const float* pred, int n_frames, long long pixels, float max_depth, float* metrics,
                                      int* counts, void* workspace, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!gt || !pred || !metrics || !workspace || n_frames < 1 || pixels < 1) return DVMVS_EINVAL;
  if (max_depth != max_depth) return DVMVS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(metrics) |
       reinterpret_cast<uintptr_t>(counts)) % 4 != 0 || reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return DVMVS_EINVAL;
  if (pixels >= (1LL << 24) || n_frames > 65535) return DVMVS_EUNSUPPORTED;
  unsigned int* tickets = static_cast<unsigned int*>(workspace);
  double* slabs = reinterpret_cast<double*>(static_cast<char*>(workspace) + err_ticket_bytes(n_frames));
  const dim3 grid(err_groups(pixels), n_frames), block(kErrThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int px = static_cast<int>(pixels), chunks = err_chunks(pixels);
  hipLaunchKernelGGL(depth_errors_kernel, grid, block, 0, s, gt, pred, px, chunks, max_depth, metrics, counts, tickets, slabs);
  return launch_status();
}
