// Point sets for the 3-D reconstruction metrics (gfx950): area-weighted samples of a triangle mesh, and one point per occupied voxel of a
// cloud.  Both reproduce their host definitions bit for bit (dvmvs/errors.py::sample_surface, voxel_down_sample; include/dvmvs_hip.h).
//   dvmvs_surface_sample_count / _emit     : verts fp32 [V,3], faces int32 [F,3], density, seed -> points fp32 [N,3] (face int32 [N])
//   dvmvs_voxel_keys                       : points fp32 [N,3], 1 / voxel -> key int64 [N]
//   dvmvs_voxel_downsample_count / _emit   : the keys and indices after a stable sort -> points fp32 [M,3] (count int32 [M])
//   dvmvs_voxel_downsample_runs            : host only: where the count step left the run starts and the points in sorted order (for
//                                            csrc/mesh_simplify.hip, whose clusters are these voxels)
//
// Everything that decides a result is an integer (areas quantised to 2^-32 m^2, their prefix sums, keys, ranks) or a float operation whose
// operands and order the definition fixes: no float atomics, no float value crosses threads, nothing is contracted into an FMA
// (contract(off) for the whole file).  Integer sums are exact, so the order of a parallel scan cannot show.
//
// surface_sample, count (3 enqueues): ss_area_kernel (A_f and, per 1024 faces, their sum) -> ss_scan_blocks_kernel (one workgroup: prefix
// of the block sums; N, the status and the total go to `counts`) -> ss_scan_apply_kernel (cum_f, inclusive, in place; the int64
// block_exclusive_scan of dvmvs_device.h).  A total of 2^63 or more is found exactly, from sums of the areas' upper and lower 32 bits.
// emit (1 enqueue): ss_emit_kernel, one thread per sample k: binary search of t_k in cum, then the point.  A large face among small ones
// is spread over as many threads as it has samples.  A face with an index outside [0, V) has A_f = 0 and is never found by the search:
// only the area kernel looks at such a face, and it reads no vertex for it.
//
// voxel_downsample: keys (3 enqueues): vx_min_kernel -> vx_min_final_kernel (mn, status = 0) -> vx_key_kernel.  The caller sorts (key,
// index) stably.  count (3 enqueues): vx_head_kernel (run heads per 1024 sorted slots; gathers the points into sorted order) ->
// vx_scan_blocks_kernel (M and the status to `counts`) -> vx_start_kernel (start slot of run m).  emit (1 enqueue): vx_mean_kernel, one
// thread per voxel walks its run of the sorted copy in order: sequential memory, fp64 sum, one division, one rounding.  Linear in N.
#include "dvmvs_device.h"

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

constexpr int kSsBlock = 256;
constexpr int kSsPerThread = 4;
constexpr int kSsChunk = kSsBlock * kSsPerThread;     // faces (or sorted slots) per workgroup of a scan
constexpr int kSsScanThreads = 1024;                  // the one workgroup that scans the workgroup totals
constexpr long long kSsMaxFaces = 1LL << 28;
constexpr long long kSsMaxPoints = 1LL << 28;
constexpr long long kSsTooLarge = 1LL << 31;            // floor(total area / 2^32) from which the total no longer fits
constexpr int kVxMinGroups = 256;
constexpr int kVxMaxCells = 1 << 21;

// A_f of the definition: 0 for a face with an index outside [0, V); -1 for an area that is not finite or does not fit (an error)
__device__ inline long long ss_face_area(const float* __restrict__ verts, long long V, const int* __restrict__ faces, long long f) {
  const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
  if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) return 0;
  return quantised_face_area(verts, ia, ib, ic);
}

// cum[f] <- A_f; totals[block] <- the sum of the block's A_f (wraps when it does not fit); high[block] <- floor(the exact sum / 2^32),
// from the separately summed upper and lower halves (neither can overflow: 1024 values below 2^31 and 2^32), + 2^31 per bad face
__global__ __launch_bounds__(kSsBlock) void ss_area_kernel(const float* __restrict__ verts, long long V, const int* __restrict__ faces, long long F,
                                                           long long* __restrict__ cum, long long* __restrict__ totals,
                                                           long long* __restrict__ high) {
  __shared__ long long lds[2][kSsBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kSsBlock + threadIdx.x) * kSsPerThread;
  long long hi = 0, lo = 0;
  for (int e = 0; e < kSsPerThread; ++e) {
    if (first + e < F) {
      long long area = ss_face_area(verts, V, faces, first + e);
      if (area < 0) {
        area = 0;
        hi += kSsTooLarge;
      }
      cum[first + e] = area;
      hi += area >> 32;
      lo += area & 0xffffffffLL;
    }
  }
  long long hi_total, lo_total;
  block_exclusive_scan<kSsBlock>(hi, lds[0], hi_total);
  block_exclusive_scan<kSsBlock>(lo, lds[1], lo_total);
  if (threadIdx.x == 0) {
    totals[blockIdx.x] = static_cast<long long>((static_cast<unsigned long long>(hi_total) << 32) + static_cast<unsigned long long>(lo_total));
    high[blockIdx.x] = hi_total + (lo_total >> 32);
  }
}

// One workgroup: totals[b] <- the sum of the totals before b; counts = {N, status, cum_F}.  status 1: the exact total is 2^63 or more
// (floor(total / 2^32) >= 2^31, from the blocks' upper halves and the sum of their lower halves), or a face was bad.
__global__ __launch_bounds__(kSsScanThreads) void ss_scan_blocks_kernel(long long* __restrict__ totals, const long long* __restrict__ high,
                                                                        int nblocks, long long D, long long* __restrict__ counts) {
  __shared__ long long s[kSsScanThreads], s_hi[kSsScanThreads], s_lo[kSsScanThreads];
  const int t = threadIdx.x;
  long long hi = 0, lo = 0;
  for (int b = t; b < nblocks; b += kSsScanThreads) {      // (before the scan overwrites the totals)
    hi += min(high[b], kSsTooLarge);                 // (capped: 2^18 blocks of 2^31 cannot overflow)
    lo += totals[b] & 0xffffffffLL;
  }
  s_hi[t] = hi;
  s_lo[t] = lo;
  const long long total = scan_totals<kSsScanThreads>(totals, nblocks, s);      // (its barriers publish s_hi and s_lo as well)
  if (t == kSsScanThreads - 1) {
    long long all_hi = 0, all_lo = 0;
    for (int i = 0; i < kSsScanThreads; ++i) {
      all_hi += s_hi[i];
      all_lo += s_lo[i];
    }
    const bool bad = all_hi + (all_lo >> 32) >= kSsTooLarge;
    const long long half = D >> 1;
    counts[0] = bad || total <= half ? 0 : (total - half - 1) / D + 1;
    counts[1] = bad ? 1 : 0;
    counts[2] = bad ? 0 : total;
  }
}

// cum[f] <- A_0 + ... + A_f
__global__ __launch_bounds__(kSsBlock) void ss_scan_apply_kernel(long long* __restrict__ cum, long long F, const long long* __restrict__ offsets) {
  __shared__ long long lds[kSsBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kSsBlock + threadIdx.x) * kSsPerThread;
  long long c[kSsPerThread], v = 0;
#pragma unroll
  for (int e = 0; e < kSsPerThread; ++e) {
    c[e] = first + e < F ? cum[first + e] : 0;
    v += c[e];
  }
  long long total;
  long long o = offsets[blockIdx.x] + block_exclusive_scan<kSsBlock>(v, lds, total);
#pragma unroll
  for (int e = 0; e < kSsPerThread; ++e) {
    o += c[e];
    if (first + e < F) cum[first + e] = o;
  }
}

__device__ __host__ inline unsigned int lowbias32(unsigned int x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__global__ __launch_bounds__(kSsBlock) void ss_emit_kernel(const float* __restrict__ verts, long long V, const int* __restrict__ faces, long long F,
                                                           const long long* __restrict__ cum, long long D, unsigned int r0, unsigned int r1,
                                                           long long N, float* __restrict__ points, int* __restrict__ face_out) {
  const long long k = static_cast<long long>(blockIdx.x) * kSsBlock + threadIdx.x;
  if (k >= N) return;
  const long long t = k * D + (D >> 1);
  long long lo = 0, hi = F;            // the first f with cum[f] > t: searchsorted(cum, t, side="right")
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (cum[mid] > t) hi = mid; else lo = mid + 1;
  }
  const long long f = lo;
  float p[3] = {0.0f, 0.0f, 0.0f};
  int found = -1;
  if (f < F) {                         // always, when N and cum come from the count step of the same mesh
    const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
    if (ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V) {      // always: such a face has an area (file comment)
      const unsigned int k32 = static_cast<unsigned int>(k);
      const unsigned int h1 = k32 * 0xC13FA9A9u + r0, h2 = k32 * 0x91E10DA5u + r1;
      float u = static_cast<float>(h1 >> 8) * 5.9604644775390625e-8f;       // 2^-24
      float v = static_cast<float>(h2 >> 8) * 5.9604644775390625e-8f;
      if (u + v > 1.0f) {
        u = 1.0f - u;
        v = 1.0f - v;
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float a = verts[static_cast<size_t>(ia) * 3 + d];
        const float b = verts[static_cast<size_t>(ib) * 3 + d];
        const float c = verts[static_cast<size_t>(ic) * 3 + d];
        p[d] = (a + u * (b - a)) + v * (c - a);
      }
      found = static_cast<int>(f);
    }
  }
  points[k * 3] = p[0];
  points[k * 3 + 1] = p[1];
  points[k * 3 + 2] = p[2];
  if (face_out) face_out[k] = found;
}

size_t ss_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

int ss_blocks(long long n) { return static_cast<int>((n + kSsChunk - 1) / kSsChunk); }      // <= 2^18

// surface_sample workspace: block totals [blocks of F] int64 | their upper halves [blocks of F] int64 | cum [F] int64
struct SsLayout {
  size_t high_off, cum_off, total;
};

SsLayout ss_layout(long long F) {
  SsLayout l;
  l.high_off = ss_align(static_cast<size_t>(ss_blocks(F)) * sizeof(long long));
  l.cum_off = 2 * l.high_off;
  l.total = l.cum_off + ss_align(static_cast<size_t>(F) * sizeof(long long));
  return l;
}

long long ss_spacing(double density) {
  const double d = rint(4294967296.0 / density);
  if (!(d >= 1.0)) return 1;
  return d < 9.2e18 ? static_cast<long long>(d) : 0x7fffffffffffffffLL;
}

// ---- voxel down-sampling ------------------------------------------------------------------------------------------------------------
struct VxHeader {
  float mn[3];
  int status;        // bit 0: a cell index of 2^21 or more (or a coordinate that is not finite)
};

// partials [gridDim.x, 3]: the minimum of x, y, z over the points i = global thread, + threads, ...
__global__ __launch_bounds__(kSsBlock) void vx_min_kernel(const float* __restrict__ pts, long long n, float* __restrict__ partials) {
  __shared__ float s[kSsBlock / kWave][3];
  const float inf = __builtin_inff();
  float v[3] = {inf, inf, inf};
  for (long long i = static_cast<long long>(blockIdx.x) * kSsBlock + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * kSsBlock) {
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = fminf(v[a], pts[i * 3 + a]);
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = fminf(v[a], __shfl_xor(v[a], m, kWave));
  }
  if (threadIdx.x % kWave == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) s[threadIdx.x / kWave][a] = v[a];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float r = s[0][threadIdx.x];
    for (int w = 1; w < kSsBlock / kWave; ++w) r = fminf(r, s[w][threadIdx.x]);
    partials[blockIdx.x * 3 + threadIdx.x] = r;
  }
}

// One wave: the minimum of the partial minima -> the header, status 0.
__global__ __launch_bounds__(kWave) void vx_min_final_kernel(const float* __restrict__ partials, int groups, VxHeader* __restrict__ hdr) {
  const float inf = __builtin_inff();
  float v[3] = {inf, inf, inf};
  for (int g = threadIdx.x; g < groups; g += kWave) {
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = fminf(v[a], partials[g * 3 + a]);
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = fminf(v[a], __shfl_xor(v[a], m, kWave));
  }
  if (threadIdx.x == 0) {
    hdr->mn[0] = v[0];
    hdr->mn[1] = v[1];
    hdr->mn[2] = v[2];
    hdr->status = 0;
  }
}

__global__ __launch_bounds__(kSsBlock) void vx_key_kernel(const float* __restrict__ pts, long long n, float inv, VxHeader* __restrict__ hdr,
                                                          long long* __restrict__ keys) {
  const long long i = static_cast<long long>(blockIdx.x) * kSsBlock + threadIdx.x;
  if (i >= n) return;
  long long key = 0;
  bool bad = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float s = (pts[i * 3 + a] - hdr->mn[a]) * inv;      // >= 0: truncation is floor
    const bool ok = s < static_cast<float>(kVxMaxCells);     // false for a NaN as well
    bad = bad || !ok;
    key = (key << 21) | static_cast<long long>(ok ? static_cast<int>(s) : 0);
  }
  keys[i] = key;
  if (bad) atomicOr(&hdr->status, 1);
}

// sorted slot j: head iff its key differs from the one before; heads per workgroup -> totals; the point of slot j -> sorted_pts[j]
__global__ __launch_bounds__(kSsBlock) void vx_head_kernel(const float* __restrict__ pts, long long n, const long long* __restrict__ sorted_keys,
                                                           const long long* __restrict__ sorted_index, float* __restrict__ sorted_pts,
                                                           int* __restrict__ totals) {
  __shared__ int lds[kSsBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kSsBlock + threadIdx.x) * kSsPerThread;
  int v = 0;
  for (int e = 0; e < kSsPerThread; ++e) {
    const long long j = first + e;
    if (j >= n) break;
    v += (j == 0 || sorted_keys[j] != sorted_keys[j - 1]) ? 1 : 0;
    const long long i = sorted_index[j];
    const bool inside = i >= 0 && i < n;      // always, for the indices of a sort of n keys
#pragma unroll
    for (int a = 0; a < 3; ++a) sorted_pts[j * 3 + a] = inside ? pts[i * 3 + a] : 0.0f;
  }
  int total;
  block_exclusive_scan<kSsBlock>(v, lds, total);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// One workgroup: totals[b] <- the sum of the totals before b; counts = {M, status}
__global__ __launch_bounds__(kSsScanThreads) void vx_scan_blocks_kernel(int* __restrict__ totals, int nblocks, const VxHeader* __restrict__ hdr,
                                                                        long long* __restrict__ counts) {
  __shared__ int s[kSsScanThreads];
  const int heads = scan_totals<kSsScanThreads>(totals, nblocks, s);
  if (threadIdx.x == 0) {
    counts[0] = heads;
    counts[1] = hdr->status;
  }
}

// starts[m] <- the sorted slot at which run m begins
__global__ __launch_bounds__(kSsBlock) void vx_start_kernel(long long n, const long long* __restrict__ sorted_keys, const int* __restrict__ offsets,
                                                            int* __restrict__ starts) {
  __shared__ int lds[kSsBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kSsBlock + threadIdx.x) * kSsPerThread;
  bool head[kSsPerThread];
  int v = 0;
#pragma unroll
  for (int e = 0; e < kSsPerThread; ++e) {
    const long long j = first + e;
    head[e] = j < n && (j == 0 || sorted_keys[j] != sorted_keys[j - 1]);
    v += head[e] ? 1 : 0;
  }
  int total;
  int rank = offsets[blockIdx.x] + block_exclusive_scan<kSsBlock>(v, lds, total);
#pragma unroll
  for (int e = 0; e < kSsPerThread; ++e) {
    if (head[e]) {
      if (rank >= 0 && rank < n) starts[rank] = static_cast<int>(first + e);      // rank < M <= n
      ++rank;
    }
  }
}

__global__ __launch_bounds__(kSsBlock) void vx_mean_kernel(const float* __restrict__ sorted_pts, long long n, const int* __restrict__ starts,
                                                           long long M, float* __restrict__ out, int* __restrict__ count_out) {
  const long long m = static_cast<long long>(blockIdx.x) * kSsBlock + threadIdx.x;
  if (m >= M) return;
  long long begin = starts[m], end = m + 1 < M ? starts[m + 1] : n;
  begin = begin < 0 ? 0 : begin;
  end = end > n ? n : end;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (long long j = begin; j < end; ++j) {
    sx += static_cast<double>(sorted_pts[j * 3]);
    sy += static_cast<double>(sorted_pts[j * 3 + 1]);
    sz += static_cast<double>(sorted_pts[j * 3 + 2]);
  }
  const double cnt = static_cast<double>(end - begin);
  out[m * 3] = static_cast<float>(sx / cnt);
  out[m * 3 + 1] = static_cast<float>(sy / cnt);
  out[m * 3 + 2] = static_cast<float>(sz / cnt);
  if (count_out) count_out[m] = static_cast<int>(end - begin);
}

int vx_min_groups(long long n) {
  const long long g = (n + kSsBlock - 1) / kSsBlock;
  return static_cast<int>(g < kVxMinGroups ? g : kVxMinGroups);
}

// voxel workspace: header | min partials [256, 3] | block totals [blocks of N] int | starts [N] int | sorted points [N, 3] fp32
struct VxLayout {
  size_t partials_off, totals_off, starts_off, sorted_off, total;
};

VxLayout vx_layout(long long n) {
  VxLayout l;
  l.partials_off = ss_align(sizeof(VxHeader));
  l.totals_off = l.partials_off + ss_align(kVxMinGroups * 3 * sizeof(float));
  l.starts_off = l.totals_off + ss_align(static_cast<size_t>(ss_blocks(n)) * sizeof(int));
  l.sorted_off = l.starts_off + ss_align(static_cast<size_t>(n) * sizeof(int));
  l.total = l.sorted_off + ss_align(static_cast<size_t>(n) * 3 * sizeof(float));
  return l;
}

bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

}  // namespace

}  // namespace dvmvs

extern "C" size_t dvmvs_surface_sample_workspace_bytes(long long F) {
  if (F <= 0 || F > dvmvs::kSsMaxFaces) return 0;
  return dvmvs::ss_layout(F).total;
}

extern "C" int dvmvs_surface_sample_count(const float* verts, long long V, const int* faces, long long F, double density, void* workspace,
                                          size_t workspace_bytes, long long* counts, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!faces || !workspace || !counts || V < 0 || F < 1 || (V > 0 && !verts) || !(density > 0.0) || density == __builtin_inf()) return DVMVS_EINVAL;
  if (misaligned(verts, 4) || misaligned(faces, 4) || misaligned(workspace, 8) || misaligned(counts, 8)) return DVMVS_EINVAL;
  if (F > kSsMaxFaces || V > 0x7fffffffLL) return DVMVS_EUNSUPPORTED;
  const SsLayout l = ss_layout(F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  long long* totals = reinterpret_cast<long long*>(ws);
  long long* high = reinterpret_cast<long long*>(ws + l.high_off);
  long long* cum = reinterpret_cast<long long*>(ws + l.cum_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int blocks = ss_blocks(F);
  hipLaunchKernelGGL(ss_area_kernel, dim3(blocks), dim3(kSsBlock), 0, s, verts, V, faces, F, cum, totals, high);
  hipLaunchKernelGGL(ss_scan_blocks_kernel, dim3(1), dim3(kSsScanThreads), 0, s, totals, high, blocks, ss_spacing(density), counts);
  hipLaunchKernelGGL(ss_scan_apply_kernel, dim3(blocks), dim3(kSsBlock), 0, s, cum, F, totals);
  return launch_status();
}

extern "C" int dvmvs_surface_sample_emit(const float* verts, long long V, const int* faces, long long F, double density, unsigned int seed,
                                         const void* workspace, long long N, float* points, int* face, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!faces || !workspace || V < 0 || F < 1 || N < 0 || (V > 0 && !verts) || !(density > 0.0) || density == __builtin_inf()) return DVMVS_EINVAL;
  if (N > 0 && !points) return DVMVS_EINVAL;
  if (misaligned(verts, 4) || misaligned(faces, 4) || misaligned(workspace, 8) || misaligned(points, 4) || misaligned(face, 4)) return DVMVS_EINVAL;
  if (F > kSsMaxFaces || V > 0x7fffffffLL || N > kSsMaxPoints) return DVMVS_EUNSUPPORTED;
  if (N == 0) return 0;
  const long long D = ss_spacing(density);
  if (D > (0x7fffffffffffffffLL - (D >> 1)) / N) return DVMVS_EINVAL;          // t_k must fit: N does not belong to this density
  const long long* cum = reinterpret_cast<const long long*>(static_cast<const char*>(workspace) + ss_layout(F).cum_off);
  hipLaunchKernelGGL(ss_emit_kernel, dim3(static_cast<unsigned int>((N + kSsBlock - 1) / kSsBlock)), dim3(kSsBlock), 0,
                     static_cast<hipStream_t>(stream), verts, V, faces, F, cum, D, lowbias32(seed), lowbias32(seed + 1u), N, points, face);
  return launch_status();
}

extern "C" size_t dvmvs_voxel_downsample_workspace_bytes(long long N) {
  if (N <= 0 || N > dvmvs::kSsMaxPoints) return 0;
  return dvmvs::vx_layout(N).total;
}

extern "C" int dvmvs_voxel_keys(const float* points, long long N, float inv_voxel, void* workspace, size_t workspace_bytes, long long* keys,
                                dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!points || !workspace || !keys || N < 1 || !(inv_voxel > 0.0f) || inv_voxel == __builtin_inff()) return DVMVS_EINVAL;
  if (misaligned(points, 4) || misaligned(workspace, 16) || misaligned(keys, 8)) return DVMVS_EINVAL;
  if (N > kSsMaxPoints) return DVMVS_EUNSUPPORTED;
  const VxLayout l = vx_layout(N);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  VxHeader* hdr = reinterpret_cast<VxHeader*>(ws);
  float* partials = reinterpret_cast<float*>(ws + l.partials_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int groups = vx_min_groups(N);
  hipLaunchKernelGGL(vx_min_kernel, dim3(groups), dim3(kSsBlock), 0, s, points, N, partials);
  hipLaunchKernelGGL(vx_min_final_kernel, dim3(1), dim3(kWave), 0, s, partials, groups, hdr);
  hipLaunchKernelGGL(vx_key_kernel, dim3(static_cast<unsigned int>((N + kSsBlock - 1) / kSsBlock)), dim3(kSsBlock), 0, s, points, N, inv_voxel, hdr,
                     keys);
  return launch_status();
}

extern "C" int dvmvs_voxel_downsample_count(const float* points, long long N, const long long* sorted_keys, const long long* sorted_index,
                                            void* workspace, size_t workspace_bytes, long long* counts, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!points || !sorted_keys || !sorted_index || !workspace || !counts || N < 1) return DVMVS_EINVAL;
  if (misaligned(points, 4) || misaligned(sorted_keys, 8) || misaligned(sorted_index, 8) || misaligned(workspace, 16) || misaligned(counts, 8))
    return DVMVS_EINVAL;
  if (N > kSsMaxPoints) return DVMVS_EUNSUPPORTED;
  const VxLayout l = vx_layout(N);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  int* totals = reinterpret_cast<int*>(ws + l.totals_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int blocks = ss_blocks(N);
  hipLaunchKernelGGL(vx_head_kernel, dim3(blocks), dim3(kSsBlock), 0, s, points, N, sorted_keys, sorted_index,
                     reinterpret_cast<float*>(ws + l.sorted_off), totals);
  hipLaunchKernelGGL(vx_scan_blocks_kernel, dim3(1), dim3(kSsScanThreads), 0, s, totals, blocks, reinterpret_cast<const VxHeader*>(ws), counts);
  hipLaunchKernelGGL(vx_start_kernel, dim3(blocks), dim3(kSsBlock), 0, s, N, sorted_keys, totals, reinterpret_cast<int*>(ws + l.starts_off));
  return launch_status();
}

extern "C" int dvmvs_voxel_downsample_emit(long long N, long long M, const void* workspace, float* out, int* count, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!workspace || !out || N < 1 || M < 1 || M > N) return DVMVS_EINVAL;
  if (misaligned(workspace, 16) || misaligned(out, 4) || misaligned(count, 4)) return DVMVS_EINVAL;
  if (N > kSsMaxPoints) return DVMVS_EUNSUPPORTED;
  const VxLayout l = vx_layout(N);
  const char* ws = static_cast<const char*>(workspace);
  hipLaunchKernelGGL(vx_mean_kernel, dim3(static_cast<unsigned int>((M + kSsBlock - 1) / kSsBlock)), dim3(kSsBlock), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const float*>(ws + l.sorted_off), N,
                     reinterpret_cast<const int*>(ws + l.starts_off), M, out, count);
  return launch_status();
}

extern "C" int dvmvs_voxel_downsample_runs(long long N, const void* workspace, const int** starts, const float** sorted_points) {
  using namespace dvmvs;
  if (!workspace || !starts || !sorted_points || N < 1) return DVMVS_EINVAL;
  if (misaligned(workspace, 16)) return DVMVS_EINVAL;
  if (N > kSsMaxPoints) return DVMVS_EUNSUPPORTED;
  const VxLayout l = vx_layout(N);
  const char* ws = static_cast<const char*>(workspace);
  *starts = reinterpret_cast<const int*>(ws + l.starts_off);
  *sorted_points = reinterpret_cast<const float*>(ws + l.sorted_off);
  return 0;
}
