// Smoothing a triangle mesh (umbrella Laplacian and Taubin's lambda / mu filter) and area-weighted vertex normals (gfx950).  It
// reproduces its host definition bit for bit (dvmvs/smooth.py::smooth_mesh, vertex_normals; include/dvmvs_hip.h).
//   dvmvs_mesh_smooth_keys        : per counting face its six directed pair keys (a << 32) | b and its three corner keys; sentinels that
//                                   sort last for a face that does not count
//   dvmvs_mesh_smooth_rows        : from the sorted pair keys the rows N(v) (offsets, neighbours) and the boundary flags, in the workspace
//   dvmvs_mesh_smooth_rows_export : the rows as arrays of the caller's (tests and tools; the smoothing itself never needs them)
//   dvmvs_mesh_smooth_steps       : ALL steps of a call, one launch per step, ping-pong between two workspace buffers, the last into
//                                   the output
//   dvmvs_mesh_smooth_normals     : the vertex normals of positions, from the stably sorted corner keys
//
// Arithmetic contract: fp64 from the fp32 inputs with +, -, *, / and sqrt only, every operation correctly rounded, nothing contracted into
// an FMA (contract(off) for the whole file).  No float atomics and no float value crosses threads: one lane owns a vertex and walks its
// row (ascending neighbour: the order of the sorted keys) or its incidences (ascending 3 f + j: the order of the stable sort) serially,
// in the order of the definition, so the result does not depend on the schedule.  A vertex with a long row (the hub of a fan) is
// therefore one long serial walk by its one lane; there is no second path for it.
//
// The step kernel, lap_step_kernel, is the hot path.  One vertex per lane: a marching-cubes row holds about six neighbours, too few to
// share among lanes.  Between steps the positions live in the workspace as 16-byte float4, so that a neighbour is one load and not
// three dwords (hipcc makes it a global_load_dwordx3 at a 16-byte aligned address: the fourth word is never used); the last step writes
// the caller's packed [V,3].  kPadded = false keeps the iterate packed, for the comparison of tools/mesh_smooth_bench.py, which the
// packed form won by 12 % of a step on the scene it measures.  The loads of kLapBatch neighbours are issued together before their sums run: indices are
// clamped into their arrays, so no branch stands around a load, and a lane past its row's end adds nothing.  One launch per step: the
// stream orders them, and there is no barrier across workgroups, no cooperative launch and no spin-wait anywhere.
//
// Everything else is integers.  Flags are plain stores of one value (boundary[a] = 1 from any number of threads); counts come from
// block_exclusive_scan and scan_totals of dvmvs_device.h.  No index read from memory becomes an address before it is checked against its
// array's size (or clamped into it), so a sort order that is no permutation (never, from a sort) or a face index outside [0, V) gives
// wrong values at worst and no access out of bounds.
//
// Launches.  keys: lap_keys_kernel.  rows: lap_clear_kernel -> lap_head_count_kernel (run heads per 1024 sorted keys; a run of length 1
// sets the flag of its a) -> lap_scan_kernel (the totals scan; E) -> lap_emit_kernel (rank of every slot = heads before it; neighbours)
// -> lap_offsets_kernel (offsets[v] = rank of the first slot whose key is >= v << 32, by binary search).  steps: lap_pack_kernel ->
// lap_step_kernel per step (lap_copy_kernel for no step).  normals: lap_run_start_kernel -> lap_normals_kernel.
#include "dvmvs_device.h"

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

constexpr int kLapBlock = 256;
constexpr int kLapPerThread = 4;
constexpr int kLapChunk = kLapBlock * kLapPerThread;      // sorted keys per workgroup of a count or a scan
constexpr int kLapScanThreads = 1024;
constexpr long long kLapMaxElements = 1LL << 28;          // V and F
constexpr int kLapMaxIterations = 1024;
constexpr int kLapBatch = 8;                              // neighbours whose loads a vertex's lane keeps in flight
constexpr int kLapFaceBatch = 4;                          // incidences likewise
constexpr int kLapNone = 0x7fffffff;                      // the corner key of a face that does not count: sorts behind every vertex
constexpr long long kLapNonePair = 0x7fffffffffffffffLL;  // its pair keys

// i clamped into [0, last]
__device__ inline long long lap_clamp(long long i, long long last) { return i < 0 ? 0 : i > last ? last : i; }

__device__ inline bool lap_counts(int a, int b, int c, long long V) {
  return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V && a != b && b != c && a != c;
}

__device__ inline long long lap_pair(int a, int b) { return (static_cast<long long>(a) << 32) | static_cast<long long>(b); }

__global__ __launch_bounds__(kLapBlock) void lap_keys_kernel(const int* __restrict__ faces, long long F, long long V,
                                                             long long* __restrict__ pair_keys, int* __restrict__ corner_keys) {
  const long long f = static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x;
  if (f >= F) return;
  const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  const bool counts = lap_counts(a, b, c, V);
  if (pair_keys) {
    pair_keys[f * 6] = counts ? lap_pair(a, b) : kLapNonePair;
    pair_keys[f * 6 + 1] = counts ? lap_pair(b, a) : kLapNonePair;
    pair_keys[f * 6 + 2] = counts ? lap_pair(b, c) : kLapNonePair;
    pair_keys[f * 6 + 3] = counts ? lap_pair(c, b) : kLapNonePair;
    pair_keys[f * 6 + 4] = counts ? lap_pair(c, a) : kLapNonePair;
    pair_keys[f * 6 + 5] = counts ? lap_pair(a, c) : kLapNonePair;
  }
  if (corner_keys) {
    corner_keys[f * 3] = counts ? a : kLapNone;
    corner_keys[f * 3 + 1] = counts ? b : kLapNone;
    corner_keys[f * 3 + 2] = counts ? c : kLapNone;
  }
}

__global__ __launch_bounds__(kLapBlock) void lap_clear_kernel(int* __restrict__ boundary, long long V) {
  const long long v = static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x;
  if (v < V) boundary[v] = 0;
}

// slot s begins a run of equal keys of a counting face
__device__ inline bool lap_head(const long long* __restrict__ sorted, long long s, long long key) {
  return key != kLapNonePair && (s == 0 || sorted[s - 1] != key);
}

__global__ __launch_bounds__(kLapBlock) void lap_head_count_kernel(const long long* __restrict__ sorted, long long n, long long V,
                                                                   int* __restrict__ totals, int* __restrict__ boundary) {
  __shared__ int lds[kLapBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x) * kLapPerThread;
  int heads = 0;
  for (int e = 0; e < kLapPerThread; ++e) {
    const long long s = first + e;
    if (s >= n) break;
    const long long key = sorted[s];
    if (!lap_head(sorted, s, key)) continue;
    ++heads;
    if (s + 1 == n || sorted[s + 1] != key) {              // a run of length 1: the pair was emitted once
      const long long a = key >> 32;
      if (a >= 0 && a < V) boundary[a] = 1;
    }
  }
  int total;
  block_exclusive_scan<kLapBlock>(heads, lds, total);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(kLapScanThreads) void lap_scan_kernel(int* __restrict__ totals, int nblocks, int* __restrict__ count) {
  __shared__ int s[kLapScanThreads];
  const int all = scan_totals<kLapScanThreads>(totals, nblocks, s);
  if (threadIdx.x == 0) count[0] = all;
}

__global__ __launch_bounds__(kLapBlock) void lap_emit_kernel(const long long* __restrict__ sorted, long long n, const int* __restrict__ totals,
                                                             int* __restrict__ rank, int* __restrict__ neighbours) {
  __shared__ int lds[kLapBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x) * kLapPerThread;
  bool head[kLapPerThread];
  long long key[kLapPerThread];
  int heads = 0;
#pragma unroll
  for (int e = 0; e < kLapPerThread; ++e) {
    const long long s = first + e;
    key[e] = s < n ? sorted[s] : kLapNonePair;
    head[e] = s < n && lap_head(sorted, s, key[e]);
    heads += head[e] ? 1 : 0;
  }
  int total;
  long long slot = totals[blockIdx.x] + block_exclusive_scan<kLapBlock>(heads, lds, total);
#pragma unroll
  for (int e = 0; e < kLapPerThread; ++e) {
    const long long s = first + e;
    if (s >= n) break;
    rank[s] = static_cast<int>(slot);                    // heads before s: at most 6 * 2^28 < 2^31
    if (!head[e]) continue;
    if (slot >= 0 && slot < n) neighbours[slot] = static_cast<int>(key[e] & 0xffffffffLL);
    ++slot;
  }
}

// offsets[v] = the number of heads whose a is below v, for v = 0 .. V
__global__ __launch_bounds__(kLapBlock) void lap_offsets_kernel(const long long* __restrict__ sorted, long long n, const int* __restrict__ rank,
                                                                const int* __restrict__ count, long long V, int* __restrict__ offsets) {
  const long long v = static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x;
  if (v > V) return;
  const long long target = v << 32;
  long long lo = 0, hi = n;                              // the first slot whose key is >= target (a sentinel is)
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] >= target) hi = mid; else lo = mid + 1;
  }
  offsets[v] = lo < n ? rank[lo] : count[0];
}

__global__ __launch_bounds__(kLapBlock) void lap_export_kernel(const int* __restrict__ offsets, const int* __restrict__ neighbours,
                                                               const int* __restrict__ boundary, long long V, long long n,
                                                               long long* __restrict__ offsets_out, int* __restrict__ neighbours_out,
                                                               unsigned char* __restrict__ boundary_out) {
  const long long i = static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x;
  if (i <= V) offsets_out[i] = offsets[i];
  if (i < V) boundary_out[i] = boundary[i] != 0;
  if (i < n) {
    const long long E = lap_clamp(offsets[V], n);
    neighbours_out[i] = i < E ? neighbours[i] : -1;
  }
}

__global__ __launch_bounds__(kLapBlock) void lap_pack_kernel(const float* __restrict__ verts, long long V, float4* __restrict__ dst) {
  const long long v = static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x;
  if (v >= V) return;
  dst[v] = make_float4(verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2], 0.0f);
}

__global__ __launch_bounds__(kLapBlock) void lap_copy_kernel(const float* __restrict__ src, long long n, float* __restrict__ dst) {
  const long long i = static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

template <bool kPadded>
__device__ inline void lap_load(const float* __restrict__ src, long long v, float& x, float& y, float& z) {
  if (kPadded) {
    const float4 p = reinterpret_cast<const float4*>(src)[v];
    x = p.x, y = p.y, z = p.z;
  } else {
    x = src[v * 3], y = src[v * 3 + 1], z = src[v * 3 + 2];
  }
}

template <bool kPadded>
__device__ inline void lap_store(float* __restrict__ dst, long long v, float x, float y, float z) {
  if (kPadded) {
    reinterpret_cast<float4*>(dst)[v] = make_float4(x, y, z, 0.0f);
  } else {
    dst[v * 3] = x, dst[v * 3 + 1] = y, dst[v * 3 + 2] = z;
  }
}

// One step with factor s: one vertex per lane; src and dst are different buffers.  `bound` is the size of `neighbours`.
template <bool kSrcPadded, bool kDstPadded>
__global__ __launch_bounds__(kLapBlock) void lap_step_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ offsets,
                                                             const int* __restrict__ neighbours, const int* __restrict__ boundary, long long V,
                                                             long long bound, double s, int fixed) {
  const long long v = static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x;
  if (v >= V) return;
  float x, y, z;
  lap_load<kSrcPadded>(src, v, x, y, z);
  const long long begin = lap_clamp(offsets[v], bound), end = lap_clamp(offsets[v + 1], bound);
  if (end <= begin || (fixed && boundary[v] != 0)) {
    lap_store<kDstPadded>(dst, v, x, y, z);                // the bits are copied
    return;
  }
  const long long last_slot = bound - 1, last_vertex = V - 1;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (long long j = begin; j < end; j += kLapBatch) {
    long long u[kLapBatch];
    float px[kLapBatch], py[kLapBatch], pz[kLapBatch];
#pragma unroll
    for (int k = 0; k < kLapBatch; ++k) u[k] = lap_clamp(neighbours[lap_clamp(j + k, last_slot)], last_vertex);
#pragma unroll
    for (int k = 0; k < kLapBatch; ++k) lap_load<kSrcPadded>(src, u[k], px[k], py[k], pz[k]);
#pragma unroll
    for (int k = 0; k < kLapBatch; ++k) {
      const bool live = j + k < end;
      const double tx = sx + static_cast<double>(px[k]), ty = sy + static_cast<double>(py[k]), tz = sz + static_cast<double>(pz[k]);
      sx = live ? tx : sx;
      sy = live ? ty : sy;
      sz = live ? tz : sz;
    }
  }
  const double n = static_cast<double>(end - begin);
  const double xv = static_cast<double>(x), yv = static_cast<double>(y), zv = static_cast<double>(z);
  const double mx = sx / n, my = sy / n, mz = sz / n;
  lap_store<kDstPadded>(dst, v, static_cast<float>(xv + s * (mx - xv)), static_cast<float>(yv + s * (my - yv)),
                        static_cast<float>(zv + s * (mz - zv)));
}

// start[v] = the first slot s with sorted[s] >= v, for v = 0 .. V
__global__ __launch_bounds__(kLapBlock) void lap_run_start_kernel(const int* __restrict__ sorted, long long n, long long V, int* __restrict__ start) {
  const long long v = static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x;
  if (v > V) return;
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] >= v) hi = mid; else lo = mid + 1;
  }
  start[v] = static_cast<int>(lo);                      // n <= 3 * 2^28 < 2^31
}

// e1 x e2 of the face with the corners p[0..2], p[3..5], p[6..8], added to the three sums when `live`
__device__ inline void lap_add_face(const float (&p)[9], bool live, double& sx, double& sy, double& sz) {
  const double p0x = static_cast<double>(p[0]), p0y = static_cast<double>(p[1]), p0z = static_cast<double>(p[2]);
  const double e1x = static_cast<double>(p[3]) - p0x, e1y = static_cast<double>(p[4]) - p0y, e1z = static_cast<double>(p[5]) - p0z;
  const double e2x = static_cast<double>(p[6]) - p0x, e2y = static_cast<double>(p[7]) - p0y, e2z = static_cast<double>(p[8]) - p0z;
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const double tx = sx + nx, ty = sy + ny, tz = sz + nz;
  sx = live ? tx : sx;
  sy = live ? ty : sy;
  sz = live ? tz : sz;
}

// One thread per vertex: step 5 of the definition
__global__ __launch_bounds__(kLapBlock) void lap_normals_kernel(const float* __restrict__ verts, long long V, const int* __restrict__ faces, long long F,
                                                                const int* __restrict__ start, const long long* __restrict__ order,
                                                                const float* __restrict__ fallback, float* __restrict__ normals) {
  const long long v = static_cast<long long>(blockIdx.x) * kLapBlock + threadIdx.x;
  if (v >= V) return;
  const long long n_inc = 3 * F;
  const long long begin = lap_clamp(start[v], n_inc), end = lap_clamp(start[v + 1], n_inc);
  const long long last_incidence = n_inc - 1, last_vertex = V - 1;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (long long s = begin; s < end; s += kLapFaceBatch) {       // (never entered when F = 0)
    long long f[kLapFaceBatch], corner[kLapFaceBatch][3];
    float p[kLapFaceBatch][9];
#pragma unroll
    for (int k = 0; k < kLapFaceBatch; ++k) f[k] = lap_clamp(order[lap_clamp(s + k, last_incidence)], last_incidence) / 3;
#pragma unroll
    for (int k = 0; k < kLapFaceBatch; ++k) {
#pragma unroll
      for (int j = 0; j < 3; ++j) corner[k][j] = lap_clamp(faces[f[k] * 3 + j], last_vertex);
    }
#pragma unroll
    for (int k = 0; k < kLapFaceBatch; ++k) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int d = 0; d < 3; ++d) p[k][j * 3 + d] = verts[corner[k][j] * 3 + d];
      }
    }
#pragma unroll
    for (int k = 0; k < kLapFaceBatch; ++k) lap_add_face(p[k], s + k < end, sx, sy, sz);
  }
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  const bool ok = len > 0.0 && len < __builtin_inf();
  const float fx = fallback ? fallback[v * 3] : 0.0f, fy = fallback ? fallback[v * 3 + 1] : 0.0f, fz = fallback ? fallback[v * 3 + 2] : 0.0f;
  normals[v * 3] = ok ? static_cast<float>(sx / len) : fx;
  normals[v * 3 + 1] = ok ? static_cast<float>(sy / len) : fy;
  normals[v * 3 + 2] = ok ? static_cast<float>(sz / len) : fz;
}

size_t lap_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

int lap_blocks(long long n) { return static_cast<int>((n + kLapChunk - 1) / kLapChunk); }      // <= 6 * 2^18

unsigned int lap_grid(long long n) { return static_cast<unsigned int>((n + kLapBlock - 1) / kLapBlock); }

// workspace: boundary [V] int | offsets [V + 1] int | inc_start [V + 1] int | count [4] int | totals [blocks of 6 F] int | rank [6 F] int |
// neighbours [6 F] int | positions A [V] float4 | positions B [V] float4
struct LapLayout {
  size_t offsets_off, start_off, count_off, totals_off, rank_off, neighbours_off, a_off, b_off, total;
};

LapLayout lap_layout(long long V, long long F) {
  LapLayout l;
  const size_t v = static_cast<size_t>(V), n = static_cast<size_t>(F) * 6;
  l.offsets_off = lap_align(v * sizeof(int));
  l.start_off = l.offsets_off + lap_align((v + 1) * sizeof(int));
  l.count_off = l.start_off + lap_align((v + 1) * sizeof(int));
  l.totals_off = l.count_off + lap_align(4 * sizeof(int));
  l.rank_off = l.totals_off + lap_align(static_cast<size_t>(lap_blocks(6 * F)) * sizeof(int));
  l.neighbours_off = l.rank_off + lap_align(n * sizeof(int));
  l.a_off = l.neighbours_off + lap_align(n * sizeof(int));
  l.b_off = l.a_off + lap_align(v * 4 * sizeof(float));
  l.total = l.b_off + lap_align(v * 4 * sizeof(float));
  return l;
}

bool lap_misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

bool lap_out_of_range(long long V, long long F) { return V > kLapMaxElements || F > kLapMaxElements; }

}  // namespace

}  // namespace dvmvs

extern "C" size_t dvmvs_mesh_smooth_workspace_bytes(long long V, long long F) {
  if (V < 0 || F < 0 || dvmvs::lap_out_of_range(V, F)) return 0;
  return dvmvs::lap_layout(V, F).total;
}

extern "C" int dvmvs_mesh_smooth_keys(const int* faces, long long V, long long F, long long* pair_keys, int* corner_keys, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (V < 0 || F < 0 || (F > 0 && (!faces || (!pair_keys && !corner_keys)))) return DVMVS_EINVAL;
  if (lap_misaligned(faces, 4) || lap_misaligned(pair_keys, 8) || lap_misaligned(corner_keys, 4)) return DVMVS_EINVAL;
  if (lap_out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  if (F == 0) return 0;
  hipLaunchKernelGGL(lap_keys_kernel, dim3(lap_grid(F)), dim3(kLapBlock), 0, static_cast<hipStream_t>(stream), faces, F, V, pair_keys, corner_keys);
  return launch_status();
}

extern "C" int dvmvs_mesh_smooth_rows(const long long* pair_sorted, long long V, long long F, void* workspace, size_t workspace_bytes,
                                      dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!workspace || V < 1 || F < 0 || (F > 0 && !pair_sorted)) return DVMVS_EINVAL;
  if (lap_misaligned(pair_sorted, 8) || lap_misaligned(workspace, 16)) return DVMVS_EINVAL;
  if (lap_out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  const LapLayout l = lap_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  int* boundary = reinterpret_cast<int*>(ws);
  int* offsets = reinterpret_cast<int*>(ws + l.offsets_off);
  int* count = reinterpret_cast<int*>(ws + l.count_off);
  int* totals = reinterpret_cast<int*>(ws + l.totals_off);
  int* rank = reinterpret_cast<int*>(ws + l.rank_off);
  int* neighbours = reinterpret_cast<int*>(ws + l.neighbours_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const long long n = 6 * F;
  const int nblocks = lap_blocks(n);
  hipLaunchKernelGGL(lap_clear_kernel, dim3(lap_grid(V)), dim3(kLapBlock), 0, s, boundary, V);
  if (nblocks > 0) hipLaunchKernelGGL(lap_head_count_kernel, dim3(nblocks), dim3(kLapBlock), 0, s, pair_sorted, n, V, totals, boundary);
  hipLaunchKernelGGL(lap_scan_kernel, dim3(1), dim3(kLapScanThreads), 0, s, totals, nblocks, count);
  if (nblocks > 0) hipLaunchKernelGGL(lap_emit_kernel, dim3(nblocks), dim3(kLapBlock), 0, s, pair_sorted, n, totals, rank, neighbours);
  // (one more thread than vertices: offsets has V + 1 entries; pair_sorted and rank are not read when n = 0)
  hipLaunchKernelGGL(lap_offsets_kernel, dim3(lap_grid(V + 1)), dim3(kLapBlock), 0, s, pair_sorted, n, rank, count, V, offsets);
  return launch_status();
}

extern "C" int dvmvs_mesh_smooth_rows_export(long long V, long long F, const void* workspace, size_t workspace_bytes, long long* offsets,
                                             int* neighbours, unsigned char* boundary, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!workspace || !offsets || !boundary || V < 1 || F < 0 || (F > 0 && !neighbours)) return DVMVS_EINVAL;
  if (lap_misaligned(workspace, 16) || lap_misaligned(offsets, 8) || lap_misaligned(neighbours, 4)) return DVMVS_EINVAL;
  if (lap_out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  const LapLayout l = lap_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  const char* ws = static_cast<const char*>(workspace);
  const long long n = 6 * F, threads = n > V + 1 ? n : V + 1;
  hipLaunchKernelGGL(lap_export_kernel, dim3(lap_grid(threads)), dim3(kLapBlock), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const int*>(ws + l.offsets_off), reinterpret_cast<const int*>(ws + l.neighbours_off),
                     reinterpret_cast<const int*>(ws), V, n, offsets, neighbours, boundary);
  return launch_status();
}

extern "C" int dvmvs_mesh_smooth_steps(const float* verts, long long V, long long F, int iterations, int taubin, double lam, double mu,
                                       int fixed_boundary, int packed, void* workspace, size_t workspace_bytes, float* verts_out,
                                       dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!verts || !workspace || !verts_out || verts == verts_out || V < 1 || F < 0 || iterations < 0) return DVMVS_EINVAL;
  if ((taubin != 0 && taubin != 1) || (fixed_boundary != 0 && fixed_boundary != 1) || (packed != 0 && packed != 1)) return DVMVS_EINVAL;
  if (!(lam > 0.0 && lam <= 1.0) || !(mu > -__builtin_inf() && mu < __builtin_inf()) || (taubin && !(mu >= -1.0 && mu < -lam))) return DVMVS_EINVAL;
  if (lap_misaligned(verts, 4) || lap_misaligned(verts_out, 4) || lap_misaligned(workspace, 16)) return DVMVS_EINVAL;
  if (lap_out_of_range(V, F) || iterations > kLapMaxIterations) return DVMVS_EUNSUPPORTED;
  const LapLayout l = lap_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  const int* boundary = reinterpret_cast<const int*>(ws);
  const int* offsets = reinterpret_cast<const int*>(ws + l.offsets_off);
  const int* neighbours = reinterpret_cast<const int*>(ws + l.neighbours_off);
  float* buffers[2] = {reinterpret_cast<float*>(ws + l.a_off), reinterpret_cast<float*>(ws + l.b_off)};
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(lap_grid(V)), block(kLapBlock);
  const long long bound = 6 * F;
  const int steps = taubin ? 2 * iterations : iterations;
  if (steps == 0) {
    hipLaunchKernelGGL(lap_copy_kernel, dim3(lap_grid(3 * V)), block, 0, s, verts, 3 * V, verts_out);
    return launch_status();
  }
  // packed: the first step reads the caller's verts; padded: they are widened to float4 into A first
  const float* src = verts;
  if (!packed) {
    hipLaunchKernelGGL(lap_pack_kernel, grid, block, 0, s, verts, V, reinterpret_cast<float4*>(buffers[0]));
    src = buffers[0];
  }
  for (int t = 0; t < steps; ++t) {
    const double factor = taubin && (t & 1) ? mu : lam;
    const bool last = t + 1 == steps;
    float* dst = last ? verts_out : buffers[(t + 1) & 1];
    if (packed)
      hipLaunchKernelGGL((lap_step_kernel<false, false>), grid, block, 0, s, src, dst, offsets, neighbours, boundary, V, bound, factor, fixed_boundary);
    else if (last)
      hipLaunchKernelGGL((lap_step_kernel<true, false>), grid, block, 0, s, src, dst, offsets, neighbours, boundary, V, bound, factor, fixed_boundary);
    else
      hipLaunchKernelGGL((lap_step_kernel<true, true>), grid, block, 0, s, src, dst, offsets, neighbours, boundary, V, bound, factor, fixed_boundary);
    src = dst;
  }
  return launch_status();
}

extern "C" int dvmvs_mesh_smooth_normals(const float* verts, long long V, const int* faces, long long F, const int* corner_sorted,
                                         const long long* corner_order, const float* fallback, void* workspace, size_t workspace_bytes,
                                         float* normals, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!verts || !workspace || !normals || normals == verts || V < 1 || F < 0) return DVMVS_EINVAL;
  if (F > 0 && (!faces || !corner_sorted || !corner_order)) return DVMVS_EINVAL;
  if (lap_misaligned(verts, 4) || lap_misaligned(faces, 4) || lap_misaligned(corner_sorted, 4) || lap_misaligned(corner_order, 8) ||
      lap_misaligned(fallback, 4) || lap_misaligned(normals, 4) || lap_misaligned(workspace, 16))
    return DVMVS_EINVAL;
  if (lap_out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  const LapLayout l = lap_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  int* start = reinterpret_cast<int*>(static_cast<char*>(workspace) + l.start_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(lap_run_start_kernel, dim3(lap_grid(V + 1)), dim3(kLapBlock), 0, s, corner_sorted, 3 * F, V, start);
  hipLaunchKernelGGL(lap_normals_kernel, dim3(lap_grid(V)), dim3(kLapBlock), 0, s, verts, V, faces, F, start, corner_order, fallback, normals);
  return launch_status();
}
