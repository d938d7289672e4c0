// Marching cubes on a voxel volume (gfx950): the iso-surface step of the reference's reconstruction script, which calls
// scikit-image's marching_cubes_lewiner on the host (sample-data/run-tsdf-reconstruction.py:313-351).
//
// Output contract (restated on the CPU by tests/marching_cubes_cpu.py and compared array for array):
//   - a corner is inside when value < level; a grid edge carries a vertex when exactly one of its endpoints is inside;
//   - each voxel owns its +x, +y, +z edges; vertices are numbered by (linear index of the owner, axis x < y < z), so the
//     mesh shares its vertices without a hash table and two runs give the same bytes;
//   - cubes are ordered by the linear index of their lowest corner, a cube's triangles by table order
//     (marching_cubes_tables.h, which also defines the corner / edge numbering);
//   - positions, normals and colours in float32 with contraction off (formulas at mc_vertices_kernel).
//
// Four launches, one thread per voxel (z fastest: a wave reads 64 consecutive floats), no atomics: the result does not depend
// on the order workgroups run in.
//   1. mc_count_kernel     per block: owned vertices and triangles of its 256 voxels / cubes -> two int32 totals
//   2. mc_scan_kernel      one workgroup: exclusive scan of the block totals (int64), V and F -> counts_dev
//   3. mc_vertices_kernel  recount, scan inside the block, write the vertices and the owner's first vertex id (int32 per voxel)
//   4. mc_faces_kernel     recount the cubes, scan, emit triangles through the owners' first vertex ids
// The host reads V and F between 2 and 3 to size the outputs; every launch is capture-safe (no allocation, no synchronisation).
#include "dvmvs_device.h"
#include "marching_cubes_tables.h"

namespace dvmvs {

namespace {

constexpr int kMcBlock = 256;
constexpr int kMcScanThreads = 1024;

struct McGeom {
  int X, Y, Z;
  long long plane;   // Y * Z
};

// (wave_inclusive_scan / block_exclusive_scan: dvmvs_device.h, over kMcBlock = 256 threads)

// Bits 0..2: the voxel's +x / +y / +z edge crosses the level.
__device__ inline unsigned owned_mask(const float* __restrict__ vol, const McGeom& g, int i, int j, int k, long long idx, float level) {
  const bool in = vol[idx] < level;
  unsigned m = 0;
  if (i + 1 < g.X && ((vol[idx + g.plane] < level) != in)) m |= 1u;
  if (j + 1 < g.Y && ((vol[idx + g.Z] < level) != in)) m |= 2u;
  if (k + 1 < g.Z && ((vol[idx + 1] < level) != in)) m |= 4u;
  return m;
}

// Case index of the cube whose lowest corner is (i, j, k), or -1 when that voxel has no cube.
__device__ inline int cube_case(const float* __restrict__ vol, const McGeom& g, int i, int j, int k, long long idx, float level) {
  if (i + 1 >= g.X || j + 1 >= g.Y || k + 1 >= g.Z) return -1;
  const long long px = g.plane, py = g.Z;
  int c = 0;
  c |= (vol[idx] < level) << 0;
  c |= (vol[idx + px] < level) << 1;
  c |= (vol[idx + px + py] < level) << 2;
  c |= (vol[idx + py] < level) << 3;
  c |= (vol[idx + 1] < level) << 4;
  c |= (vol[idx + px + 1] < level) << 5;
  c |= (vol[idx + px + py + 1] < level) << 6;
  c |= (vol[idx + py + 1] < level) << 7;
  return c;
}

__device__ inline void voxel_coords(const McGeom& g, long long idx, int& i, int& j, int& k) {
  i = static_cast<int>(idx / g.plane);
  const int rem = static_cast<int>(idx - i * g.plane);
  j = rem / g.Z;
  k = rem - j * g.Z;
}

__global__ __launch_bounds__(kMcBlock) void mc_count_kernel(const float* __restrict__ vol, McGeom g, long long total, float level,
                                                            int* __restrict__ block_counts) {
  __shared__ int lds_v[kMcBlock / 64], lds_f[kMcBlock / 64];
  const long long idx = static_cast<long long>(blockIdx.x) * kMcBlock + threadIdx.x;
  int nv = 0, nt = 0;
  if (idx < total) {
    int i, j, k;
    voxel_coords(g, idx, i, j, k);
    nv = __popc(owned_mask(vol, g, i, j, k, idx, level));
    const int c = cube_case(vol, g, i, j, k, idx, level);
    nt = c >= 0 ? kMcTriCount[c] : 0;
  }
  int tv, tf;
  block_exclusive_scan(nv, lds_v, tv);
  block_exclusive_scan(nt, lds_f, tf);
  if (threadIdx.x == 0) {
    block_counts[2 * blockIdx.x] = tv;
    block_counts[2 * blockIdx.x + 1] = tf;
  }
}

// One workgroup: exclusive prefix sums of the per-block (vertex, triangle) counts; totals -> counts_dev[0..1].
__global__ __launch_bounds__(kMcScanThreads) void mc_scan_kernel(const int* __restrict__ block_counts, int nblocks,
                                                                 long long* __restrict__ block_offsets, long long* __restrict__ counts_dev) {
  __shared__ long long sv[kMcScanThreads], sf[kMcScanThreads];
  const int t = threadIdx.x;
  const int chunk = (nblocks + kMcScanThreads - 1) / kMcScanThreads;
  const int begin = min(t * chunk, nblocks), end = min(begin + chunk, nblocks);
  long long v = 0, f = 0;
  for (int b = begin; b < end; ++b) {
    v += block_counts[2 * b];
    f += block_counts[2 * b + 1];
  }
  sv[t] = v;
  sf[t] = f;
  __syncthreads();
  for (int off = 1; off < kMcScanThreads; off <<= 1) {   // Hillis-Steele inclusive scan
    const long long av = t >= off ? sv[t - off] : 0, af = t >= off ? sf[t - off] : 0;
    __syncthreads();
    sv[t] += av;
    sf[t] += af;
    __syncthreads();
  }
  long long ov = sv[t] - v, of = sf[t] - f;
  for (int b = begin; b < end; ++b) {
    block_offsets[2 * b] = ov;
    block_offsets[2 * b + 1] = of;
    ov += block_counts[2 * b];
    of += block_counts[2 * b + 1];
  }
  if (t == 0) {
    counts_dev[0] = sv[kMcScanThreads - 1];
    counts_dev[1] = sf[kMcScanThreads - 1];
  }
}

#pragma clang fp contract(off)
// np.gradient's rule along `axis` at voxel (c[0], c[1], c[2]) (the extent is >= 2): central inside, one-sided at the borders.
__device__ inline float gradient(const float* __restrict__ vol, const McGeom& g, const int c[3], long long idx, int axis) {
  const int n = axis == 0 ? g.X : (axis == 1 ? g.Y : g.Z);
  const long long s = axis == 0 ? g.plane : (axis == 1 ? static_cast<long long>(g.Z) : 1LL);
  if (c[axis] == 0) return vol[idx + s] - vol[idx];
  if (c[axis] == n - 1) return vol[idx] - vol[idx - s];
  return (vol[idx + s] - vol[idx - s]) * 0.5f;
}

// Vertex on the +axis edge of voxel a = (i, j, k), b = a + e_axis:
//   t = (level - v_a) / (v_b - v_a);  index-space p = float(i) + t on the edge axis, float(j) on the others;
//   position = p * voxel_size + origin;  normal = g_a + t * (g_b - g_a) with np.gradient's g, divided by
//   sqrt(nx*nx + ny*ny + nz*nz) (zero stays zero);  colour = the colour voxel at rint(p), decoded as the reference does.
__global__ __launch_bounds__(kMcBlock) void mc_vertices_kernel(const float* __restrict__ vol, const float* __restrict__ color_vol, McGeom g,
                                                               long long total, float level, float ox, float oy, float oz, float voxel_size,
                                                               const long long* __restrict__ block_offsets, int* __restrict__ vertex_base,
                                                               float* __restrict__ verts, float* __restrict__ normals,
                                                               unsigned char* __restrict__ colors, long long V) {
  __shared__ int lds[kMcBlock / 64];
  const long long idx = static_cast<long long>(blockIdx.x) * kMcBlock + threadIdx.x;
  int c[3] = {0, 0, 0};
  unsigned mask = 0;
  if (idx < total) {
    voxel_coords(g, idx, c[0], c[1], c[2]);
    mask = owned_mask(vol, g, c[0], c[1], c[2], idx, level);
  }
  int tv;
  const int local = block_exclusive_scan(__popc(mask), lds, tv);
  if (mask == 0) return;
  long long vid = block_offsets[2 * blockIdx.x] + local;
  if (vid >= V) return;
  vertex_base[idx] = static_cast<int>(vid);
  const float origin[3] = {ox, oy, oz};
  const float va = vol[idx];
  float ga[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) ga[a] = gradient(vol, g, c, idx, a);
  for (int axis = 0; axis < 3; ++axis, mask >>= 1) {
    if (!(mask & 1u)) continue;
    if (vid >= V) return;
    const long long s = axis == 0 ? g.plane : (axis == 1 ? static_cast<long long>(g.Z) : 1LL);
    const float vb = vol[idx + s];
    const float t = (level - va) / (vb - va);
    int cb[3] = {c[0], c[1], c[2]};
    cb[axis] += 1;
    float p[3], n[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p[a] = static_cast<float>(c[a]);
      const float gb = gradient(vol, g, cb, idx + s, a);
      n[a] = ga[a] + t * (gb - ga[a]);
    }
    p[axis] = p[axis] + t;
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      verts[3 * vid + a] = p[a] * voxel_size + origin[a];
      normals[3 * vid + a] = len == 0.0f ? 0.0f : n[a] / len;
    }
    if (colors) {
      const int dims[3] = {g.X, g.Y, g.Z};
      int q[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) q[a] = min(max(static_cast<int>(rintf(p[a])), 0), dims[a] - 1);
      const float col = color_vol[q[0] * g.plane + static_cast<long long>(q[1]) * g.Z + q[2]];
      const float cb_ = floorf(col / 65536.0f);
      const float cg = floorf((col - cb_ * 65536.0f) / 256.0f);
      const float cr = col - cb_ * 65536.0f - cg * 256.0f;
      colors[3 * vid + 0] = static_cast<unsigned char>(floorf(cr));
      colors[3 * vid + 1] = static_cast<unsigned char>(floorf(cg));
      colors[3 * vid + 2] = static_cast<unsigned char>(floorf(cb_));
    }
    ++vid;
  }
}
#pragma clang fp contract(fast)

// Vertex id of the +axis edge of voxel o: its first vertex id plus the owner's crossing edges of lower axis.
__device__ inline int vertex_id(const float* __restrict__ vol, const int* __restrict__ vertex_base, const McGeom& g, int oi, int oj, int ok,
                                int axis, float level) {
  const long long o = oi * g.plane + static_cast<long long>(oj) * g.Z + ok;
  int id = vertex_base[o];
  if (axis > 0) {
    const bool in = vol[o] < level;
    if (oi + 1 < g.X && ((vol[o + g.plane] < level) != in)) ++id;
    if (axis > 1 && oj + 1 < g.Y && ((vol[o + g.Z] < level) != in)) ++id;
  }
  return id;
}

__global__ __launch_bounds__(kMcBlock) void mc_faces_kernel(const float* __restrict__ vol, McGeom g, long long total, float level,
                                                            const long long* __restrict__ block_offsets, const int* __restrict__ vertex_base,
                                                            int* __restrict__ faces, long long F) {
  __shared__ int lds[kMcBlock / 64];
  const long long idx = static_cast<long long>(blockIdx.x) * kMcBlock + threadIdx.x;
  int i = 0, j = 0, k = 0, c = -1;
  if (idx < total) {
    voxel_coords(g, idx, i, j, k);
    c = cube_case(vol, g, i, j, k, idx, level);
  }
  const int nt = c >= 0 ? kMcTriCount[c] : 0;
  int tf;
  const int local = block_exclusive_scan(nt, lds, tf);
  long long f = block_offsets[2 * blockIdx.x + 1] + local;
  for (int s = 0; s < nt; ++s, ++f) {
    if (f >= F) return;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const int e = kMcTriTable[c][3 * s + v];
      faces[3 * f + v] = vertex_id(vol, vertex_base, g, i + kMcEdgeOwner[e][0], j + kMcEdgeOwner[e][1], k + kMcEdgeOwner[e][2],
                                   kMcEdgeOwner[e][3], level);
    }
  }
}

// Workspace: int32 per voxel (first vertex id of its owner), then int32 [2 * blocks] counts, int64 [2 * blocks] offsets.
struct McLayout {
  size_t base_bytes, counts_off, offsets_off, total;
  long long nblocks;
};

McLayout mc_layout(int X, int Y, int Z) {
  McLayout l;
  const long long n = static_cast<long long>(X) * Y * Z;
  l.nblocks = (n + kMcBlock - 1) / kMcBlock;
  l.base_bytes = (static_cast<size_t>(n) * 4 + 255) / 256 * 256;
  l.counts_off = l.base_bytes;
  l.offsets_off = l.counts_off + (static_cast<size_t>(l.nblocks) * 8 + 255) / 256 * 256;
  l.total = l.offsets_off + static_cast<size_t>(l.nblocks) * 16;
  return l;
}

bool mc_supported(int X, int Y, int Z) { return static_cast<long long>(X) * Y * Z < (1LL << 31); }

}  // namespace

}  // namespace dvmvs

extern "C" size_t dvmvs_marching_cubes_workspace_bytes(int X, int Y, int Z) {
  if (X <= 0 || Y <= 0 || Z <= 0 || !dvmvs::mc_supported(X, Y, Z)) return 0;
  return dvmvs::mc_layout(X, Y, Z).total;
}

extern "C" int dvmvs_marching_cubes_count(const float* vol, int X, int Y, int Z, float level, void* workspace, size_t workspace_bytes,
                                          long long* counts_dev, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!vol || !workspace || !counts_dev || X <= 0 || Y <= 0 || Z <= 0) return DVMVS_EINVAL;
  if (!mc_supported(X, Y, Z)) return DVMVS_EUNSUPPORTED;
  const McLayout l = mc_layout(X, Y, Z);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  int* counts = reinterpret_cast<int*>(ws + l.counts_off);
  long long* offsets = reinterpret_cast<long long*>(ws + l.offsets_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const McGeom g{X, Y, Z, static_cast<long long>(Y) * Z};
  // a volume thinner than 2 voxels on some axis has no cube: no vertex either (the scan over zero blocks writes V = F = 0)
  const bool empty = X < 2 || Y < 2 || Z < 2;
  if (!empty)
    hipLaunchKernelGGL(mc_count_kernel, dim3(static_cast<unsigned>(l.nblocks)), dim3(kMcBlock), 0, s, vol, g,
                       static_cast<long long>(X) * Y * Z, level, counts);
  hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kMcScanThreads), 0, s, counts, empty ? 0 : static_cast<int>(l.nblocks), offsets, counts_dev);
  return launch_status();
}

extern "C" int dvmvs_marching_cubes_emit(const float* vol, const float* color_vol, int X, int Y, int Z, float level, float ox, float oy,
                                         float oz, float voxel_size, void* workspace, float* verts, float* normals, unsigned char* colors,
                                         int* faces, long long V, long long F, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!vol || !workspace || X <= 0 || Y <= 0 || Z <= 0 || V < 0 || F < 0) return DVMVS_EINVAL;
  if (V > 0 && (!verts || !normals || (color_vol && !colors))) return DVMVS_EINVAL;
  if (F > 0 && !faces) return DVMVS_EINVAL;
  if (!mc_supported(X, Y, Z) || V >= (1LL << 31) || F >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  if (X < 2 || Y < 2 || Z < 2 || (V == 0 && F == 0)) return 0;
  const McLayout l = mc_layout(X, Y, Z);
  char* ws = static_cast<char*>(workspace);
  int* base = reinterpret_cast<int*>(ws);
  const long long* offsets = reinterpret_cast<const long long*>(ws + l.offsets_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const McGeom g{X, Y, Z, static_cast<long long>(Y) * Z};
  const long long total = static_cast<long long>(X) * Y * Z;
  const dim3 grid(static_cast<unsigned>(l.nblocks));
  hipLaunchKernelGGL(mc_vertices_kernel, grid, dim3(kMcBlock), 0, s, vol, color_vol, g, total, level, ox, oy, oz, voxel_size, offsets, base,
                     verts, normals, color_vol ? colors : nullptr, V);
  if (F > 0)
    hipLaunchKernelGGL(mc_faces_kernel, grid, dim3(kMcBlock), 0, s, vol, g, total, level, offsets, base, faces, F);
  return launch_status();
}
