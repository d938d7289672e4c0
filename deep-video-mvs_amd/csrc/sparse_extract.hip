// Marching cubes straight from the pool of the sparse TSDF volume (gfx950): the mesh of the unbounded volume whose voxels are the
// allocated bricks' and (tsdf 1, weight 0, colour 0) everywhere else, without the dense copy -- DESIGN.md section 4.8s, contract in
// include/dvmvs_hip.h, brick arithmetic and the handling rule in sparse_extract_grid.h.
//
// The surface contract is that of csrc/marching_cubes.hip at level 0 (inside = value < 0, the voxel at an edge's lower end owns its
// vertex, tables of marching_cubes_tables.h, a cube's triangles in table order, the statements of mc_vertices_kernel for position,
// normal and colour with the global signed voxel index in place of the dense one); the normal's gradient is ALWAYS the central
// difference, because the unbounded volume has no border.
//
// Order (part of the contract: the same pool state gives the same bytes).  Vertices: by (pool slot of the handling brick, place of the
// owner voxel in that brick's 9 x 9 x 9 lattice of local coordinates -1 .. 7, x slowest, axis x < y < z).  Faces: by (pool slot of the
// handling brick, place of the cube's lowest corner in the same lattice, table order).
//
// Launches, one stream, no atomics -- nothing depends on the order workgroups run in:
//   neighbours  one thread per (slot, d): bounded binary search of brick b + d in the sorted keys -> neighbour[slot][27]   (cached by the caller)
//   count       one workgroup per pool slot (max_bricks of them; slots >= n_bricks, read on the device, return at once): the brick's tsdf
//               with a halo of local -2 .. 9 per axis from the up to 27 neighbours into LDS (12^3 floats, missing neighbours read 1), then
//               owned crossing edges and triangles of the voxels the brick handles -> two int32 totals per slot
//   scan        one workgroup: exclusive scan of the slot totals (int64); (n_bricks, dropped bricks, dropped marks, V, F) -> summary
//   -- the one host read: summary, to size the outputs and the workspace (9^3 int32 per ALLOCATED brick) --
//   vertices    stage again, recount, scan inside the workgroup, write vertices and each owner's first vertex id
//   faces       stage again, recount the cubes, scan, emit triangles; a corner's owner is found through the neighbour row and the handling rule
// Every loop is bounded by a constant or by a count fixed before the launch; every pool index comes from a neighbour entry checked
// against [0, n_bricks); every store is guarded by V / F.
#include "dvmvs_device.h"
#include "marching_cubes_tables.h"
#include "sparse_extract_grid.h"

#include <math.h>

namespace dvmvs {

namespace {

constexpr int kSeThreads = 256;
constexpr int kSeRounds = (kExtractCells + kSeThreads - 1) / kSeThreads;     // 3
constexpr int kSeHalo = 12;                                                 // local -2 .. 9
constexpr int kSeHaloCells = kSeHalo * kSeHalo * kSeHalo;                   // 1728 floats = 6912 bytes
constexpr int kSeScanThreads = 1024;
enum { kSeStatBricks = 0, kSeStatDroppedPool = 1, kSeStatDroppedTable = 2 };

struct SeTile {
  float halo[kSeHaloCells];
  int row[kExtractRow];
  unsigned char handled[kExtractRow];     // by class (se_class)
};

__device__ inline float halo_at(const SeTile& t, int lx, int ly, int lz) { return t.halo[((lx + 2) * kSeHalo + (ly + 2)) * kSeHalo + (lz + 2)]; }

// The neighbour row (entries outside [0, n) count as missing), the classes of voxels the brick handles, and the tsdf halo.
__device__ inline void stage_tile(SeTile& t, const float* __restrict__ pool_tsdf, const int* __restrict__ neighbour, long long slot, long long n) {
  const int tid = threadIdx.x;
  if (tid < kExtractRow) {
    const int s = neighbour[slot * kExtractRow + tid];
    t.row[tid] = (s >= 0 && s < n) ? s : -1;
  }
  __syncthreads();
  if (tid < kExtractRow) t.handled[tid] = se_handles_class(t.row, tid);
#pragma unroll
  for (int r = 0; r < (kSeHaloCells + kSeThreads - 1) / kSeThreads; ++r) {
    const int i = r * kSeThreads + tid;
    if (i < kSeHaloCells) {
      const int lx = i / (kSeHalo * kSeHalo) - 2, ly = (i / kSeHalo) % kSeHalo - 2, lz = i % kSeHalo - 2;
      const int dx = se_floor8(lx), dy = se_floor8(ly), dz = se_floor8(lz);
      const int s = t.row[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)];
      float v = 1.0f;
      if (s >= 0) v = pool_tsdf[static_cast<long long>(s) * kBrickVoxels + ((lx - 8 * dx) * 64 + (ly - 8 * dy) * 8 + (lz - 8 * dz))];
      t.halo[i] = v;
    }
  }
  __syncthreads();
}

// Cell `cell` (0 .. 728; beyond: none) of the brick's lattice: its local coordinates, and whether the brick handles it.
__device__ inline bool handled_cell(const SeTile& t, int cell, int& lx, int& ly, int& lz) {
  lx = cell / 81 - 1;
  ly = (cell / 9) % 9 - 1;
  lz = cell % 9 - 1;
  return cell < kExtractCells && t.handled[se_class(lx, ly, lz)] != 0;
}

// Bits 0..2: the voxel's +x / +y / +z edge crosses zero.
__device__ inline unsigned owned_mask(const SeTile& t, int lx, int ly, int lz) {
  const bool in = halo_at(t, lx, ly, lz) < 0.0f;
  unsigned m = 0;
  if ((halo_at(t, lx + 1, ly, lz) < 0.0f) != in) m |= 1u;
  if ((halo_at(t, lx, ly + 1, lz) < 0.0f) != in) m |= 2u;
  if ((halo_at(t, lx, ly, lz + 1) < 0.0f) != in) m |= 4u;
  return m;
}

__device__ inline int cube_case(const SeTile& t, int lx, int ly, int lz) {
  int c = 0;
  c |= (halo_at(t, lx, ly, lz) < 0.0f) << 0;
  c |= (halo_at(t, lx + 1, ly, lz) < 0.0f) << 1;
  c |= (halo_at(t, lx + 1, ly + 1, lz) < 0.0f) << 2;
  c |= (halo_at(t, lx, ly + 1, lz) < 0.0f) << 3;
  c |= (halo_at(t, lx, ly, lz + 1) < 0.0f) << 4;
  c |= (halo_at(t, lx + 1, ly, lz + 1) < 0.0f) << 5;
  c |= (halo_at(t, lx + 1, ly + 1, lz + 1) < 0.0f) << 6;
  c |= (halo_at(t, lx, ly + 1, lz + 1) < 0.0f) << 7;
  return c;
}

__device__ inline long long bricks_on_device(const unsigned long long* status, long long max_bricks) {
  const long long n = static_cast<long long>(status[kSeStatBricks]);
  return n < 0 ? 0 : (n > max_bricks ? max_bricks : n);
}

__global__ __launch_bounds__(kSeThreads) void sparse_neighbours_kernel(const long long* __restrict__ pool_key, const long long* __restrict__ sorted,
                                                                        const long long* __restrict__ sort_index,
                                                                        const unsigned long long* __restrict__ status, long long max_bricks,
                                                                        int* __restrict__ neighbour) {
  const long long idx = static_cast<long long>(blockIdx.x) * kSeThreads + threadIdx.x;
  const long long n = bricks_on_device(status, max_bricks);
  if (idx >= n * kExtractRow) return;
  const long long slot = idx / kExtractRow;
  const int entry = static_cast<int>(idx - slot * kExtractRow);
  int bx, by, bz;
  sg_unpack(pool_key[slot], bx, by, bz);
  neighbour[idx] = se_neighbour(sorted, sort_index, n, bx, by, bz, entry);
}

__global__ __launch_bounds__(kSeThreads) void sparse_extract_count_kernel(const float* __restrict__ pool_tsdf, const int* __restrict__ neighbour,
                                                                           const unsigned long long* __restrict__ status, long long max_bricks,
                                                                           int* __restrict__ counts) {
  __shared__ SeTile tile;
  __shared__ int lds_v[kSeThreads / 64], lds_f[kSeThreads / 64];
  const long long slot = blockIdx.x;
  const long long n = bricks_on_device(status, max_bricks);
  if (slot >= n) return;
  stage_tile(tile, pool_tsdf, neighbour, slot, n);
  int nv = 0, nt = 0;
#pragma unroll
  for (int r = 0; r < kSeRounds; ++r) {
    int lx, ly, lz;
    if (handled_cell(tile, r * kSeThreads + threadIdx.x, lx, ly, lz)) {
      nv += __popc(owned_mask(tile, lx, ly, lz));
      nt += kMcTriCount[cube_case(tile, lx, ly, lz)];
    }
  }
  int tv, tf;
  block_exclusive_scan(nv, lds_v, tv);
  block_exclusive_scan(nt, lds_f, tf);
  if (threadIdx.x == 0) {
    counts[2 * slot] = tv;
    counts[2 * slot + 1] = tf;
  }
}

// One workgroup: exclusive prefix sums of the (vertex, triangle) totals of the slots < n_bricks; thread t takes `chunk` consecutive slots
// (chunk = ceil(max_bricks / threads), fixed by the host).  summary = (n_bricks, dropped bricks, dropped marks, V, F).
__global__ __launch_bounds__(kSeScanThreads) void sparse_extract_scan_kernel(const int* __restrict__ counts,
                                                                             const unsigned long long* __restrict__ status, long long max_bricks,
                                                                             long long chunk, long long* __restrict__ offsets,
                                                                             long long* __restrict__ summary) {
  __shared__ long long sv[kSeScanThreads], sf[kSeScanThreads];
  const int t = threadIdx.x;
  const long long n = bricks_on_device(status, max_bricks);
  const long long begin = min(t * chunk, n), end = min(begin + chunk, n);
  long long v = 0, f = 0;
  for (long long b = begin; b < end; ++b) {
    v += counts[2 * b];
    f += counts[2 * b + 1];
  }
  sv[t] = v;
  sf[t] = f;
  __syncthreads();
  for (int off = 1; off < kSeScanThreads; off <<= 1) {   // Hillis-Steele inclusive scan
    const long long av = t >= off ? sv[t - off] : 0, af = t >= off ? sf[t - off] : 0;
    __syncthreads();
    sv[t] += av;
    sf[t] += af;
    __syncthreads();
  }
  long long ov = sv[t] - v, of = sf[t] - f;
  for (long long b = begin; b < end; ++b) {
    offsets[2 * b] = ov;
    offsets[2 * b + 1] = of;
    ov += counts[2 * b];
    of += counts[2 * b + 1];
  }
  if (t == 0) {
    summary[0] = n;
    summary[1] = static_cast<long long>(status[kSeStatDroppedPool]);
    summary[2] = static_cast<long long>(status[kSeStatDroppedTable]);
    summary[3] = sv[kSeScanThreads - 1];
    summary[4] = sf[kSeScanThreads - 1];
  }
}

#pragma clang fp contract(off)
// The central difference along `axis` at local (lx, ly, lz), each in [-1, 8].
__device__ inline float central(const SeTile& t, int lx, int ly, int lz, int axis) {
  if (axis == 0) return (halo_at(t, lx + 1, ly, lz) - halo_at(t, lx - 1, ly, lz)) * 0.5f;
  if (axis == 1) return (halo_at(t, lx, ly + 1, lz) - halo_at(t, lx, ly - 1, lz)) * 0.5f;
  return (halo_at(t, lx, ly, lz + 1) - halo_at(t, lx, ly, lz - 1)) * 0.5f;
}

// Vertex on the +axis edge of voxel a, b = a + e_axis, the statements of mc_vertices_kernel at level 0 with a's global index:
//   t = (0 - v_a) / (v_b - v_a);  p = float(a) + t on the edge axis, float(a) on the others;  position = p * voxel_size + origin;
//   normal = g_a + t * (g_b - g_a), g the central difference, divided by its length (zero stays zero);
//   colour = the folded colour voxel at rint(p) (0 where no brick is allocated), decoded as there.
__global__ __launch_bounds__(kSeThreads) void sparse_extract_vertices_kernel(const float* __restrict__ pool_tsdf, const float* __restrict__ pool_color,
                                                                              const long long* __restrict__ pool_key,
                                                                              const int* __restrict__ neighbour, long long n,
                                                                              const long long* __restrict__ offsets, float ox, float oy, float oz,
                                                                              float voxel_size, int* __restrict__ vertex_base,
                                                                              float* __restrict__ verts, float* __restrict__ normals,
                                                                              unsigned char* __restrict__ colors, long long V) {
  __shared__ SeTile tile;
  __shared__ int lds[kSeRounds][kSeThreads / 64];
  const long long slot = blockIdx.x;
  if (slot >= n) return;
  stage_tile(tile, pool_tsdf, neighbour, slot, n);
  int brick[3];
  sg_unpack(pool_key[slot], brick[0], brick[1], brick[2]);
  const float origin[3] = {ox, oy, oz};
  long long base = offsets[2 * slot];
#pragma unroll
  for (int r = 0; r < kSeRounds; ++r) {
    const int cell = r * kSeThreads + threadIdx.x;
    int l[3];
    unsigned mask = 0;
    if (handled_cell(tile, cell, l[0], l[1], l[2])) mask = owned_mask(tile, l[0], l[1], l[2]);
    int total;
    const int local = block_exclusive_scan(__popc(mask), lds[r], total);
    long long vid = base + local;
    base += total;
    if (mask == 0 || vid >= V) continue;
    vertex_base[slot * kExtractCells + cell] = static_cast<int>(vid);
    const float va = halo_at(tile, l[0], l[1], l[2]);
    float ga[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) ga[a] = central(tile, l[0], l[1], l[2], a);
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      if (!(mask & (1u << axis)) || vid >= V) continue;
      const int e[3] = {axis == 0, axis == 1, axis == 2};
      const float vb = halo_at(tile, l[0] + e[0], l[1] + e[1], l[2] + e[2]);
      const float t = (0.0f - va) / (vb - va);
      float p[3], nrm[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        p[a] = static_cast<float>(brick[a] * kBrick + l[a]);
        const float gb = central(tile, l[0] + e[0], l[1] + e[1], l[2] + e[2], a);
        nrm[a] = ga[a] + t * (gb - ga[a]);
      }
      p[axis] = p[axis] + t;
      const float len = sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        verts[3 * vid + a] = p[a] * voxel_size + origin[a];
        normals[3 * vid + a] = len == 0.0f ? 0.0f : nrm[a] / len;
      }
      if (colors) {
        int q[3];      // local coordinates of the colour voxel: the owner or its +axis neighbour
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const int step = static_cast<int>(rintf(p[a])) - (brick[a] * kBrick + l[a]);
          q[a] = l[a] + (a == axis ? min(max(step, 0), 1) : 0);
        }
        const int dx = se_floor8(q[0]), dy = se_floor8(q[1]), dz = se_floor8(q[2]);
        const int s = tile.row[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)];
        float col = 0.0f;
        if (s >= 0) col = pool_color[static_cast<long long>(s) * kBrickVoxels + ((q[0] - 8 * dx) * 64 + (q[1] - 8 * dy) * 8 + (q[2] - 8 * dz))];
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
}
#pragma clang fp contract(fast)

__global__ __launch_bounds__(kSeThreads) void sparse_extract_faces_kernel(const float* __restrict__ pool_tsdf, const int* __restrict__ neighbour,
                                                                           long long n, const long long* __restrict__ offsets,
                                                                           const int* __restrict__ vertex_base, int* __restrict__ faces,
                                                                           long long F) {
  __shared__ SeTile tile;
  __shared__ int lds[kSeRounds][kSeThreads / 64];
  const long long slot = blockIdx.x;
  if (slot >= n) return;
  stage_tile(tile, pool_tsdf, neighbour, slot, n);
  long long base = offsets[2 * slot + 1];
#pragma unroll
  for (int r = 0; r < kSeRounds; ++r) {
    int lx, ly, lz, c = 0;
    if (handled_cell(tile, r * kSeThreads + threadIdx.x, lx, ly, lz)) c = cube_case(tile, lx, ly, lz);
    const int nt = kMcTriCount[c];
    int total;
    const int local = block_exclusive_scan(nt, lds[r], total);
    long long f = base + local;
    base += total;
    for (int s = 0; s < nt && s < DVMVS_MC_MAX_TRIS; ++s, ++f) {
      if (f >= F) break;
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const int e = kMcTriTable[c][3 * s + v];
        const int ox_ = lx + kMcEdgeOwner[e][0], oy_ = ly + kMcEdgeOwner[e][1], oz_ = lz + kMcEdgeOwner[e][2], axis = kMcEdgeOwner[e][3];
        int hs, cell, id = 0;
        if (se_handler(tile.row, ox_, oy_, oz_, hs, cell)) {
          id = vertex_base[static_cast<long long>(hs) * kExtractCells + cell];
          if (axis > 0) {      // plus the owner's crossing edges of lower axis
            const bool in = halo_at(tile, ox_, oy_, oz_) < 0.0f;
            if ((halo_at(tile, ox_ + 1, oy_, oz_) < 0.0f) != in) ++id;
            if (axis > 1 && ((halo_at(tile, ox_, oy_ + 1, oz_) < 0.0f) != in)) ++id;
          }
        }
        faces[3 * f + v] = id;
      }
    }
  }
}

}  // namespace

}  // namespace dvmvs

extern "C" int dvmvs_sparse_neighbours(const long long* pool_key, const long long* sorted, const long long* sort_index, const long long* status,
                                       long long max_bricks, int* neighbour, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!pool_key || !sorted || !sort_index || !status || !neighbour || max_bricks < 1) return DVMVS_EINVAL;
  if (max_bricks >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  const long long groups = (max_bricks * kExtractRow + kSeThreads - 1) / kSeThreads;
  if (groups >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  hipLaunchKernelGGL(sparse_neighbours_kernel, dim3(static_cast<unsigned>(groups)), dim3(kSeThreads), 0, static_cast<hipStream_t>(stream), pool_key,
                     sorted, sort_index, reinterpret_cast<const unsigned long long*>(status), max_bricks, neighbour);
  return launch_status();
}

extern "C" int dvmvs_sparse_extract_count(const float* pool_tsdf, const int* neighbour, const long long* status, long long max_bricks,
                                          int* counts, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!pool_tsdf || !neighbour || !status || !counts || max_bricks < 1) return DVMVS_EINVAL;
  if (max_bricks >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  hipLaunchKernelGGL(sparse_extract_count_kernel, dim3(static_cast<unsigned>(max_bricks)), dim3(kSeThreads), 0, static_cast<hipStream_t>(stream),
                     pool_tsdf, neighbour, reinterpret_cast<const unsigned long long*>(status), max_bricks, counts);
  return launch_status();
}

extern "C" int dvmvs_sparse_extract_scan(const int* counts, const long long* status, long long max_bricks, long long* offsets,
                                         long long* summary, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!counts || !status || !offsets || !summary || max_bricks < 1) return DVMVS_EINVAL;
  if (max_bricks >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  const long long chunk = (max_bricks + kSeScanThreads - 1) / kSeScanThreads;
  hipLaunchKernelGGL(sparse_extract_scan_kernel, dim3(1), dim3(kSeScanThreads), 0, static_cast<hipStream_t>(stream), counts,
                     reinterpret_cast<const unsigned long long*>(status), max_bricks, chunk, offsets, summary);
  return launch_status();
}

extern "C" int dvmvs_sparse_extract_emit(const float* pool_tsdf, const float* pool_color, const long long* pool_key, const int* neighbour,
                                         const long long* offsets, long long n_bricks, float origin_x, float origin_y, float origin_z,
                                         float voxel_size, int* vertex_base, float* verts, float* normals, unsigned char* colors, int* faces,
                                         long long V, long long F, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!pool_tsdf || !pool_key || !neighbour || !offsets || n_bricks < 0 || V < 0 || F < 0) return DVMVS_EINVAL;
  if (V > 0 && (!vertex_base || !verts || !normals || (pool_color && !colors))) return DVMVS_EINVAL;
  if (F > 0 && (!faces || !vertex_base)) return DVMVS_EINVAL;
  if (n_bricks >= (1LL << 31) || V >= (1LL << 31) || F >= (1LL << 31)) return DVMVS_EUNSUPPORTED;
  if (n_bricks == 0 || (V == 0 && F == 0)) return 0;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(n_bricks));
  if (V > 0)
    hipLaunchKernelGGL(sparse_extract_vertices_kernel, grid, dim3(kSeThreads), 0, s, pool_tsdf, pool_color, pool_key, neighbour, n_bricks, offsets,
                       origin_x, origin_y, origin_z, voxel_size, vertex_base, verts, normals, pool_color ? colors : nullptr, V);
  if (F > 0)
    hipLaunchKernelGGL(sparse_extract_faces_kernel, grid, dim3(kSeThreads), 0, s, pool_tsdf, neighbour, n_bricks, offsets, vertex_base, faces, F);
  return launch_status();
}
