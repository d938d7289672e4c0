// Connected components of a triangle mesh and their removal by size (gfx950).  Both reproduce their host definitions bit for bit
// (dvmvs/components.py::mesh_components, filter_components; include/dvmvs_hip.h).  Everything that decides a result is an integer; the one
// float computation, a face's quantised area, stays inside its thread and is the quantised_face_area of dvmvs_device.h that
// surface_sample.hip uses (contract(off) there and for this whole file).  Integer sums are exact, so no order of the atomics can show.
//   dvmvs_mesh_components_fwd : faces int32 [F,3] (verts fp32 [V,3]) -> labels int32 [V], face_labels int32 [F], face_count int32 [V],
//                               area int64 [V], result int64 [2] = {n_components, status}
//   dvmvs_mesh_filter_count   : those + the thresholds -> counts int64 [3] = {V', F', status}
//   dvmvs_mesh_filter_emit    : the compacted, re-indexed mesh with its optional attributes and the old indices
//
// Labelling is a lock-free union-find over the vertices, three enqueues: cc_init_kernel (parent[v] = v) -> cc_hook_kernel (one thread per
// valid face: union(a, b), union(b, c)) -> cc_flatten_kernel (labels[v] = the root of v, into a SEPARATE array; it only reads parent).
// THE INVARIANT, which every line that touches `parent` inside the hook launch keeps:
//   (1) parent[v] <= v, always;
//   (2) an entry only ever decreases, and every value it takes is a vertex of v's component;
//   (3) every write to parent inside the hook launch is an atomic: the compare-and-swap of a hook (parent[larger root]: larger -> smaller)
//       or the atomicMin of path halving (parent[v] <- its grandparent).
// The atomics execute at the memory side; the reads are relaxed agent-scope loads that an XCD's L2 may serve with an OLDER value.  By (2) an
// older value is larger and still a vertex of the component, so a stale read can only make a find stop early at a vertex that was a root
// once; the compare-and-swap, which expects the vertex to be its own parent AT THE MEMORY SIDE, then fails, returns what is there, and the
// union goes on from that.  A stale read costs a retry, never a wrong hook.  The smallest vertex of a component can never be hooked (a
// hook goes under a smaller vertex of the same component), so after the launch every vertex's chain ends at it: the canonical labelling,
// whatever the schedule.  No loop is unbounded: a find moves to a strictly smaller vertex each step (at most v steps; a value outside
// [0, v] ends it with status 2), and a union makes at most kCcMaxRetries compare-and-swaps (each failure continues from strictly smaller
// vertices, so V bounds it as well), then gives up with status 2.
//
// Sizes, three enqueues: cc_count_kernel (one thread per face: face_labels; face_count and the area's separately summed upper and lower 32
// bits by integer atomics at the root: the faces of the workgroup's leading root are summed over the workgroup (1024 consecutive faces) and
// added once, the others once per wave where a wave's share a root, as neighbouring faces of a marching-cubes mesh mostly do, else one by
// one; the mesh's totals per workgroup) -> cc_finalize_kernel (area[r] from its halves; n_components) -> cc_result_kernel (the
// status: 2^63 units or more in total, decided exactly from the halves, or a face whose area is not finite: 1).
//
// Filtering.  Whether root r is kept is a function of face_count[r], area[r] and the thresholds; with keep_largest also of the winner, found
// by integer atomic passes after mf_best_init_kernel: mf_best_kernel<0> (max area) -> <1> (max face count among those) -> <2> (min label
// among those).  mf_flag_count_kernel counts kept faces and kept vertices per 1024 (a vertex is kept when its root is: a
// component with a face has no vertex outside its faces), mf_scan_blocks_kernel (one workgroup) scans the workgroup totals (scan_totals of
// dvmvs_device.h) and writes counts.  emit: mf_emit_verts_kernel (order-preserving compaction with block_exclusive_scan; the new index of
// every vertex goes to the workspace) -> mf_emit_faces_kernel.
#include "dvmvs_device.h"

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

constexpr int kCcBlock = 256;
constexpr int kCcPerThread = 4;
constexpr int kCcChunk = kCcBlock * kCcPerThread;      // faces or vertices per workgroup of a count or a scan
constexpr int kCcScanThreads = 1024;                   // the one workgroup that scans the workgroup totals
constexpr long long kCcMaxElements = 1LL << 28;        // V and F
constexpr int kCcMaxRetries = 1 << 16;                 // compare-and-swaps of one union before it gives up (status 2)
constexpr long long kCcTooLarge = 1LL << 31;           // floor(total area / 2^32) from which the total no longer fits

// the header of the workspace, 8-byte words
enum {
  kHdrTotalHi = 0,     // sum of the areas' upper halves over the mesh
  kHdrTotalLo,         // ... lower halves
  kHdrBadArea,         // a face whose area is not finite or does not fit
  kHdrExhausted,       // a union gave up, or parent held a value the invariant excludes
  kHdrBestArea,        // keep_largest: the winner's area, face count, label
  kHdrBestCount,
  kHdrBestLabel,
  kHdrWords = 32
};

typedef unsigned long long u64;

__device__ inline int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of v as far as this thread can see it (file comment).  Path halving, only as atomicMin(parent[v], grandparent).
__device__ inline int cc_find(int* __restrict__ parent, int v, bool& broken) {
  for (;;) {                                           // v strictly decreases: at most v steps
    const int p = cc_load(parent + v);
    if (p == v) return v;
    if (p < 0 || p > v) {
      broken = true;
      return v;
    }
    const int g = cc_load(parent + p);
    if (g == p) return p;
    if (g < 0 || g > p) {
      broken = true;
      return p;
    }
    atomicMin(parent + v, g);
    v = g;
  }
}

__device__ inline void cc_union(int* __restrict__ parent, int a, int b, u64* __restrict__ hdr) {
  bool broken = false;
  a = cc_find(parent, a, broken);
  b = cc_find(parent, b, broken);
  int tries = 0;
  while (a != b && !broken) {
    if (tries++ == kCcMaxRetries) {
      broken = true;
      break;
    }
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) break;                              // hi was a root at the memory side and now hangs under lo
    if (old < 0 || old > hi) {
      broken = true;
      break;
    }
    a = cc_find(parent, old, broken);                  // both below hi: the next attempt is at a strictly smaller vertex
    b = cc_find(parent, lo, broken);
  }
  if (broken) atomicOr(hdr + kHdrExhausted, 1ULL);
}

// parent[v] = v; the per-root sums, the header and the result start at 0
__global__ __launch_bounds__(kCcBlock) void cc_init_kernel(int* __restrict__ parent, int* __restrict__ face_count, u64* __restrict__ area_hi,
                                                           u64* __restrict__ area_lo, long long V, u64* __restrict__ hdr,
                                                           long long* __restrict__ result) {
  const long long v = static_cast<long long>(blockIdx.x) * kCcBlock + threadIdx.x;
  if (v < V) {
    parent[v] = static_cast<int>(v);
    face_count[v] = 0;
    area_hi[v] = 0;
    area_lo[v] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < kHdrWords) hdr[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x < 2) result[threadIdx.x] = 0;
}

__device__ inline bool cc_valid(int ia, int ib, int ic, long long V) { return ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V; }

__global__ __launch_bounds__(kCcBlock) void cc_hook_kernel(const int* __restrict__ faces, long long F, long long V, int* __restrict__ parent,
                                                           u64* __restrict__ hdr) {
  const long long f = static_cast<long long>(blockIdx.x) * kCcBlock + threadIdx.x;
  if (f >= F) return;
  const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
  if (!cc_valid(ia, ib, ic, V)) return;
  cc_union(parent, ia, ib, hdr);
  cc_union(parent, ib, ic, hdr);
}

// labels[v] = the end of v's chain.  Reads parent only (plain loads: the hook launch is complete), writes another array.
__global__ __launch_bounds__(kCcBlock) void cc_flatten_kernel(const int* __restrict__ parent, long long V, int* __restrict__ labels,
                                                              u64* __restrict__ hdr) {
  const long long i = static_cast<long long>(blockIdx.x) * kCcBlock + threadIdx.x;
  if (i >= V) return;
  int v = static_cast<int>(i);
  for (;;) {                                           // v strictly decreases
    const int p = parent[v];
    if (p == v) break;
    if (p < 0 || p > v) {
      atomicOr(hdr + kHdrExhausted, 1ULL);
      break;
    }
    v = p;
  }
  labels[i] = v;
}

// Workgroup b takes the faces [1024 b, 1024 b + 1024), thread t the faces 1024 b + 256 e + t: in step e a wave holds 64 consecutive faces.
__global__ __launch_bounds__(kCcBlock) void cc_count_kernel(const float* __restrict__ verts, long long V, const int* __restrict__ faces, long long F,
                                                            const int* __restrict__ labels, int* __restrict__ face_labels,
                                                            int* __restrict__ face_count, u64* __restrict__ area_hi, u64* __restrict__ area_lo,
                                                            u64* __restrict__ hdr) {
  __shared__ u64 s[5][kCcBlock / kWave];
  __shared__ int s_first[kCcBlock / kWave];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  int root[kCcPerThread];
  u64 hi[kCcPerThread], lo[kCcPerThread];
  bool bad = false;
  int mine = -1;                                       // the root of this thread's first valid face
#pragma unroll
  for (int e = 0; e < kCcPerThread; ++e) {
    const long long f = static_cast<long long>(blockIdx.x) * kCcChunk + e * kCcBlock + threadIdx.x;
    root[e] = -1;
    hi[e] = lo[e] = 0;
    if (f < F) {
      const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
      if (cc_valid(ia, ib, ic, V)) {
        int r = labels[ia];
        if (r < 0 || r >= V) r = -1;                   // never, for the labels of the flatten launch
        if (r >= 0 && verts) {
          long long area = quantised_face_area(verts, ia, ib, ic);
          if (area < 0) {
            area = 0;
            bad = true;
          }
          hi[e] = static_cast<u64>(area) >> 32;
          lo[e] = static_cast<u64>(area) & 0xffffffffULL;
        }
        root[e] = r;
      }
      face_labels[f] = root[e];
    }
    if (mine < 0) mine = root[e];
  }
  // the workgroup's own root: that of the first wave with a valid face, of its lowest such lane.  Its faces are summed over the
  // workgroup and added once; which root it is changes the number of atomics and not one sum.
  const u64 have = __ballot(mine >= 0);
  const int wave_first = have ? __shfl(mine, __ffsll(static_cast<long long>(have)) - 1, kWave) : -1;
  if (lane == 0) s_first[wave] = wave_first;
  __syncthreads();
  int own_root = -1;
#pragma unroll
  for (int w = kCcBlock / kWave - 1; w >= 0; --w)
    if (s_first[w] >= 0) own_root = s_first[w];
  u64 own_n = 0, own_hi = 0, own_lo = 0, total_hi = 0, total_lo = 0;      // of this thread's faces
#pragma unroll
  for (int e = 0; e < kCcPerThread; ++e) {
    total_hi += hi[e];
    total_lo += lo[e];
    const bool own = root[e] >= 0 && root[e] == own_root;
    if (own) {
      own_n += 1;
      own_hi += hi[e];
      own_lo += lo[e];
    }
    // the faces of other roots: one set of atomics for the wave where they share a root, else one per face
    const int other = own ? -1 : root[e];
    const u64 valid = __ballot(other >= 0);
    if (valid == 0) continue;                          // (wave-uniform)
    const int first = __shfl(other, __ffsll(static_cast<long long>(valid)) - 1, kWave);
    if (__all(other < 0 || other == first)) {
      const u64 n = static_cast<u64>(__popcll(valid)), wave_hi = wave_sum(own ? 0 : hi[e]), wave_lo = wave_sum(own ? 0 : lo[e]);
      if (lane == 0) {
        atomicAdd(face_count + first, static_cast<int>(n));
        if (verts) {
          atomicAdd(area_hi + first, wave_hi);
          atomicAdd(area_lo + first, wave_lo);
        }
      }
    } else if (other >= 0) {
      atomicAdd(face_count + other, 1);
      if (verts) {
        atomicAdd(area_hi + other, hi[e]);
        atomicAdd(area_lo + other, lo[e]);
      }
    }
  }
  const u64 sums[5] = {wave_sum(own_n), wave_sum(own_hi), wave_sum(own_lo), wave_sum(total_hi), wave_sum(total_lo)};
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k][wave] = sums[k];
  }
  if (bad) atomicOr(hdr + kHdrBadArea, 1ULL);
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 block[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < kCcBlock / kWave; ++w) {
#pragma unroll
      for (int k = 0; k < 5; ++k) block[k] += s[k][w];
    }
    if (own_root >= 0 && block[0]) {                   // (at most 1024 faces: the count fits an int)
      atomicAdd(face_count + own_root, static_cast<int>(block[0]));
      if (verts) {
        atomicAdd(area_hi + own_root, block[1]);
        atomicAdd(area_lo + own_root, block[2]);
      }
    }
    if (block[3]) atomicAdd(hdr + kHdrTotalHi, block[3]);      // 2^28 values below 2^31 and 2^32: neither can wrap
    if (block[4]) atomicAdd(hdr + kHdrTotalLo, block[4]);
  }
}

// area[r] from its halves (wraps where the status will say so); n_components += the roots with a face
__global__ __launch_bounds__(kCcBlock) void cc_finalize_kernel(const int* __restrict__ face_count, const u64* __restrict__ area_hi,
                                                               const u64* __restrict__ area_lo, long long V, long long* __restrict__ area,
                                                               long long* __restrict__ result) {
  __shared__ int s[kCcBlock / kWave];
  const long long v = static_cast<long long>(blockIdx.x) * kCcBlock + threadIdx.x;
  bool counted = false;
  if (v < V) {
    counted = face_count[v] > 0;
    if (area) area[v] = static_cast<long long>((area_hi[v] << 32) + area_lo[v]);
  }
  const int n = __popcll(__ballot(counted));
  if (threadIdx.x % kWave == 0) s[threadIdx.x / kWave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int block = 0;
    for (int w = 0; w < kCcBlock / kWave; ++w) block += s[w];
    if (block) atomicAdd(reinterpret_cast<u64*>(result), static_cast<u64>(block));
  }
}

__global__ void cc_result_kernel(const u64* __restrict__ hdr, long long* __restrict__ result) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool too_large = hdr[kHdrTotalHi] + (hdr[kHdrTotalLo] >> 32) >= static_cast<u64>(kCcTooLarge);
  result[1] = hdr[kHdrExhausted] ? 2 : (hdr[kHdrBadArea] || too_large) ? 1 : 0;
}

// ---- filtering ------------------------------------------------------------------------------------------------------------------------
struct MfRule {
  long long min_area;       // in units of 2^-32 m^2
  long long min_faces;
  int keep_largest;
};

__device__ inline bool mf_candidate(const int* __restrict__ face_count, long long V, long long r) { return r >= 0 && r < V && face_count[r] > 0; }

// whether the component of root r is kept
__device__ inline bool mf_keep(const int* __restrict__ face_count, const long long* __restrict__ area, long long V, long long r, const MfRule& rule,
                               const u64* __restrict__ hdr) {
  if (!mf_candidate(face_count, V, r)) return false;
  if (face_count[r] < rule.min_faces || area[r] < rule.min_area) return false;
  return !rule.keep_largest || static_cast<long long>(hdr[kHdrBestLabel]) == r;
}

__global__ void mf_best_init_kernel(u64* __restrict__ hdr) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  hdr[kHdrBestArea] = 0;
  hdr[kHdrBestCount] = 0;
  hdr[kHdrBestLabel] = ~0ULL;                          // (no candidate: no root equals it)
}

// pass 0: the greatest area; pass 1: the greatest face count among those; pass 2: the smallest label among those
template <int kPass>
__global__ __launch_bounds__(kCcBlock) void mf_best_kernel(const int* __restrict__ face_count, const long long* __restrict__ area, long long V,
                                                           u64* __restrict__ hdr) {
  const long long r = static_cast<long long>(blockIdx.x) * kCcBlock + threadIdx.x;
  if (!mf_candidate(face_count, V, r)) return;
  const u64 a = static_cast<u64>(area[r] < 0 ? 0 : area[r]), n = static_cast<u64>(face_count[r]);
  if (kPass == 0) {
    if (a > 0) atomicMax(hdr + kHdrBestArea, a);       // (0 is where it starts)
  } else if (a == hdr[kHdrBestArea]) {
    if (kPass == 1) atomicMax(hdr + kHdrBestCount, n);
    if (kPass == 2 && n == hdr[kHdrBestCount]) atomicMin(hdr + kHdrBestLabel, static_cast<u64>(r));
  }
}

// Workgroups [0, fblocks): kept faces per 1024 faces -> totals[b]; workgroups [fblocks, fblocks + vblocks): kept vertices per 1024 vertices.
// Thread t of a workgroup takes the 4 consecutive elements 1024 b + 4 t ..., as the emit kernels do.
__global__ __launch_bounds__(kCcBlock) void mf_flag_count_kernel(const int* __restrict__ labels, const int* __restrict__ face_labels,
                                                                 const int* __restrict__ face_count, const long long* __restrict__ area,
                                                                 long long V, long long F, MfRule rule, const u64* __restrict__ hdr, int fblocks,
                                                                 int* __restrict__ ftotals, int* __restrict__ vtotals) {
  __shared__ int lds[kCcBlock / 64];
  const bool is_face = static_cast<int>(blockIdx.x) < fblocks;
  const int b = is_face ? blockIdx.x : blockIdx.x - fblocks;
  const long long n = is_face ? F : V;
  const int* __restrict__ roots = is_face ? face_labels : labels;
  const long long first = (static_cast<long long>(b) * kCcBlock + threadIdx.x) * kCcPerThread;
  int v = 0;
  for (int e = 0; e < kCcPerThread; ++e)
    if (first + e < n && mf_keep(face_count, area, V, roots[first + e], rule, hdr)) ++v;
  int total;
  block_exclusive_scan<kCcBlock>(v, lds, total);
  if (threadIdx.x == 0) (is_face ? ftotals : vtotals)[b] = total;
}

__global__ __launch_bounds__(kCcScanThreads) void mf_scan_blocks_kernel(int* __restrict__ ftotals, int fblocks, int* __restrict__ vtotals, int vblocks,
                                                                        const long long* __restrict__ result, long long* __restrict__ counts) {
  __shared__ int s[kCcScanThreads];
  const int kept_faces = scan_totals<kCcScanThreads>(ftotals, fblocks, s);
  const int kept_verts = scan_totals<kCcScanThreads>(vtotals, vblocks, s);
  if (threadIdx.x == 0) {
    const long long status = result[1];
    counts[0] = status ? 0 : kept_verts;
    counts[1] = status ? 0 : kept_faces;
    counts[2] = status;
  }
}

// kept vertex v -> slot new_index[v] of the outputs (order-preserving); new_index[v] = -1 for the others
__global__ __launch_bounds__(kCcBlock) void mf_emit_verts_kernel(const float* __restrict__ verts, const float* __restrict__ normals,
                                                                 const unsigned char* __restrict__ colors, const int* __restrict__ labels,
                                                                 const int* __restrict__ face_count, const long long* __restrict__ area, long long V,
                                                                 MfRule rule, const u64* __restrict__ hdr, const int* __restrict__ offsets,
                                                                 long long V_out, int* __restrict__ new_index, float* __restrict__ verts_out,
                                                                 float* __restrict__ normals_out, unsigned char* __restrict__ colors_out,
                                                                 int* __restrict__ vertex_index) {
  __shared__ int lds[kCcBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kCcBlock + threadIdx.x) * kCcPerThread;
  bool keep[kCcPerThread];
  int n = 0;
#pragma unroll
  for (int e = 0; e < kCcPerThread; ++e) {
    keep[e] = first + e < V && mf_keep(face_count, area, V, labels[first + e], rule, hdr);
    n += keep[e] ? 1 : 0;
  }
  int total;
  long long slot = offsets[blockIdx.x] + block_exclusive_scan<kCcBlock>(n, lds, total);
#pragma unroll
  for (int e = 0; e < kCcPerThread; ++e) {
    const long long v = first + e;
    if (v >= V) break;
    const bool ok = keep[e] && slot >= 0 && slot < V_out;      // always, when V_out comes from the count step of the same mesh and rule
    new_index[v] = ok ? static_cast<int>(slot) : -1;
    if (!ok) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      verts_out[slot * 3 + d] = verts[v * 3 + d];
      if (normals_out) normals_out[slot * 3 + d] = normals[v * 3 + d];
      if (colors_out) colors_out[slot * 3 + d] = colors[v * 3 + d];
    }
    if (vertex_index) vertex_index[slot] = static_cast<int>(v);
    ++slot;
  }
}

__global__ __launch_bounds__(kCcBlock) void mf_emit_faces_kernel(const int* __restrict__ faces, const int* __restrict__ face_labels,
                                                                 const int* __restrict__ face_count, const long long* __restrict__ area, long long V,
                                                                 long long F, MfRule rule, const u64* __restrict__ hdr, const int* __restrict__ offsets,
                                                                 const int* __restrict__ new_index, long long F_out, int* __restrict__ faces_out,
                                                                 int* __restrict__ face_index) {
  __shared__ int lds[kCcBlock / 64];
  const long long first = (static_cast<long long>(blockIdx.x) * kCcBlock + threadIdx.x) * kCcPerThread;
  bool keep[kCcPerThread];
  int n = 0;
#pragma unroll
  for (int e = 0; e < kCcPerThread; ++e) {
    keep[e] = first + e < F && mf_keep(face_count, area, V, face_labels[first + e], rule, hdr);
    n += keep[e] ? 1 : 0;
  }
  int total;
  long long slot = offsets[blockIdx.x] + block_exclusive_scan<kCcBlock>(n, lds, total);
#pragma unroll
  for (int e = 0; e < kCcPerThread; ++e) {
    const long long f = first + e;
    if (f >= F) break;
    if (!keep[e] || slot < 0 || slot >= F_out) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int old = faces[f * 3 + d];
      faces_out[slot * 3 + d] = old >= 0 && old < V ? new_index[old] : -1;      // (a kept face is valid and its vertices are kept)
    }
    if (face_index) face_index[slot] = static_cast<int>(f);
    ++slot;
  }
}

size_t cc_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

int cc_blocks(long long n) { return static_cast<int>((n + kCcChunk - 1) / kCcChunk); }      // <= 2^18

unsigned int cc_grid(long long n) { return static_cast<unsigned int>((n + kCcBlock - 1) / kCcBlock); }

// workspace: header [32] int64 | area_hi [V] int64 | area_lo [V] int64 | parent [V] int32 | new_index [V] int32 | face block totals
// [blocks of F] int32 | vertex block totals [blocks of V] int32
struct CcLayout {
  size_t hi_off, lo_off, parent_off, index_off, ftotals_off, vtotals_off, total;
};

CcLayout cc_layout(long long V, long long F) {
  CcLayout l;
  l.hi_off = cc_align(kHdrWords * sizeof(u64));
  l.lo_off = l.hi_off + cc_align(static_cast<size_t>(V) * sizeof(u64));
  l.parent_off = l.lo_off + cc_align(static_cast<size_t>(V) * sizeof(u64));
  l.index_off = l.parent_off + cc_align(static_cast<size_t>(V) * sizeof(int));
  l.ftotals_off = l.index_off + cc_align(static_cast<size_t>(V) * sizeof(int));
  l.vtotals_off = l.ftotals_off + cc_align(static_cast<size_t>(cc_blocks(F)) * sizeof(int));
  l.total = l.vtotals_off + cc_align(static_cast<size_t>(cc_blocks(V)) * sizeof(int));
  return l;
}

bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

bool out_of_range(long long V, long long F) { return V > kCcMaxElements || F > kCcMaxElements; }

}  // namespace

}  // namespace dvmvs

extern "C" size_t dvmvs_mesh_components_workspace_bytes(long long V, long long F) {
  if (V < 0 || F < 0 || dvmvs::out_of_range(V, F)) return 0;
  return dvmvs::cc_layout(V, F).total;
}

extern "C" int dvmvs_mesh_components_fwd(const float* verts, long long V, const int* faces, long long F, void* workspace, size_t workspace_bytes,
                                         int* labels, int* face_labels, int* face_count, long long* area, long long* result,
                                         dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!workspace || !result || V < 0 || F < 0 || (F > 0 && (!faces || !face_labels)) || (V > 0 && (!labels || !face_count))) return DVMVS_EINVAL;
  if ((verts == nullptr) != (area == nullptr) && V > 0) return DVMVS_EINVAL;          // the areas need the vertices, and only they do
  if (misaligned(verts, 4) || misaligned(faces, 4) || misaligned(labels, 4) || misaligned(face_labels, 4) || misaligned(face_count, 4) ||
      misaligned(area, 8) || misaligned(result, 8) || misaligned(workspace, 16))
    return DVMVS_EINVAL;
  if (out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  const CcLayout l = cc_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  u64* hdr = reinterpret_cast<u64*>(ws);
  u64* area_hi = reinterpret_cast<u64*>(ws + l.hi_off);
  u64* area_lo = reinterpret_cast<u64*>(ws + l.lo_off);
  int* parent = reinterpret_cast<int*>(ws + l.parent_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const float* v_in = V > 0 ? verts : nullptr;
  hipLaunchKernelGGL(cc_init_kernel, dim3(V > 0 ? cc_grid(V) : 1), dim3(kCcBlock), 0, s, parent, face_count, area_hi, area_lo, V, hdr, result);
  if (V > 0 && F > 0) hipLaunchKernelGGL(cc_hook_kernel, dim3(cc_grid(F)), dim3(kCcBlock), 0, s, faces, F, V, parent, hdr);
  if (V > 0) hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_grid(V)), dim3(kCcBlock), 0, s, parent, V, labels, hdr);
  if (F > 0)
    hipLaunchKernelGGL(cc_count_kernel, dim3(cc_blocks(F)), dim3(kCcBlock), 0, s, v_in, V, faces, F, labels, face_labels, face_count, area_hi,
                       area_lo, hdr);
  if (V > 0)
    hipLaunchKernelGGL(cc_finalize_kernel, dim3(cc_grid(V)), dim3(kCcBlock), 0, s, face_count, area_hi, area_lo, V, v_in ? area : nullptr, result);
  hipLaunchKernelGGL(cc_result_kernel, dim3(1), dim3(kWave), 0, s, hdr, result);
  return launch_status();
}

extern "C" int dvmvs_mesh_filter_count(const int* labels, const int* face_labels, const int* face_count, const long long* area,
                                       const long long* result, long long V, long long F, long long min_area_units, long long min_faces,
                                       int keep_largest, void* workspace, size_t workspace_bytes, long long* counts, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!workspace || !result || !counts || V < 0 || F < 0 || (F > 0 && !face_labels) || (V > 0 && (!labels || !face_count || !area)))
    return DVMVS_EINVAL;
  if (min_area_units < 0 || min_faces < 0 || (keep_largest != 0 && keep_largest != 1)) return DVMVS_EINVAL;
  if (misaligned(labels, 4) || misaligned(face_labels, 4) || misaligned(face_count, 4) || misaligned(area, 8) || misaligned(result, 8) ||
      misaligned(counts, 8) || misaligned(workspace, 16))
    return DVMVS_EINVAL;
  if (out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  const CcLayout l = cc_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  u64* hdr = reinterpret_cast<u64*>(ws);
  int* ftotals = reinterpret_cast<int*>(ws + l.ftotals_off);
  int* vtotals = reinterpret_cast<int*>(ws + l.vtotals_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const MfRule rule = {min_area_units, min_faces, keep_largest};
  const int fblocks = cc_blocks(F), vblocks = cc_blocks(V);
  if (keep_largest) {
    hipLaunchKernelGGL(mf_best_init_kernel, dim3(1), dim3(kWave), 0, s, hdr);
    if (V > 0) {
      hipLaunchKernelGGL(mf_best_kernel<0>, dim3(cc_grid(V)), dim3(kCcBlock), 0, s, face_count, area, V, hdr);
      hipLaunchKernelGGL(mf_best_kernel<1>, dim3(cc_grid(V)), dim3(kCcBlock), 0, s, face_count, area, V, hdr);
      hipLaunchKernelGGL(mf_best_kernel<2>, dim3(cc_grid(V)), dim3(kCcBlock), 0, s, face_count, area, V, hdr);
    }
  }
  if (fblocks + vblocks > 0)
    hipLaunchKernelGGL(mf_flag_count_kernel, dim3(fblocks + vblocks), dim3(kCcBlock), 0, s, labels, face_labels, face_count, area, V, F, rule, hdr,
                       fblocks, ftotals, vtotals);
  hipLaunchKernelGGL(mf_scan_blocks_kernel, dim3(1), dim3(kCcScanThreads), 0, s, ftotals, fblocks, vtotals, vblocks, result, counts);
  return launch_status();
}

extern "C" int dvmvs_mesh_filter_emit(const float* verts, const int* faces, const float* normals, const unsigned char* colors, const int* labels,
                                      const int* face_labels, const int* face_count, const long long* area, long long V, long long F,
                                      long long min_area_units, long long min_faces, int keep_largest, void* workspace, size_t workspace_bytes,
                                      long long V_out, long long F_out, float* verts_out, int* faces_out, float* normals_out,
                                      unsigned char* colors_out, int* vertex_index, int* face_index, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!workspace || V < 1 || F < 1 || !verts || !faces || !labels || !face_labels || !face_count || !area) return DVMVS_EINVAL;
  if (V_out < 0 || F_out < 0 || V_out > V || F_out > F || (V_out > 0 && !verts_out) || (F_out > 0 && !faces_out)) return DVMVS_EINVAL;
  if ((normals == nullptr) != (normals_out == nullptr) && V_out > 0) return DVMVS_EINVAL;
  if ((colors == nullptr) != (colors_out == nullptr) && V_out > 0) return DVMVS_EINVAL;
  if (min_area_units < 0 || min_faces < 0 || (keep_largest != 0 && keep_largest != 1)) return DVMVS_EINVAL;
  if (misaligned(verts, 4) || misaligned(faces, 4) || misaligned(normals, 4) || misaligned(labels, 4) || misaligned(face_labels, 4) ||
      misaligned(face_count, 4) || misaligned(area, 8) || misaligned(workspace, 16) || misaligned(verts_out, 4) || misaligned(faces_out, 4) ||
      misaligned(normals_out, 4) || misaligned(vertex_index, 4) || misaligned(face_index, 4))
    return DVMVS_EINVAL;
  if (out_of_range(V, F)) return DVMVS_EUNSUPPORTED;
  const CcLayout l = cc_layout(V, F);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  if (V_out == 0 && F_out == 0) return 0;
  char* ws = static_cast<char*>(workspace);
  const u64* hdr = reinterpret_cast<const u64*>(ws);
  int* new_index = reinterpret_cast<int*>(ws + l.index_off);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const MfRule rule = {min_area_units, min_faces, keep_largest};
  hipLaunchKernelGGL(mf_emit_verts_kernel, dim3(cc_blocks(V)), dim3(kCcBlock), 0, s, verts, normals, colors, labels, face_count, area, V, rule, hdr,
                     reinterpret_cast<const int*>(ws + l.vtotals_off), V_out, new_index, verts_out, V_out > 0 ? normals_out : nullptr,
                     V_out > 0 ? colors_out : nullptr, vertex_index);
  if (F_out > 0)
    hipLaunchKernelGGL(mf_emit_faces_kernel, dim3(cc_blocks(F)), dim3(kCcBlock), 0, s, faces, face_labels, face_count, area, V, F, rule, hdr,
                       reinterpret_cast<const int*>(ws + l.ftotals_off), new_index, F_out, faces_out, face_index);
  return launch_status();
}
