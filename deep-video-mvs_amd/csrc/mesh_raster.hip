// Rasterising a triangle mesh to depth maps with a z-buffer, for N views in one call, and the per-vertex visibility against depth maps
// (gfx950).  Both reproduce the definition in include/dvmvs_hip.h bit for bit (tests/mesh_raster_reference.py restates it in numpy).
//   dvmvs_mesh_raster_fwd      : verts fp32 [V,3], faces int32 [F,3], cam_intr [N,3,3], cam_w2c [N,3,4] -> depth fp32 [N,H,W], face int32
//                                [N,H,W], overflow int32 [N]
//   dvmvs_mesh_visibility_fwd  : verts, depth [N,H,W], the cameras -> count int32 [V]
//
// What decides a pixel is integer arithmetic (int64 edge functions of vertices snapped to 1/256 px, the top-left rule) and float
// operations whose operands and order the definition fixes (contract(off) for the whole file).  The z-buffer is a 64-bit atomicMin of
// (depth bits << 32 | face): the smallest key wins whatever the order of arrival, so neither the launch shape, nor the path a triangle
// takes, nor the order of the faces can show in the result.
//
// Four enqueues: mr_init_kernel (keys <- all ones, list count and overflow <- 0: the workspace needs no initial state) -> mr_face_kernel
// (one thread per (view, face): set-up, near-plane clipping into one or two triangles; a triangle whose clipped box holds at most
// `large_box` pixels is rasterised by its thread, a larger one is cut into the 16x16 tiles of the image grid that its box meets and
// appended, as (view, face, piece, tile), to the work list in the workspace) -> mr_list_kernel (a fixed number of workgroups stride over
// the list, whose length they read from the workspace; an entry's 256 pixels go across the 256 lanes, the set-up is repeated per entry)
// -> mr_resolve_kernel (key -> depth, face).  List space is reserved with ONE atomic add per wave (a scan over the lanes' needs): the
// counter is a single address, and a compare-and-swap loop per triangle on it took 40 ms for 6 000 large triangles where this takes
// microseconds.  The list has a fixed capacity; a triangle handed a range beyond it fills what lies below the capacity with empty
// entries and is rasterised by its own thread (slow, same bits).  No workgroup waits for another one.
//   dvmvs_mesh_raster_cameras  : camera-to-world [N,4,4] -> world-to-camera [N,3,4], the fp64 inverse rounded once (one tiny launch)
#include "dvmvs_device.h"

#pragma clang fp contract(off)

namespace dvmvs {

namespace {

constexpr int kMrBlock = 256;
constexpr int kMrTile = 16;                              // a list entry: kMrTile x kMrTile pixels = the lanes of one workgroup
constexpr int kMrListGroups = 2048;                      // workgroups of the list kernel (8 per CU)
constexpr long long kMrMaxFaces = 1LL << 28;
constexpr int kMrMaxSide = 16384;
constexpr long long kMrMaxEntries = 1LL << 20;           // 16 MiB of list at most
constexpr float kMrSnapLimit = 536870912.0f;             // 2^21 px in units of 1/256 px
constexpr unsigned long long kMrEmpty = ~0ull;

struct MrHeader {
  unsigned long long count;  // entries asked for; those below the capacity are written
  unsigned long long pad[31];
};

struct MrEntry {
  int view, face, piece, tile;
};

struct MrCamera {
  float fx, fy, cx, cy;
  float m[12];
};

struct MrPlane {
  float nx, ny, nz, na, lo, hi;
};

struct MrTriangle {
  int X[3], Y[3];            // snapped, in 1/256 px
};

struct MrSetup {
  int ntri, overflow;
  MrTriangle tri[2];
  MrPlane plane;
};

// edge i: covered iff a[i] u + b[i] v + c[i] >= 0 for the pixel (u, v); the fill rule is folded into c
struct MrEdges {
  long long a[3], b[3], c[3];
  int u0, u1, v0, v1;        // the pixels of the box inside the image, inclusive; u0 > u1: none
};

__device__ inline MrCamera mr_camera(const float* __restrict__ cam_intr, const float* __restrict__ cam_w2c, int r) {
  MrCamera c;
  const float* K = cam_intr + static_cast<size_t>(r) * 9;
  c.fx = K[0];
  c.fy = K[4];
  c.cx = K[2];
  c.cy = K[5];
#pragma unroll
  for (int i = 0; i < 12; ++i) c.m[i] = cam_w2c[static_cast<size_t>(r) * 12 + i];
  return c;
}

__device__ inline void mr_to_camera(const MrCamera& c, const float* __restrict__ v, float* p) {
  const float x = v[0], y = v[1], z = v[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = ((c.m[i * 4] * x + c.m[i * 4 + 1] * y) + c.m[i * 4 + 2] * z) + c.m[i * 4 + 3];
}

// the point of the edge a -> b (a behind the near plane, b not) on the plane z = near
__device__ inline void mr_clip(const float* a, const float* b, float near, float* o) {
  const float t = (near - a[2]) / (b[2] - a[2]);
  o[0] = a[0] + t * (b[0] - a[0]);
  o[1] = a[1] + t * (b[1] - a[1]);
  o[2] = near;
}

// steps 1-4 of the definition for face f in one view
__device__ inline void mr_setup(const float* __restrict__ verts, long long V, const int* __restrict__ faces, long long f, const MrCamera& cam,
                                float near, int cull, MrSetup& s) {
  s.ntri = 0;
  s.overflow = 0;
  const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return;
  float p[3][3];
  mr_to_camera(cam, verts + static_cast<size_t>(i0) * 3, p[0]);
  mr_to_camera(cam, verts + static_cast<size_t>(i1) * 3, p[1]);
  mr_to_camera(cam, verts + static_cast<size_t>(i2) * 3, p[2]);
  const float inf = __builtin_inff();
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (!(fabsf(p[j][i]) < inf)) return;
  const bool b0 = p[0][2] < near, b1 = p[1][2] < near, b2 = p[2][2] < near;
  const int nb = (b0 ? 1 : 0) + (b1 ? 1 : 0) + (b2 ? 1 : 0);
  if (nb == 3) return;
  float e1[3], e2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    e1[i] = p[1][i] - p[0][i];
    e2[i] = p[2][i] - p[0][i];
  }
  MrPlane& pl = s.plane;
  pl.nx = e1[1] * e2[2] - e1[2] * e2[1];
  pl.ny = e1[2] * e2[0] - e1[0] * e2[2];
  pl.nz = e1[0] * e2[1] - e1[1] * e2[0];
  pl.na = (pl.nx * p[0][0] + pl.ny * p[0][1]) + pl.nz * p[0][2];
  if (cull && !(pl.na < 0.0f)) return;
  pl.lo = fmaxf(fminf(fminf(p[0][2], p[1][2]), p[2][2]), near);
  pl.hi = fmaxf(fmaxf(p[0][2], p[1][2]), p[2][2]);
  // the polygon in front of the near plane: 3 or 4 corners
  float q[4][3];
  int nq = 3;
  if (nb == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) q[j][i] = p[j][i];
  } else {
    // rotated so that the odd one out (the one behind, or the one in front) comes first; the cyclic order is kept
    const int k = nb == 1 ? (b0 ? 0 : (b1 ? 1 : 2)) : (!b0 ? 0 : (!b1 ? 1 : 2));
    float v[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) v[j][i] = k == 0 ? p[j][i] : (k == 1 ? p[(j + 1) % 3][i] : p[(j + 2) % 3][i]);
    if (nb == 1) {
      mr_clip(v[0], v[1], near, q[0]);
      mr_clip(v[0], v[2], near, q[3]);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        q[1][i] = v[1][i];
        q[2][i] = v[2][i];
      }
      nq = 4;
    } else {
      mr_clip(v[1], v[0], near, q[1]);
      mr_clip(v[2], v[0], near, q[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) q[0][i] = v[0][i];
    }
  }
  int X[4], Y[4];
  bool ok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ok[j] = true;
    X[j] = Y[j] = 0;
    if (j < nq) {
      const float sx = rintf(256.0f * ((q[j][0] / q[j][2]) * cam.fx + cam.cx));
      const float sy = rintf(256.0f * ((q[j][1] / q[j][2]) * cam.fy + cam.cy));
      ok[j] = fabsf(sx) <= kMrSnapLimit && fabsf(sy) <= kMrSnapLimit;        // false for a NaN
      if (ok[j]) {
        X[j] = static_cast<int>(sx);
        Y[j] = static_cast<int>(sy);
      }
    }
  }
  if (ok[0] && ok[1] && ok[2]) {
    MrTriangle& t = s.tri[s.ntri++];
    t.X[0] = X[0]; t.X[1] = X[1]; t.X[2] = X[2];
    t.Y[0] = Y[0]; t.Y[1] = Y[1]; t.Y[2] = Y[2];
  } else {
    ++s.overflow;
  }
  if (nq == 4) {
    if (ok[0] && ok[2] && ok[3]) {
      MrTriangle& t = s.tri[s.ntri++];
      t.X[0] = X[0]; t.X[1] = X[2]; t.X[2] = X[3];
      t.Y[0] = Y[0]; t.Y[1] = Y[2]; t.Y[2] = Y[3];
    } else {
      ++s.overflow;
    }
  }
}

// step 5: the edge functions and the pixel box of a snapped triangle; false for one without area or without a pixel in its box
__device__ inline bool mr_edges(const MrTriangle& t, int H, int W, MrEdges& e) {
  long long X[3] = {t.X[0], t.X[1], t.X[2]}, Y[3] = {t.Y[0], t.Y[1], t.Y[2]};
  const long long area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
  if (area == 0) return false;
  if (area < 0) {
    const long long tx = X[1], ty = Y[1];
    X[1] = X[2]; Y[1] = Y[2];
    X[2] = tx; Y[2] = ty;
  }
  const long long xmin = min(min(X[0], X[1]), X[2]), xmax = max(max(X[0], X[1]), X[2]);
  const long long ymin = min(min(Y[0], Y[1]), Y[2]), ymax = max(max(Y[0], Y[1]), Y[2]);
  e.u0 = static_cast<int>(max((xmin + 255) >> 8, 0LL));
  e.u1 = static_cast<int>(min(xmax >> 8, static_cast<long long>(W - 1)));
  e.v0 = static_cast<int>(max((ymin + 255) >> 8, 0LL));
  e.v1 = static_cast<int>(min(ymax >> 8, static_cast<long long>(H - 1)));
  if (e.u0 > e.u1 || e.v0 > e.v1) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = (i + 1) % 3;
    const long long dx = X[j] - X[i], dy = Y[j] - Y[i];
    const bool top_left = dy < 0 || (dy == 0 && dx > 0);
    e.a[i] = -dy * 256;
    e.b[i] = dx * 256;
    e.c[i] = (dy * X[i] - dx * Y[i]) - (top_left ? 0 : 1);
  }
  return true;
}

// steps 6-7 for a covered pixel
__device__ inline void mr_shade(const MrPlane& pl, const MrCamera& cam, int u, int v, float far, unsigned int face,
                                unsigned long long* __restrict__ key) {
  const float dx = (static_cast<float>(u) - cam.cx) / cam.fx;
  const float dy = (static_cast<float>(v) - cam.cy) / cam.fy;
  const float den = (pl.nx * dx + pl.ny * dy) + pl.nz;
  float z = pl.na / den;
  z = fminf(fmaxf(z, pl.lo), pl.hi);         // fmaxf(NaN, lo) = lo: always finite, near <= lo <= z <= hi
  if (z > far) return;
  atomicMin(key, (static_cast<unsigned long long>(__float_as_uint(z)) << 32) | face);
}

// one thread walks the box [u0, u1] x [v0, v1]
__device__ inline void mr_walk(const MrEdges& e, int u0, int u1, int v0, int v1, const MrPlane& pl, const MrCamera& cam, float far,
                               unsigned int face, unsigned long long* __restrict__ keys, int W) {
  long long row[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) row[i] = e.a[i] * u0 + e.b[i] * v0 + e.c[i];
  for (int v = v0; v <= v1; ++v) {
    long long w0 = row[0], w1 = row[1], w2 = row[2];
    for (int u = u0; u <= u1; ++u) {
      if ((w0 | w1 | w2) >= 0) mr_shade(pl, cam, u, v, far, face, keys + static_cast<size_t>(v) * W + u);
      w0 += e.a[0];
      w1 += e.a[1];
      w2 += e.a[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) row[i] += e.b[i];
  }
}

__global__ __launch_bounds__(kMrBlock) void mr_init_kernel(unsigned long long* __restrict__ keys, long long n_keys, MrHeader* __restrict__ hdr,
                                                           int* __restrict__ overflow, int n_views) {
  const long long stride = static_cast<long long>(gridDim.x) * kMrBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kMrBlock + threadIdx.x;
  for (long long i = first; i < n_keys; i += stride) keys[i] = kMrEmpty;
  if (first < n_views) overflow[first] = 0;
  if (first == 0) hdr->count = 0;
}

__global__ __launch_bounds__(kMrBlock) void mr_face_kernel(const float* __restrict__ verts, long long V, const int* __restrict__ faces, long long F,
                                                           const float* __restrict__ cam_intr, const float* __restrict__ cam_w2c, int H, int W,
                                                           float near, float far, int cull, int large_box, unsigned long long* __restrict__ keys,
                                                           MrHeader* __restrict__ hdr, MrEntry* __restrict__ list, unsigned int capacity,
                                                           int* __restrict__ overflow) {
  const long long f = static_cast<long long>(blockIdx.x) * kMrBlock + threadIdx.x;
  const int r = blockIdx.y;
  const MrCamera cam = mr_camera(cam_intr, cam_w2c, r);
  MrSetup s;
  s.ntri = 0;
  s.overflow = 0;
  if (f < F) mr_setup(verts, V, faces, f, cam, near, cull, s);         // (no early return: every lane takes part in the scan below)
  if (s.overflow) atomicAdd(overflow + r, s.overflow);
  unsigned long long* view_keys = keys + static_cast<size_t>(r) * H * W;
  const int tiles_x = (W + kMrTile - 1) / kMrTile;
  MrEdges e[2];
  bool live[2] = {false, false};
  unsigned int want[2] = {0, 0};         // list entries of a large piece
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (k < s.ntri) live[k] = mr_edges(s.tri[k], H, W, e[k]);
    if (live[k] && static_cast<long long>(e[k].u1 - e[k].u0 + 1) * (e[k].v1 - e[k].v0 + 1) > large_box)
      want[k] = static_cast<unsigned int>((e[k].u1 / kMrTile - e[k].u0 / kMrTile + 1) * (e[k].v1 / kMrTile - e[k].v0 / kMrTile + 1));
  }
  // one reservation per wave: the count only grows, and whoever is handed a range below the capacity writes all of it
  const int need = static_cast<int>(want[0] + want[1]);               // < 2^21
  const int incl = wave_inclusive_scan(need);
  const int total = __shfl(incl, kWave - 1, kWave);
  unsigned long long base = 0;
  if ((threadIdx.x & (kWave - 1)) == kWave - 1 && total > 0) base = atomicAdd(&hdr->count, static_cast<unsigned long long>(total));
  base = __shfl(base, kWave - 1, kWave);
  unsigned long long at = base + static_cast<unsigned long long>(incl - need);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (!live[k]) continue;
    if (want[k] > 0) {
      const bool fits = at <= capacity && want[k] <= capacity - at;
      if (fits) {
        MrEntry* out = list + at;
        for (int ty = e[k].v0 / kMrTile; ty <= e[k].v1 / kMrTile; ++ty)
          for (int tx = e[k].u0 / kMrTile; tx <= e[k].u1 / kMrTile; ++tx) {
            MrEntry en;
            en.view = r;
            en.face = static_cast<int>(f);
            en.piece = k;
            en.tile = ty * tiles_x + tx;
            *out++ = en;
          }
      } else {
        // the list is full: the part of the range below the capacity is filled with entries that say "nothing" ...
        MrEntry none;
        none.view = none.face = none.piece = none.tile = -1;
        for (unsigned long long i = at; i < capacity && i < at + want[k]; ++i) list[i] = none;
      }
      at += want[k];
      if (fits) continue;
    }
    // ... and the thread takes the triangle itself, as it does every small one
    mr_walk(e[k], e[k].u0, e[k].u1, e[k].v0, e[k].v1, s.plane, cam, far, static_cast<unsigned int>(f), view_keys, W);
  }
}

__global__ __launch_bounds__(kMrBlock) void mr_list_kernel(const float* __restrict__ verts, long long V, const int* __restrict__ faces, long long F,
                                                           const float* __restrict__ cam_intr, const float* __restrict__ cam_w2c, int n_views,
                                                           int H, int W, float near, float far, int cull, unsigned long long* __restrict__ keys,
                                                           const MrHeader* __restrict__ hdr, const MrEntry* __restrict__ list,
                                                           unsigned int capacity) {
  const unsigned int count = static_cast<unsigned int>(min(hdr->count, static_cast<unsigned long long>(capacity)));
  const int tiles_x = (W + kMrTile - 1) / kMrTile, tiles_y = (H + kMrTile - 1) / kMrTile;
  const int lx = threadIdx.x % kMrTile, ly = threadIdx.x / kMrTile;
  for (unsigned int i = blockIdx.x; i < count; i += gridDim.x) {
    const MrEntry en = list[i];
    // (always, for an entry the face kernel of the same call wrote)
    if (en.view < 0 || en.view >= n_views || en.face < 0 || en.face >= F || en.tile < 0 || en.tile >= tiles_x * tiles_y) continue;
    const MrCamera cam = mr_camera(cam_intr, cam_w2c, en.view);
    MrSetup s;
    mr_setup(verts, V, faces, en.face, cam, near, cull, s);
    if (en.piece < 0 || en.piece >= s.ntri) continue;
    MrEdges e;
    if (!mr_edges(en.piece == 0 ? s.tri[0] : s.tri[1], H, W, e)) continue;
    const int u = (en.tile % tiles_x) * kMrTile + lx, v = (en.tile / tiles_x) * kMrTile + ly;
    if (u < e.u0 || u > e.u1 || v < e.v0 || v > e.v1) continue;
    const long long w0 = e.a[0] * u + e.b[0] * v + e.c[0];
    const long long w1 = e.a[1] * u + e.b[1] * v + e.c[1];
    const long long w2 = e.a[2] * u + e.b[2] * v + e.c[2];
    if ((w0 | w1 | w2) >= 0)
      mr_shade(s.plane, cam, u, v, far, static_cast<unsigned int>(en.face), keys + (static_cast<size_t>(en.view) * H + v) * W + u);
  }
}

__global__ __launch_bounds__(kMrBlock) void mr_resolve_kernel(const unsigned long long* __restrict__ keys, long long n_keys, float* __restrict__ depth,
                                                              int* __restrict__ face) {
  const long long stride = static_cast<long long>(gridDim.x) * kMrBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kMrBlock + threadIdx.x; i < n_keys; i += stride) {
    const unsigned long long k = keys[i];
    const bool hit = k != kMrEmpty;
    depth[i] = hit ? __uint_as_float(static_cast<unsigned int>(k >> 32)) : 0.0f;
    face[i] = hit ? static_cast<int>(static_cast<unsigned int>(k)) : -1;
  }
}

// one thread per vertex, the views in order
__global__ __launch_bounds__(kMrBlock) void mr_visibility_kernel(const float* __restrict__ verts, long long V, const float* __restrict__ depth,
                                                                 const float* __restrict__ cam_intr, const float* __restrict__ cam_w2c, int n_views,
                                                                 int H, int W, float near, float relative, float absolute, int* __restrict__ count) {
  const long long i = static_cast<long long>(blockIdx.x) * kMrBlock + threadIdx.x;
  if (i >= V) return;
  const float scale = 1.0f + relative;
  const float xmax = static_cast<float>(W - 1), ymax = static_cast<float>(H - 1);
  int seen = 0;
  for (int r = 0; r < n_views; ++r) {
    const MrCamera cam = mr_camera(cam_intr, cam_w2c, r);
    float p[3];
    mr_to_camera(cam, verts + i * 3, p);
    if (!(p[2] >= near)) continue;
    const float xp = (p[0] / p[2]) * cam.fx + cam.cx, yp = (p[1] / p[2]) * cam.fy + cam.cy;
    if (!(xp >= 0.0f && xp <= xmax && yp >= 0.0f && yp <= ymax)) continue;       // false for a NaN
    const int x0 = static_cast<int>(floorf(xp)), y0 = static_cast<int>(floorf(yp));
    const float* map = depth + static_cast<size_t>(r) * H * W;
    float best = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
        if (x0 + dx < W && y0 + dy < H) {
          const float d = map[static_cast<size_t>(y0 + dy) * W + (x0 + dx)];
          if (d > best) best = d;            // false for a NaN
        }
    if (best > 0.0f && p[2] <= best * scale + absolute) ++seen;
  }
  count[i] = seen;
}

// world-to-camera [n,3,4] fp32 <- the inverse of camera-to-world [n,4,4] fp32, in fp64 by cofactors, rounded once; one thread per view
__global__ __launch_bounds__(kWave) void mr_cameras_kernel(const float* __restrict__ cam_pose, float* __restrict__ cam_w2c, int n_views) {
  const int r = blockIdx.x * kWave + threadIdx.x;
  if (r >= n_views) return;
  double P[16], inv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) P[i] = static_cast<double>(cam_pose[static_cast<size_t>(r) * 16 + i]);
  inverse4(P, inv);
#pragma unroll
  for (int i = 0; i < 12; ++i) cam_w2c[static_cast<size_t>(r) * 12 + i] = static_cast<float>(inv[i]);
}

size_t mr_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

// workspace: header | keys [N,H,W] uint64 | list [capacity] of 16 bytes
struct MrLayout {
  size_t keys_off, list_off, total;
  unsigned int capacity;
};

bool mr_shape_ok(long long n_views, long long n_faces, long long im_h, long long im_w) {
  return n_views >= 1 && n_views <= 65535 && n_faces >= 1 && n_faces <= kMrMaxFaces && im_h >= 1 && im_w >= 1 && im_h <= kMrMaxSide &&
         im_w <= kMrMaxSide && n_views * im_h * im_w < (1LL << 31) &&
         // (the 64-bit count of list entries asked for cannot wrap)
         static_cast<double>(n_views) * static_cast<double>(n_faces) * 2.0 * static_cast<double>(((im_h + kMrTile - 1) / kMrTile) * ((im_w + kMrTile - 1) / kMrTile)) < 4.0e18;
}

MrLayout mr_layout(long long n_views, long long n_faces, long long im_h, long long im_w) {
  MrLayout l;
  const long long tiles = ((im_h + kMrTile - 1) / kMrTile) * ((im_w + kMrTile - 1) / kMrTile);
  // every (view, face) can give two triangles over every tile; beyond 2^20 entries a triangle is rasterised by its own thread
  long long cap = kMrMaxEntries;
  if (n_faces <= kMrMaxEntries / 2 && n_views * n_faces * 2 <= kMrMaxEntries && n_views * n_faces * 2 * tiles <= kMrMaxEntries)
    cap = n_views * n_faces * 2 * tiles;
  l.capacity = static_cast<unsigned int>(cap);
  l.keys_off = mr_align(sizeof(MrHeader));
  l.list_off = l.keys_off + mr_align(static_cast<size_t>(n_views * im_h * im_w) * sizeof(unsigned long long));
  l.total = l.list_off + mr_align(static_cast<size_t>(cap) * sizeof(MrEntry));
  return l;
}

bool mr_misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

int mr_stride_groups(long long n) {
  const long long g = (n + kMrBlock - 1) / kMrBlock;
  return static_cast<int>(g < 4096 ? g : 4096);
}

}  // namespace

}  // namespace dvmvs

extern "C" size_t dvmvs_mesh_raster_workspace_bytes(long long n_views, long long n_faces, long long im_h, long long im_w) {
  if (!dvmvs::mr_shape_ok(n_views, n_faces, im_h, im_w)) return 0;
  return dvmvs::mr_layout(n_views, n_faces, im_h, im_w).total;
}

extern "C" int dvmvs_mesh_raster_cameras(const float* cam_pose, float* cam_w2c, int n_views, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!cam_pose || !cam_w2c || n_views < 1 || mr_misaligned(cam_pose, 4) || mr_misaligned(cam_w2c, 4)) return DVMVS_EINVAL;
  if (n_views > 65535) return DVMVS_EUNSUPPORTED;
  hipLaunchKernelGGL(mr_cameras_kernel, dim3((n_views + kWave - 1) / kWave), dim3(kWave), 0, static_cast<hipStream_t>(stream), cam_pose, cam_w2c,
                     n_views);
  return launch_status();
}

extern "C" int dvmvs_mesh_raster_fwd(const float* verts, long long V, const int* faces, long long F, const float* cam_intr, const float* cam_w2c,
                                     int n_views, int im_h, int im_w, float near, float far, int cull_backfaces, int large_box, void* workspace,
                                     size_t workspace_bytes, float* depth, int* face, int* overflow, dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!verts || !faces || !cam_intr || !cam_w2c || !workspace || !depth || !face || !overflow) return DVMVS_EINVAL;
  if (V < 1 || F < 1 || n_views < 1 || im_h < 1 || im_w < 1 || large_box < 1) return DVMVS_EINVAL;
  if (!(near > 0.0f) || near == __builtin_inff() || far != far || (cull_backfaces != 0 && cull_backfaces != 1)) return DVMVS_EINVAL;
  if (mr_misaligned(verts, 4) || mr_misaligned(faces, 4) || mr_misaligned(cam_intr, 4) || mr_misaligned(cam_w2c, 4) ||
      mr_misaligned(workspace, 16) || mr_misaligned(depth, 4) || mr_misaligned(face, 4) || mr_misaligned(overflow, 4))
    return DVMVS_EINVAL;
  if (V > 0x7fffffffLL || !mr_shape_ok(n_views, F, im_h, im_w)) return DVMVS_EUNSUPPORTED;
  const MrLayout l = mr_layout(n_views, F, im_h, im_w);
  if (workspace_bytes < l.total) return DVMVS_EINVAL;
  char* ws = static_cast<char*>(workspace);
  MrHeader* hdr = reinterpret_cast<MrHeader*>(ws);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + l.keys_off);
  MrEntry* list = reinterpret_cast<MrEntry*>(ws + l.list_off);
  const long long n_keys = static_cast<long long>(n_views) * im_h * im_w;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mr_init_kernel, dim3(mr_stride_groups(n_keys > n_views ? n_keys : n_views)), dim3(kMrBlock), 0, s, keys, n_keys, hdr, overflow,
                     n_views);
  hipLaunchKernelGGL(mr_face_kernel, dim3(static_cast<unsigned int>((F + kMrBlock - 1) / kMrBlock), n_views), dim3(kMrBlock), 0, s, verts, V, faces,
                     F, cam_intr, cam_w2c, im_h, im_w, near, far, cull_backfaces, large_box, keys, hdr, list, l.capacity, overflow);
  hipLaunchKernelGGL(mr_list_kernel, dim3(kMrListGroups), dim3(kMrBlock), 0, s, verts, V, faces, F, cam_intr, cam_w2c, n_views, im_h, im_w, near,
                     far, cull_backfaces, keys, hdr, list, l.capacity);
  hipLaunchKernelGGL(mr_resolve_kernel, dim3(mr_stride_groups(n_keys)), dim3(kMrBlock), 0, s, keys, n_keys, depth, face);
  return launch_status();
}

extern "C" int dvmvs_mesh_visibility_fwd(const float* verts, long long V, const float* depth, const float* cam_intr, const float* cam_w2c,
                                         int n_views, int im_h, int im_w, float near, float relative, float absolute, int* count,
                                         dvmvs_stream_t stream) {
  using namespace dvmvs;
  if (!verts || !depth || !cam_intr || !cam_w2c || !count) return DVMVS_EINVAL;
  if (V < 1 || n_views < 1 || im_h < 1 || im_w < 1) return DVMVS_EINVAL;
  if (!(near > 0.0f) || near == __builtin_inff() || relative != relative || absolute != absolute) return DVMVS_EINVAL;
  if (mr_misaligned(verts, 4) || mr_misaligned(depth, 4) || mr_misaligned(cam_intr, 4) || mr_misaligned(cam_w2c, 4) || mr_misaligned(count, 4))
    return DVMVS_EINVAL;
  if (V > 0x7fffffffLL || !mr_shape_ok(n_views, 1, im_h, im_w)) return DVMVS_EUNSUPPORTED;
  hipLaunchKernelGGL(mr_visibility_kernel, dim3(static_cast<unsigned int>((V + kMrBlock - 1) / kMrBlock)), dim3(kMrBlock), 0,
                     static_cast<hipStream_t>(stream), verts, V, depth, cam_intr, cam_w2c, n_views, im_h, im_w, near, relative, absolute, count);
  return launch_status();
}
