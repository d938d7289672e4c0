// Brick arithmetic of the ray-caster of the sparse TSDF volume (csrc/sparse_raycast.hip): the render index
// (key -> pool slot and crossing flag) with its bounded probe, the brick and local index of a cell's eight corners and of a brick's 9^3
// corner lattice, and the rule that flags a brick.  Functions that the host compiler takes too (tools/sparse_raycast_check.cpp runs them
// under the address and undefined-behaviour sanitizers on a CPU, before a GPU sees them).
//
// Render index.  An open-addressing table of `slots` entries, a power of two >= 2 * max_bricks, so it is at most half full.  Entry e is
// two int64 words: index[2 e] the brick's key (kBrickEmpty = free), index[2 e + 1] its value = pool slot | crossing flag << 32.  One
// lookup answers "is this brick allocated, where, and can a hit end in it".  A key is placed by sg_hash / sg_probe, linear probing; insert
// and lookup make at most `slots` attempts, and a lookup ends at the first free entry (nothing is ever removed).  Which entry a key lands
// in depends on the order of insertion; what a lookup returns does not: a key is in the table once, on the probe path from its hash
// with no free entry before it.
//
// Corners of a cell.  The cell at local l in [0, 7]^3 of brick b has the corners l + e, e in {0, 1}^3 (e = ex * 4 + ey * 2 + ez, the order
// of the dense sampler); corner l + e lies in brick b + ((l + e) >> 3), entry ((dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)) of b's neighbour
// row (sparse_extract_grid.h; entry 13 is b itself), at local index ((l + e) & 7), x * 64 + y * 8 + z.
//
// Flag rule.  A brick is flagged when one of the 9^3 corners of its 8^3 cells (local 0 .. 8 per axis: its own voxels and the first
// layer of its seven forward neighbours) has weight > 0 && tsdf <= 0; a corner of an unallocated brick has weight 0.
#pragma once

#include "sparse_grid.h"

namespace dvmvs {

constexpr int kRaycastRow = 27;             // neighbour entries per brick, as kExtractRow
constexpr int kRaycastOwn = 13;             // the brick itself in its row
constexpr int kRaycastCorners = 729;        // 9^3 corners of a brick's cells
constexpr int kRaycastFlagShift = 32;

DVMVS_SG_HD long long sr_value(long long slot, bool flag) { return slot | (static_cast<long long>(flag ? 1 : 0) << kRaycastFlagShift); }
DVMVS_SG_HD int sr_slot(long long value) { return static_cast<int>(value & 0x7fffffffLL); }
DVMVS_SG_HD bool sr_flag(long long value) { return ((value >> kRaycastFlagShift) & 1) != 0; }

// Entry of `key` in the index of `slots` entries (a power of two), or -1.  At most `slots` attempts.
DVMVS_SG_HD long long sr_find(const long long* index, uint64_t slots, long long key) {
  const uint64_t mask = slots - 1, hash = sg_hash(key);
  for (uint64_t i = 0; i < slots; ++i) {
    const uint64_t e = sg_probe(hash, i, mask);
    const long long k = index[2 * e];
    if (k == key) return static_cast<long long>(e);
    if (k == kBrickEmpty) return -1;
  }
  return -1;
}

// The value of `key` (>= 0), or -1 when the brick is not in the index.
DVMVS_SG_HD long long sr_lookup(const long long* index, uint64_t slots, long long key) {
  const long long e = sr_find(index, slots, key);
  return e < 0 ? -1 : index[2 * e + 1];
}

// Sequential insert (one writer: the host check; the device inserts with a compare-and-swap on the same probe path).  The entry the key
// took or already had, or -1 when the table is full.
DVMVS_SG_HD long long sr_insert(long long* index, uint64_t slots, long long key, long long value) {
  const uint64_t mask = slots - 1, hash = sg_hash(key);
  for (uint64_t i = 0; i < slots; ++i) {
    const uint64_t e = sg_probe(hash, i, mask);
    if (index[2 * e] == kBrickEmpty) index[2 * e] = key;
    if (index[2 * e] == key) {
      index[2 * e + 1] = value;
      return static_cast<long long>(e);
    }
  }
  return -1;
}

// Row entry of the brick at step (dx, dy, dz), each in {-1, 0, 1}.
DVMVS_SG_HD int sr_row_entry(int dx, int dy, int dz) { return (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1); }

// The voxel at local (x, y, z), each in [0, 8], seen from a brick: its brick's row entry and its local index there.
DVMVS_SG_HD void sr_voxel(int x, int y, int z, int& entry, int& local) {
  entry = sr_row_entry(x >> 3, y >> 3, z >> 3);
  local = (x & 7) * 64 + (y & 7) * 8 + (z & 7);
}

// Corner e = ex * 4 + ey * 2 + ez of the cell at local (lx, ly, lz), each in [0, 7].
DVMVS_SG_HD void sr_corner(int lx, int ly, int lz, int e, int& entry, int& local) {
  sr_voxel(lx + ((e >> 2) & 1), ly + ((e >> 1) & 1), lz + (e & 1), entry, local);
}

// All eight corners of the cell lie in the brick itself.
DVMVS_SG_HD bool sr_interior(int lx, int ly, int lz) { return lx < 7 && ly < 7 && lz < 7; }

// Corner i = 0 .. 728 of the brick's 9^3 lattice, z fastest.
DVMVS_SG_HD void sr_lattice_corner(int i, int& entry, int& local) { sr_voxel(i / 81, (i / 9) % 9, i % 9, entry, local); }

DVMVS_SG_HD bool sr_crossing(float tsdf, float weight) { return weight > 0.0f && tsdf <= 0.0f; }

}  // namespace dvmvs
