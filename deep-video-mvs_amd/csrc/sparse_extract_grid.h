// Brick arithmetic of the mesh extraction from the sparse TSDF volume (csrc/sparse_extract.hip): the bounded
// binary search that rebuilds key -> pool slot, the neighbour row of a brick, and the rule that says which allocated brick HANDLES a
// voxel.  Functions that the host compiler takes too (tools/sparse_extract_check.cpp runs them under the address and
// undefined-behaviour sanitizers on a CPU, before a GPU sees them).
//
// Neighbour row.  row[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)] is the pool slot of brick b + d, d in {-1, 0, 1}^3, or -1 when that brick
// is not allocated or leaves |b| <= 2^20 - 1; row[13] is the brick's own slot.
//
// Local coordinates.  Voxel w seen from brick b has l = w - 8 b per axis.  Everything here takes l in [-1, 8]^3: the corners of the cubes
// of the voxels a brick can handle.  The brick of w is b + floor(l / 8), in the row.
//
// Handling rule.  A voxel of an allocated brick is handled by that brick.  A voxel w of an unallocated brick u, with the coordinates
// lu = w - 8 u inside u, has a cube that touches the bricks u + e, e in {0, 1}^3 with e_a = 1 only where lu_a = 7; the allocated one with
// the SMALLEST KEY among them handles w (its owned edges and its cube), and when none is allocated nobody does: all its corners are 1.
// Keys ascend lexicographically in (x, y, z), so the first allocated u + e in the order e = 000, 001, 010, ... (z fastest) is the handler.
// Seen from any brick b with l in [-1, 8]^3, u + e = b + floor(l / 8) + e has every component in {-1, 0, 1}: e_a = 1 needs lu_a = 7,
// i.e. l_a = -1 (floor = -1) or l_a = 7 (floor = 0).  So b's own row decides, and every brick that looks at w names the same handler.
// In the handler's coordinates w sits at lu - 8 e in [-1, 7]^3: slot (lu_x - 8 e_x + 1) * 81 + (lu_y - 8 e_y + 1) * 9 + (lu_z - 8 e_z + 1)
// of its 9 x 9 x 9 lattice of handled voxels.
#pragma once

#include "sparse_grid.h"

namespace dvmvs {

constexpr int kExtractRow = 27;          // neighbour entries per brick
constexpr int kExtractCells = 729;       // voxels a brick can handle: local -1 .. 7 per axis, 9^3
constexpr int kExtractSearchSteps = 32;  // > log2 of any pool size (max_bricks < 2^31)

// Position of `key` in sorted[0 .. n) (ascending, no duplicates), or -1.  Exactly kExtractSearchSteps steps, whatever the data.
DVMVS_SG_HD long long se_find(const long long* sorted, long long n, long long key) {
  long long lo = 0, hi = n > 0 ? n : 0;
  for (int step = 0; step < kExtractSearchSteps; ++step) {
    if (lo < hi) {
      const long long mid = lo + ((hi - lo) >> 1);
      if (sorted[mid] < key) lo = mid + 1;
      else hi = mid;
    }
  }
  return (lo < n && lo == hi && sorted[lo] == key) ? lo : -1;
}

// Entry `entry` (0 .. 26) of the row of brick (bx, by, bz): the value of index[] at the neighbour's place in sorted[0 .. n), or -1.
DVMVS_SG_HD int se_neighbour(const long long* sorted, const long long* index, long long n, int bx, int by, int bz, int entry) {
  const int dx = entry / 9 - 1, dy = (entry / 3) % 3 - 1, dz = entry % 3 - 1;
  const int x = bx + dx, y = by + dy, z = bz + dz;
  if (!sg_in_range(x, y, z)) return -1;
  const long long at = se_find(sorted, n, sg_pack(x, y, z));
  if (at < 0) return -1;
  const long long slot = index[at];
  return (slot >= 0 && slot < n) ? static_cast<int>(slot) : -1;
}

DVMVS_SG_HD int se_floor8(int l) { return l < 0 ? -1 : (l > 7 ? 1 : 0); }      // floor(l / 8) for l in [-8, 15]

DVMVS_SG_HD int se_clamp_local(int l) { return l < -1 ? -1 : (l > 8 ? 8 : l); }

// The handler of the voxel at local (lx, ly, lz), each clamped to [-1, 8], seen from the brick with neighbour row `row`: its pool slot in
// `slot` and the voxel's place in the handler's 9^3 lattice in `cell`; false (slot = -1, cell = 0) when nobody handles the voxel.
DVMVS_SG_HD bool se_handler(const int* row, int lx, int ly, int lz, int& slot, int& cell) {
  lx = se_clamp_local(lx);
  ly = se_clamp_local(ly);
  lz = se_clamp_local(lz);
  const int dx = se_floor8(lx), dy = se_floor8(ly), dz = se_floor8(lz);
  const int ux = lx - 8 * dx, uy = ly - 8 * dy, uz = lz - 8 * dz;      // inside its own brick, 0 .. 7
  const int own = row[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)];
  if (own >= 0) {
    slot = own;
    cell = (ux + 1) * 81 + (uy + 1) * 9 + (uz + 1);
    return true;
  }
  const int mx = ux == 7 ? 1 : 0, my = uy == 7 ? 1 : 0, mz = uz == 7 ? 1 : 0;
  for (int e = 1; e < 8; ++e) {      // ascending key; e = 0 is the unallocated brick itself
    const int ex = e >> 2, ey = (e >> 1) & 1, ez = e & 1;
    if (ex > mx || ey > my || ez > mz) continue;
    const int s = row[(dx + ex + 1) * 9 + (dy + ey + 1) * 3 + (dz + ez + 1)];
    if (s >= 0) {
      slot = s;
      cell = (ux - 8 * ex + 1) * 81 + (uy - 8 * ey + 1) * 9 + (uz - 8 * ez + 1);
      return true;
    }
  }
  slot = -1;
  cell = 0;
  return false;
}

// Which of its 9^3 local voxels the brick with row `row` handles depends on each axis only through l = -1, 0 .. 6, 7: class
// c = cx * 9 + cy * 3 + cz, with 0 / 1 / 2 for those three (se_class).  Whether the brick handles the voxels of class c:
DVMVS_SG_HD bool se_handles_class(const int* row, int c) {
  const int rep[3] = {-1, 3, 7};
  int slot, cell;
  return se_handler(row, rep[c / 9], rep[(c / 3) % 3], rep[c % 3], slot, cell) && slot == row[13];
}

DVMVS_SG_HD int se_class(int lx, int ly, int lz) {
  return (lx < 0 ? 0 : (lx == 7 ? 2 : 1)) * 9 + (ly < 0 ? 0 : (ly == 7 ? 2 : 1)) * 3 + (lz < 0 ? 0 : (lz == 7 ? 2 : 1));
}

}  // namespace dvmvs
