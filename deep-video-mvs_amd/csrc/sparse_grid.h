// The brick lattice of the sparse TSDF volume (csrc/sparse_volume.hip): key packing, the hash and the probe
// sequence, as functions that the host compiler takes too (tools/sparse_grid_check.cpp runs them under the address and undefined-behaviour
// sanitizers on a CPU, before a GPU sees the bounded probe).
//
// A brick is 8 x 8 x 8 voxels; brick b = floor(v / 8) per component, |b| < 2^20 (so |v| < 2^23 and float(v) is exact).  Each component is
// stored with the bias 2^20 - 1 in 21 bits, x in the highest: a field lies in [0, 2^21 - 2], the key in [0, 2^63), ascending keys are the
// bricks in lexicographic (x, y, z) order, and the all-ones word 2^63 - 1 is no brick: it marks a free table slot and fills sort scratch.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DVMVS_SG_HD __host__ __device__ inline
#else
#define DVMVS_SG_HD inline
#endif

namespace dvmvs {

constexpr int kBrick = 8;                       // voxels per brick edge
constexpr int kBrickVoxels = 512;
constexpr int kBrickLimit = (1 << 20) - 1;      // |b| <= kBrickLimit
constexpr long long kBrickEmpty = 0x7fffffffffffffffLL;

DVMVS_SG_HD bool sg_in_range(int bx, int by, int bz) {
  return bx >= -kBrickLimit && bx <= kBrickLimit && by >= -kBrickLimit && by <= kBrickLimit && bz >= -kBrickLimit && bz <= kBrickLimit;
}

// the key of a brick in range (a precondition)
DVMVS_SG_HD long long sg_pack(int bx, int by, int bz) {
  const uint64_t x = static_cast<uint64_t>(static_cast<int64_t>(bx) + kBrickLimit);
  const uint64_t y = static_cast<uint64_t>(static_cast<int64_t>(by) + kBrickLimit);
  const uint64_t z = static_cast<uint64_t>(static_cast<int64_t>(bz) + kBrickLimit);
  return static_cast<long long>((x << 42) | (y << 21) | z);
}

DVMVS_SG_HD void sg_unpack(long long key, int& bx, int& by, int& bz) {
  const uint64_t k = static_cast<uint64_t>(key);
  bx = static_cast<int>((k >> 42) & 0x1fffffu) - kBrickLimit;
  by = static_cast<int>((k >> 21) & 0x1fffffu) - kBrickLimit;
  bz = static_cast<int>(k & 0x1fffffu) - kBrickLimit;
}

// splitmix64's finaliser: neighbouring bricks differ in a few low bits of a field and must not land in neighbouring slots
DVMVS_SG_HD uint64_t sg_hash(long long key) {
  uint64_t h = static_cast<uint64_t>(key);
  h ^= h >> 30;
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 27;
  h *= 0x94d049bb133111ebull;
  h ^= h >> 31;
  return h;
}

// Slot of attempt i = 0 .. slots - 1 in a table of `slots` = mask + 1 entries, a power of two: linear probing from the hash.  Over
// i = 0 .. mask the sequence is a rotation of 0 .. mask, so it visits every slot exactly once, and a probe loop of `slots` attempts that
// finds neither the key nor a free slot has seen the whole table.
DVMVS_SG_HD uint64_t sg_probe(uint64_t hash, uint64_t i, uint64_t mask) { return (hash + i) & mask; }

}  // namespace dvmvs
